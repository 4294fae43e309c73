"""The assembled trunk - ConvStack.forward's routing, functional._ConvUnit and the ConvLink protocol - against float64, shared by
tests/test_gpu_trunk_stack.py (MI355X) and tests/test_emu_trunk_stack.py (CPU emulation, the units driven by
conv_epilogue_cases.forward_by_hand).  Not a test module.

The judge.  A float64 twin of the stack cannot judge a gradient: a ReLU output within rounding of zero has either sign, and ONE sign
that differs between fp32 and float64 moves the input gradient and the first layer's gradients by about 1 / sqrt(elements)
(1e-3 .. 1e-2), a thousand times the rounding the test is after.  So the reference is float64 AT THE PATTERN THE DEVICE CHOSE: every
prefix of the stack that ends behind a ReLU or a pool runs on the device under no_grad (the kernels are deterministic and the pooled
epilogue forms the un-pooled one's values, so these are the internal maps of the full run), the ReLU pattern of a layer is `out > 0`
and the argmax of a pool is the first maximum in window order (ATen's rule, which the kernels copy).  `forced` is the stack in plain
torch with a product by that 0/1 mask for the ReLU and a gather at that argmax for the pool: a LINEAR function, in which no value near
zero can move a gradient.  In float64 it is the reference; in fp32, on the CPU, it is the yardstick - the reference's own rounding.

  forward    every layer's device output against relu(conv2d(a, w) + b) in float64, a the DEVICE's previous map (teacher forcing):
             |difference| <= c S elementwise, S = conv2d(|a|, |w|) + |b|, c = conv_fwd_cases.bound(Cin) for the 3 x 3 kernels.  The first
             layer (hk_conv1_bias_relu_fwd, fp32 FMA chains of 27 products and a bias: at most 28 roundings of partial sums that S
             bounds, c = 28 2^-24) also keeps its bound of tests/test_gpu_kernels.py, a relative norm below 1e-6.  Wherever
             |pre-activation64| > c S the sign is determined, and the device's pattern has to show it
  cap        the share of outputs with |pre-activation64| <= c S - where the pattern is free - is at most 0.02 % of a stack's outputs
             (the reference alone: 0.004 % at twice c on the short stack, 0.007 % on VGG-16), so that nothing passes by being free
  gradients  relative 2-norm distance to the float64 forced reference per parameter tensor and per image of dx, single shot; every
             one within FACTOR = 5 times the largest yardstick over the stack's tensors - the ratio the project grants its kernels over
             the fp32 library (c = 1e-6 .. 1.5e-6 against the library's measured 0.4 .. 3.1e-7).  One wrong pixel of a
             5,000-pixel map is about 1e-2."""
import torch

from conv_epilogue_cases import Calls, forward_by_hand, make_stack, same_bits
from conv_fwd_cases import bound

KNOBS = ('conv_fwd', 'conv_bwd_data', 'conv_wrw', 'wrw_split', 'wrw_wide')
FACTOR = 5.0
FREE_CAP = 2e-4
C_FIRST = 28 * 2.0 ** -24
COUNTED = ('hk_conv1_bias_relu_fwd', 'hk_bias_relu_fwd', 'hk_bias_relu_pool_fwd', 'hk_bias_relu_bwd', 'hk_bias_relu_pool_bwd',
           'hk_conv3x3_bias_relu_fwd', 'hk_conv3x3_bias_relu_pool_fwd', 'hk_conv3x3_masked_bwd_data', 'hk_conv3x3_fwd',
           'hk_conv3x3_bwd_data', 'hk_conv3x3_wrw')
conv2d = torch.nn.functional.conv2d
nn = torch.nn


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------ the stacks
def vgg_case(dev):
    """The whole VGG-16 stack on 2 x 3 x 32 x 80: maps of 32 x 80, 16 x 40, 8 x 20, 4 x 10 and 2 x 5 - every width ragged against
    the 32-column strip, H = 2 below the 4-row tile, the last stage odd (its pool is the MaxPool2d child).  The input needs no
    gradient: the first layer is hk_conv1_bias_relu's."""
    from hawkeye_amd.model.backbone.vgg import VGG16_LAYOUT, conv_stack
    torch.manual_seed(41)
    stack = conv_stack(VGG16_LAYOUT)
    with torch.no_grad():
        for m in stack:
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_in', nonlinearity='relu')       # maps of one size through thirteen layers
                m.bias.normal_(0.0, 0.1)                                                     # signed biases
    stack = stack.to(dev).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(43)
    x = nhwc(torch.randn(2, 3, 32, 80, generator=g)).to(dev)
    dy = nhwc(torch.randn(2, 512, 1, 2, generator=g)).to(dev)
    return stack, x, dy, False


def short_case(dev, by_hand=False):
    """conv_epilogue_cases.make_stack: 64 -> 64, 64 -> 64 + pool, 64 -> 128, 128 -> 128 + pool on 2 x 64 x 8 x 36 (emulated:
    1 x 64 x 4 x 36), the input requiring a gradient."""
    return make_stack(dev, *((1, 4, 36) if by_hand else (2, 8, 36))) + (True,)


def tiny_case(dev):
    """A batch of one with a 2 x 2 map: 64 -> 64, 64 -> 64 + pool, then 64 -> 128 and 128 -> 128 (a linked pair) at 1 x 1, where
    every tap but the centre is outside the image."""
    from hawkeye_amd.model.backbone.vgg import ConvStack
    torch.manual_seed(47)
    mods = []
    for cin, cout, pool in ((64, 64, False), (64, 64, True), (64, 128, False), (128, 128, False)):
        mods += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(inplace=True)] + ([nn.MaxPool2d(2, 2)] if pool else [])
    stack = ConvStack(*mods).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in stack:
            if isinstance(m, nn.Conv2d):
                m.bias.normal_(0.0, 0.3)
    g = torch.Generator().manual_seed(53)
    x = nhwc(torch.randn(1, 64, 2, 2, generator=g)).to(dev)
    dy = nhwc(torch.randn(1, 128, 1, 1, generator=g)).to(dev)
    return stack, x, dy, True


def layers_of(stack):
    """(index of the convolution, the convolution, whether a pool follows its ReLU) per layer."""
    mods = list(stack)
    return [(i, m, i + 2 < len(mods) and isinstance(mods[i + 2], nn.MaxPool2d)) for i, m in enumerate(mods) if isinstance(m, nn.Conv2d)]


def convs_of(stack):
    return [m for m in stack if isinstance(m, nn.Conv2d)]


def forward_of(F, by_hand):
    return (lambda stack, x: forward_by_hand(F, stack, x)) if by_hand else (lambda stack, x: stack(x))


# ------------------------------------------------------------------------------------------------------------------ the pattern
def windows(t):
    """[N, C, H, W] -> [N, C, H // 2, W // 2, 4]: the 2 x 2 windows in ATen's order (an odd last row or column belongs to none)."""
    n, c, h, w = t.shape
    ho, wo = h // 2, w // 2
    return t[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)


def first_argmax(t):
    """ATen's max_pool2d rule, which hk_bias_relu_pool_fwd and the pooled epilogue copy: (val > max) || isnan(val), so the first
    maximum in window order wins."""
    v = windows(t)
    best, idx = v[..., 0].clone(), torch.zeros(v.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        take = (v[..., k] > best) | torch.isnan(v[..., k])
        best, idx = torch.where(take, v[..., k], best), torch.where(take, torch.full_like(idx, k), idx)
    return idx


def prefix_maps(fwd, stack, x):
    """(map behind the ReLU, map behind the pool or None) of every layer, on the CPU: stack[:k] run under no_grad for every k."""
    maps = []
    with torch.no_grad():
        for i, _, pool in layers_of(stack):
            r = fwd(stack[:i + 2], x).cpu()
            maps.append((r, fwd(stack[:i + 3], x).cpu() if pool else None))
    return maps


def patterns_of(maps, asserting=True):
    """(ReLU pattern, argmax or None) per layer.  For nothing extra: the prefix behind a pool equals, bit for bit, max_pool2d of the
    prefix in front of it, and the gather at the argmax."""
    pats = []
    for k, (r, p) in enumerate(maps):
        am = None
        if p is not None:
            am = first_argmax(r)
            ok = same_bits(p, torch.nn.functional.max_pool2d(r, 2, 2)) and same_bits(p, windows(r).gather(-1, am.unsqueeze(-1)).squeeze(-1))
            assert ok or not asserting, f'layer {k}: the pooled prefix is not the max-pool of the prefix in front of it'
        pats.append((r > 0, am))
    return pats


def same_patterns(a, b):
    return all(torch.equal(ma, mb) and (ia is None or torch.equal(ia, ib)) for (ma, ia), (mb, ib) in zip(a, b))


def params_of(stack):
    return [(m.weight.detach().cpu(), m.bias.detach().cpu(), pool) for _, m, pool in layers_of(stack)]


# ------------------------------------------------------------------------------------------------------------------ the reference
def forced(stack_params, x, patterns, dtype):
    """The stack of `stack_params` ((weight, bias, pool) per layer) on x in `dtype` with the ReLU replaced by a product with the given
    0/1 mask and the pool by a gather at the given argmax: plain torch, linear in x and in every parameter of one layer.  Returns
    the output and the leaves (x, [(weight, bias)]) for the usual autograd backward."""
    xl = x.detach().to(dtype).requires_grad_(True)
    leaves, a = [], xl
    for (w, b, pool), (mask, am) in zip(stack_params, patterns):
        wl, bl = w.detach().to(dtype).requires_grad_(True), b.detach().to(dtype).requires_grad_(True)
        leaves.append((wl, bl))
        a = conv2d(a, wl, bl, padding=1) * mask.to(dtype)
        if pool:
            a = windows(a).gather(-1, am.unsqueeze(-1)).squeeze(-1)
    return a, xl, leaves


def forced_grads(stack_params, x, patterns, dy, dtype):
    y, xl, leaves = forced(stack_params, x.cpu(), patterns, dtype)
    y.backward(dy.detach().cpu().to(dtype))
    out = {'dx': xl.grad}
    for k, (wl, bl) in enumerate(leaves):
        out[f'dW{k}'], out[f'db{k}'] = wl.grad, bl.grad
    return out


def distances(got, ref64):
    """Relative 2-norm distance per parameter tensor and per image of dx."""
    d = {}
    for name, r in ref64.items():
        if name not in got:
            continue
        g = got[name].detach().double().cpu()
        if name == 'dx':
            for i in range(r.shape[0]):
                d[f'dx[{i}]'] = float((g[i] - r[i]).norm() / r[i].norm())
        else:
            d[name] = float((g - r).norm() / r.norm())
    return d


class Judge:
    """The float64 forced reference and the fp32 yardstick of one stack on one input at the pattern of `maps`; computed once and
    left unchanged."""

    def __init__(self, stack, x, dy, maps, asserting=True):
        self.params, self.maps, self.x = params_of(stack), maps, x.detach().cpu()
        self.patterns = patterns_of(maps, asserting)
        self.ref = forced_grads(self.params, x, self.patterns, dy, torch.float64)
        self.yard = distances(forced_grads(self.params, x, self.patterns, dy, torch.float32), self.ref)

    def forward(self, what):
        """Every layer's device map against float64 on the device's previous map; returns the free-pattern share."""
        free = total = 0
        a = self.x.double()
        for k, ((w, b, pool), (r, p)) in enumerate(zip(self.params, self.maps)):
            w64, b64 = w.double(), b.double()
            pre = conv2d(a, w64, b64, padding=1)
            s = conv2d(a.abs(), w64.abs(), None, padding=1) + b64.abs().view(1, -1, 1, 1)
            cin = w.shape[1]
            c = bound(cin) if cin % 64 == 0 else C_FIRST
            diff = (r.double() - torch.relu(pre)).abs()
            worst = float((diff / s.clamp_min(1e-300)).max())
            decided = pre.abs() > c * s
            wrong = int((decided & ((r > 0) != (pre > 0))).sum())
            nfree = int((~decided).sum())
            free, total = free + nfree, total + pre.numel()
            rel = float((r.double() - torch.relu(pre)).norm() / torch.relu(pre).norm())
            print(f'[{what}] layer {k} ({cin} -> {w.shape[0]}, {r.shape[2]} x {r.shape[3]}{", pool" if pool else ""}): max |y - y64| / S = '
                  f'{worst:.3e} (bound {c:.2e}), relative norm {rel:.2e}, free {nfree} of {pre.numel()}, decided signs wrong {wrong}')
            assert bool((diff <= c * s).all()), (what, k, worst)
            if cin % 64 != 0:
                assert rel < 1e-6, (what, k, rel)                           # the first layer's bound of tests/test_gpu_kernels.py
            assert wrong == 0, (what, k, wrong)
            a = (p if pool else r).double()
        share = free / total
        print(f'[{what}] free pattern: {free} of {total} outputs = {100 * share:.4f} % (cap {100 * FREE_CAP:.2f} %)')
        assert share <= FREE_CAP, (what, share)
        return share

    def gradients(self, what, got, asserting=True):
        """Every tensor's distance to the forced float64 reference beside 5 x its own yardstick; asserted against 5 x the largest."""
        d = distances(got, self.ref)
        allowed = FACTOR * max(self.yard[name] for name in d)
        for name, v in d.items():
            print(f'[{what}] {name}: {v:.3e} to float64 at the device\'s pattern; 5 x its own yardstick {FACTOR * self.yard[name]:.3e}; '
                  f'asserted {allowed:.3e}')
        assert all(v == v and v != float('inf') for v in d.values()), (what, d)
        if asserting:
            bad = {name: v for name, v in d.items() if not v <= allowed}
            assert not bad, (what, f'farther than {allowed:.3e} from float64', bad)
        return d


# ------------------------------------------------------------------------------------------------------------------ the device runs
def train_run(fwd, stack, x, dy, x_grad):
    """One forward and backward: y, dx (where the input takes one), dW and db of every layer that takes them, on the CPU."""
    stack.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(x_grad)
    y = fwd(stack, xi)
    y.backward(dy)
    return collect(stack, y, xi)


def collect(stack, y, xi):
    out = {'y': y.detach().cpu()}
    if xi.grad is not None:
        out['dx'] = xi.grad.cpu()
    for k, m in enumerate(convs_of(stack)):
        if m.weight.grad is not None:
            out[f'dW{k}'] = m.weight.grad.cpu()
        if m.bias.grad is not None:
            out[f'db{k}'] = m.bias.grad.cpu()
    return out


def differing(a, b, names=None):
    """The names at which two runs differ in a bit (or in which tensors they hold)."""
    names = (set(a) | set(b)) if names is None else names
    return sorted(n for n in names if n not in a or n not in b or not same_bits(a[n], b[n]))


def expected_calls(stack, maps, x_grad):
    """What a training step of the stack at `conv_epi` 2 calls with every knob of KNOBS at 1, from the stack's structure: every
    layer of a multiple of 64 input channels is one fused unit, pooled inside the kernel where its map is even; an un-pooled unit
    whose next child is a convolution hands that one its mask (a linked pair)."""
    mods, ls = list(stack), layers_of(stack)
    e = dict.fromkeys(COUNTED, 0)
    for k, (i, m, pool) in enumerate(ls):
        if m.in_channels % 64 != 0:
            e['hk_conv1_bias_relu_fwd'] += 1
            continue
        h, w = maps[k][0].shape[2:]
        fused_pool = pool and h % 2 == 0 and w % 2 == 0
        e['hk_conv3x3_bias_relu_pool_fwd' if fused_pool else 'hk_conv3x3_bias_relu_fwd'] += 1
        e['hk_conv3x3_wrw'] += 1
        linked_in = k > 0 and ls[k - 1][1].in_channels % 64 == 0 and ls[k - 1][0] + 2 == i
        linked_out = i + 2 < len(mods) and isinstance(mods[i + 2], nn.Conv2d) and mods[i + 2].in_channels % 64 == 0
        if fused_pool:
            e['hk_bias_relu_pool_bwd'] += 1
        elif not linked_out:
            e['hk_bias_relu_bwd'] += 1
        if k > 0 or x_grad:
            e['hk_conv3x3_masked_bwd_data' if linked_in else 'hk_conv3x3_bwd_data'] += 1
    return e


def linked_producers(stack):
    """The layers whose bias gradient the NEXT layer's input gradient sums at `conv_epi` 2, in another order than hk_bias_relu_bwd."""
    mods = list(stack)
    return [k for k, (i, m, pool) in enumerate(layers_of(stack))
            if m.in_channels % 64 == 0 and i + 2 < len(mods) and isinstance(mods[i + 2], nn.Conv2d)]


def check_judged(F, lib, dev, tune, monkeypatch, case, by_hand=False):
    """Section 1 on one stack: `conv_epi` 2, 1 and 0, each run twice (the same bits), the three levels against each other as
    conv_epilogue_cases.check_stack does (all but the linked layers' bias gradients at level 2, which are summed in another order,
    bit for bit), the calls of level 2 from the stack's structure, and every level judged against float64 at the device's pattern."""
    for knob in KNOBS:
        tune(knob, 1)
    stack, x, dy, x_grad = case
    fwd = forward_of(F, by_hand)
    what = f'{len(layers_of(stack))} layers on {"x".join(map(str, x.shape))}'
    tune('conv_epi', 2)
    maps = prefix_maps(fwd, stack, x)
    judge = Judge(stack, x, dy, maps)
    judge.forward(what)
    calls = Calls(lib, monkeypatch, COUNTED)
    runs, counted = {}, {}
    for epi in (2, 1, 0):
        tune('conv_epi', epi)
        calls.take()
        runs[epi] = train_run(fwd, stack, x, dy, x_grad)
        counted[epi] = calls.take()
        judge.gradients(f'{what}, conv_epi {epi}', runs[epi])                      # the float64 judge first, single shot
        assert same_bits(runs[epi]['y'], maps[-1][0] if maps[-1][1] is None else maps[-1][1]), (epi, 'the last prefix is not the full run')
        again = train_run(fwd, stack, x, dy, x_grad)
        assert not differing(runs[epi], again), (epi, 'a second pass differs in', differing(runs[epi], again))
    expect = expected_calls(stack, maps, x_grad)
    assert counted[2] == expect, ('a layer left the fused route', {k: (counted[2][k], expect[k]) for k in expect if counted[2][k] != expect[k]})
    free_db = {f'db{k}' for k in linked_producers(stack)}
    assert not differing(runs[1], runs[0]), differing(runs[1], runs[0])
    assert not differing(runs[2], runs[0], set(runs[0]) - free_db), differing(runs[2], runs[0], set(runs[0]) - free_db)
    return judge, runs


# ------------------------------------------------------------------------------------------------------------------ section 3
def _grads(outs, names):
    return {n: (None if g is None else g.detach().cpu()) for n, g in zip(names, outs)}


def _freeze(ps, on=False):
    for p in ps:
        p.requires_grad_(on)


def link_case(F, lib, dev, tune, monkeypatch, epi, name, by_hand=False):
    """One configuration of the link protocol on the short stack: the gradients it computes against the all-trainable run of the same
    stack on the same input (which section 1 judges against float64), bit for bit - the kernels are deterministic and every gradient
    is formed by the same calls, so a difference is a fault of the glue."""
    for knob in KNOBS:
        tune(knob, 1)
    tune('conv_epi', epi)
    stack, x, dy, _ = short_case(dev, by_hand)
    fwd = forward_of(F, by_hand)
    convs = convs_of(stack)
    ref = train_run(fwd, stack, x, dy, True)
    every = set(ref) - {'y'}
    calls = Calls(lib, monkeypatch, ('hk_conv3x3_masked_bwd_data', 'hk_bias_relu_bwd', 'hk_conv3x3_bwd_data'))

    def equal(got, names):
        assert set(got) - {'y'} == set(names), (name, sorted(got), sorted(names))
        assert not differing(got, ref, set(names) | {'y'}), (name, differing(got, ref, set(names) | {'y'}))

    try:
        if name == 'input-without-gradient':                         # the training case
            equal(train_run(fwd, stack, x, dy, False), every - {'dx'})
            c = calls.take()
            assert (c['hk_conv3x3_masked_bwd_data'], c['hk_conv3x3_bwd_data']) == ((2, 1) if epi == 2 else (0, 3))
        elif name == 'producer-frozen':                              # the third layer, weight and bias; the first two train
            _freeze([convs[2].weight, convs[2].bias])
            equal(train_run(fwd, stack, x, dy, True), every - {'dW2', 'db2'})
        elif name == 'producer-bias-frozen':                         # the consumer still sums it: dropped, not delivered
            _freeze([convs[2].bias])
            equal(train_run(fwd, stack, x, dy, True), every - {'db2'})
        elif name == 'consumer-weight-frozen':                       # the masked input gradient is still needed
            _freeze([convs[3].weight, convs[1].weight])
            equal(train_run(fwd, stack, x, dy, True), every - {'dW3', 'dW1'})
            assert calls.take()['hk_conv3x3_masked_bwd_data'] == (2 if epi == 2 else 0)
        elif name == 'first-two-frozen':                             # and no input gradient: no mask exists in front of the pool
            _freeze([convs[0].weight, convs[0].bias, convs[1].weight, convs[1].bias])
            equal(train_run(fwd, stack, x, dy, False), {'dW2', 'db2', 'dW3', 'db3'})
            c = calls.take()
            assert (c['hk_conv3x3_masked_bwd_data'], c['hk_bias_relu_bwd'], c['hk_conv3x3_bwd_data']) == ((1, 0, 0) if epi == 2 else (0, 1, 1))
        elif name == 'accumulation':                                 # two backward passes through one graph: exactly twice
            stack.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = fwd(stack, xi)
            y.backward(dy, retain_graph=True)
            y.backward(dy, retain_graph=True)
            got = collect(stack, y, xi)
            twice = {n: (g if n == 'y' else g + g) for n, g in ref.items()}
            assert not differing(got, twice), (name, differing(got, twice))
        elif name == 'partial-backward':                             # leaves a bias gradient in a link unconsumed
            stack.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = fwd(stack, xi)
            (dw3,) = torch.autograd.grad(y, convs[3].weight, dy, retain_graph=True)
            assert same_bits(dw3.cpu(), ref['dW3'])
            y.backward(dy)
            equal(collect(stack, y, xi), every)
        elif name == 'overlapping-graphs':                           # two forwards before either backward (twin-BCNN, pairwise)
            x2 = nhwc(torch.randn(x.shape, generator=torch.Generator().manual_seed(31))).to(dev)
            ref2 = train_run(fwd, stack, x2, dy, True)
            stack.zero_grad(set_to_none=True)
            leaves = [p for m in convs for p in (m.weight, m.bias)]
            names = ['dx'] + [f'd{t}{k}' for k in range(len(convs)) for t in ('W', 'b')]
            xa, xb = x.clone().requires_grad_(True), x2.clone().requires_grad_(True)
            ya = fwd(stack, xa)
            yb = fwd(stack, xb)
            ga = _grads(torch.autograd.grad(ya, [xa] + leaves, dy), names)          # the first graph's backward first: the other
            gb = _grads(torch.autograd.grad(yb, [xb] + leaves, dy), names)          # order than autograd's own, last in first out
            ga['y'], gb['y'] = ya.detach().cpu(), yb.detach().cpu()
            assert not differing(ga, ref), (name, 'first', differing(ga, ref))
            assert not differing(gb, ref2), (name, 'second', differing(gb, ref2))
            assert differing(ref, ref2) == sorted(ref)               # (the two inputs really give other gradients)
        elif name == 'no-grad-then-training':                        # no stale state from a forward that keeps nothing
            with torch.no_grad():
                y0 = fwd(stack, x).cpu()
            assert same_bits(y0, ref['y'])
            equal(train_run(fwd, stack, x, dy, True), every)
        elif name == 'checkpoint':
            from torch.utils.checkpoint import checkpoint
            stack.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = checkpoint(lambda t: fwd(stack, t), xi, use_reentrant=False)
            y.backward(dy)
            equal(collect(stack, y, xi), every)
        else:
            raise KeyError(name)
    finally:
        _freeze(stack.parameters(), True)


LINK_CASES = ('input-without-gradient', 'producer-frozen', 'producer-bias-frozen', 'consumer-weight-frozen', 'first-two-frozen',
              'accumulation', 'partial-backward', 'overlapping-graphs', 'no-grad-then-training', 'checkpoint')
