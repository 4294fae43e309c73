"""The checks shared by tests/test_emu_conv_epilogue.py (CPU emulation) and tests/test_gpu_conv_epilogue.py (MI355X): the epilogues
inside conv3x3_split_kernel (csrc/conv_fwd.hip, EPI) against the two-kernel paths they replace, bit for bit.  Not a test module.

  (a) hk_conv3x3_bias_relu_fwd       against hk_conv3x3_fwd, then hk_bias_relu_fwd               map and mask bit-equal
  (b) hk_conv3x3_bias_relu_pool_fwd  against hk_conv3x3_fwd, then hk_bias_relu_pool_fwd          p and argmax bit-equal
  (c) hk_conv3x3_masked_bwd_data     against hk_conv3x3_bwd_data, then hk_bias_relu_bwd          dx bit-equal; db within the bound below
  (d) a ConvStack with `conv_epi` 1 and 2 against 0

Bound on db (c, d): every order of fp32 additions of n terms stays within (n - 1) 2^-24 sum |term| of the exact sum (each of the n - 1
additions rounds a partial sum that is no larger than sum |term| by at most 2^-24 of it), so |db - db64| <= n_pixels 2^-24 sum |masked dx|
per channel, db64 the float64 column sums of the (bit-equal) masked dx.  The parent's order obeys the same bound.

Inputs come from tests/conv_fwd_cases.py; every output lies between guard rows of 1e30 (bytes: 0xA5) that have to survive."""
import ctypes

import torch

from conv_fwd_cases import case

SHAPES_A = [(1, 1, 1, 64, 64), (2, 3, 5, 64, 64), (1, 5, 33, 64, 128), (2, 7, 34, 128, 64), (1, 4, 28, 192, 192), (1, 10, 40, 64, 64)]
SHAPES_B = [(1, 2, 2, 64, 64), (2, 4, 6, 64, 64), (1, 6, 34, 64, 128), (1, 10, 40, 128, 64), (1, 4, 28, 192, 192)]
ids = lambda shapes: ['x'.join(map(str, s)) for s in shapes]
GUARD_BYTE = 0xA5


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Guarded:
    """A dense buffer of `numel` elements inside a larger allocation whose other elements hold a guard value."""

    def __init__(self, numel, dtype, dev, pad):
        self.fill = 1e30 if dtype == torch.float32 else GUARD_BYTE
        self.big = torch.full((numel + 2 * pad,), self.fill, dtype=dtype, device=dev)
        self.inner = self.big[pad:pad + numel]
        self.pad, self.numel = pad, numel
        assert self.inner.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.big[:self.pad] == self.fill).all()) and bool((self.big[self.pad + self.numel:] == self.fill).all())


def _nhwc_mem(t):
    """The NHWC memory of a channels_last [N, C, H, W] tensor as a flat view."""
    return t.permute(0, 2, 3, 1).reshape(-1)


def _as_nchw(flat, n, h, w, c):
    return flat.view(n, h, w, c).permute(0, 3, 1, 2)


def forward_inputs(shape, variant, dev):
    """x, w, bias on `dev`.  'signed': a signed bias, channel 5 driven wholly negative, one NaN in x; 'zero': a zero bias and image 0 all
    zeros (exact zeros out, clear mask bits, four equal values in every pooling window: the first wins, code 0)."""
    n, h, w, cin, cout = shape
    x, wt = case(shape)[:2]
    x, wt = x.clone(), wt.clone()
    g = torch.Generator().manual_seed(7 + sum(shape))
    if variant == 'signed':
        bias = torch.randn(cout, generator=g)
        bias[5] = -1e6
        x[n - 1, 3, h // 2, w // 2] = float('nan')
    else:
        bias = torch.zeros(cout)
        x[0] = 0.0
    return x.to(dev), wt.to(dev), bias.to(dev)


def _conv_ws(lib, cin, cout, dev):
    nws = lib.hk_conv3x3_ws_bytes(cin, cout)
    return torch.empty(max(nws, 16), dtype=torch.uint8, device=dev), nws


def check_bias_relu(F, lib, dev, shape, variant):
    n, h, w, cin, cout = shape
    x, wt, bias = forward_inputs(shape, variant, dev)
    ref = F.conv3x3_fwd_raw(x, wt)
    ref_mask = torch.empty(n, h, w, cout // 4, dtype=torch.uint8, device=dev)
    assert lib.hk_bias_relu_fwd(_p(ref), _p(bias), _p(ref_mask), n * h * w, cout, F.stream()) == 0
    row = w * cout
    y, mk = Guarded(n * h * w * cout, torch.float32, dev, 3 * row), Guarded(n * h * w * cout // 4, torch.uint8, dev, 16 * (row // 4))
    ws, nws = _conv_ws(lib, cin, cout, dev)
    rc = lib.hk_conv3x3_bias_relu_fwd(_p(x), _p(wt), _p(bias), _p(y.inner), _p(mk.inner), n, h, w, cin, cout, _p(ws), nws, F.stream())
    assert rc == 0, rc
    got, got_mask = _as_nchw(y.inner, n, h, w, cout), mk.inner.view(n, h, w, cout // 4)
    assert same_bits(_nhwc_mem(got), _nhwc_mem(ref)), (shape, variant, 'map')
    assert torch.equal(got_mask, ref_mask), (shape, variant, 'mask')
    assert y.intact() and mk.intact(), (shape, variant, 'guard rows')
    # without a mask (a forward that needs no gradient): the same map
    y2 = Guarded(n * h * w * cout, torch.float32, dev, 3 * row)
    assert lib.hk_conv3x3_bias_relu_fwd(_p(x), _p(wt), _p(bias), _p(y2.inner), None, n, h, w, cin, cout, _p(ws), nws, F.stream()) == 0
    assert same_bits(y2.inner, y.inner) and y2.intact()
    if variant == 'signed':
        nan5 = torch.isnan(got[:, 5])                                                            # channel 5: bit 1 of quad 1
        assert bool(((got[:, 5] == 0) | nan5).all()) and bool((((got_mask[..., 1] & 2) == 0) | nan5).all())
        hh, ww = h // 2, w // 2
        win = got[n - 1, :, max(hh - 1, 0):hh + 2, max(ww - 1, 0):ww + 2]
        assert bool(torch.isnan(win).all())                                                      # NaN + (-1e6) is NaN, too
        assert bool((got_mask[n - 1, max(hh - 1, 0):hh + 2, max(ww - 1, 0):ww + 2] == 15).all())  # a NaN output passes its gradient
    else:
        assert bool((bits(got[0]) == 0).all()) and bool((got_mask[0] == 0).all())                 # exact +0, clear bits


def check_bias_relu_pool(F, lib, dev, shape, variant):
    n, h, w, cin, cout = shape
    ho, wo = h // 2, w // 2
    x, wt, bias = forward_inputs(shape, variant, dev)
    full = F.conv3x3_fwd_raw(x, wt)
    ref = torch.empty(n, ho, wo, cout, device=dev)
    ref_am = torch.empty(n, ho, wo, cout // 4, dtype=torch.uint8, device=dev)
    assert lib.hk_bias_relu_pool_fwd(_p(full), _p(bias), _p(ref), _p(ref_am), n, h, w, cout, F.stream()) == 0
    row = wo * cout
    p, am = Guarded(n * ho * wo * cout, torch.float32, dev, 3 * row), Guarded(n * ho * wo * cout // 4, torch.uint8, dev, 16 * (row // 4))
    ws, nws = _conv_ws(lib, cin, cout, dev)
    rc = lib.hk_conv3x3_bias_relu_pool_fwd(_p(x), _p(wt), _p(bias), _p(p.inner), _p(am.inner), n, h, w, cin, cout, _p(ws), nws, F.stream())
    assert rc == 0, rc
    assert same_bits(p.inner, ref.reshape(-1)), (shape, variant, 'p')
    assert torch.equal(am.inner, ref_am.reshape(-1)), (shape, variant, 'argmax')
    assert p.intact() and am.intact(), (shape, variant, 'guard rows')
    if variant == 'zero':
        assert bool((bits(p.inner.view(n, -1)[0]) == 0).all()) and bool((am.inner.view(n, -1)[0] == 0).all())      # four equal values: the first wins
    else:
        assert bool(torch.isnan(p.inner).any())


def backward_inputs(shape, variant, dev):
    """dy, w, mask of the map the gradient is for ([N][H][W][Cin / 4] bytes).  'random': random sign bits with channel 6 clear
    everywhere; 'set': every bit set."""
    n, h, w, cin, cout = shape
    wt, dy = case(shape)[1:3]
    g = torch.Generator().manual_seed(11 + sum(shape))
    if variant == 'random':
        mask = torch.randint(0, 16, (n, h, w, cin // 4), generator=g, dtype=torch.uint8)
        mask[..., 1] &= 0xB                                                                     # channel 6 = bit 2 of quad 1
    else:
        mask = torch.full((n, h, w, cin // 4), 15, dtype=torch.uint8)
    return dy.to(dev), wt.to(dev), mask.to(dev)


def db_bound(dx_masked_nchw):
    """(db64, allowed) per channel from the masked input gradient (see the module's docstring)."""
    d = dx_masked_nchw.detach().double().cpu()
    npix = d.shape[0] * d.shape[2] * d.shape[3]
    return d.sum((0, 2, 3)), npix * 2.0 ** -24 * d.abs().sum((0, 2, 3))


def check_masked_bwd_data(F, lib, dev, shape, variant):
    n, h, w, cin, cout = shape
    dy, wt, mask = backward_inputs(shape, variant, dev)
    plain = F.conv3x3_bwd_data_raw(dy, wt)
    parent_db = None
    if 256 % (cin // 4) == 0:
        ref = torch.empty_like(plain, memory_format=torch.channels_last)
        parent_db = torch.empty(cin, device=dev)
        nws = lib.hk_trunk_ws_bytes(cin)
        tws = torch.empty(nws, dtype=torch.uint8, device=dev)
        assert lib.hk_bias_relu_bwd(_p(plain), None, _p(mask), _p(ref), _p(parent_db), n * h * w, cin, _p(tws), nws, F.stream()) == 0
    else:
        # hk_bias_relu_bwd refuses channel counts whose quads do not divide 256 (192): its select, spelled in torch
        keep = ((mask.unsqueeze(-1) >> torch.arange(4, device=dev, dtype=torch.uint8)) & 1).bool().view(n, h, w, cin).permute(0, 3, 1, 2)
        ref = torch.where(keep, plain, torch.zeros_like(plain))
    row = w * cin
    nws = lib.hk_conv3x3_masked_ws_bytes(n, h, w, cin, cout)
    assert nws >= lib.hk_conv3x3_ws_bytes(cin, cout) + 4 * cin
    outs = []
    for _ in range(2):
        dx, db = Guarded(n * h * w * cin, torch.float32, dev, 3 * row), Guarded(cin, torch.float32, dev, 64)
        ws = Guarded(nws, torch.uint8, dev, 4096)
        rc = lib.hk_conv3x3_masked_bwd_data(_p(dy), _p(wt), _p(mask), _p(dx.inner), _p(db.inner), n, h, w, cin, cout, _p(ws.inner), nws,
                                            F.stream())
        assert rc == 0, rc
        assert dx.intact() and db.intact() and ws.intact(), (shape, variant, 'guard rows')
        outs.append((dx.inner.clone(), db.inner.clone()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), (shape, variant, 'two launches')
    dx, db = outs[0]
    assert same_bits(dx, _nhwc_mem(ref)), (shape, variant, 'dx')
    db64, allowed = db_bound(ref)
    err = (db.double().cpu() - db64).abs()
    line = f'masked input gradient {shape} {variant}: max |db - db64| = {float(err.max()):.3e} (allowed at that channel {float(allowed[err.argmax()]):.3e})'
    if parent_db is not None:
        perr = (parent_db.double().cpu() - db64).abs()
        line += f'; two-kernel path {float(perr.max()):.3e}'
    print(line)
    assert bool((err <= allowed).all()), (shape, variant, float((err - allowed).max()))
    if variant == 'random':
        assert bool((bits(db[6:7]) == 0).all()) and bool((bits(_as_nchw(dx, n, h, w, cin)[:, 6]) == 0).all())      # the clear channel
    if parent_db is not None:
        nz = perr > 0
        assert bool((err[nz] <= 2 * perr[nz]).all()), (shape, variant, 'db farther from float64 than twice the two-kernel path',
                                                      float((err[nz] / perr[nz]).max()))


def make_stack(dev, n=2, h=8, w=36):
    from hawkeye_amd.model.backbone.vgg import ConvStack
    nn = torch.nn
    torch.manual_seed(23)
    mods = []
    for cin, cout, pool in ((64, 64, False), (64, 64, True), (64, 128, False), (128, 128, True)):
        mods += [nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(inplace=True)] + ([nn.MaxPool2d(2, 2)] if pool else [])
    stack = ConvStack(*mods).to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        for m in stack:
            if isinstance(m, nn.Conv2d):
                m.bias.normal_(0.0, 0.3)                       # signed biases: ReLU masks with both values
    g = torch.Generator().manual_seed(29)
    x = torch.randn(n, 64, h, w, generator=g).contiguous(memory_format=torch.channels_last).to(dev)
    dy = torch.randn(n, 128, h // 4, w // 4, generator=g).contiguous(memory_format=torch.channels_last).to(dev)
    return stack, x, dy


class Calls:
    """Counts the calls of entry points at the library handle."""

    def __init__(self, lib, monkeypatch, names):
        self.count = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(lib, k, self._wrap(k, getattr(lib, k)))

    def _wrap(self, name, real):
        def call(*a):
            self.count[name] += 1
            return real(*a)
        return call

    def take(self):
        c = dict(self.count)
        for k in self.count:
            self.count[k] = 0
        return c


def forward_by_hand(F, stack, x):
    """ConvStack.forward's loop with every GEMM on the kernels, for the CPU emulation: ConvStack itself sends tensors that are not
    HIP tensors to nn.Sequential's forward, so there the units and their links are driven from here."""
    epi, bwd = F.conv3x3_epi_level(), F._knob(b'conv_bwd_data') != 0
    mods, link = list(stack), None
    for i, m in enumerate(mods):
        if not isinstance(m, torch.nn.Conv2d):
            continue
        pool = i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.MaxPool2d)
        if epi >= 1:
            masked = link is not None and link.mask is not None and epi >= 2 and bwd
            with F.ConvEpilogue(m.bias, pool, masked, link) as unit:
                x = F.conv3x3(x, m.weight, True, bwd, True)
            link = unit.link
        else:
            y = F.conv3x3(x, m.weight, True, bwd, True)
            x, link = (F.bias_relu_pool if pool else F.bias_relu)(y, m.bias), None
    return x


def check_stack(F, lib, dev, tune, monkeypatch, by_hand=False):
    """64 -> 64, 64 -> 64, pool, 64 -> 128, 128 -> 128, pool on a 2 x 64 x 8 x 36 input that requires a gradient (the emulation, which
    drives the units by hand: 1 x 64 x 4 x 36 - one row tile per map, the same strips, pools and links)."""
    for knob in ('conv_fwd', 'conv_bwd_data', 'conv_wrw', 'wrw_split', 'wrw_wide'):
        tune(knob, 1)
    stack, x, dy = make_stack(dev, *((1, 4, 36) if by_hand else (2, 8, 36)))
    n, _, h, w = x.shape
    # the (masked) gradient every layer's weight gradient receives; two layers share each shape, the backward pass reaches the linked
    # one (the first, the third) last
    masked = {}
    real_wrw = F.conv3x3_wrw_raw
    monkeypatch.setattr(F, 'conv3x3_wrw_raw', lambda xx, g: (masked.__setitem__(tuple(g.shape), g.detach().clone()), real_wrw(xx, g))[1])
    calls = Calls(lib, monkeypatch, ('hk_bias_relu_fwd', 'hk_bias_relu_pool_fwd', 'hk_bias_relu_bwd', 'hk_bias_relu_pool_bwd',
                                     'hk_conv3x3_bias_relu_fwd', 'hk_conv3x3_bias_relu_pool_fwd', 'hk_conv3x3_masked_bwd_data',
                                     'hk_conv3x3_fwd', 'hk_conv3x3_bwd_data', 'hk_conv3x3_wrw'))

    def run(epi):
        tune('conv_epi', epi)
        stack.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y = forward_by_hand(F, stack, xi) if by_hand else stack(xi)
        y.backward(dy)
        convs = [m for m in stack if isinstance(m, torch.nn.Conv2d)]
        return y.detach(), xi.grad, [m.weight.grad.clone() for m in convs], [m.bias.grad.clone() for m in convs], calls.take()

    y0, dx0, dw0, db0, c0 = run(0)
    assert (c0['hk_conv3x3_fwd'], c0['hk_bias_relu_fwd'], c0['hk_bias_relu_pool_fwd'], c0['hk_bias_relu_bwd'], c0['hk_bias_relu_pool_bwd'],
            c0['hk_conv3x3_bwd_data'], c0['hk_conv3x3_wrw']) == (4, 2, 2, 2, 2, 4, 4)
    assert c0['hk_conv3x3_bias_relu_fwd'] == c0['hk_conv3x3_bias_relu_pool_fwd'] == c0['hk_conv3x3_masked_bwd_data'] == 0
    for epi in (1, 2):
        y, dx, dw, db, c = run(epi)
        assert same_bits(y, y0) and same_bits(dx, dx0), epi
        assert all(same_bits(a, b) for a, b in zip(dw, dw0)), epi
        assert (c['hk_conv3x3_fwd'], c['hk_bias_relu_fwd'], c['hk_bias_relu_pool_fwd']) == (0, 0, 0)
        assert (c['hk_conv3x3_bias_relu_fwd'], c['hk_conv3x3_bias_relu_pool_fwd'], c['hk_bias_relu_pool_bwd'], c['hk_conv3x3_wrw']) == (2, 2, 2, 4)
        if epi == 1:
            assert all(same_bits(a, b) for a, b in zip(db, db0))
            assert (c['hk_bias_relu_bwd'], c['hk_conv3x3_masked_bwd_data'], c['hk_conv3x3_bwd_data']) == (2, 0, 4)
        else:
            # the two linked layers (the first and the third): their masks are applied by the second and the fourth layer's input gradient
            assert (c['hk_bias_relu_bwd'], c['hk_conv3x3_masked_bwd_data'], c['hk_conv3x3_bwd_data']) == (0, 2, 2)
            assert same_bits(db[1], db0[1]) and same_bits(db[3], db0[3])                      # the pooled layers' own pass
    # db of the linked layers against float64 column sums of the masked gradient that reached them (bit-equal in all three routings: it
    # feeds the bit-equal weight gradients)
    for layer, shp in ((0, (n, 64, h, w)), (2, (n, 128, h // 2, w // 2))):
        db64, allowed = db_bound(masked[shp])
        err, perr = (db[layer].double().cpu() - db64).abs(), (db0[layer].double().cpu() - db64).abs()
        print(f'stack layer {layer}: max |db - db64| = {float(err.max()):.3e}, two-kernel path {float(perr.max()):.3e}, allowed there '
              f'{float(allowed[err.argmax()]):.3e}')
        assert bool((err <= allowed).all()), layer
    # the consumer's input gradient forced to the library: no mask travels, hk_bias_relu_bwd runs again
    tune('conv_bwd_data', 0)
    y, dx, dw, db, c = run(2)
    assert (c['hk_bias_relu_bwd'], c['hk_conv3x3_masked_bwd_data'], c['hk_conv3x3_bwd_data']) == (2, 0, 0)
    assert same_bits(y, y0) and same_bits(db[3], db0[3])        # (the other bias gradients follow the library's input gradients)
