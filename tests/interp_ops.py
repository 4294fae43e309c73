"""The InterpParts checks that the emulated tier (test_emu_interp.py) and the GPU tier (test_gpu_interp.py) share: each takes
the device to run on.  Values are judged by the project's rule (tests/golden/crossx_inputs.py: judge_value) - at most 4 x the
float32 reference's own distance from the float64 result, floor 1e-6; what is exactly zero in float64 must be exactly zero.
The grouping unit is judged against the reference's own op sequence (Interp_Parts.py:56-122: bmm, pow(2).sum(1), clamp,
softmax, the permuted bmm, clamp, the residual coding, normalize, permute) in torch on the CPU and its autograd - float64, with
its float32 run as the yardstick - computed once per case; the loss against the reference's goldens.  Not a test module."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

import interp_inputs as T

GOLDEN = T.load()
LOSS_CASES = T.load_loss_cases(GOLDEN)
GRADS = ('d_outputs_t', 'd_assign')
RESULTS = ('outputs_t', 'assign', 'dx', 'd_weight', 'd_smooth')


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------- grouping
def group_reference(a, dtype, use=GRADS):
    """GroupingUnit.forward's op sequence in torch on the CPU, forward and backward; the upstream gradients named in `use`
    enter, the others are zero."""
    inputs, weight, smooth = (torch.from_numpy(a[k]).to(dtype).requires_grad_(True) for k in ('x', 'weight', 'smooth'))
    n, c, h, w = inputs.shape
    k = weight.shape[0]
    centers = weight.contiguous().view(1, k, c).expand(n, k, c)
    cx = torch.bmm(centers, inputs.contiguous().view(n, c, h * w)).contiguous().view(n, k, h, w)
    x_sq = inputs.pow(2).sum(1, keepdim=True).expand(-1, k, -1, -1)
    c_sq = centers.pow(2).sum(2).unsqueeze(2).unsqueeze(3).expand(-1, -1, h, w)
    beta = torch.sigmoid(smooth)
    beta_batch = beta.unsqueeze(0).unsqueeze(2).unsqueeze(3).expand(n, -1, h, w)
    assign = TF.softmax((2 * cx - x_sq - c_sq).clamp(max=0.0) / beta_batch, dim=1)
    x = inputs.contiguous().view(n, c, -1).permute(0, 2, 1)
    assign = assign.contiguous().view(n, k, -1)
    qx = torch.bmm(assign, x)
    sum_ass = torch.sum(assign, dim=2, keepdim=True).expand(-1, -1, c).clamp(min=1e-5)
    sigma = (beta / 2).sqrt()
    out = ((qx / sum_ass) - centers) / sigma.unsqueeze(0).unsqueeze(2)
    assign = assign.contiguous().view(n, k, h, w)
    outputs_t = TF.normalize(out, dim=2).permute(0, 2, 1)
    total = inputs.sum() * 0 + weight.sum() * 0 + smooth.sum() * 0
    if 'd_outputs_t' in use:
        total = total + (outputs_t * torch.from_numpy(a['d_outputs_t']).to(dtype)).sum()
    if 'd_assign' in use:
        total = total + (assign * torch.from_numpy(a['d_assign']).to(dtype)).sum()
    total.backward()
    got = dict(outputs_t=outputs_t, assign=assign, dx=inputs.grad, d_weight=weight.grad, d_smooth=smooth.grad)
    return {key: np.ascontiguousarray(v.detach().numpy()) for key, v in got.items()}


@functools.lru_cache(maxsize=None)
def group_case(case):
    a = T.clamp_inputs() if case == T.CLAMP_CASE else T.group_inputs(case)
    return a, group_reference(a, torch.float32), group_reference(a, torch.float64)


def group_tensors(a, device):
    return {k: torch.from_numpy(v).to(device) for k, v in a.items()}


def run_group(a, device, use=GRADS, tensors=None, need=(True, True, True)):
    """Forward through the autograd node, backward through the raw entry point."""
    from hawkeye_amd.functional import _IPGroup
    HF = F()
    t = tensors or group_tensors(a, device)
    n, c, h, w = a['x'].shape
    k = a['weight'].shape[0]

    class Ctx:                                             # the node's forward, with its saved tensors in hand
        needs_input_grad = (False, False, False)

        def save_for_backward(self, *ts):
            self.saved = ts

        def set_materialize_grads(self, flag):
            pass
    ctx = Ctx()
    with torch.no_grad():
        outputs_t, assign = _IPGroup.forward(ctx, t['x'], t['weight'], t['smooth'])
        again = HF.ip_group(t['x'], t['weight'], t['smooth'])
    assert outputs_t.shape == (n, c, k) and assign.shape == (n, k, h, w)
    assert torch.equal(again[0], outputs_t) and torch.equal(again[1], assign)
    grads = HF.ip_group_bwd(*ctx.saved, *[t[g] if g in use else None for g in GRADS], need=need)
    for g, shape, wanted in zip(grads, ((n, c, h, w), (k, c), (k,)), need):
        assert (g is None) != wanted and (g is None or tuple(g.shape) == shape)
    out = dict(outputs_t=outputs_t, assign=assign, dx=grads[0], d_weight=grads[1], d_smooth=grads[2])
    return {key: np_(v) for key, v in out.items() if v is not None}


def judge_group(label, got, r32, r64, names=RESULTS):
    return max(T.judge_value(label, name, got[name], r32[name], r64[name]) for name in names)


def check_group_case(case, device):
    a, r32, r64 = group_case(tuple(case))
    got = run_group(a, device)
    worst = judge_group(f'group {T.group_case_id(case)}', got, r32, r64)
    assert np.allclose(got['assign'].sum(1), 1.0, atol=1e-5)
    if case[2] == 1:                                       # one part: the softmax is identically 1 and nothing passes through it
        assert (got['assign'] == 1).all()
        only_direct = run_group(dict(a, d_assign=np.zeros_like(a['d_assign'])), device)
        assert np.array_equal(got['d_weight'], only_direct['d_weight']) and np.array_equal(got['d_smooth'], only_direct['d_smooth'])
        n, c, k, h, w = case
        if h * w > 1:                                      # dx: through q alone, a[k,p] dq[k,c]
            assert np.array_equal(got['dx'], only_direct['dx'])
    return worst


def check_group_null_gradient(missing, device, case=(3, 64, 5, 7, 9)):
    """One of d_outputs_t, d_assign missing: through the raw call, and through autograd with that output unused."""
    HF = F()
    a = group_case(tuple(case))[0]
    use = tuple(g for g in GRADS if g != missing)
    got = run_group(a, device, use)
    judge_group(f'group without {missing}', got, group_reference(a, torch.float32, use), group_reference(a, torch.float64, use))
    dense = run_group(dict(a, **{missing: np.zeros_like(a[missing])}), device)
    assert all(got[k].tobytes() == dense[k].tobytes() for k in RESULTS), missing                 # NULL is a tensor of zeros
    t = group_tensors(a, device)
    leaves = [t['x'].clone().requires_grad_(True), t['weight'].clone().view(*t['weight'].shape, 1, 1).requires_grad_(True),
              t['smooth'].clone().requires_grad_(True)]
    outputs_t, assign = HF.ip_group(*leaves)
    kept = dict(d_outputs_t=outputs_t, d_assign=assign)[use[0]]
    (kept * t[use[0]]).sum().backward()
    assert leaves[1].grad.shape == leaves[1].shape and leaves[2].grad.shape == leaves[2].shape        # the parameters' own shapes
    assert np_(leaves[0].grad).tobytes() == got['dx'].tobytes()
    assert np_(leaves[1].grad).reshape(got['d_weight'].shape).tobytes() == got['d_weight'].tobytes()
    assert np_(leaves[2].grad).tobytes() == got['d_smooth'].tobytes()


def check_group_need_flags(device, case=(3, 64, 5, 7, 9)):
    a = group_case(tuple(case))[0]
    full = run_group(a, device)
    for off in range(3):
        need = tuple(i != off for i in range(3))
        got = run_group(a, device, need=need)
        assert RESULTS[2 + off] not in got
        assert all(got[k].tobytes() == full[k].tobytes() for k in got), need


def check_group_views(device, case=(2, 64, 32, 5, 5), aligned_case=(2, 128, 1, 4, 4)):
    """A map behind a base pointer that is not 16-byte aligned (the scalar path, where the dense map takes the 16-byte one) and
    non-contiguous tensors give the bits of the dense, aligned ones."""
    for cs in (aligned_case, case):
        a = group_case(tuple(cs))[0]
        dense = run_group(a, device)
        t = group_tensors(a, device)
        buf = torch.zeros(t['x'].numel() + 5, device=device)
        view = buf[1:1 + t['x'].numel()].view(t['x'].shape)
        view.copy_(t['x'])
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        got = run_group(a, device, tensors=dict(t, x=view))
        assert all(got[k].tobytes() == dense[k].tobytes() for k in dense), ('offset view', cs)
        twice = lambda v: torch.stack([v, v], -1)[..., 0]
        strided = dict(t, **{k: twice(t[k]) for k in ('x', 'weight', 'd_assign', 'd_outputs_t')})
        assert not any(strided[k].is_contiguous() for k in ('x', 'weight', 'd_assign', 'd_outputs_t'))
        got = run_group(a, device, tensors=strided)
        assert all(got[k].tobytes() == dense[k].tobytes() for k in dense), ('strided views', cs)


def check_group_reruns(device, case=(3, 64, 5, 7, 9)):
    a = group_case(tuple(case))[0]
    first, again = run_group(a, device), run_group(a, device)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


def check_group_clamp(device):
    """One pixel equal to a centre: its pre-clamp logit is rounding noise around 0.  The clamp holds it at or below 0 - then
    that part's logit is the pixel's largest and its assignment at least 1 / K, at most 1 - and the forward stays within
    the rule; the gradients are finite (across the clamp's corner the reference's float32 and float64 runs may take
    different sides, so they are not judged here)."""
    a, r32, r64 = group_case(T.CLAMP_CASE)
    got = run_group(a, device)
    n, c, k, h, w = T.CLAMP_CASE
    at = got['assign'].reshape(n, k, h * w)[0, :, T.CLAMP_AT]
    assert at[T.CLAMP_PART] == at.max() and 1.0 / k <= at[T.CLAMP_PART] <= 1.0
    assert all(np.isfinite(got[name]).all() for name in RESULTS)
    return judge_group('group clamp', got, r32, r64, RESULTS[:2])


def s_clamp_inputs(case=(2, 64, 3, 3, 5), far=2, shift=0.4):
    """One centre moved away from every pixel: its assignments sum to far less than 1e-5, the clamp of that sum is active."""
    a = {k: v.copy() for k, v in T.group_inputs(case).items()}
    a['weight'][far] += np.float32(shift)
    raw, sums = T.group_margins(a)
    assert 0 < sums[:, far].max() < 1e-6 < 1e-4 < sums[:, :far].min() and np.abs(raw).min() >= 1e-3
    return a


def check_group_s_clamp(device):
    """The active side of the clamp of sum_p a: q is divided by 1e-5 and no gradient passes through the sum - forward and all
    three gradients within the rule against the reference's sequence and its autograd."""
    a = s_clamp_inputs()
    got = run_group(a, device)
    return judge_group('group S clamp', got, group_reference(a, torch.float32), group_reference(a, torch.float64))


def check_group_refused(device):
    """K = 33 and C = 96: HK_ERR_UNSUPPORTED before any launch - guard rows around every output untouched."""
    from hawkeye_amd import _lib
    HF = F()
    lib = _lib.load()
    for n, c, k, h, w in ((1, 64, 33, 2, 2), (1, 96, 3, 2, 2)):
        try:
            HF.ip_group(torch.zeros(n, c, h, w, device=device), torch.zeros(k, c, 1, 1, device=device), torch.zeros(k, device=device))
        except _lib.HawkeyeHipError as e:
            assert ('parts' if k == 33 else 'multiple of 64') in str(e)
        else:
            raise AssertionError((c, k))
        assert lib.hk_ip_group_fwd_ws_bytes(n, c, k, h, w) == 0 and lib.hk_ip_group_bwd_ws_bytes(n, c, k, h, w) == 0
        mk = lambda *s: torch.full(s, 7.0, device=device)
        x, cw, sm = mk(n, c, h, w), mk(k, c), mk(k)
        guarded = [mk(2 + numel) for numel in (n * c * k, n * k * h * w, n * k, n * k, n * c * h * w, k * c, k)]
        inner = [g[1:-1] for g in guarded]
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
        rc = lib.hk_ip_group_fwd(HF.ptr(x), HF.ptr(cw), HF.ptr(sm), *[HF.ptr(g) for g in inner[:4]], n, c, k, h, w, HF.ptr(ws), 1 << 16,
                                 HF.stream())
        assert rc == _lib.HK_ERR_UNSUPPORTED
        rc = lib.hk_ip_group_bwd(HF.ptr(x), HF.ptr(cw), HF.ptr(sm), *[HF.ptr(g) for g in inner[:1] + inner[2:4]], None, None,
                                 *[HF.ptr(g) for g in inner[4:]], n, c, k, h, w, HF.ptr(ws), 1 << 16, HF.stream())
        assert rc == _lib.HK_ERR_UNSUPPORTED
        assert all((g == 7).all() for g in guarded)


def check_group_workspace(device, case=(3, 64, 5, 7, 9)):
    """The size query is what the call needs: with exactly that many bytes it runs (the emulated tier's sanitizer build sees
    any access beyond them), with one byte less it returns HK_ERR_WORKSPACE and writes nothing."""
    from hawkeye_amd import _lib
    HF = F()
    lib = _lib.load()
    a = group_case(tuple(case))[0]
    t = group_tensors(a, device)
    n, c, k, h, w = case
    full = run_group(a, device)
    outs = [torch.full(s, 7.0, device=device) for s in ((n, c, k), (n, k, h, w), (n, k), (n, k))]
    need = lib.hk_ip_group_fwd_ws_bytes(n, c, k, h, w)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    call = lambda nbytes: lib.hk_ip_group_fwd(HF.ptr(t['x']), HF.ptr(t['weight']), HF.ptr(t['smooth']), *[HF.ptr(o) for o in outs], n, c, k, h,
                                              w, HF.ptr(ws), nbytes, HF.stream())
    assert call(need - 1) == _lib.HK_ERR_WORKSPACE and all((o == 7).all() for o in outs)
    assert call(need) == _lib.HK_OK and np_(outs[0]).tobytes() == full['outputs_t'].tobytes()
    grads = [torch.full(s, 7.0, device=device) for s in ((n, c, h, w), (k, c), (k,))]
    bneed = lib.hk_ip_group_bwd_ws_bytes(n, c, k, h, w)
    bws = torch.zeros(bneed, dtype=torch.uint8, device=device)
    bcall = lambda nbytes: lib.hk_ip_group_bwd(HF.ptr(t['x']), HF.ptr(t['weight']), HF.ptr(t['smooth']), HF.ptr(outs[0]), HF.ptr(outs[2]),
                                               HF.ptr(outs[3]), HF.ptr(t['d_outputs_t']), HF.ptr(t['d_assign']), *[HF.ptr(g) for g in grads], n,
                                               c, k, h, w, HF.ptr(bws), nbytes, HF.stream())
    assert bcall(bneed - 1) == _lib.HK_ERR_WORKSPACE and all((g == 7).all() for g in grads)
    assert bcall(bneed) == _lib.HK_OK and np_(grads[0]).tobytes() == full['dx'].tobytes()


# ---------------------------------------------------------------------------------------------------------- loss
def loss_tensors(case, device, grad=True):
    return [torch.from_numpy(case[k]).to(device).requires_grad_(grad) for k in ('logits', 'assign')], torch.from_numpy(case['y']).to(device)


def run_loss(case, device, weight=1.0, coeff=None):
    leaves, y = loss_tensors(case, device)
    total, terms = F().ip_loss_with_terms(*leaves, y, case['radius'], case['std'], case['alpha'], case['beta'],
                                          case['coeff'] if coeff is None else coeff)
    assert total.dim() == 0 and terms.shape == (2,) and not terms.requires_grad
    (total * weight).backward()
    got = dict(loss=np.concatenate([np_(total).reshape(1), np_(terms)]))
    for name, t in zip(T.LOSS_RESULTS[1:], leaves):
        got[name] = np_(t.grad)
    return got


def check_loss_case(case, device):
    got = run_loss(case, device)
    n, k = case['shape'][:2]
    assert np.count_nonzero(got['d_assign']) == n * k * (2 * case['radius'] + 1) ** 2
    assert np.array_equal(got['d_assign'] != 0, case['d_assign_f64'] != 0)                         # the argmax and the rank's owner
    return T.judge_loss(case, got)


def check_loss_coeff(case, device):
    """coeff 0: d_assign exactly zero and the total equal to the cross entropy; a power of two scales d_assign exactly."""
    zero, one, four = run_loss(case, device, coeff=0.0), run_loss(case, device, coeff=0.5), run_loss(case, device, coeff=2.0)
    assert not zero['d_assign'].any() and zero['loss'][0] == zero['loss'][1]
    assert zero['loss'][1:].tobytes() == one['loss'][1:].tobytes() and zero['d_logits'].tobytes() == one['d_logits'].tobytes()
    assert np.array_equal(one['d_assign'] * np.float32(4.0), four['d_assign']) and one['d_assign'].any()
    scaled = run_loss(case, device, weight=4.0, coeff=0.5)
    assert np.array_equal(one['d_assign'] * np.float32(4.0), scaled['d_assign'])
    assert np.array_equal(one['d_logits'] * np.float32(4.0), scaled['d_logits'])


def check_loss_all_equal(device, shape=(4, 3, 6, 7, 5), radius=2, std=0.4, alpha=1.0, beta=2.0):
    """Every map constant: every maximum and every rank tied at once.  The lowest flat index holds each maximum, sample n takes
    rank n; the value is the rule's, evaluated here in float64."""
    n, k, h, w, classes = shape
    rs = np.random.RandomState(77)
    case = dict(logits=rs.randn(n, classes).astype(np.float32), assign=np.full((n, k, h, w), 1.0 / k, dtype=np.float32),
                y=rs.randint(0, classes, n).astype(np.int64), radius=radius, std=std, alpha=alpha, beta=beta, coeff=0.5, shape=shape)
    got = run_loss(case, device)
    emp = float(T.blurred64(case['assign'], radius, std)[0, 0, 0, 0])
    want = np.abs(np.log(emp + T.EPS) - np.log(T.prior64(n, alpha, beta) + T.EPS)).mean()
    assert abs(got['loss'][2] - want) <= 4e-6 * want, (got['loss'], want)
    assert np.isfinite(got['d_assign']).all() and np.isfinite(got['d_logits']).all()
    d = 2 * radius + 1
    hit = got['d_assign'] != 0
    assert hit[:, :, :d, :d].all() and hit.sum() == n * k * d * d                                # the window at flat index 0
    sign = np.sign(got['d_assign'][:, 0, 0, 0])
    assert np.array_equal(sign, np.sign(np.log(emp + T.EPS) - np.log(T.prior64(n, alpha, beta) + T.EPS)))      # sample n holds rank n


def check_loss_refused(device):
    from hawkeye_amd import _lib
    HF = F()
    logits, y = torch.zeros(2, 3, device=device), torch.zeros(2, dtype=torch.int64, device=device)
    assign = torch.full((2, 2, 4, 5), 0.5, device=device)
    try:
        HF.ip_loss(logits, assign, y, radius=2)
    except _lib.HawkeyeHipError as e:
        assert 'smaller than the 5 x 5 window' in str(e)
    else:
        raise AssertionError('a 4 x 5 map has no 5 x 5 window')
    lib = _lib.load()
    outs = [torch.full(s, 7.0, device=device) for s in ((3,), (2, 3), (2, 2, 4, 5))]
    win, prior = torch.full((25,), 0.04, device=device), torch.ones(2, device=device)
    need = lib.hk_ip_loss_ws_bytes(2, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    call = lambda h, nbytes: lib.hk_ip_loss(HF.ptr(logits), HF.ptr(y), HF.ptr(assign), HF.ptr(win), HF.ptr(prior), 0.5, *[HF.ptr(o) for o in outs],
                                            2, 3, 2, h, 5, 2, HF.ptr(ws), nbytes, HF.stream())
    assert call(4, need) == _lib.HK_ERR_BAD_ARG and call(4, need - 1) == _lib.HK_ERR_BAD_ARG
    assert all((o == 7).all() for o in outs)


def check_loss_bad_labels(case, device):
    for bad in (10 ** 6 + case['shape'][4], -3):
        broken = dict(case, y=case['y'].copy())
        broken['y'][1] = bad
        leaves, y = loss_tensors(broken, device)
        total, terms = F().ip_loss_with_terms(*leaves, y, case['radius'], case['std'], case['alpha'], case['beta'], case['coeff'])
        assert torch.isnan(total) and torch.isnan(terms[0]) and torch.isfinite(terms[1])
        total.backward()
        assert all(torch.isfinite(t.grad).all() for t in leaves)                                   # the label's one-hot is read nowhere


def check_loss_reruns(case, device):
    first, again = run_loss(case, device), run_loss(case, device)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


# --------------------------------------------------------------------------------------------------------- model
def short_model(plugin, case, device):
    from inputs import seeded_init
    net = plugin.ResNet(plugin.Bottleneck, list(case['layers']), case['classes'], case['parts'])
    seeded_init(net, case['init_seed'])
    return net.to(device)


def check_model(plugin, mode, device):
    """The whole short-`layers` model against the reference's run with the same seeded weights: logits, att and assign by the
    rule, and the class of the logits."""
    case = T.load_model_case(GOLDEN)
    net = short_model(plugin, case, device).train(mode == 'train')
    with torch.no_grad():
        out = net(torch.from_numpy(case['images']).to(device))
    b, k = case['B'], case['parts']
    assert isinstance(out, tuple) and [tuple(t.shape) for t in out] == [(b, case['classes']), (b, 1, k, 1), (b, k, 4, 4)]
    worst = max(T.judge_value(f'model {mode}', name, np_(t), case[f'{mode}_{name}_f32'], case[f'{mode}_{name}_f64'])
                for name, t in zip(T.MODEL_OUTPUTS, out))
    assert np_(out[0]).argmax(1).tolist() == case[f'{mode}_logits_f64'].argmax(1).tolist()
    return worst
