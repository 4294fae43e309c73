"""The CrossX checks that the emulated tier (test_emu_crossx.py) and the GPU tier (test_gpu_crossx.py) share: each takes
the device to run on.  Indices are compared exactly; values are judged by the rule of tests/golden/crossx_inputs.py - at
most 4 x the float32 reference's own distance from the float64 result, floor 1e-6; what is exactly zero in float64 must
be exactly zero.  The multi-excitation block and the upsample + add are judged against the reference's own op sequence
in torch on the CPU (float64, with its float32 run as the yardstick), computed once per case; the loss against the
reference's goldens.  Not a test module itself."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

import crossx_inputs as T

LOSS_CASES = T.load_loss_cases()


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------- multi-excitation block
def me_reference(x, pool, dtype, use=('d_main', 'd_parts', 'd_pooled', 'dz')):
    """The reference's op sequence (CrossX.py:62-70, 109-119, 225-226) in torch on the CPU: x holds numpy arrays
    [N,C,HW]; the upstream gradients named in `use` enter, the others are zero."""
    out, res, gates = (torch.from_numpy(x[k]).to(dtype).requires_grad_(True) for k in ('out', 'res', 'gates'))
    n, c, hw = out.shape
    o4, r4 = out.view(n, c, hw, 1), res.view(n, c, hw, 1)
    main = torch.relu(o4 + r4)
    parts = [torch.relu(o4 * gates[p].view(n, c, 1, 1) + r4) for p in range(gates.shape[0])]
    if pool == 'max':
        pooled, index = zip(*[TF.adaptive_max_pool2d(part, 1, return_indices=True) for part in parts])
    else:
        pooled, index = [TF.adaptive_avg_pool2d(part, 1) for part in parts], None
    z = TF.adaptive_avg_pool2d(o4, 1).view(n, c)
    g = {k: torch.from_numpy(x[k]).to(dtype) for k in ('d_main', 'd_parts', 'd_pooled', 'dz')}
    total = out.sum() * 0
    if 'd_main' in use:
        total = total + (main.view(n, c, hw) * g['d_main']).sum()
    if 'd_parts' in use:
        total = total + sum((part.view(n, c, hw) * g['d_parts'][p]).sum() for p, part in enumerate(parts))
    if 'd_pooled' in use:
        total = total + sum((pl.view(n, c) * g['d_pooled'][p]).sum() for p, pl in enumerate(pooled))
    if 'dz' in use:
        total = total + (z * g['dz']).sum()
    total.backward()
    r = dict(main=main.view(n, c, hw), parts=torch.stack(parts).view(-1, n, c, hw), pooled=torch.stack(list(pooled)).view(-1, n, c),
             d_out=out.grad, d_res=res.grad, d_gates=gates.grad)
    r = {k: v.detach().numpy() for k, v in r.items()}
    if index is not None:
        r['argmax'] = torch.stack(list(index)).view(-1, n, c).numpy()
    return r


@functools.lru_cache(maxsize=None)
def me_case(case):
    x = T.me_inputs(case)
    return x, me_reference(x, case[4], torch.float32), me_reference(x, case[4], torch.float64)


def me_tensors(x, device):
    """[N,C,HW] arrays -> [N,C,H,W] device tensors (a square map where HW is a square, else HW x 1)."""
    n, c, hw = x['out'].shape
    h = int(round(hw ** 0.5))
    h, w = (h, h) if h * h == hw else (hw, 1)
    t = lambda a, *lead: torch.from_numpy(a).to(device).view(*lead, n, c, h, w)
    return dict(out=t(x['out']), res=t(x['res']), gates=torch.from_numpy(x['gates']).to(device), d_main=t(x['d_main']),
                d_parts=t(x['d_parts'], -1), d_pooled=torch.from_numpy(x['d_pooled']).to(device), dz=torch.from_numpy(x['dz']).to(device))


def run_me(x, pool, device, use=('d_main', 'd_parts', 'd_pooled', 'dz'), tensors=None):
    """Forward through the autograd node, backward through the raw entry point (which also takes dz)."""
    HF = F()
    t = tensors or me_tensors(x, device)
    n, c, hw = x['out'].shape
    with torch.no_grad():
        main, parts, pooled = HF.crossx_me(t['out'], t['res'], t['gates'], pool)
    assert main.shape == t['out'].shape and parts.shape == (t['gates'].shape[0], *t['out'].shape) and pooled.shape == t['gates'].shape
    argmax = None
    if pool == 'max':                                      # the positions, as the kernel stored them
        argmax = torch.empty(pooled.shape, dtype=torch.int32, device=main.device)
        scratch = [torch.empty_like(v) for v in (main, parts, pooled)]
        from hawkeye_amd import _lib
        dense = [t[k].contiguous() for k in ('out', 'res', 'gates')]               # held until the call has been enqueued
        rc = _lib.load().hk_crossx_me_fwd(*[HF.ptr(v) for v in dense], *[HF.ptr(v) for v in scratch], HF.ptr(argmax), parts.shape[0], n, c, hw, 0,
                                          HF.stream())
        assert rc == 0 and all(torch.equal(a, b) for a, b in zip(scratch, (main, parts, pooled)))
    g = {k: (t[k] if k in use else None) for k in ('d_main', 'd_parts', 'd_pooled', 'dz')}
    d_out, d_res, d_gates = HF.crossx_me_bwd(g['d_main'], g['d_parts'], g['d_pooled'], argmax, g['dz'], t['out'], t['gates'], main, parts, pool)
    r = dict(main=main.reshape(n, c, hw), parts=parts.reshape(-1, n, c, hw), pooled=pooled, d_out=d_out.reshape(n, c, hw), d_res=d_res.reshape(n, c, hw),
             d_gates=d_gates)
    r = {k: np_(v) for k, v in r.items()}
    if argmax is not None:
        r['argmax'] = np_(argmax)
    return r


def judge_me(label, got, r32, r64):
    worst = 0.0
    for name in ('main', 'parts', 'pooled', 'd_out', 'd_res', 'd_gates'):
        worst = max(worst, T.judge_value(label, name, got[name], r32[name], r64[name]))
    for name in ('main', 'parts'):                          # a ReLU's zeros are exact, element by element
        assert np.array_equal(got[name] == 0, r64[name] == 0), (label, name)
    if 'argmax' in r64:
        assert np.array_equal(got['argmax'], r64['argmax']) and np.array_equal(r32['argmax'], r64['argmax']), label
    return worst


def check_me_case(case, device):
    x, r32, r64 = me_case(tuple(case))
    return judge_me(f'me {T.me_case_id(case)}', run_me(x, case[4], device), r32, r64)


def check_me_null_gradient(missing, device, case=(2, 2, 8, 196, 'avg')):
    """One of d_main, d_parts, dz handed over as NULL: the result of the reference with that gradient left out."""
    x = me_case(tuple(case))[0]
    use = tuple(k for k in ('d_main', 'd_parts', 'd_pooled', 'dz') if k != missing)
    got = run_me(x, case[4], device, use)
    judge_me(f'me without {missing}', got, me_reference(x, case[4], torch.float32, use), me_reference(x, case[4], torch.float64, use))
    zeros = dict(x, **{missing: np.zeros_like(x[missing])})
    dense = run_me(zeros, case[4], device)
    assert all(np.array_equal(got[k], dense[k]) for k in ('d_out', 'd_res', 'd_gates')), missing      # NULL is a map of zeros


def special_rows():
    """P = 2, one sample, three channels of 12 pixels, max pooling.  Channel 0: `out` and `res` all negative.  Channel 1:
    `out` zero and the maximum of `res` twice, at 3 and at 7.  Channel 2: random."""
    rs = np.random.RandomState(71)
    x = {k: v.copy() for k, v in T.me_inputs((2, 1, 3, 12, 'max'), base_seed=7700).items() if k != 'seed'}
    x['out'][0, 0], x['res'][0, 0] = -np.abs(rs.randn(12)).astype(np.float32) - 0.1, -np.abs(rs.randn(12)).astype(np.float32) - 0.1
    x['out'][0, 1] = 0
    x['res'][0, 1] = rs.rand(12).astype(np.float32)
    x['res'][0, 1, [3, 7]] = 2.5
    return x


def check_me_special_rows(device):
    x = special_rows()
    use = ('d_main', 'd_parts', 'd_pooled')
    got = run_me(x, 'max', device, use)
    judge_me('me special rows', got, me_reference(x, 'max', torch.float32, use), me_reference(x, 'max', torch.float64, use))
    assert not got['parts'][:, 0, 0].any() and not got['main'][0, 0].any()
    assert not got['pooled'][:, 0, 0].any() and not got['argmax'][:, 0, 0].any()                   # 0 at index 0
    assert not got['d_out'][0, 0].any() and not got['d_res'][0, 0].any() and not got['d_gates'][:, 0, 0].any()
    assert got['argmax'][:, 0, 1].tolist() == [3, 3] and (got['pooled'][:, 0, 1] == 2.5).all()
    only_pool = run_me(x, 'max', device, ('d_pooled',))
    want = np.zeros(12, dtype=np.float32)
    want[3] = x['d_pooled'][0, 0, 1] + x['d_pooled'][1, 0, 1]
    assert np.array_equal(only_pool['d_res'][0, 1], want)                                          # the lower index takes it all


def check_me_autograd(device, case=(3, 1, 5, 49, 'max')):
    """The autograd node hands the raw backward what arrives and nothing else: an unused output is NULL."""
    HF = F()
    x = me_case(tuple(case))[0]
    t = me_tensors(x, device)
    leaves = [t[k].clone().requires_grad_(True) for k in ('out', 'res', 'gates')]
    main, parts, pooled = HF.crossx_me(*leaves, case[4])
    ((parts * t['d_parts']).sum() + (pooled * t['d_pooled']).sum()).backward()                     # main is not used
    want = run_me(x, case[4], device, ('d_parts', 'd_pooled'))
    n, c, hw = x['out'].shape
    assert np.array_equal(np_(leaves[0].grad).reshape(n, c, hw), want['d_out']) and np.array_equal(np_(leaves[1].grad).reshape(n, c, hw), want['d_res'])
    assert np.array_equal(np_(leaves[2].grad), want['d_gates'])


def check_me_views(device, case=(2, 2, 8, 196, 'avg')):
    """Inputs behind a base pointer that is not 16-byte aligned (the scalar path) and non-contiguous inputs give the bits
    of the dense, aligned ones - the mean's summation order does not depend on the path."""
    x = me_case(tuple(case))[0]
    dense = run_me(x, case[4], device)
    t = me_tensors(x, device)

    def offset(v):
        buf = torch.zeros(v.numel() + 5, device=v.device)
        view = buf[1:1 + v.numel()].view(v.shape)
        view.copy_(v)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    shifted = dict(t, out=offset(t['out']), res=offset(t['res']), d_main=offset(t['d_main']), d_parts=offset(t['d_parts']))
    got = run_me(x, case[4], device, tensors=shifted)
    assert all(np.array_equal(got[k], dense[k]) for k in dense), 'offset views'
    strided = dict(t, out=t['out'].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), res=torch.stack([t['res'], t['res']], -1)[..., 0],
                   gates=torch.stack([t['gates'], t['gates']], -1)[..., 1], d_parts=torch.stack([t['d_parts'], t['d_parts']], -1)[..., 0])
    assert not any(strided[k].is_contiguous() for k in ('out', 'res', 'gates', 'd_parts'))
    got = run_me(x, case[4], device, tensors=strided)
    assert all(np.array_equal(got[k], dense[k]) for k in dense), 'strided views'


# ----------------------------------------------------------------------------------------------- upsample + add
def up_reference(a, b, g, dtype):
    a, b = (torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (a, b))
    y = torch.add(a, TF.interpolate(b, a.shape[2:]))
    (y * torch.from_numpy(g).to(dtype)).sum().backward()
    return y.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def check_up_add_case(case, device):
    a, b, g = T.up_inputs(case)
    r32, r64 = up_reference(a, b, g, torch.float32), up_reference(a, b, g, torch.float64)
    ta, tb = (torch.from_numpy(v).to(device).requires_grad_(True) for v in (a, b))
    y = F().crossx_up_add(ta, tb)
    (y * torch.from_numpy(g).to(device)).sum().backward()
    assert np.array_equal(np_(y), r32[0])                                          # one addition per element: the reference's bits
    assert np.array_equal(np_(ta.grad), g)
    T.judge_value(f'up_add {case}', 'd_b', np_(tb.grad), r32[2], r64[2])
    buf = torch.zeros(ta.numel() + 5, device=device)                               # an unaligned `a`: the scalar path, the same bits
    view = buf[1:1 + ta.numel()].view(ta.shape).copy_(ta.detach())
    assert torch.equal(F().crossx_up_add(view, tb.detach()), y.detach())


def check_up_add_refused(device):
    from hawkeye_amd import _lib
    n, c, hi, wi, ho, wo = T.UP_REFUSED
    a, b = torch.zeros(n, c, ho, wo, device=device), torch.zeros(n, c, hi, wi, device=device)
    try:
        F().crossx_up_add(a, b)
    except _lib.HawkeyeHipError as e:
        assert 'multiple' in str(e)
    else:
        raise AssertionError('28 is no multiple of 5')
    y = torch.zeros_like(a)
    lib = _lib.load()
    assert lib.hk_crossx_up_add_fwd(F().ptr(a), F().ptr(b), F().ptr(y), n, c, hi, wi, ho, wo, F().stream()) == _lib.HK_ERR_UNSUPPORTED
    assert lib.hk_crossx_up_add_bwd(F().ptr(a), F().ptr(b), n, c, hi, wi, ho, wo, F().stream()) == _lib.HK_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------- loss
def loss_tensors(case, device, grad=True):
    logits = [torch.from_numpy(case[k]).to(device).requires_grad_(grad) for k in ('ulti', 'plty', 'cmbn')]
    feats = [torch.from_numpy(case[k]).to(device).requires_grad_(grad) for k in ('f_ulti', 'f_plty', 'f_cmbn')]
    return logits, feats, torch.from_numpy(case['y']).to(device)


def as_lists(feats):
    """[P,B,C] -> the model's lists of P features [B,C,1,1]"""
    return [[f[i].view(f.shape[1], f.shape[2], 1, 1) for i in range(f.shape[0])] for f in feats]


def run_loss(case, device, weight=1.0, gamma=T.GAMMA, lists=True):
    logits, feats, y = loss_tensors(case, device)
    total, terms = F().crossx_loss_with_terms(*logits, *(as_lists(feats) if lists else feats), y, gamma)
    assert total.dim() == 0 and terms.shape == (5,) and not terms.requires_grad
    (total * weight).backward()
    got = dict(loss=np.concatenate([np_(total).reshape(1), np_(terms)]))
    for name, t in zip(T.LOSS_RESULTS[1:], logits + feats):
        got[name] = np_(t.grad)
    return got


def check_loss_case(case, device):
    got = run_loss(case, device)
    worst = T.judge_loss(case, got)
    again = run_loss(case, device, lists=False)                                   # one [P,B,C] tensor per list: the same bits
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    return worst


def check_loss_scaling(case, device, weight=4.0):
    """A power-of-two loss weight scales every gradient exactly - through autograd and through the entry point's own weight."""
    from hawkeye_amd import _lib
    HF = F()
    one, four = run_loss(case, device), run_loss(case, device, weight)
    for name in T.LOSS_RESULTS[1:]:
        assert np.array_equal(one[name] * np.float32(weight), four[name]), name
    assert one['loss'].tobytes() == four['loss'].tobytes()
    logits, feats, y = loss_tensors(case, device, grad=False)
    lib = _lib.load()
    b, k = logits[0].shape
    p, cs = feats[0].shape[0], [f.shape[2] for f in feats]
    loss = torch.empty(6, device=device)
    grads = [torch.empty_like(t) for t in logits + feats]
    nws = lib.hk_crossx_loss_ws_bytes(b, k, p, *cs)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    rc = lib.hk_crossx_loss(*[HF.ptr(t) for t in logits], HF.ptr(y), *[HF.ptr(t) for t in feats], *T.GAMMA, weight, HF.ptr(loss),
                            *[HF.ptr(g) for g in grads], b, k, p, *cs, HF.ptr(ws), nws, HF.stream())
    assert rc == 0 and np_(loss).tobytes() == one['loss'].tobytes()
    for name, g in zip(T.LOSS_RESULTS[1:], grads):
        assert np.array_equal(np_(g), four[name]), name


def check_loss_zero_gamma(case, device):
    """gamma_l = 0: that term and its features' gradient are exactly zero, the others do not move."""
    full = run_loss(case, device)
    for l, name in enumerate(('df_ulti', 'df_plty', 'df_cmbn')):
        gamma = [g if i != l else 0.0 for i, g in enumerate(T.GAMMA)]
        got = run_loss(case, device, gamma=gamma)
        assert got['loss'][3 + l] == 0 and not got[name].any(), name
        for other in T.LOSS_RESULTS[1:]:
            if other != name:
                assert np.array_equal(got[other], full[other]), (name, other)
        assert np.array_equal(np.delete(got['loss'][1:], 2 + l), np.delete(full['loss'][1:], 2 + l))


def check_loss_bad_labels(case, device):
    case = dict(case, y=case['y'].copy())
    for bad in (case['K'] + 1000000, -3):
        case['y'][1] = bad
        logits, feats, y = loss_tensors(case, device)
        total, terms = F().crossx_loss_with_terms(*logits, *feats, y, T.GAMMA)
        assert torch.isnan(total) and torch.isnan(terms[0]) and torch.isfinite(terms[1:]).all()
        total.backward()
        assert all(torch.isfinite(t.grad).all() for t in logits + feats)           # the label's one-hot is read nowhere


def check_loss_refuses_one_sample(device):
    from hawkeye_amd import _lib
    HF = F()
    case = LOSS_CASES[0]
    logits, feats, y = loss_tensors(case, device, grad=False)
    try:
        HF.crossx_loss(*[t[:1] for t in logits], *[f[:, :1] for f in feats], y[:1], T.GAMMA)
    except _lib.HawkeyeHipError as e:
        assert 'at least 2' in str(e)
    else:
        raise AssertionError('B = 1 must be refused')
    lib = _lib.load()
    k, p, cs = case['K'], case['P'], list(case['widths'])
    assert lib.hk_crossx_loss_ws_bytes(1, k, p, *cs) == 0 and lib.hk_crossx_loss_ws_bytes(2, k, p, *cs) > 0
    loss = torch.zeros(6, device=device)
    grads = [torch.zeros_like(t) for t in logits + feats]
    ws = torch.zeros(4096, dtype=torch.uint8, device=device)
    rc = lib.hk_crossx_loss(*[HF.ptr(t) for t in logits], HF.ptr(y), *[HF.ptr(t) for t in feats], *T.GAMMA, 1.0, HF.ptr(loss),
                            *[HF.ptr(g) for g in grads], 1, k, p, *cs, HF.ptr(ws), 4096, HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED and not loss.any() and not any(g.any() for g in grads)


def check_loss_zero_feature_row(device):
    """A feature row of zeros has no direction: NaN, as in the reference."""
    case = dict(LOSS_CASES[0])
    case['f_plty'] = case['f_plty'].copy()
    case['f_plty'][1, 0] = 0
    got = run_loss(case, device)
    assert np.isnan(got['loss'][0]) and np.isnan(got['loss'][4]) and np.isfinite(got['loss'][[1, 2, 3, 5]]).all()


def check_loss_reruns(case, device):
    first, again = run_loss(case, device), run_loss(case, device)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)

