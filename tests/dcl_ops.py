"""The DCL checks that the emulated tier (test_emu_dcl.py) and the GPU tier (test_gpu_dcl.py) share: each takes the device
to run on.  Indices are compared exactly; values are judged by the project's rule (tests/golden/crossx_inputs.py:
judge_value) - at most 4 x the float32 reference's own distance from the float64 result, floor 1e-6; what is exactly
zero in float64 must be exactly zero.  The head is judged against the reference's own op sequence in torch on the CPU
(Conv2d 1 x 1, AvgPool2d(2), tanh, view, AdaptiveAvgPool2d(1); float64, with its float32 run as the yardstick), computed
once per case; the loss and the swap law against the reference's goldens.  Not a test module itself."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

import dcl_inputs as T

GOLDEN = T.load()
LOSS_CASES = T.load_loss_cases(GOLDEN)
GRADS = ('d_pooled', 'd_mask')


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- head
def head_reference(x, dtype, use=GRADS):
    """The reference's op sequence (DCL.py:33-39) in torch on the CPU, forward and backward; the upstream gradients named
    in `use` enter, the others are zero."""
    xt, w, bias = (torch.from_numpy(x[k]).to(dtype).requires_grad_(True) for k in ('x', 'w', 'bias'))
    b, c = xt.shape[:2]
    mask = torch.tanh(TF.avg_pool2d(TF.conv2d(xt, w.view(1, c, 1, 1), bias), 2, stride=2))
    mask = mask.view(mask.size(0), -1)
    pooled = TF.adaptive_avg_pool2d(xt, 1).view(b, -1)
    total = xt.sum() * 0 + w.sum() * 0 + bias.sum() * 0
    if 'd_pooled' in use:
        total = total + (pooled * torch.from_numpy(x['d_pooled']).to(dtype)).sum()
    if 'd_mask' in use:
        total = total + (mask * torch.from_numpy(x['d_mask']).to(dtype)).sum()
    total.backward()
    return {k: v.detach().numpy() for k, v in dict(pooled=pooled, mask=mask, dx=xt.grad, dw=w.grad, dbias=bias.grad).items()}


@functools.lru_cache(maxsize=None)
def head_case(case):
    x = T.head_inputs(case)
    return x, head_reference(x, torch.float32), head_reference(x, torch.float64)


def head_tensors(x, device):
    return {k: torch.from_numpy(v).to(device) for k, v in x.items()}


def run_head(x, device, use=GRADS, tensors=None):
    """Forward through the autograd node, backward through the raw entry point."""
    HF = F()
    t = tensors or head_tensors(x, device)
    b, c, h, w = x['x'].shape
    with torch.no_grad():
        pooled, mask = HF.dcl_head(t['x'], t['w'], t['bias'])
    assert pooled.shape == (b, c) and mask.shape == (b, (h // 2) * (w // 2))
    dx, dw, dbias = HF.dcl_head_bwd(t['x'], t['w'], mask, *[t[k] if k in use else None for k in GRADS])
    assert dx.shape == t['x'].shape and dw.shape == (c,) and dbias.shape == (1,)
    return {k: np_(v) for k, v in dict(pooled=pooled, mask=mask, dx=dx, dw=dw, dbias=dbias).items()}


def judge_head(label, got, r32, r64):
    return max(T.judge_value(label, name, got[name], r32[name], r64[name]) for name in ('pooled', 'mask', 'dx', 'dw', 'dbias'))


def check_head_case(case, device):
    x, r32, r64 = head_case(tuple(case))
    got = run_head(x, device)
    b, c, h, w = case
    if h % 2 or w % 2:                                     # outside the pooled area only the mean's gradient arrives
        edge = np.ones((h, w), dtype=bool)
        edge[:h - h % 2, :w - w % 2] = False
        want = np.broadcast_to((x['d_pooled'] / np.float32(h * w))[:, :, None], (b, c, int(edge.sum())))
        assert np.array_equal(got['dx'][:, :, edge], want)
    return judge_head(f'head {T.head_case_id(case)}', got, r32, r64)


def check_head_null_gradient(missing, device, case=(2, 70, 7, 7)):
    """One of d_pooled, d_mask missing: through the raw call, and through autograd with that output unused."""
    HF = F()
    x = head_case(tuple(case))[0]
    use = tuple(k for k in GRADS if k != missing)
    got = run_head(x, device, use)
    judge_head(f'head without {missing}', got, head_reference(x, torch.float32, use), head_reference(x, torch.float64, use))
    dense = run_head(dict(x, **{missing: np.zeros_like(x[missing])}), device)
    assert all(np.array_equal(got[k], dense[k]) for k in ('dx', 'dw', 'dbias')), missing             # NULL is a tensor of zeros
    if missing == 'd_mask':
        assert not got['dw'].any() and not got['dbias'].any()
    t = head_tensors(x, device)
    leaves = [t[k].clone().requires_grad_(True) for k in ('x', 'w', 'bias')]
    leaves[1] = leaves[1].detach().view(1, -1, 1, 1).requires_grad_(True)                           # Convmask's own shapes
    pooled, mask = HF.dcl_head(*leaves)
    kept = dict(d_pooled=pooled, d_mask=mask)[use[0]]
    (kept * t[use[0]]).sum().backward()
    assert np.array_equal(np_(leaves[0].grad), got['dx']) and np.array_equal(np_(leaves[1].grad).reshape(-1), got['dw'])
    assert leaves[1].grad.shape == leaves[1].shape and np.array_equal(np_(leaves[2].grad), got['dbias'])


def check_head_zero_d_mask(device, case=(3, 5, 5, 6)):
    """A d_mask of zeros (not NULL): dw and dbias exactly zero, dx the mean's gradient alone."""
    x = head_case(tuple(case))[0]
    got = run_head(dict(x, d_mask=np.zeros_like(x['d_mask'])), device)
    assert not got['dw'].any() and not got['dbias'].any()
    b, c, h, w = case
    assert np.array_equal(got['dx'], np.broadcast_to((x['d_pooled'] / np.float32(h * w))[:, :, None, None], got['dx'].shape))


def check_head_views(device, case=(2, 130, 4, 4)):
    """A map behind a base pointer that is not 16-byte aligned (the scalar path) and a non-contiguous map give the bits of
    the dense, aligned one."""
    x = head_case(tuple(case))[0]
    dense = run_head(x, device)
    t = head_tensors(x, device)
    buf = torch.zeros(t['x'].numel() + 5, device=device)
    view = buf[1:1 + t['x'].numel()].view(t['x'].shape)
    view.copy_(t['x'])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got = run_head(x, device, tensors=dict(t, x=view))
    assert all(np.array_equal(got[k], dense[k]) for k in dense), 'offset view'
    strided = dict(t, x=torch.stack([t['x'], t['x']], -1)[..., 0], w=torch.stack([t['w'], t['w']], -1)[..., 1],
                   d_mask=torch.stack([t['d_mask'], t['d_mask']], -1)[..., 0])
    assert not any(strided[k].is_contiguous() for k in ('x', 'w', 'd_mask'))
    got = run_head(x, device, tensors=strided)
    assert all(np.array_equal(got[k], dense[k]) for k in dense), 'strided views'


def check_head_reruns(device, case=(2, 2048, 14, 14)):
    x = head_case(tuple(case))[0]
    a, b = run_head(x, device), run_head(x, device)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def check_head_refused(device):
    """H = 1: the reference's pool has no output there."""
    from hawkeye_amd import _lib
    HF = F()
    x, w, bias = torch.zeros(1, 3, 1, 4, device=device), torch.zeros(3, device=device), torch.zeros(1, device=device)
    try:
        HF.dcl_head(x, w, bias)
    except _lib.HawkeyeHipError as e:
        assert '2 x 2' in str(e)
    else:
        raise AssertionError('H = 1 must be refused')
    lib = _lib.load()
    pooled, mask, ws = torch.zeros(1, 3, device=device), torch.zeros(1, 4, device=device), torch.zeros(4096, dtype=torch.uint8, device=device)
    assert lib.hk_dcl_head_fwd_ws_bytes(1, 3, 1, 4) == 0 and lib.hk_dcl_head_bwd_ws_bytes(1, 3, 4, 1) == 0
    rc = lib.hk_dcl_head_fwd(HF.ptr(x), HF.ptr(w), HF.ptr(bias), HF.ptr(pooled), HF.ptr(mask), 1, 3, 1, 4, HF.ptr(ws), 4096, HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED
    rc = lib.hk_dcl_head_bwd(HF.ptr(x), HF.ptr(w), HF.ptr(mask), None, None, HF.ptr(torch.zeros_like(x)), None, None, 1, 3, 4, 1, HF.ptr(ws),
                             4096, HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------- loss
def loss_tensors(case, device, grad=True):
    leaves = [torch.from_numpy(case[k]).to(device).requires_grad_(grad) for k in ('logits', 'swap', 'mask')]
    return leaves, [torch.from_numpy(case[k]).to(device) for k in ('y', 'ys', 'law')]


def run_loss(case, device, weight=1.0, coef=T.COEF):
    leaves, rest = loss_tensors(case, device)
    total, terms = F().dcl_loss_with_terms(*leaves, *rest, *coef, T.SMOOTHING)
    assert total.dim() == 0 and terms.shape == (3,) and not terms.requires_grad
    (total * weight).backward()
    got = dict(loss=np.concatenate([np_(total).reshape(1), np_(terms)]))
    for name, t in zip(T.LOSS_RESULTS[1:], leaves):
        got[name] = np_(t.grad)
    return got


def check_loss_case(case, device):
    got = run_loss(case, device)
    if case['k'] == T.TIE_CASE:
        for b, e in T.TIES:
            assert case['mask'][b, e] == case['law'][b, e] and got['d_mask'][b, e] == 0                 # exactly zero, as torch's sign(0)
        assert np.count_nonzero(got['d_mask'] == 0) == len(T.TIES)
    return T.judge_loss(case, got)


def check_loss_scaling(case, device, weight=4.0):
    """A power-of-two loss weight scales every gradient exactly - through autograd and through the entry point's own weight."""
    from hawkeye_amd import _lib
    HF = F()
    one, four = run_loss(case, device), run_loss(case, device, weight)
    for name in T.LOSS_RESULTS[1:]:
        assert np.array_equal(one[name] * np.float32(weight), four[name]), name
    assert one['loss'].tobytes() == four['loss'].tobytes()
    leaves, rest = loss_tensors(case, device, grad=False)
    loss = torch.empty(4, device=device)
    grads = [torch.empty_like(t) for t in leaves]
    rc = _lib.load().hk_dcl_loss(*[HF.ptr(t) for t in leaves], *[HF.ptr(t) for t in rest], *T.COEF, T.SMOOTHING, weight, HF.ptr(loss),
                                 *[HF.ptr(g) for g in grads], case['N'], case['K'], case['S'], case['M'], HF.stream())
    assert rc == 0 and np_(loss).tobytes() == one['loss'].tobytes()
    for name, g in zip(T.LOSS_RESULTS[1:], grads):
        assert np.array_equal(np_(g), four[name]), name


def check_loss_zero_coefficients(case, device):
    """alpha = beta = gamma = 0: the total and the three gradients are exactly zero; the terms do not move."""
    full, got = run_loss(case, device), run_loss(case, device, coef=(0.0, 0.0, 0.0))
    assert got['loss'][0] == 0 and np.array_equal(got['loss'][1:], full['loss'][1:])
    for name in T.LOSS_RESULTS[1:]:
        assert not got[name].any(), name


def check_loss_bad_labels(case, device):
    for which, term in (('y', 0), ('ys', 1)):
        for bad in (10 ** 6 + case['K'] + case['S'], -3):
            broken = dict(case, **{which: case[which].copy()})
            broken[which][1] = bad
            leaves, rest = loss_tensors(broken, device)
            total, terms = F().dcl_loss_with_terms(*leaves, *rest, *T.COEF, T.SMOOTHING)
            other = [i for i in range(3) if i != term]
            assert torch.isnan(total) and torch.isnan(terms[term]) and torch.isfinite(terms[other]).all()
            total.backward()
            assert all(torch.isfinite(t.grad).all() for t in leaves)                                # the label's one-hot is read nowhere


def check_loss_reruns(case, device):
    first, again = run_loss(case, device), run_loss(case, device)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


# ------------------------------------------------------------------------------------------------------ swap law
def run_law(unswap, swapped, device, grid=T.LAW_GRID):
    law, index = F().dcl_swap_law(torch.from_numpy(unswap)[None].to(device), torch.from_numpy(swapped)[None].to(device), grid)
    parts = grid[0] * grid[1]
    assert law.shape == index.shape == (1, parts) and law.dtype == torch.float32 and index.dtype == torch.int32
    index, law = np_(index)[0], np_(law)[0]
    assert law.tobytes() == T.law_values(index, parts).tobytes()                                    # divided in float64, then rounded
    return index, law


def check_law_case(name, device):
    unswap, swapped = T.LAW_CASES[name]()
    index, law = run_law(unswap, swapped, device)
    want = GOLDEN[f'law_{name}_index']
    assert np.array_equal(index, want), (name, np.nonzero(index != want)[0].tolist())
    if name == 'permutation':
        assert np.array_equal(index, T.law_permutation_case()[2])
    if name == 'constant':
        assert not index.any() and (law == np.float32(-24 / 49)).all()
    if name == 'equal_total':
        assert index[12] == 30


def check_law_batch(device):
    """Several images in one call: each image's law is that of the image alone."""
    pairs = [T.LAW_CASES[name]() for name in ('permutation', 'permutation', 'constant')]
    pairs[1] = (pairs[1][1], pairs[1][0])                                                           # the inverse permutation
    pairs[2] = tuple(np.ascontiguousarray(v[:14, :14]) for v in pairs[2])
    un, sw = (torch.from_numpy(np.stack([p[k] for p in pairs])).to(device) for k in (0, 1))
    law, index = F().dcl_swap_law(un, sw, T.LAW_GRID)
    perm = T.law_permutation_case()[2]
    assert np.array_equal(np_(index)[0], perm) and np.array_equal(np_(index)[1], np.argsort(perm)) and not np_(index)[2].any()


def check_law_refused(device):
    from hawkeye_amd import _lib
    HF = F()
    tiny = torch.zeros(1, 3, 3, 3, dtype=torch.uint8, device=device)
    try:
        HF.dcl_swap_law(tiny, tiny, (7, 7))
    except _lib.HawkeyeHipError as e:
        assert 'empty' in str(e)
    else:
        raise AssertionError('a 3 x 3 image has no 7 x 7 patches')
    bounds = torch.zeros(8, dtype=torch.int32, device=device)
    index, law = torch.zeros(1, 49, dtype=torch.int32, device=device), torch.zeros(1, 49, device=device)
    rc = _lib.load().hk_dcl_swap_law(HF.ptr(tiny), HF.ptr(tiny), HF.ptr(bounds), HF.ptr(bounds), HF.ptr(index), HF.ptr(law), 1, 3, 3, 7, 7,
                                     HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED
