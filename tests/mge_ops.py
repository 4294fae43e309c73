"""The MGE-CNN checks that the emulated tier (test_emu_mge.py) and the GPU tier (test_gpu_mge.py) share: each takes the device to
run on.  Inputs, seeds, preconditions and the float64 references: tests/mge_inputs.py.  Not a test module.

Bounds.
  part pool forward   |pooled - pooled64| <= (Cin + 8) 2^-24 (|b| + sum_c |w x|) at the pixel the kernel names (the border: |b| alone):
                      the worst case of any fp32 summation order of Cin products, plus the bias addition.  The kernel's argmax is
                      valid when the float64 response there is within that bound of the float64 maximum; -1 when the float64
                      maximum is within its own bound of the border's 0.
  part pool backward  |dW - dW64| <= B 2^-23 sum_b |g x| per element (B products and B - 1 additions of fp32, each 2^-24 relative,
                      bounded by B 2^-23 times the sum of the terms' magnitudes), db likewise against sum_b |g|.
  CAM box             exact integers, under the asserted precondition of mge_inputs.cam_float64.
  loss, crop, model   the project's rule (tests/golden/nts_inputs.py: judge_value): at most 4 x the float32 reference's own distance
                      from the float64 result, floor 1e-6."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as TF

import mge_inputs as T
from nts_inputs import judge_value

EPS24, EPS23 = T.EPS24, T.EPS23


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


def dev_(a, device, *names):
    return [torch.from_numpy(np.ascontiguousarray(a[n])).to(device) for n in names]


# ------------------------------------------------------------------------------------------------------- part pool
def judge_pool_forward(a, r, pooled, argmax):
    """-> the worst |error| / bound."""
    b, cin = a['x'].shape[:2]
    pooled, argmax = pooled.astype(np.float64), argmax.astype(np.int64)
    assert ((argmax >= -1) & (argmax < r['resp'].shape[2])).all()
    at = np.take_along_axis(r['bound'], np.maximum(argmax, 0)[..., None], 2)[..., 0]
    bound = np.where(argmax >= 0, at, r['border_bound'])
    err = np.abs(pooled - r['pooled'])
    print(f'pooled: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
    assert (err <= bound).all(), float(np.max(err / np.maximum(bound, 1e-300)))
    resp_at = np.take_along_axis(r['resp'], np.maximum(argmax, 0)[..., None], 2)[..., 0]
    top_bound = np.take_along_axis(r['bound'], r['best'][..., None], 2)[..., 0]
    inside = argmax >= 0
    assert (np.where(inside, np.maximum(r['top'], 0.0) - resp_at <= at, r['top'] <= top_bound)).all()
    return float(np.max(err / np.maximum(bound, 1e-300)))


def run_pool(a, device):
    x, wt, bias, g = dev_(a, device, 'x', 'weight', 'bias', 'g')
    pooled, argmax = F().mge_partpool_fwd(x, wt, bias)
    dw, db = F().mge_partpool_bwd(x, g, pooled, argmax)
    return np_(pooled), np_(argmax), np_(dw), np_(db)


def judge_pool_backward(a, dw, db, pooled, argmax):
    b = a['x'].shape[0]
    dw64, db64, dw_abs, db_abs = T.pool_gather64(a, pooled, argmax)
    ew, eb = np.abs(dw - dw64), np.abs(db - db64)
    assert (ew <= b * EPS23 * dw_abs).all() and (eb <= b * EPS23 * db_abs).all()
    assert not dw[dw_abs == 0].any() and not db[db_abs == 0].any()
    return dw64, db64, dw_abs, db_abs


def check_pool_case(case, device):
    a, r = T.pool_case(tuple(case))
    assert T.pool_margin(a, r) > 0, 'precondition: a seed whose every decision is wider than the forward bound'
    pooled, argmax, dw, db = run_pool(a, device)
    worst = judge_pool_forward(a, r, pooled, argmax)
    assert np.array_equal(argmax, r['argmax'])             # (follows from the precondition)
    judge_pool_backward(a, dw, db, pooled.astype(np.float64), argmax)
    # ... and against autograd of the reference's op sequence in float64 (the same decisions, by the precondition)
    pooled_ref, dw_ref, db_ref = T.pool_reference_grads(a)
    assert np.allclose(pooled_ref, r['pooled'], rtol=1e-12, atol=1e-12)
    _, _, dw_abs, db_abs = T.pool_gather64(a, r['pooled'], r['argmax'])
    b = a['x'].shape[0]
    assert (np.abs(dw - dw_ref) <= b * EPS23 * dw_abs).all() and (np.abs(db - db_ref) <= b * EPS23 * db_abs).all()
    # the autograd node gives the raw calls' bits
    x, wt, bias, g = dev_(a, device, 'x', 'weight', 'bias', 'g')
    wt4, bias = wt.view(*wt.shape, 1, 1).requires_grad_(True), bias.requires_grad_(True)
    out = F().mge_partpool(x.requires_grad_(True), wt4, bias)
    out.backward(g)
    assert x.grad is None and wt4.grad.shape == wt4.shape
    assert np.array_equal(np_(out), pooled) and np.array_equal(np_(wt4.grad).reshape(dw.shape), dw) and np.array_equal(np_(bias.grad), db)
    return worst


def directed_pool(device, kind):
    rs = np.random.RandomState(7)
    b, cin, cout, h, w = 2, 32, 70, 3, 5
    x = np.abs(rs.randn(b, cin, h, w)).astype(np.float32) + 0.1
    wt = -np.abs(rs.randn(cout, cin)).astype(np.float32) - 0.1             # every interior response negative
    bias = (np.abs(rs.randn(cout)) + 0.1).astype(np.float32)
    g = rs.randn(b, cout).astype(np.float32)
    if kind == 'all_negative':
        bias = -bias
    if kind == 'zero_image':
        wt = rs.randn(cout, cin).astype(np.float32)
        x[1] = 0.0
        bias[::2] *= -1
    a = dict(x=x, weight=wt, bias=bias, g=g)
    pooled, argmax, dw, db = run_pool(a, device)
    if kind == 'border_wins':
        assert (argmax == -1).all() and np.array_equal(pooled, np.broadcast_to(bias, pooled.shape))
        assert not dw.any() and np.array_equal(db, (g[0] + g[1]).astype(np.float32))
    elif kind == 'all_negative':
        assert (argmax == -1).all() and not pooled.any() and not dw.any() and not db.any()
    else:
        assert (argmax[1] == -1).all() and np.array_equal(pooled[1], np.maximum(bias, 0))          # responses exactly 0: the border
        r = T.pool_float64(a)
        judge_pool_forward(a, r, pooled, argmax)
        judge_pool_backward(a, dw, db, pooled.astype(np.float64), argmax)


def check_pool_null_outputs(device):
    """A NULL dW and a NULL db: raw and through autograd; the other output keeps its bits."""
    a, _ = T.pool_case(T.POOL_CASES[1])
    x, wt, bias, g = dev_(a, device, 'x', 'weight', 'bias', 'g')
    pooled, argmax = F().mge_partpool_fwd(x, wt, bias)
    dw, db = F().mge_partpool_bwd(x, g, pooled, argmax)
    only_w, none_b = F().mge_partpool_bwd(x, g, pooled, argmax, need=(True, False))
    none_w, only_b = F().mge_partpool_bwd(x, g, pooled, argmax, need=(False, True))
    assert none_b is None and none_w is None and torch.equal(only_w, dw) and torch.equal(only_b, db)
    assert F().mge_partpool_bwd(x, g, pooled, argmax, need=(False, False)) == (None, None)
    for need_w, need_b in ((True, False), (False, True)):
        w_leaf, b_leaf = wt.clone().requires_grad_(need_w), bias.clone().requires_grad_(need_b)
        F().mge_partpool(x, w_leaf, b_leaf).backward(g)
        assert (w_leaf.grad is None) != need_w and (b_leaf.grad is None) != need_b
        assert torch.equal(w_leaf.grad, dw) if need_w else torch.equal(b_leaf.grad, db)


def check_pool_views(device):
    """A strided map and an offset weight give the bits of their dense copies."""
    a, _ = T.pool_case(T.POOL_CASES[1])
    x, wt, bias, g = dev_(a, device, 'x', 'weight', 'bias', 'g')
    want = F().mge_partpool_fwd(x, wt, bias)
    xs = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    buf = torch.zeros(wt.numel() + 3, device=device)
    buf[3:] = wt.reshape(-1)
    ws = buf[3:].view_as(wt)                               # dense, but not 16-byte aligned
    assert not xs.is_contiguous() and ws.data_ptr() % 16 != 0
    for got in (F().mge_partpool_fwd(xs, wt, bias), F().mge_partpool_fwd(x, ws, bias)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    dw = F().mge_partpool_bwd(x, g, *want)
    dws = F().mge_partpool_bwd(xs, g.t().contiguous().t(), *want)
    assert torch.equal(dw[0], dws[0]) and torch.equal(dw[1], dws[1])
    again = F().mge_partpool_fwd(x, wt, bias)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])                       # two runs, one result


def check_pool_refused_and_workspace(device):
    from hawkeye_amd import _lib
    lib = _lib.load()
    HF = F()
    with np.testing.assert_raises(_lib.HawkeyeHipError):
        HF.mge_partpool(torch.zeros(1, 48, 3, 3, device=device), torch.zeros(5, 48, device=device), torch.zeros(5, device=device))
    assert lib.hk_mge_partpool_fwd_ws_bytes(1, 48, 5, 3, 3) == 0 and lib.hk_mge_partpool_fwd_ws_bytes(0, 32, 5, 3, 3) == 0
    b, cin, cout, h, w = 3, 96, 80, 9, 9
    a, _ = T.pool_case((b, cin, cout, h, w))
    x, wt, bias = dev_(a, device, 'x', 'weight', 'bias')
    need = lib.hk_mge_partpool_fwd_ws_bytes(b, cin, cout, h, w)
    assert need == b * cout * 2 * 8                        # 81 pixels: two column tiles, a float and an int each
    pooled, argmax = torch.zeros(b, cout, device=device), torch.zeros(b, cout, dtype=torch.int32, device=device)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    p, st = HF.ptr, HF.stream

    def call(cin_=cin, nbytes=need, first=None):
        return lib.hk_mge_partpool_fwd(p(x) if first is None else first, p(wt), p(bias), p(pooled), p(argmax), b, cin_, cout, h, w, p(ws), nbytes, st())
    assert call(cin_=48) == _lib.HK_ERR_BAD_ARG and call(first=ctypes.c_void_p(0)) == _lib.HK_ERR_BAD_ARG
    assert call(nbytes=need - 1) == _lib.HK_ERR_WORKSPACE
    assert not pooled.any() and not argmax.any()           # nothing launched
    assert call() == _lib.HK_OK
    want = HF.mge_partpool_fwd(x, wt, bias)
    assert torch.equal(pooled, want[0]) and torch.equal(argmax, want[1])
    g = torch.ones(b, cout, device=device)
    assert lib.hk_mge_partpool_bwd(p(x), p(g), p(pooled), p(argmax), None, None, b, 48, cout, h, w, st()) == _lib.HK_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------------- CAM box
def run_cam(a, rate, s, device):
    conv5, wt, index = dev_(a, device, 'conv5', 'cls_weight', 'index')
    boxes = F().mge_cam_bbox(conv5, wt, index, rate, s)
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (conv5.shape[0], 1, 4)
    return np_(boxes)


def check_cam_case(case, rate, device):
    a, boxes64, closest = T.cam_case(tuple(case), rate)
    assert closest >= 1.0, 'precondition: every row and column maximum at least the margin away from the rate'
    got = run_cam(a, rate, case[4], device)
    assert np.array_equal(got, boxes64), (got.tolist(), boxes64.tolist())
    assert not (boxes64.reshape(-1, 4) == np.array([0, 0, case[4], case[4]])).all()                # not only whole images
    conv5, wt, index = dev_(a, device, 'conv5', 'cls_weight', 'index')
    again = F().mge_cam_bbox(conv5.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), wt, index.long(), rate, case[4])
    assert np.array_equal(np_(again), got)


def directed_cam(device, kind):
    c, h, w, s, rate = 6, 4, 4, 64, 0.3
    conv5 = np.zeros((1, c, h, w), dtype=np.float32)
    wt = np.ones((2, c), dtype=np.float32)
    if kind == 'constant':
        conv5[:] = 0.7
        want = [0, 0, s, s]
    elif kind == 'single_maximum':                         # only the sampled peak reaches the rate: x1 == x2, the reference's fall-back
        conv5[0, :, 1, 2] = 1.0
        s, rate = 4, 0.99                                  # S = h: the map itself, one pixel at 1.0
        want = [0, 0, s, s]
    elif kind == 'hot_corner':
        conv5[0, :, 3, 3] = 1.0
        a = dict(conv5=conv5, cls_weight=wt, index=np.array([1], dtype=np.int32))
        want = T.cam_float64(a, rate, s)[0].reshape(4).tolist()
        assert want[2] == s - 1 and want[3] == s - 1 and 0 < want[0] < s - 1              # touches the last row; the exclusive end drops it
    elif kind == 'hot_first_corner':
        conv5[0, :, 0, 0] = 1.0
        a = dict(conv5=conv5, cls_weight=wt, index=np.array([1], dtype=np.int32))
        want = T.cam_float64(a, rate, s)[0].reshape(4).tolist()
        assert want[0] == 0 and want[1] == 0 and 0 < want[2] < s - 1
    elif kind == 'index_out_of_range':
        conv5[0, :, 1, 1] = 1.0
        want = [0, 0, s, s]
    index = np.array([7 if kind == 'index_out_of_range' else 1], dtype=np.int32)
    got = run_cam(dict(conv5=conv5, cls_weight=wt, index=index), rate, s, device)
    assert got.reshape(4).tolist() == want, (kind, got.tolist(), want)


def check_cam_crop(device):
    """The box through nts_crop_resize against F.interpolate(x[k,:,y1:y2,x1:x2], align_corners=True)."""
    case, rate = T.CAM_CASES[1], 0.3
    a, boxes64, _ = T.cam_case(case, rate)
    b, s = case[0], case[4]
    images = np.random.RandomState(5).randn(b, 3, s, s).astype(np.float32)
    boxes = F().mge_cam_bbox(*dev_(a, device, 'conv5', 'cls_weight', 'index'), rate, s)
    got = F().nts_crop_resize(torch.from_numpy(images).to(device), boxes, 0, s)
    refs = []
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(images).to(dtype)
        refs.append(torch.cat([TF.interpolate(x[k:k + 1, :, y1:y2, x1:x2], size=(s, s), mode='bilinear', align_corners=True)
                               for k, (y1, x1, y2, x2) in enumerate(boxes64.reshape(b, 4).tolist())]).numpy())
    return judge_value('mge crop', 'out', np_(got), refs[0], refs[1])


def check_cam_refused(device):
    from hawkeye_amd import _lib
    with np.testing.assert_raises(_lib.HawkeyeHipError):
        F().mge_cam_bbox(torch.zeros(1, 4, 23, 23, device=device), torch.zeros(2, 4, device=device), torch.zeros(1, dtype=torch.int64, device=device), 0.2, 64)
    lib = _lib.load()
    p = F().ptr
    x, wt, idx = torch.zeros(1, 4, 23, 23, device=device), torch.zeros(2, 4, device=device), torch.zeros(1, dtype=torch.int32, device=device)
    out = torch.zeros(1, 1, 4, dtype=torch.int32, device=device)
    assert lib.hk_mge_cam_bbox(p(x), p(wt), p(idx), p(out), 1, 4, 23, 23, 2, 0.2, 64, F().stream()) == _lib.HK_ERR_UNSUPPORTED
    assert lib.hk_mge_cam_bbox(p(x), p(wt), p(idx), p(out), 1, 4, 2, 2, 2, 0.2, 4096, F().stream()) == _lib.HK_ERR_UNSUPPORTED
    assert lib.hk_mge_cam_bbox(None, p(wt), p(idx), p(out), 1, 4, 2, 2, 2, 0.2, 64, F().stream()) == _lib.HK_ERR_BAD_ARG
    assert not out.any()


def check_cam_closed_form():
    """relu(W[idx]) / (h w) against the reference's own GradCam output (its autograd path), both calls, y given and y=None."""
    g = T.load('mge_ops.npz')
    n = 0
    for key in g.files:
        if not key.endswith('_weights'):
            continue
        stem = key[:-len('_weights')]
        want, index, hw = g[key], g[stem + '_index'], int(g[stem + '_hw'])
        got = np_(F().mge_cam_weights(torch.from_numpy(g['cam_cls_weight']), torch.from_numpy(index), hw))
        assert want.any() and np.all(np.abs(got - want) <= 4 * EPS24 * np.abs(want)), stem
        n += 1
    assert n == 4                                          # {first, second call} x {y given, y=None}


# ------------------------------------------------------------------------------------------------------- loss
def run_loss(logits, labels, device):
    leaves = [torch.from_numpy(v).to(device).requires_grad_(True) for v in logits]
    total, terms = F().mge_loss_with_terms(leaves, torch.from_numpy(labels).to(device), T.SMOOTHING)
    total.backward()
    return dict(loss=np.concatenate([np_(total).reshape(1), np_(terms)]), grads=[np_(t.grad) for t in leaves])


def judge_loss(label, got, r32, r64):
    worst = 0.0
    for i in range(len(r64['loss'])):
        worst = max(worst, judge_value(label, f'loss[{i}]', got['loss'][i], r32['loss'][i], r64['loss'][i]))
    for i, (g, a, b) in enumerate(zip(got['grads'], r32['grads'], r64['grads'])):
        worst = max(worst, judge_value(label, f'd_logits[{i}]', g, a, b))
    return worst


def check_loss_case(case, device):
    logits, labels = T.loss_arrays(case)
    got = run_loss(logits, labels, device)
    r32, r64 = (T.loss_reference(logits, labels, dt) for dt in (torch.float32, torch.float64))
    worst = judge_loss(f'mge loss {T.loss_case_id(case)}', got, r32, r64)
    k = case[0]
    # each row of a cross entropy's gradient sums to zero: w (sum p - smoothing - (1 - smoothing)) with w = 1 / (B K).  In fp32 the
    # three terms have magnitudes sum p = 1, smoothing and 1 - smoothing, 2 in all; sum p carries the C roundings of the sum of the
    # exponentials and every element a handful more (expf, the product with 1 / sum, two subtractions, the weight): (C + 16) 2^-24 each
    for g in got['grads']:
        assert np.all(np.abs(g.astype(np.float64).sum(1)) <= (g.shape[1] + 16) * EPS24 * 2.0 / (case[0] * case[1]))
    assert abs(float(np.mean(got['loss'][1:].astype(np.float64))) - float(got['loss'][0])) <= (k + 1) * EPS24 * abs(float(got['loss'][0]))
    if tuple(case) in T.LOSS_GOLDEN_CASES:                 # the reference trainer's ten-criterion sum, as stored
        gold = T.load('mge_ops.npz')
        stem = 'loss_' + T.loss_case_id(case)
        r32 = dict(loss=gold[stem + '_loss_f32'], grads=list(gold[stem + '_grads_f32']))
        r64 = dict(loss=gold[stem + '_loss_f64'], grads=list(gold[stem + '_grads_f64']))
        worst = max(worst, judge_loss(f'mge golden loss {T.loss_case_id(case)}', got, r32, r64))
    return worst


def check_loss_refused(device):
    from hawkeye_amd import _lib
    logits = [torch.zeros(2, 3, device=device) for _ in range(17)]
    y = torch.zeros(2, dtype=torch.int64, device=device)
    with np.testing.assert_raises(_lib.HawkeyeHipError):
        F().mge_loss(logits, y)
    lib = _lib.load()
    table = (ctypes.c_void_p * 17)(*[F().ptr(t).value for t in logits])
    out, y32 = torch.zeros(18, device=device), y.int()
    assert lib.hk_mge_loss_ws_bytes(17, 2) == 0 and lib.hk_mge_loss_ws_bytes(16, 2) == 16 * 2 * 4
    ws = torch.zeros(1024, dtype=torch.uint8, device=device)
    p = F().ptr
    assert lib.hk_mge_loss(table, p(y32), 0.1, p(out), table, 17, 2, 3, p(ws), 1024, F().stream()) == _lib.HK_ERR_BAD_ARG
    assert lib.hk_mge_loss(table, p(y32), 0.1, p(out), table, 16, 2, 3, p(ws), 127, F().stream()) == _lib.HK_ERR_WORKSPACE
    assert not out.any()
    got = F().mge_loss_with_terms([t[:, :3] for t in [torch.randn(2, 5, device=device)] * 2], y)   # strided views are served
    assert torch.isfinite(got[0]).item() and got[1][0] == got[1][1]


# ------------------------------------------------------------------------------------------------------- model
def short_trunk(plugin_or_backbone):
    from hawkeye_amd.model.backbone import ResNet, Bottleneck
    return lambda pretrained=False, **kw: ResNet(Bottleneck, list(T.MODEL_CASE['layers']))


def short_model(plugin, device, monkeypatch):
    from hawkeye_amd.config import CfgNode
    from inputs import seeded_init
    c = T.MODEL_CASE
    monkeypatch.setattr(plugin, 'resnet50', short_trunk(plugin))
    net = plugin.MGE_CNN(CfgNode(dict(num_classes=c['classes'], box_thred=c['box_thred'], image_size=c['size'])))
    seeded_init(net, c['init_seed'])
    return net.to(device)


def check_model_eval(plugin, device, monkeypatch):
    g = T.load('mge_model.npz')
    c = T.MODEL_CASE
    net = short_model(plugin, device, monkeypatch).eval()
    images = torch.from_numpy(T.model_images(int(g['model_recipe'][0]), c['B'], c['size'])).to(device)
    with torch.no_grad():
        out = net(images)
    assert len(out['logits']) == 10
    worst = 0.0
    for i, t in enumerate(out['logits'] + [out['pr_gate']]):
        name = f'logits{i}' if i < 10 else 'pr_gate'
        want = g[f'eval_{name}_f64']
        got = np_(t)
        err = float(np.max(np.abs(got - want)))
        print(f'model eval {name}: max abs error {err:.2e}')
        assert err <= 1e-4 and got.argmax(1).tolist() == want.argmax(1).tolist(), (name, err)
        worst = max(worst, err)
    for k, boxes in enumerate(net.boxes):
        assert np.array_equal(np_(boxes).reshape(-1, 4), g[f'eval_boxes{k + 1}']), k
    return worst


def check_model_train_step(plugin, device, monkeypatch):
    """Train mode, y=None (the extra no-grad eval-mode forward picks the class), the criterion on the kernel, against the
    reference's loss and torch.autograd.grad of it."""
    from hawkeye_amd.model.loss import MGELoss
    from hawkeye_amd.config import CfgNode
    g = T.load('mge_model.npz')
    c = T.MODEL_CASE
    net = short_model(plugin, device, monkeypatch).train()
    before = {k: v.clone() for k, v in net.state_dict().items() if 'running' in k and 'gate' not in k}
    images = torch.from_numpy(T.model_images(int(g['model_recipe'][0]), c['B'], c['size'])).to(device)
    out = net(images)
    loss = MGELoss(CfgNode({}))(out, torch.tensor(c['labels'], device=device))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad(loss, [params[n] for n in T.TRAIN_GRADS])
    worst = judge_value('mge train', 'loss', np_(loss), g['train_loss_f32'], g['train_loss_f64'])
    for k, boxes in enumerate(net.boxes):
        assert np.array_equal(np_(boxes).reshape(-1, 4), g[f'train_boxes{k + 1}']), k
    for n, t in zip(T.TRAIN_GRADS, grads):
        worst = max(worst, judge_value('mge train', n, T.grad_sample(np_(t)), g[f'train_grad_{n}_f32'], g[f'train_grad_{n}_f64']))
    assert all(q.grad is None for q in net.parameters())   # the plugin leaves .grad alone
    momentum = net.conv5[0].bn1.momentum                   # one train-mode update per BatchNorm: the extra forward moved nothing
    ref = short_model(plugin, device, monkeypatch).train()
    with torch.no_grad():
        ref.conv5(ref.conv4(images))
    for k, v in ref.state_dict().items():
        if k.startswith(('conv4.', 'conv5.')) and 'running' in k:
            assert torch.allclose(net.state_dict()[k], v, rtol=1e-5, atol=1e-6), k
    assert momentum == 0.1 and before
    return worst


def check_trainer(device, tmp_path, monkeypatch):
    """MGE_CNNTrainer from configs/MGE_CNN_synthetic.yaml with the short trunk on 64 x 64 images: two steps through the part pool,
    the Grad-CAM boxes, the crops and the criterion - a finite loss, a gradient on every parameter the forward uses, the two parameter groups at
    lr and 0.1 lr, the warm-up schedule, and a validation pass."""
    import importlib
    import os
    import sys
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.registry import MODEL
    from hawkeye_amd.train import Trainer
    modules = ('hawkeye_amd.model.methods.MGE_CNN', 'hawkeye_amd.examples.MGE_CNN')
    assert 'MGE_CNN' not in MODEL
    ex = importlib.import_module(modules[1])               # the trainer does the opt-in import of the plugin
    plug = sys.modules[modules[0]]
    try:
        assert 'MGE_CNN' in MODEL
        if device.type == 'cpu':
            monkeypatch.setattr(Trainer, 'select_device', lambda self, cfg: torch.device('cpu'))
        monkeypatch.setattr(plug, 'resnet50', short_trunk(plug))
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        cfg = CfgNode.load_cfg(open(os.path.join(root, 'configs', 'MGE_CNN_synthetic.yaml')))
        cfg.dataset.samples, cfg.dataset.batch_size, cfg.dataset.num_workers = 4, 2, 0
        cfg.dataset.transformer.image_size, cfg.dataset.transformer.resize_size = 64, 72
        cfg.model.image_size, cfg.model.num_classes = 64, 5
        cfg.experiment.log_dir = str(tmp_path)
        cfg.freeze()
        tr = ex.MGE_CNNTrainer(cfg)
        net = tr.model
        assert isinstance(tr.criterion, ex.MGELoss) and isinstance(tr.optimizer, torch.optim.Adam)
        assert isinstance(tr.scheduler, torch.optim.lr_scheduler.SequentialLR)
        groups = tr.optimizer.param_groups
        assert [g['initial_lr'] for g in groups] == [0.0004, 0.0004 * 0.1] and all(g['weight_decay'] == 0.00002 for g in groups)
        assert sum(len(g['params']) for g in groups) == len(list(net.parameters()))
        seen, step = [], tr.optimizer.step

        def recording_step(*a, **k):
            seen.append({n: float(q.grad.abs().max()) for n, q in net.named_parameters() if q.grad is not None})
            return step(*a, **k)
        monkeypatch.setattr(tr.optimizer, 'step', recording_step)
        tr.train()
        assert len(seen) == 2
        for grads in seen:
            # (cls_cat_a is built and never called, in the reference as here)
            assert sorted(grads) == sorted(n for n, _ in net.named_parameters() if not n.startswith('cls_cat_a.'))
            assert all(np.isfinite(v) for v in grads.values()), grads
            assert all(grads[n] > 0 for n in ('conv6.weight', 'conv6_2.bias', 'classifier_box.fc.weight', 'cls_cat.fc.weight', 'cls_gate.0.fc.weight', 'conv4_box_2.0.weight')), grads
        loss = tr.performance_meters['train']['loss'].values
        assert len(loss) == 1 and np.isfinite(loss[0])
        assert len(tr.performance_meters['val']['acc'].values) == 1
    finally:
        MODEL.pop('MGE_CNN', None)
        for name in modules:
            sys.modules.pop(name, None)
