"""The NTS-Net checks that the emulated tier (test_emu_nts.py) and the GPU tier (test_gpu_nts.py) share: each takes the
device to run on.  Indices, boxes and indicators are compared exactly; values are judged by the rule of
tests/golden/nts_inputs.py - at most 4 x the float32 reference's own distance from the float64 result, floor 1e-6.
Not a test module itself."""
import numpy as np
import torch

import nts_inputs as T

GOLDEN = T.load()
NMS_CASES = T.load_nms_cases(GOLDEN)
CROP_CASES = T.load_crop_cases(GOLDEN)
LOSS_CASES = T.load_loss_cases(GOLDEN)


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------- NMS
def run_nms(scores, anchors, device, topn=T.TOPN, thresh=T.IOU):
    index, boxes = F().nts_nms(torch.from_numpy(np.asarray(scores)).to(device), torch.from_numpy(np.asarray(anchors)).to(device), topn, thresh)
    assert index.dtype == torch.int64 and boxes.dtype == torch.int32
    assert index.shape == (len(scores), topn) and boxes.shape == (len(scores), topn, 4)
    return np_(index), np_(boxes)


def check_nms_case(case, device):
    index, boxes = run_nms(case['scores'], case['anchors'], device)
    assert np.array_equal(index, case['index']), (index, case['index'])
    assert np.array_equal(boxes, case['boxes'])
    assert np.array_equal(boxes, case['anchors'][index])


def check_nms_ties(device):
    """Five anchors that do not touch each other, equal scores: the highest index first - a stable ascending sort read
    from its end."""
    anchors = np.array([[0, 10 * k, 8, 10 * k + 8] for k in range(5)], dtype=np.int32)
    index, _ = run_nms(np.array([[1.0, 2.0, 2.0, 1.0, 2.0], [0.5] * 5], dtype=np.float32), anchors, device, topn=5)
    assert index.tolist() == [[4, 2, 1, 3, 0], [4, 3, 2, 1, 0]]


def small_table(a, seed):
    """`a` boxes on a 64 x 64 canvas with sides from 4 to 40."""
    rs = np.random.RandomState(seed)
    y0, x0 = rs.randint(0, 40, a), rs.randint(0, 40, a)
    return np.stack([y0, x0, y0 + rs.randint(4, 41, a), x0 + rs.randint(4, 41, a)], 1).astype(np.int32)


def check_nms_table(device, a, b, seed, topn=T.TOPN):
    """A table of `a` random boxes against the float64 restatement in nts_inputs.nms_trace (ties included: the scores are
    drawn from a few values)."""
    anchors = small_table(a, seed)
    rs = np.random.RandomState(seed + 1)
    scores = rs.randint(0, max(a // 3, 2), (b, a)).astype(np.float32) / 8
    index, boxes = run_nms(scores, anchors, device, topn)
    want = np.stack([T.nms_trace(row, anchors, topn)[0] for row in scores])
    assert np.array_equal(index, want), (index, want)
    assert np.array_equal(boxes, anchors[want])
    return index


def check_nms_fill(device):
    """Fewer survivors than topn: the last chosen anchor fills the rest.  Three nested boxes and a far one; then two empty
    boxes at one point (0 / 0: NaN < thresh is false in the reference too, so the second goes) and a far one."""
    anchors = np.array([[0, 0, 20, 20], [1, 1, 19, 19], [2, 2, 18, 18], [40, 40, 50, 50]], dtype=np.int32)
    index, boxes = run_nms(np.array([[3.0, 2.0, 1.0, 0.0]], dtype=np.float32), anchors, device, topn=4)
    assert index.tolist() == [[0, 3, 3, 3]]
    assert boxes[0].tolist() == [[0, 0, 20, 20]] + [[40, 40, 50, 50]] * 3
    anchors = np.array([[5, 5, 5, 5], [5, 5, 5, 5], [30, 30, 40, 40]], dtype=np.int32)
    index, _ = run_nms(np.array([[3.0, 2.0, 1.0]], dtype=np.float32), anchors, device, topn=3)
    assert index.tolist() == [[0, 2, 2]] and T.nms_trace([3.0, 2.0, 1.0], anchors, 3)[0].tolist() == [0, 2, 2]
    index, _ = run_nms(np.array([[0.0, float('nan'), 1.0, float('-inf'), 0.5]], dtype=np.float32),
                       np.array([[0, 10 * k, 8, 10 * k + 8] for k in range(5)], dtype=np.int32), device, topn=6)
    assert index.tolist() == [[2, 4, 0, 3, 1, 1]]            # NaN counts as -inf; equal scores: the highest index; then the fill


# ----------------------------------------------------------------------------------------------------- crops
def crop_ref(images, boxes, pad, out, dtype):
    """F.pad + slice + F.interpolate(align_corners=True) in torch on the CPU; an empty slice gives zeros."""
    x = torch.from_numpy(images).to(dtype)
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    b, n = boxes.shape[:2]
    res = torch.zeros(b, n, x.shape[1], *out, dtype=dtype)
    for i in range(b):
        for j in range(n):
            y0, x0, y1, x1 = (int(v) + pad for v in boxes[i, j])
            piece = xp[i:i + 1, :, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)]
            if piece.numel():
                res[i, j] = torch.nn.functional.interpolate(piece, size=out, mode='bilinear', align_corners=True)[0]
    return res.view(b * n, x.shape[1], *out).numpy()


def check_crop_case(case, device):
    got = F().nts_crop_resize(torch.from_numpy(case['images']).to(device), torch.from_numpy(case['boxes']).to(device), case['pad'], case['out'])
    assert got.shape == case['out_f64'].shape
    if not np.array_equal(case['out_f32'], case['out_f64']):
        T.judge_value(f"crop case {case['k']}", 'out', np_(got), case['out_f32'], case['out_f64'])
    else:                                                   # out 1 x 1: the box's first pixel, copied
        assert np.array_equal(np_(got), case['out_f64'].astype(np.float32))
    return got


def check_crop_shapes(device, out, seed=11, unaligned=False, strided=False):
    """Random boxes - inside, across every edge, wholly in the padding, past the padded extent, empty and inverted -
    against the torch restatement; out widths that are and are not a multiple of four."""
    rs = np.random.RandomState(seed)
    b, c, h, w, n, pad = 3, 2, 21, 19, 5, 7
    images = rs.randn(b, c, h, w).astype(np.float32)
    y0, x0 = rs.randint(-pad - 3, h + 2, (b, n)), rs.randint(-pad - 3, w + 2, (b, n))
    boxes = np.stack([y0, x0, y0 + rs.randint(-2, h + pad, (b, n)), x0 + rs.randint(-2, w + pad, (b, n))], -1).astype(np.int32)
    boxes[0, 0] = [-pad - 5, -pad - 9, h + pad + 4, w + pad + 6]            # larger than the padded image: clipped to it
    boxes[1, 1] = [h + 1, w + 1, h + pad, w + pad]                          # wholly in the padding: zeros
    boxes[2, 2] = [4, 4, 4, 9]                                              # empty
    clipped = boxes.copy()
    clipped[..., :2] = np.maximum(boxes[..., :2], -pad)
    ref32, ref64 = (crop_ref(images, clipped, pad, out, dt) for dt in (torch.float32, torch.float64))
    x = torch.from_numpy(images).to(device)
    bx = torch.from_numpy(boxes).to(device)
    if strided:                                             # non-contiguous views of both inputs
        x = torch.from_numpy(np.ascontiguousarray(images.transpose(0, 1, 3, 2))).to(device).permute(0, 1, 3, 2)
        bx = torch.from_numpy(boxes).to(device).long().repeat_interleave(2, dim=2)[:, :, ::2]
        assert not x.is_contiguous() and not bx.is_contiguous()
    got = F().nts_crop_resize(x, bx, pad, out)
    T.judge_value(f'crop out {out}', 'out', np_(got), ref32, ref64)
    per_box = np_(got).reshape(b, n, -1)
    assert not per_box[1, 1].any() and not per_box[2, 2].any()
    return got


def check_crop_unaligned_output(device):
    """The ABI with an output behind a base pointer that is not 16-byte aligned (a dense view one float into a buffer):
    the scalar-store path gives the bits of the vector path."""
    import ctypes
    from hawkeye_amd import _lib
    lib = _lib.load()
    case = CROP_CASES[0]
    x = torch.from_numpy(case['images']).to(device)
    bx = torch.from_numpy(case['boxes']).to(device)
    want = F().nts_crop_resize(x, bx, case['pad'], case['out'])
    buf = torch.zeros(want.numel() + 5, device=device)
    view = buf[1:1 + want.numel()]
    assert view.data_ptr() % 16 == 4 and want.data_ptr() % 16 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = None if device.type == 'cpu' else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.hk_nts_crop_resize(p(x), p(bx), p(view), case['B'], case['N'], case['C'], case['H'], case['W'], case['pad'], *case['out'], st)
    assert rc == 0
    assert torch.equal(view.view_as(want), want) and buf[0] == 0 and not buf[1 + want.numel():].any()


# ----------------------------------------------------------------------------------------------------- loss
def loss_tensors(case, device, grad=True):
    return [torch.from_numpy(case[k]).to(device).requires_grad_(grad) for k in ('raw', 'concat', 'part', 'prob')] + \
        [torch.from_numpy(case['y']).to(device)]


def run_loss(case, device, weight=1.0):
    raw, cat, part, prob, y = loss_tensors(case, device)
    total, parts = F().nts_loss_with_parts(raw, cat, part, prob, y)
    assert total.dim() == 0 and parts.shape == (4,) and not parts.requires_grad
    (total * weight).backward()
    return dict(loss=np.concatenate([np_(total).reshape(1), np_(parts)]), draw=np_(raw.grad), dconcat=np_(cat.grad), dpart=np_(part.grad),
                dprob=np_(prob.grad))


def kernel_indicator(case, device):
    """The indicator matrix as the kernel takes it, exactly: with every score zero each gated hinge is 1 and active, so
    B x d rank / d s_bk = #{i: part_loss_bk > part_loss_bi} - #{j: part_loss_bj > part_loss_bk} - the place of k in its
    sample's order of part losses, from which ind[b, i, j] = part_loss_bj > part_loss_bi follows."""
    raw, cat, part, prob, y = loss_tensors(case, device)
    zero = torch.zeros_like(prob).requires_grad_(True)
    F().nts_loss(raw, cat, part, zero, y).backward()
    scaled = np_(zero.grad).astype(np.float64) * case['B']
    place = np.round(scaled)
    assert np.abs(scaled - place).max() < 1e-5              # an integer, up to the rounding of the division by B
    return place[:, None, :] > place[:, :, None]


def check_loss_case(case, device):
    got = run_loss(case, device)
    worst = T.judge_loss(case, got['loss'], got['draw'], got['dconcat'], got['dpart'], got['dprob'])
    assert np.array_equal(kernel_indicator(case, device), case['indicator'])
    raw, cat, part, prob, y = loss_tensors(case, device, grad=False)
    assert torch.equal(F().nts_loss(raw, cat, part, prob, y.int()), F().nts_loss(raw, cat, part, prob, y))
    return worst


def check_loss_scaling(case, device, weight=4.0):
    """A power-of-two loss weight scales every gradient exactly."""
    one, four = run_loss(case, device), run_loss(case, device, weight)
    for name in ('draw', 'dconcat', 'dpart', 'dprob'):
        assert np.array_equal(one[name] * np.float32(weight), four[name]), name
    assert one['loss'].tobytes() == four['loss'].tobytes()


def check_loss_gradient_routes(case, device):
    """part_logits hears from the part-class CE only (the gate has no gradient), top_n_prob from the rank term only."""
    raw, cat, part, prob, y = loss_tensors(case, device)
    F().nts_loss(raw, cat, part, prob, y).backward()
    b, n, c = case['B'], case['N'], case['C']
    lp = torch.from_numpy(case['part']).double().requires_grad_(True)
    torch.nn.functional.cross_entropy(lp.view(b * n, c), torch.from_numpy(case['y']).repeat_interleave(n), label_smoothing=0.1).backward()
    assert T.distance(np_(part.grad), lp.grad.numpy()) < 1e-5
    shifted = torch.from_numpy(case['prob'] + 1.0).to(device).requires_grad_(True)          # the hinge sees differences only
    F().nts_loss(raw.detach(), cat.detach(), part.detach(), shifted, y).backward()
    assert np.array_equal(np_(shifted.grad), np_(prob.grad))


def check_loss_bad_labels(device):
    case = dict(LOSS_CASES[3])
    case['y'] = case['y'].copy()
    case['y'][1] = case['C'] + 1000000
    raw, cat, part, prob, y = loss_tensors(case, device)
    total, parts = F().nts_loss_with_parts(raw, cat, part, prob, y)
    assert torch.isnan(total) and torch.isnan(parts[:3]).all() and torch.isfinite(parts[3])
    total.backward()
    assert np.isfinite(np_(raw.grad)[0]).all() and np.isfinite(np_(part.grad)[0]).all() and np.isfinite(np_(prob.grad)).all()
    case['y'][1] = -3
    assert torch.isnan(F().nts_loss(*loss_tensors(case, device)))


def check_noncontiguous(device):
    """Strided views of every input give the bits of their dense copies."""
    HF = F()
    case = NMS_CASES[1]
    s = torch.from_numpy(case['scores']).to(device)
    a = torch.from_numpy(case['anchors']).to(device)
    s2 = torch.stack([s, s], 2)[:, :, 0]
    a2 = a.long().t().contiguous().t()
    assert not s2.is_contiguous() and not a2.is_contiguous()
    for x, y in zip(HF.nts_nms(s2, a2, T.TOPN), HF.nts_nms(s, a, T.TOPN)):
        assert torch.equal(x, y)
    case = LOSS_CASES[1]
    dense = loss_tensors(case, device, grad=False)
    views = [torch.stack([t, t], -1)[..., 1] for t in dense[:4]]
    assert not any(v.is_contiguous() for v in views)
    ld = [t.requires_grad_(True) for t in dense[:4]]
    lv = [v.requires_grad_(True) for v in views]
    one, two = HF.nts_loss(*ld, dense[4]), HF.nts_loss(*lv, dense[4])
    one.backward()
    two.backward()
    assert torch.equal(one, two) and all(torch.equal(p.grad, q.grad) for p, q in zip(ld, lv))
