"""The checks of the first-generation heads (csrc/apcnn.hip, apcnn_roi2.hip, osme.hip, mamc.hip) that the emulated tier
(test_emu_apcnn.py) and the GPU tier (test_gpu_apcnn.py) share: each takes the device to run on.  Values are judged by the
project's rule (tests/golden/crossx_inputs.py: judge_value) - at most 4 x the float32 reference's own distance from the
float64 result, floor 1e-6; what is exactly zero in float64 must be exactly zero.  The reference is the reference model's op
sequence in torch on the CPU with autograd, in float64, and its float32 run is the yardstick; both are computed once per
case.  Index and integer results (the ROI selection) are bit-exact.  Not a test module."""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

import hawkeye_oracle as O
from crossx_inputs import judge_value


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


def dev_(a, device, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).requires_grad_(grad)


# ---------------------------------------------------------------------------------------------- ROI crop + resize
# map sizes: the generic kernels (a side above 64), the <16>, <13> and <4> instances with 16-byte and scalar staging, maps
# smaller than the 8-, 6- and 3-tap windows
ROI_MAPS = ((72, 72), (65, 9), (7, 80), (64, 64), (56, 56), (33, 47), (32, 32), (5, 7), (4, 4), (2, 9))
ROI_CPB_CASES = ((41, 201, 4, 4), (33, 130, 5, 6))          # 32 and 16 maps per workgroup, last group of 9 and 2 maps
ROI_TROW_CW = 44                                             # apcnn_roi2.hip: the widest crop of the separable table path
ROI_BRANCHES = ('empty', 'window 3', 'window 4', 'window 8', 'window 6', 'table separable', 'table per pixel', 'table wide')
DROP_KINDS = ('none', 'inside', 'straddle', 'outside', 'one axis')
NO_DROP = (0.0, 0.0, -1.0, -1.0)

# boxes added until the case list reaches every branch of the backward's dispatch (check_roi_branch_coverage)
ROI_EXTRA_BOXES = {
    (56, 56): ((5.2, 6.1, 39.3, 40.7), (20.5, 21.5, 36.4, 37.9), (10.3, 12.6, 34.9, 36.2), (6.0, 20.2, 50.3, 32.7)),
    (64, 64): ((7.4, 9.2, 47.6, 49.1), (30.5, 11.5, 46.4, 27.9), (12.3, 8.6, 40.9, 36.2), (10.0, 30.2, 50.3, 44.7)),
    (33, 47): ((10.2, 5.3, 22.9, 14.8),),
    (32, 32): ((8.5, 9.5, 17.4, 18.9),),
}


def roi_boxes(h, w):
    """The float boxes (x1, y1, x2, y2) of one call, scaled to the map: the full map, a box past the right and bottom border,
    a mid-size fractional box, a 2 x 1-pixel crop, a full-width strip 4 rows high and its transpose, an empty crop."""
    x0, y0 = min(int(0.4 * w), w - 2), min(int(0.4 * h), h - 1)
    ys, xs = min(int(0.3 * h), max(h - 4, 0)), min(int(0.3 * w), max(w - 4, 0))
    boxes = [(0.0, 0.0, w, h),
             (int(0.3 * w) + 0.5, int(0.4 * h) + 0.25, w + 3.5, h + 2.25),
             (0.21 * w + 0.3, 0.17 * h + 0.6, 0.71 * w + 0.4, 0.77 * h + 0.2),
             (x0 + 0.3, y0 + 0.6, x0 + 2.5, y0 + 1.7),
             (0.0, ys, w, ys + 4.2),
             (xs + 0.1, 0.0, xs + 4.9, h),
             (0.5 * w, 1.0, 0.5 * w, h)]
    return np.asarray(boxes + list(ROI_EXTRA_BOXES.get((h, w), ())), dtype=np.float32)


def int_rect(r, h, w):
    """.long() truncation and the clipping of a python slice: (x1, y1, x2, y2) with x2 >= x1, y2 >= y1 (coordinates >= 0)."""
    x1, y1, x2, y2 = (int(v) for v in r)
    assert min(x1, y1) >= 0 and (x2 >= 0 or tuple(r) == NO_DROP)
    x1, x2, y1, y2 = min(x1, w), min(max(x2, 0), w), min(y1, h), min(max(y2, 0), h)
    return x1, y1, max(x2, x1), max(y2, y1)


def drop_rect(kind, box, h, w):
    """The drop rectangle of one kind, placed relative to the integer crop of `box`."""
    x1, y1, x2, y2 = int_rect(box, h, w)
    cw, ch = x2 - x1, y2 - y1
    if kind == 'none' or cw == 0 or ch == 0:
        return NO_DROP
    if kind == 'inside':
        a, b = x1 + cw // 4, y1 + ch // 4
        return a + 0.3, b + 0.2, a + max(1, cw // 2) + 0.6, b + max(1, ch // 2) + 0.5
    if kind == 'straddle':                                   # over the crop's left and bottom edge
        return max(x1 - 2, 0) + 0.5, y1 + ch // 2 + 0.1, x1 + max(1, cw // 2) + 0.7, y2 + 3.2
    if kind == 'outside':
        if x2 + 1 < w:
            return x2 + 0.2, y1 + 0.3, float(w), y2 + 0.4
        if x1 >= 1:
            return 0.0, y1 + 0.3, x1 + 0.9, y2 + 0.4
        if y2 < h:
            return 0.2, y2 + 0.1, float(w), h + 2.0
        if y1 >= 1:
            return 0.0, 0.0, float(w), y1 + 0.5
        return w + 1.5, h + 1.5, w + 5.0, h + 4.0            # the crop is the map: a rectangle beyond it
    assert kind == 'one axis'                                # d2 > d0, d3 <= d1: the kernels' test passes, nothing is dropped
    return x1 + 0.2, y1 + ch // 2 + 0.9, float(x2), y1 + ch // 2 + 0.1


def mask_sum(box, drop, h, w):
    x1, y1, x2, y2 = int_rect(box, h, w)
    m = np.ones((h, w))
    if drop[2] > drop[0] or drop[3] > drop[1]:
        dx1, dy1, dx2, dy2 = int_rect(drop, h, w)
        m[dy1:dy2, dx1:dx2] = 0
    return m[y1:y2, x1:x2].sum()


@functools.lru_cache(maxsize=None)
def roi_inputs(h, w, c, training, b=None):
    """x, wt [B, C, h, w], box, drop [B, 4].  b None: every box of roi_boxes, in train mode under two kinds of drop each
    (all five kinds occur); b given: the boxes and the kinds dealt round."""
    boxes = roi_boxes(h, w)
    if b is None:
        pairs = [(i, k) for i in range(len(boxes)) for k in sorted({i % 5, (2 * i + 1) % 5} if training else {i % 5})]
    else:
        pairs = [(i % len(boxes), (i // len(boxes) + i) % 5) for i in range(b)]
    box = np.stack([boxes[i] for i, _ in pairs])
    drop = np.asarray([drop_rect(DROP_KINDS[k], boxes[i], h, w) for i, k in pairs], dtype=np.float32)
    assert {DROP_KINDS[k] for _, k in pairs} == set(DROP_KINDS)
    for bx, dr in zip(box, drop):                            # a wholly dropped crop has a NaN rate in the reference itself
        x1, y1, x2, y2 = int_rect(bx, h, w)
        assert (x2 - x1) * (y2 - y1) == 0 or mask_sum(bx, dr, h, w) > 0, (h, w, bx, dr)
    rs = np.random.RandomState(1000 * h + 10 * w + int(training))
    shape = (len(pairs), c, h, w)
    return dict(x=rs.randn(*shape).astype(np.float32), wt=rs.randn(*shape).astype(np.float32), box=box, drop=drop)


def roi_reference(a, training, dtype):
    """get_roi_crop_feat's per-image sequence (APCNN.py:478-531) from box / drop rows, and its autograd under `wt`."""
    x = torch.from_numpy(a['x']).to(dtype).requires_grad_(True)
    n, c, h, w = x.shape
    outs = []
    for i in range(n):
        xx1, yy1, xx2, yy2 = torch.from_numpy(a['box'][i]).to(dtype)
        if training:
            mask = torch.ones(c, h, w, dtype=dtype)
            d = torch.from_numpy(a['drop'][i]).to(dtype)
            if d[2] > d[0] or d[3] > d[1]:                   # (the kernels' encoding of "no drop": [0, 0, -1, -1])
                mask[:, d[1].long():d[3].long(), d[0].long():d[2].long()] = 0
            crop = (x[i] * mask)[:, yy1.long():yy2.long(), xx1.long():xx2.long()].contiguous().unsqueeze(0)
            if crop.numel():
                rate = c * (yy2 - yy1) * (xx2 - xx1) / torch.sum(mask[:, yy1.long():yy2.long(), xx1.long():xx2.long()])
                crop = crop * rate
        else:
            crop = x[i, :, yy1.long():yy2.long(), xx1.long():xx2.long()].contiguous().unsqueeze(0)
        outs.append(TF.interpolate(crop, (h, w), mode='bilinear', align_corners=False) if crop.numel()
                    else (x[i] * 0).unsqueeze(0))            # an empty crop gives zeros
    y = torch.cat(outs, 0)
    (y * torch.from_numpy(a['wt']).to(dtype)).sum().backward()
    return dict(y=y.detach().numpy(), dx=x.grad.numpy())


@functools.lru_cache(maxsize=None)
def roi_case(h, w, c, training, b=None):
    a = roi_inputs(h, w, c, training, b)
    return a, roi_reference(a, training, torch.float32), roi_reference(a, training, torch.float64)


def run_roi(a, training, device):
    x = dev_(a['x'], device, True)
    y = F().roi_crop_resize(x, dev_(a['box'], device), dev_(a['drop'], device), training)
    (y * dev_(a['wt'], device)).sum().backward()
    return dict(y=np_(y), dx=np_(x.grad))


def roi_channels(h, w):
    return 2 + (h + w) % 2


def check_roi_exact(a, got, training):
    """dx is exactly zero outside the crop and inside the drop rectangle; in eval mode the full-map box copies x."""
    n, c, h, w = a['x'].shape
    for i in range(n):
        x1, y1, x2, y2 = int_rect(a['box'][i], h, w)
        live = np.zeros((h, w), dtype=bool)
        live[y1:y2, x1:x2] = True
        d = a['drop'][i]
        if training and (d[2] > d[0] or d[3] > d[1]):
            dx1, dy1, dx2, dy2 = int_rect(d, h, w)
            live[dy1:dy2, dx1:dx2] = False
        assert not got['dx'][i][:, ~live].any(), (i, a['box'][i], d)
        if not training and (x1, y1, x2, y2) == (0, 0, w, h):
            assert got['y'][i].tobytes() == a['x'][i].tobytes(), i      # scale 1: integer source positions, weights 1 and 0


def judge_roi(label, a, got, r32, r64):
    """y and dx per image: each image has its own geometry, and a small crop must not hide behind a large one."""
    worst = 0.0
    for i in range(a['x'].shape[0]):
        for name in ('y', 'dx'):
            worst = max(worst, judge_value(label, f'{name}[{i}]', got[name][i], r32[name][i], r64[name][i]))
    return worst


def check_roi_case(h, w, training, device, c=None, b=None):
    c = c or roi_channels(h, w)
    a, r32, r64 = roi_case(h, w, c, training, b)
    got = run_roi(a, training, device)
    check_roi_exact(a, got, training)
    return judge_roi(f"roi {h}x{w} {'train' if training else 'eval'}", a, got, r32, r64)


def check_roi_cpb(shape, device):
    b, c, h, w = shape
    cpb = 8
    while cpb < 32 and b * -(-c // cpb) > 512:               # roi_crop_fwd_v2 / roi_crop_bwd_v2
        cpb *= 2
    assert (cpb, c % cpb) == {ROI_CPB_CASES[0]: (32, 9), ROI_CPB_CASES[1]: (16, 2)}[tuple(shape)]
    return check_roi_case(h, w, True, device, c=c, b=b)


def check_roi_kernel_pairs(h, w, device, tune):
    """Maps of at most 64 x 64: the LDS-staged kernels (the default) and the round-1 table kernels (roi_bwd = 1) give the same
    bits, in train mode too."""
    assert h <= 64 and w <= 64
    for training in (True, False):
        a = roi_inputs(h, w, roi_channels(h, w), training)
        res = []
        for flag in (1, 0):
            tune('roi_bwd', flag)
            res.append(run_roi(a, training, device))
        assert res[0]['y'].tobytes() == res[1]['y'].tobytes(), (h, w, training)
        assert res[0]['dx'].tobytes() == res[1]['dx'].tobytes() and res[0]['dx'].any(), (h, w, training)


def src_index_f32(scale, dst, n):
    """numpy twin of src_index (hk_roi.h) in float32 for every dst in range(dst) -> i0, i1, l0, l1."""
    f = np.float32
    s = np.maximum(f(scale) * (np.arange(dst, dtype=f) + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(s.astype(np.int32), n - 1)
    i1 = i0 + (i0 < n - 1)
    l1 = s - i0.astype(f)
    return i0, i1, f(1) - l1, l1


def tap_range(out, n):
    """The largest number of output coordinates between the first and the last that sample one source coordinate."""
    i0, i1, l0, l1 = src_index_f32(np.float32(n) / np.float32(out), out, n)
    lo, hi = np.full(n, out), np.full(n, -1)
    for o in range(out):
        for i, l in ((i0[o], l0[o]), (i1[o], l1[o])):
            if l != 0:
                lo[i], hi[i] = min(lo[i], o), max(hi[i], o)
    return max(1, int((hi - lo + 1).max()))


def roi_branch(h, w, box):
    """Which branch of roi_crop_bwd_tab3_kernel's dispatch a box takes on an h x w map (<= 64 x 64) -> (name, ch, cw, KY, KX).
    This looks at the inputs, not into the kernel."""
    x1, y1, x2, y2 = int_rect(box, h, w)
    cw, ch = x2 - x1, y2 - y1
    if cw == 0 or ch == 0:
        return 'empty', ch, cw, 0, 0
    ky, kx = min(tap_range(h, ch), h), min(tap_range(w, cw), w)
    fits = lambda k: ky <= k and kx <= k and h >= k and w >= k
    if fits(3):
        name = 'window 3'
    elif fits(4):
        name = 'window 4'
    elif fits(8) and ch * cw <= 512:
        name = 'window 8'
    elif fits(6) and ch * cw <= 1536:
        name = 'window 6'
    elif ch * cw <= 512 and cw <= ROI_TROW_CW:
        name = 'table separable'                              # row sums once, then the column sum per pixel
    elif cw <= ROI_TROW_CW:
        name = 'table per pixel'
    else:
        name = 'table wide'                                   # wider than one column chunk of the row-sum buffer
    return name, ch, cw, ky, kx


def check_roi_branch_coverage():
    seen = {}
    for h, w in ROI_MAPS:
        if h > 64 or w > 64:
            continue
        for box in roi_boxes(h, w):
            name, ch, cw, ky, kx = roi_branch(h, w, box)
            seen.setdefault(name, []).append(f'{h}x{w} crop {ch}x{cw} taps {ky}x{kx}')
    for name in ROI_BRANCHES:
        print(f'{name}: {"; ".join(seen.get(name, ()))}')
    assert set(seen) == set(ROI_BRANCHES), sorted(set(ROI_BRANCHES) - set(seen))
    for h, w in ((5, 7), (4, 4), (2, 9)):                    # maps smaller than the 8-, 6- and 3-tap windows: no such window
        names = {roi_branch(h, w, box)[0] for box in roi_boxes(h, w)}
        assert not names & {'window 8', 'window 6'} and (h >= 3 or not names & {'window 3', 'window 4'}), (h, w, names)
    assert any(roi_branch(2, 9, box)[0].startswith('table') for box in roi_boxes(2, 9))
    return seen


# ------------------------------------------------------------------------------------------ attention ROI selection
# (h, w, feature stride, anchor size, img_h, img_w, IoU threshold, topk, scores rounded to quarters)
SELECT_CASES = ((10, 14, 16, 128.0, 150, 200, 0.05, 3, False),
                (20, 12, 8, 64.0, 140, 90, 0.3, 5, False),
                (5, 31, 32, 256.0, 150, 900, 0.05, 12, False),      # topk above the number of survivors
                (37, 3, 8, 64.0, 280, 20, 0.05, 4, False),
                (20, 12, 16, 96.0, 300, 170, 0.3, 6, True),         # ties everywhere
                (96, 100, 4, 64.0, 380, 390, 0.05, 5, False))       # 75 KB of LDS
SELECT_LEVELS = (((20, 12), (8, 32.0, 5)), ((10, 14), (16, 64.0, 3)), ((5, 31), (32, 256.0, 2)))


def select_case_id(case):
    return '{}x{}-s{}-a{:.0f}-k{}{}'.format(*case[:4], case[7], '-ties' if case[8] else '')


def select_mask(h, w, ties=False, b=2):
    rs = np.random.RandomState(100 * h + w)
    m = 1.0 / (1.0 + np.exp(-2.0 * rs.randn(b, 1, h, w)))
    if ties:
        m = np.round(m * 4) / 4
    return torch.from_numpy(m.astype(np.float32))


def compact(rois, cnt):
    rows = []
    for i in range(rois.shape[0]):
        k = int(cnt[i])
        rows.append(torch.cat([torch.full((k, 1), float(i)), rois[i, :k].cpu()], 1))
    return torch.cat(rows, 0)


@functools.lru_cache(maxsize=None)
def select_reference(case, ncls, swapped=False):
    h, w, stride, anchor, img_h, img_w, thr, topk, ties = case
    if swapped:
        img_h, img_w = img_w, img_h
    return O.att_roi(select_mask(h, w, ties), stride, anchor, img_h, img_w, ncls, thr, topk)


def check_select_case(case, ncls, device):
    h, w, stride, anchor, img_h, img_w, thr, topk, ties = case
    m = select_mask(h, w, ties)
    ref = select_reference(case, ncls)
    rois, cnt = F().att_roi_select(m.to(device), stride, anchor, img_h, img_w, ncls, thr, topk)
    assert rois.shape == (m.shape[0], topk, 5) and cnt.dtype == torch.int32
    got = compact(rois, cnt)
    assert got.shape == ref.shape and torch.equal(got, ref), case
    for i in range(m.shape[0]):                              # rows past the count are zero
        assert not rois[i, int(cnt[i]):].any()
    # the inputs tell h from w: the clamp with img_h and img_w exchanged gives other boxes
    assert h > 40 or not torch.equal(ref, select_reference(case, ncls, True)), case
    if case[7] == 12:
        assert int(cnt.max()) < topk
    if ties:
        assert len(np.unique(np_(m))) <= 5


def check_select_levels(ncls, device, img_h=150, img_w=100, thr=0.05):
    masks = [select_mask(h, w, b=3).to(device) for (h, w), _ in SELECT_LEVELS]
    levels = [lv for _, lv in SELECT_LEVELS]
    tabs = F().att_roi_select_levels(masks, levels, img_h, img_w, ncls, thr)
    for m, (s, a, k), (rois, cnt) in zip(masks, levels, tabs):
        r1, c1 = F().att_roi_select(m, s, a, img_h, img_w, ncls, thr, k)
        assert torch.equal(rois, r1) and torch.equal(cnt, c1), (m.shape, s, a, k)
        assert torch.equal(compact(rois, cnt), O.att_roi(m.cpu(), s, a, img_h, img_w, ncls, thr, k))


def check_select_refused(device, h=140, w=140, topk=3, b=2):
    """2 h w floats of LDS above 150 KB: HK_ERR_UNSUPPORTED before any launch - rois, count and their guards untouched."""
    from hawkeye_amd import _lib
    HF = F()
    lib = _lib.load()
    assert 2 * h * w * 4 > 150 * 1024
    m = select_mask(h, w, b=b).to(device)
    try:
        HF.att_roi_select(m, 4, 64.0, 560, 560, 200, 0.05, topk)
    except _lib.HawkeyeHipError:
        pass
    else:
        raise AssertionError('a 140 x 140 map was not refused')
    try:
        HF.att_roi_select_levels([select_mask(8, 8, b=b).to(device), m, select_mask(4, 4, b=b).to(device)],
                                 [(8, 32.0, 2)] * 3, 560, 560, 200, 0.05)
    except _lib.HawkeyeHipError:
        pass
    else:
        raise AssertionError('a 140 x 140 level was not refused')
    rois = torch.full((2 + b * topk * 5,), 7.0, device=device)
    cnt = torch.full((2 + b,), 7, dtype=torch.int32, device=device)
    rc = lib.hk_att_roi_select(HF.ptr(m), HF.ptr(rois[1:-1]), HF.ptr(cnt[1:-1]), b, h, w, 4, 64.0, 560, 560, 28, 112, 28, 112, 0.05,
                               topk, HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED
    assert (rois == 7).all() and (cnt == 7).all()


# ------------------------------------------------------------------------------------------------ attention pooling
POOL_CASES = ((1, 1, 1, 1), (3, 7, 1, 5), (2, 5, 16, 16), (2, 5, 1, 257), (3, 3, 33, 31))
POOL_LEVEL_CASES = ((3, 7, (8, 4, 2)), (2, 5, (9, 4, 2)))  # 21 rows in one launch; ragged maps: the per-level launches


@functools.lru_cache(maxsize=None)
def pool_inputs(b, c, h, w, seed=0):
    rs = np.random.RandomState(31 * b + 7 * c + 3 * h + w + 1000 * seed)
    f32 = lambda v: v.astype(np.float32)
    return dict(f=f32(rs.randn(b, c, h, w)), a=f32(1.0 / (1.0 + np.exp(-rs.randn(b, 1, h, w)))), w1=f32(rs.randn(b, c)),
                w2=f32(rs.randn(b, c)))


def pool_reference(a, dtype, att=True):
    f, s = (torch.from_numpy(a[k]).to(dtype).requires_grad_(True) for k in ('f', 'a'))
    w1, w2 = (torch.from_numpy(a[k]).to(dtype) for k in ('w1', 'w2'))
    gap = f.mean(dim=(2, 3))
    total = (gap * w1).sum()
    out = dict(gap=gap)
    if att:
        out['sgap'] = (s * f).mean(dim=(2, 3))
        total = total + (out['sgap'] * w2).sum()
    total.backward()
    out['df'] = f.grad
    if att:
        out['da'] = s.grad
    return {k: v.detach().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def pool_case(b, c, h, w, att=True, seed=0):
    a = pool_inputs(b, c, h, w, seed)
    return a, pool_reference(a, torch.float32, att), pool_reference(a, torch.float64, att)


def run_pool(a, device, att=True):
    f, s = dev_(a['f'], device, True), dev_(a['a'], device, True)
    gap, sgap = F().att_pool(f, s if att else None)
    total = (gap * dev_(a['w1'], device)).sum()
    out = dict(gap=gap)
    if att:
        out['sgap'] = sgap
        total = total + (sgap * dev_(a['w2'], device)).sum()
    else:
        assert sgap is None
    total.backward()
    out['df'] = f.grad
    if att:
        out['da'] = s.grad
    return {k: np_(v) for k, v in out.items()}


def check_pool_case(case, att, device):
    a, r32, r64 = pool_case(*case, att=att)
    got = run_pool(a, device, att)
    return max(judge_value(f"att_pool {case} {'attention' if att else 'plain'}", k, got[k], r32[k], r64[k]) for k in r64)


def check_pool_levels(case, device):
    """att_pool_levels: the bits of three att_pool calls, and within the rule against float64."""
    b, c, sizes = case
    HF = F()
    ins = [pool_inputs(b, c, s, s, seed=1 + i) for i, s in enumerate(sizes)]
    fs = [dev_(a['f'], device, True) for a in ins]
    as_ = [dev_(a['a'], device, True) for a in ins]
    gap, sgap = HF.att_pool_levels(fs, as_)
    assert gap.shape == (3, b, c) and sgap.shape == (3, b, c)
    w1, w2 = (torch.stack([dev_(a[k], device) for a in ins]) for k in ('w1', 'w2'))
    ((gap * w1).sum() + (sgap * w2).sum()).backward()
    worst = 0.0
    for i, (a, s) in enumerate(zip(ins, sizes)):
        single = run_pool(a, device)
        got = dict(gap=np_(gap[i]), sgap=np_(sgap[i]), df=np_(fs[i].grad), da=np_(as_[i].grad))
        assert all(got[k].tobytes() == single[k].tobytes() for k in got), (case, i)
        _, r32, r64 = pool_case(b, c, s, s, seed=1 + i)
        worst = max([worst] + [judge_value(f'att_pool_levels {case} level {i}', k, got[k], r32[k], r64[k]) for k in r64])
    return worst


def check_pool_refused(device, c=8193):
    """2 C floats of LDS above 64 KB: the forward runs, the backward returns HK_ERR_UNSUPPORTED before any launch."""
    from hawkeye_amd import _lib
    HF = F()
    lib = _lib.load()
    assert 2 * c * 4 > 64 * 1024 >= 2 * (c - 1) * 4
    a, r32, r64 = pool_case(1, c, 1, 1)
    f, s = dev_(a['f'], device, True), dev_(a['a'], device, True)
    gap, sgap = HF.att_pool(f, s)
    worst = max(judge_value(f'att_pool C={c}', k, np_(v), r32[k], r64[k]) for k, v in (('gap', gap), ('sgap', sgap)))
    try:
        ((gap * dev_(a['w1'], device)).sum() + (sgap * dev_(a['w2'], device)).sum()).backward()
    except _lib.HawkeyeHipError:
        pass
    else:
        raise AssertionError(f'att_pool backward with {c} channels was not refused')
    df, da = torch.full((2 + c,), 7.0, device=device), torch.full((3,), 7.0, device=device)
    ins = [f.detach(), s.detach(), dev_(a['w1'], device), dev_(a['w2'], device), df[1:-1], da[1:-1]]
    rc = lib.hk_att_pool_bwd(*[HF.ptr(t) for t in ins], 1, c, 1, HF.stream())
    assert rc == _lib.HK_ERR_UNSUPPORTED and (df == 7).all() and (da == 7).all()
    return worst


# ------------------------------------------------------------------------------------------------------------ OSME
OSME_CASES = ((1, 1, 1, 1, 1), (3, 7, 7, 7, 2), (2, 5, 8, 8, 3), (2, 3, 5, 13, 1), (3, 2, 10, 13, 2))    # N, C, H, W, P


@functools.lru_cache(maxsize=None)
def osme_inputs(n, c, h, w, p):
    rs = np.random.RandomState(1000 * n + 100 * c + 10 * h + w + p)
    f32 = lambda v: v.astype(np.float32)
    return dict(x=f32(rs.randn(n, c, h, w)), m=f32(rs.rand(p, n, c)), wz=f32(rs.randn(n, c)), ws=f32(rs.randn(p, n, c, h, w)))


def osme_reference(a, dtype, both=True):
    x, m = (torch.from_numpy(a[k]).to(dtype).requires_grad_(True) for k in ('x', 'm'))
    z = x.mean((2, 3))
    s = m[..., None, None] * x
    total = (s * torch.from_numpy(a['ws']).to(dtype)).sum()
    if both:
        total = total + (z * torch.from_numpy(a['wz']).to(dtype)).sum()
    total.backward()
    return {k: v.detach().numpy() for k, v in dict(z=z, s=s, dx=x.grad, dm=m.grad).items()}


@functools.lru_cache(maxsize=None)
def osme_case(case, both):
    a = osme_inputs(*case)
    return a, osme_reference(a, torch.float32, both), osme_reference(a, torch.float64, both)


def check_osme_case(case, device):
    """Gradients through both outputs - by autograd over the two nodes, and by the raw backward with dz handed in - and through
    osme_scale alone, where dz arrives as NULL; dx and dm judged separately."""
    from hawkeye_amd import _lib
    HF = F()
    lib = _lib.load()
    n, c, h, w, p = case
    worst = 0.0
    for both in (True, False):
        a, r32, r64 = osme_case(tuple(case), both)
        x, m = dev_(a['x'], device, True), dev_(a['m'], device, True)
        z, s = HF.osme_gap(x), HF.osme_scale(x, m)
        assert z.shape == (n, c) and s.shape == (p, n, c, h, w)
        total = (s * dev_(a['ws'], device)).sum()
        if both:
            total = total + (z * dev_(a['wz'], device)).sum()
        total.backward()
        got = dict(z=np_(z), s=np_(s), dx=np_(x.grad), dm=np_(m.grad))
        label = f"osme {case} {'gap + scale' if both else 'scale alone'}"
        worst = max([worst] + [judge_value(label, k, got[k], r32[k], r64[k]) for k in ('z', 's', 'dx', 'dm')])
        if both:                                             # the fused form: dz joins dx inside hk_osme_scale_bwd
            dx, dm = torch.full((2 + n * c * h * w,), 7.0, device=device), torch.full((2 + p * n * c,), 7.0, device=device)
            ins = [x.detach(), m.detach(), dev_(a['ws'], device), dev_(a['wz'], device), dx[1:-1], dm[1:-1]]
            rc = lib.hk_osme_scale_bwd(*[HF.ptr(t) for t in ins], p, n, c, h * w, HF.stream())
            assert rc == _lib.HK_OK and float(dx[0]) == float(dx[-1]) == float(dm[0]) == float(dm[-1]) == 7.0
            worst = max(worst, judge_value(label + ' fused', 'dx', np_(dx[1:-1]).reshape(n, c, h, w), r32['dx'], r64['dx']),
                        judge_value(label + ' fused', 'dm', np_(dm[1:-1]).reshape(p, n, c), r32['dm'], r64['dm']))
    return worst


# ---------------------------------------------------------------------------------------------------- n-pairs loss
# (b, p, D, classes): n = 260 and 261 - the row kernel's loops take two trips, the GEMMs have a ragged k; n = 257; one
# all-zero row (the clamped normalisation, D above one trip of the normalisation's loops); empty positive / negative sets
NPAIRS_CASES = ((130, 2, 8, 9), (87, 3, 5, 4), (257, 1, 4, 3), (5, 2, 300, 2), (1, 1, 3, 1), (2, 1, 7, 1))
NPAIRS_ZERO_ROW = {(5, 2, 300, 2): 3}


def npairs_inputs(case):
    b, p, d, classes = case
    rs = np.random.RandomState(97 * b + 13 * p + d)
    x = rs.randn(b, p, d).astype(np.float32)
    y = rs.randint(0, classes, b).astype(np.int64)
    if case in NPAIRS_ZERO_ROW:
        x.reshape(b * p, d)[NPAIRS_ZERO_ROW[case]] = 0
        y[:2] = (0, 1)                                        # both classes occur
    return x, y


def npairs_reference(case, dtype):
    x, y = npairs_inputs(case)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    loss = O.npairs_loss(xt, torch.from_numpy(y))
    loss.backward()
    return dict(loss=loss.detach().numpy(), dx=xt.grad.numpy())


@functools.lru_cache(maxsize=None)
def npairs_case(case):
    return npairs_inputs(case), npairs_reference(case, torch.float32), npairs_reference(case, torch.float64)


def check_npairs_case(case, device):
    (x, y), r32, r64 = npairs_case(tuple(case))
    b, p, d, classes = case
    xt = dev_(x, device, True)
    loss = F().npairs_loss(xt, torch.from_numpy(y).to(device))
    assert loss.dim() == 0
    loss.backward()
    got = dict(loss=np_(loss), dx=np_(xt.grad))
    label = f'npairs {case}'
    worst = judge_value(label, 'loss', got['loss'], r32['loss'], r64['loss'])
    if classes == 1:                                         # no negatives anywhere: exactly zero
        assert not r64['loss'].any() and not r64['dx'].any() and not got['loss'].any() and not got['dx'].any()
    rows = lambda v: v.reshape(b * p, d)
    if tuple(case) in NPAIRS_ZERO_ROW:                       # the row divided by 1e-12 would hide every other row: judged apart
        z = NPAIRS_ZERO_ROW[tuple(case)]
        rest = np.arange(b * p) != z
        assert not rows(x)[z].any() and np.abs(rows(r64['dx'])[z]).max() > 1e6
        worst = max(worst, judge_value(label, 'dx zero row', rows(got['dx'])[z], rows(r32['dx'])[z], rows(r64['dx'])[z]),
                    judge_value(label, 'dx other rows', rows(got['dx'])[rest], rows(r32['dx'])[rest], rows(r64['dx'])[rest]))
    else:
        worst = max(worst, judge_value(label, 'dx', got['dx'], r32['dx'], r64['dx']))
    return worst
