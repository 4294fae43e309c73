"""Inputs, seeds, preconditions and float64 references of the MGE-CNN checks (tests/mge_ops.py); also read by
tools/gen_mge_golden.py, which writes the fixtures tests/golden/mge_*.  Not a test module.

Seeds are fixed here.  Each was found on the CPU by walking the seeds from 0 until the case's precondition held
(`find_pool_seed`, `find_cam_seed`); the checks assert the precondition again, they never skip.

Part pool.  x ~ N(0,1), weight ~ N(0,1) / sqrt(Cin), bias ~ 0.3 N(0,1), g ~ N(0,1).  With Cin = 1024 the forward bound
(Cin + 8) 2^-24 (|b| + sum |w x|) is about 1.2e-3 of a response's standard deviation, and among thousands of (image, channel)
pairs some top-two gap falls below that for every seed; there each pixel p carries a code u_p ~ N(0,1)^Cin (x[b,:,p] += u_p) and
each channel o one pixel's code (w_o += u_t(o) / sqrt(Cin), t(o) = (7 o + 3) mod HW): the coded pixel answers with about
sqrt(Cin) = 32 against a noise of about 2, so the winner is known and every gap is wide, while every channel of x and w still
carries O(1) random data into every sum."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23

# ------------------------------------------------------------------------------------------------------- part pool
# (B, Cin, Cout, H, W)
POOL_CASES = ((2, 32, 80, 5, 7), (3, 96, 80, 9, 9), (2, 64, 130, 8, 8), (1, 1024, 72, 4, 4))
POOL_CASE_YAML = (2, 1024, 2000, 14, 14)                   # GPU tier only
POOL_SEEDS = {(2, 32, 80, 5, 7): 0, (3, 96, 80, 9, 9): 0, (2, 64, 130, 8, 8): 0, (1, 1024, 72, 4, 4): 0, POOL_CASE_YAML: 0}


def pool_case_id(case):
    return 'B{}_Cin{}_Cout{}_{}x{}'.format(*case)


def pool_arrays(case, seed):
    b, cin, cout, h, w = case
    rs = np.random.RandomState(1000 + seed)
    x = rs.randn(b, cin, h * w)
    wt = rs.randn(cout, cin)
    if cin >= 1024:                                        # the coded recipe of the module's docstring
        codes = rs.randn(cin, h * w)
        x = x + codes[None]
        wt = wt + codes[:, (7 * np.arange(cout) + 3) % (h * w)].T
    wt = wt / np.sqrt(cin)
    bias, g = 0.3 * rs.randn(cout), rs.randn(b, cout)
    return dict(x=x.reshape(b, cin, h, w).astype(np.float32), weight=wt.astype(np.float32), bias=bias.astype(np.float32),
                g=g.astype(np.float32))


def pool_float64(a):
    """The float64 restatement: the interior responses [B,Cout,HW], the forward bound at each, pooled and the argmax (-1: the
    border ring), and the smallest distance of any (image, channel) from a different decision."""
    x, wt, bias = (a[k].astype(np.float64) for k in ('x', 'weight', 'bias'))
    b, cin, h, w = x.shape
    x = x.reshape(b, cin, h * w)
    resp = np.einsum('oc,bcp->bop', wt, x)
    bound = (cin + 8) * EPS24 * (np.abs(bias)[None, :, None] + np.einsum('oc,bcp->bop', np.abs(wt), np.abs(x)))
    border_bound = (cin + 8) * EPS24 * np.abs(bias)[None, :]
    best = resp.argmax(2)
    top = np.take_along_axis(resp, best[..., None], 2)[..., 0]
    inside = top > 0
    pooled = np.maximum(bias[None] + np.where(inside, top, 0.0), 0.0)
    argmax = np.where(inside, best, -1)
    return dict(resp=resp, bound=bound, border_bound=border_bound, pooled=pooled, argmax=argmax, top=top, best=best)


def pool_margin(a, r=None):
    """min over (image, channel) of (top-two gap, the border counted as a candidate at 0, and |bias + max| for the ReLU) minus the
    forward bound there: positive means that fp32 in any summation order decides as float64 does."""
    r = r or pool_float64(a)
    resp, bound = r['resp'], r['bound']
    second = np.sort(resp, 2)[..., -2] if resp.shape[2] > 1 else np.full(r['top'].shape, -np.inf)
    top_bound = np.take_along_axis(bound, r['best'][..., None], 2)[..., 0]
    gap = np.minimum(r['top'] - second, np.abs(r['top']))              # the next pixel, and the border's 0
    relu_gap = np.abs(a['bias'].astype(np.float64)[None] + np.maximum(r['top'], 0.0))
    return float(np.min(np.minimum(gap, relu_gap) - 2.0 * top_bound))


def find_pool_seed(case, tries=64):
    for seed in range(tries):
        if pool_margin(pool_arrays(case, seed)) > 0:
            return seed
    raise RuntimeError(f'no seed for {case}')


@functools.lru_cache(maxsize=None)
def pool_case(case):
    """-> (arrays, float64 results); computed once and shared, never modified."""
    a = pool_arrays(case, POOL_SEEDS[tuple(case)])
    r = pool_float64(a)
    for v in list(a.values()) + [v for v in r.values() if isinstance(v, np.ndarray)]:
        v.setflags(write=False)
    return a, r


def pool_reference_grads(a):
    """Autograd of the reference's op sequence in float64: conv6 with padding 1, ReLU, the global max pool, times g."""
    x, wt, bias, g = (torch.from_numpy(a[k].astype(np.float64)) for k in ('x', 'weight', 'bias', 'g'))
    wt, bias = wt.requires_grad_(True), bias.requires_grad_(True)
    cout, cin = wt.shape
    pooled = TF.adaptive_max_pool2d(TF.relu(TF.conv2d(x, wt.view(cout, cin, 1, 1), bias, 1, 1)), 1).flatten(1)
    (pooled * g).sum().backward()
    return pooled.detach().numpy(), wt.grad.numpy(), bias.grad.numpy()


def pool_gather64(a, pooled, argmax):
    """dW, db and the per-element sums of |terms| from a given (pooled, argmax), in float64."""
    x, g = a['x'].astype(np.float64), a['g'].astype(np.float64)
    b, cin, h, w = x.shape
    x = x.reshape(b, cin, h * w)
    live = (pooled > 0)
    gd = g * live
    picked = np.take_along_axis(x, np.maximum(argmax, 0)[:, None, :], 2)          # [B,Cin,Cout]
    terms = (gd * (argmax >= 0))[:, None, :] * picked
    return terms.sum(0).T, gd.sum(0), np.abs(terms).sum(0).T, np.abs(gd).sum(0)


# ------------------------------------------------------------------------------------------------------- CAM box
# (B, C, h, w, S); classes
CAM_CASES = ((3, 16, 3, 3, 96), (2, 70, 7, 7, 224), (1, 2048, 7, 7, 224))
CAM_RATES = (0.2, 0.3)
CAM_CLASSES = 5
CAM_SEEDS = {((3, 16, 3, 3, 96), 0.2): 0, ((3, 16, 3, 3, 96), 0.3): 0, ((2, 70, 7, 7, 224), 0.2): 0, ((2, 70, 7, 7, 224), 0.3): 0,
             ((1, 2048, 7, 7, 224), 0.2): 1, ((1, 2048, 7, 7, 224), 0.3): 0}


def cam_case_id(case):
    return 'B{}_C{}_{}x{}_S{}'.format(*case)


def cam_arrays(case, seed):
    b, c, h, w, s = case
    rs = np.random.RandomState(2000 + seed)
    cy, cx = rs.uniform(0.25, 0.75, (2, b, 1, 1, 1)) * np.array([h - 1, w - 1]).reshape(2, 1, 1, 1, 1)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    bump = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * (0.22 * max(h, w)) ** 2))      # one hot region per image: an interior box
    conv5 = (0.5 + np.maximum(rs.randn(b, c, h, w), 0.0)) * (0.02 + bump)                      # a post-ReLU map
    cls_weight = rs.randn(CAM_CLASSES, c) / np.sqrt(c)
    index = rs.randint(0, CAM_CLASSES, b)
    return dict(conv5=conv5.astype(np.float32), cls_weight=cls_weight.astype(np.float32), index=index.astype(np.int32))


def cam_float64(a, rate, s):
    """get_bbox's arithmetic (MGE.py:48-72) in float64 -> boxes [B,1,4] = y0, x0, y1, x1 as the reference slices them (the whole
    image where its slice is empty, where the map is constant or nothing reaches the rate), and the smallest distance of any row or
    column maximum of the normalised map from `rate`, in units of the precondition's margin."""
    conv5, wt = torch.from_numpy(a['conv5'].astype(np.float64)), torch.from_numpy(a['cls_weight'].astype(np.float64))
    index = torch.from_numpy(a['index'].astype(np.int64))
    b, c, h, w = conv5.shape
    weights = torch.relu(wt[index]) / (h * w)
    cam = (conv5.view(b, c, -1) * weights.unsqueeze(-1)).sum(1).view(b, 1, h, w)
    boxes, closest = [], np.inf
    for k in range(b):
        if not float(cam[k].max() - cam[k].min()) > 0:
            boxes.append([0, 0, s, s])
            continue
        up = TF.interpolate(cam[k:k + 1], size=(s, s), mode='bilinear', align_corners=True)[0, 0]
        rng = float(up.max() - up.min())                   # (not the CAM's own range: interior cells need not be sampled)
        norm = (up - up.min()) / rng
        margin = 4 * (c + 16) * EPS24 * float(cam[k].abs().max()) / rng
        lines = torch.cat([norm.max(1)[0], norm.max(0)[0]])
        closest = min(closest, float((lines - rate).abs().min()) / margin)
        hit = (norm >= rate).nonzero()
        if hit.numel() == 0:
            boxes.append([0, 0, s, s])
            continue
        y1, x1 = hit.min(0)[0].tolist()
        y2, x2 = hit.max(0)[0].tolist()
        boxes.append([0, 0, s, s] if x1 == x2 or y1 == y2 else [y1, x1, y2, x2])
    return np.array(boxes, dtype=np.int32).reshape(b, 1, 4), closest


def find_cam_seed(case, rate, tries=256):
    for seed in range(tries):
        if cam_float64(cam_arrays(case, seed), rate, case[4])[1] >= 1.0:
            return seed
    raise RuntimeError(f'no seed for {case} {rate}')


@functools.lru_cache(maxsize=None)
def cam_case(case, rate):
    a = cam_arrays(case, CAM_SEEDS[tuple(case), rate])
    boxes, closest = cam_float64(a, rate, case[4])
    return a, boxes, closest


# ------------------------------------------------------------------------------------------------------- loss
LOSS_KS, LOSS_BS, LOSS_CS = (1, 10, 16), (1, 5), (3, 200)
LOSS_CASES = tuple((k, b, c) for k in LOSS_KS for b in LOSS_BS for c in LOSS_CS)
LOSS_GOLDEN_CASES = ((10, 5, 3), (10, 1, 200))             # stored from the reference trainer's arithmetic (mge_ops.npz)
SMOOTHING = 0.1


def loss_case_id(case):
    return 'K{}_B{}_C{}'.format(*case)


def loss_arrays(case):
    k, b, c = case
    rs = np.random.RandomState(3000 + 97 * k + 13 * b + c)
    return [(2.0 * rs.randn(b, c)).astype(np.float32) for _ in range(k)], rs.randint(0, c, b).astype(np.int64)


def loss_reference(logits, labels, dtype):
    """Examples/MGE_CNN.py:43-45 restated: one CrossEntropyLoss(label_smoothing=0.1) per tensor, sum(losses) / len(losses)."""
    crit = torch.nn.CrossEntropyLoss(label_smoothing=SMOOTHING)
    leaves = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in logits]
    y = torch.from_numpy(labels)
    losses = [crit(t, y) for t in leaves]
    total = sum(losses) / len(losses)
    total.backward()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    return dict(loss=np.array([total.item()] + [t.item() for t in losses], dtype=np_dtype), grads=[t.grad.numpy() for t in leaves])


# ------------------------------------------------------------------------------------------------------- model
# a short trunk (one block per stage, three in layer4: Grad-CAM's target layer is its block "2") on 96 x 96 images (a 6 x 6 layer-3 and a 3 x 3 layer-4 map)
MODEL_CASE = dict(layers=(1, 1, 1, 3), classes=4, size=96, B=2, init_seed=31, box_thred=0.6, labels=(1, 3))


TRAIN_GRADS = ('classifier.fc.weight', 'classifier_box.fc.weight', 'classifier_box_2.fc.bias', 'conv6.weight', 'conv6.bias', 'conv6_1.weight',
               'conv6_2.weight', 'cls_part.fc.weight', 'cls_cat_1.fc.weight', 'cls_cat_2.fc.weight', 'cls_gate.1.fc.weight')


def grad_sample(g):
    """Every n-th element of a gradient, at most 512 of them: what the fixture stores of it."""
    flat = np.ascontiguousarray(g).reshape(-1)
    return flat[::-(-flat.size // 512)]


def model_images(seed, b, size):
    rs = np.random.RandomState(seed)
    return rs.randn(b, 3, size, size).astype(np.float32)


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def state_dict_keys():
    return json.load(open(os.path.join(GOLDEN, 'mge_state_dict.json')))
