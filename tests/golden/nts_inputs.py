"""Inputs of the NTS-Net cases (tests/golden/nts_*.npz store only their recipe - seed and sizes -, the reference's anchor
tables and the reference's results) and the rule by which results are judged.

numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions.  The proposal scores of an NMS
case are a permutation of distinct, evenly spaced values: no rounding can reorder them, so indices and boxes are
compared exactly."""
import os

import numpy as np

CLASSES = 200
TOPN = 6
IOU = 0.25
FILES = ('nts_ops.npz', 'nts_model.npz')

# (image size, B, kind): 'random' - a plain permutation; 'overlap' - the highest scores sit on the anchors that overlap one
# anchor most; 'quarter' - the winner has partners at IoU exactly 0.25, which hold the next-highest scores (they must go:
# the survival test is a strict <)
NMS_CASES = [(224, 1, 'random'), (224, 3, 'random'), (448, 1, 'random'), (448, 3, 'random'), (224, 1, 'overlap'), (448, 1, 'overlap'),
             (224, 1, 'quarter'), (448, 3, 'quarter')]
# images [B,C,H,W], N boxes per image, padding, output size
CROP_CASES = [dict(B=2, C=3, H=40, W=36, N=3, pad=16, out=(8, 12)), dict(B=2, C=3, H=40, W=36, N=3, pad=16, out=(1, 1))]
# y0, x0, y1, x1 in image coordinates: inside ; into the padding on the low side ; one pixel high //
# past the padded extent on the high side (clipped) ; the whole image ; one pixel wide
CROP_BOXES = [[[5, 4, 30, 28], [-10, -8, 20, 22], [12, 7, 13, 30]],
              [[30, 20, 50, 60], [0, 0, 40, 36], [3, 10, 25, 11]]]
LOSS_CASES = [(1, 2, 5), (3, 6, 200), (4, 6, 200), (2, 3, 70)]          # B, N, C
MODEL_CASE = dict(B=2, size=224, init_seed=951, proposal_num=6, cat_num=4)


def iou_matrix_row(anchors, w):
    """float64 IoU of every anchor with anchor w: corner differences without + 1, intersection 0 when a side is negative."""
    a = anchors.astype(np.float64)
    lo = np.maximum(a[:, :2], a[w, :2])
    hi = np.minimum(a[:, 2:], a[w, 2:])
    side = hi - lo
    inter = np.where((side < 0).any(1), 0.0, side[:, 0] * side[:, 1])
    area = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (area + area[w] - inter)


def quarter_partners(anchors, w):
    """Anchors whose IoU with anchor w is exactly 1/4, decided in integers (4 x intersection == union)."""
    a = anchors.astype(np.int64)
    lo = np.maximum(a[:, :2], a[w, :2])
    hi = np.minimum(a[:, 2:], a[w, 2:])
    side = hi - lo
    inter = np.where((side < 0).any(1), 0, side[:, 0] * side[:, 1])
    area = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    return np.where(4 * inter == area + area[w] - inter)[0]


def nms_scores(seed, b, kind, anchors):
    """-> scores [b, A] float32, each row a permutation of (k - A / 2) / 64, k < A: distinct, exactly representable."""
    rs = np.random.RandomState(int(seed))
    a = len(anchors)
    values = ((np.arange(a) - a // 2) / 64.0).astype(np.float32)           # ascending
    out = np.empty((b, a), dtype=np.float32)
    for i in range(b):
        order = rs.permutation(a)                                          # order[k]: the anchor that gets the k-th highest score
        if kind == 'overlap':
            w = int(rs.randint(a))
            near = np.argsort(-iou_matrix_row(anchors, w), kind='stable')[:24]
            order = np.concatenate([near, order[~np.isin(order, near)]])
        elif kind == 'quarter':
            cands = [w for w in rs.permutation(a) if len(quarter_partners(anchors, w)) >= 2]
            w = int(cands[0])
            first = np.concatenate([[w], quarter_partners(anchors, w)])
            order = np.concatenate([first, order[~np.isin(order, first)]])
        out[i, order] = values[::-1]
    return out


def nms_trace(scores, anchors, topn=TOPN, thresh=IOU):
    """One image's greedy NMS in float64, written from the published rule: the highest live score (equal scores: the
    highest index), then only anchors with IoU < thresh stay live; an empty live set repeats the last pick.
    -> (index [topn], gaps [topn]: each pick's score minus the best other live score, inf without a rival)."""
    s = np.asarray(scores, dtype=np.float64)
    live = np.ones(len(s), dtype=bool)
    index, gaps, last = [], [], 0
    for _ in range(topn):
        ids = np.where(live)[0]
        if len(ids) == 0:
            index.append(last)
            gaps.append(np.inf)
            continue
        best = s[ids].max()
        w = int(ids[s[ids] == best].max())
        rest = s[ids[ids != w]]
        gaps.append(best - rest.max() if len(rest) else np.inf)
        index.append(w)
        last = w
        live &= iou_matrix_row(anchors, w) < thresh
        live[w] = False
    return np.array(index, dtype=np.int64), np.array(gaps)


def crop_images(seed, b, c, h, w):
    return np.random.RandomState(int(seed)).randn(b, c, h, w).astype(np.float32)


def loss_inputs(seed, b, n, c):
    """-> raw, concat [b,c], part [b,n,c], prob [b,n] float32, labels [b] int64.  The label's logit is raised so that its
    probability is of the order of a half (a trained net, not 1 / c); the scores are wide enough for hinge arguments on
    both sides of zero."""
    rs = np.random.RandomState(int(seed))
    y = rs.randint(0, c, b)
    plant = float(round(np.log(c) + 0.7))
    raw, cat, part = rs.randn(b, c), rs.randn(b, c), rs.randn(b, n, c)
    raw[np.arange(b), y] += plant
    cat[np.arange(b), y] += plant
    part[np.arange(b), :, y] += plant * rs.rand(b, n)
    prob = 1.2 * rs.randn(b, n)
    return raw.astype(np.float32), cat.astype(np.float32), part.astype(np.float32), prob.astype(np.float32), y.astype(np.int64)


def model_images(seed, b, size):
    return np.random.RandomState(int(seed)).randn(b, 3, size, size).astype(np.float32)


def load(path=None):
    here = path or os.path.dirname(os.path.abspath(__file__))
    out = {}
    for name in FILES:
        with np.load(os.path.join(here, name)) as z:
            for k in z.files:
                assert k not in out, k
                out[k] = z[k]
    return out


def load_nms_cases(z=None):
    z = z or load()
    cases = []
    for k, (size, b, kind) in enumerate(NMS_CASES):
        seed, zsize, zb = (int(v) for v in z[f'n{k}_recipe'])
        assert (zsize, zb) == (size, b)
        anchors = z[f'anchors_{size}']
        cases.append(dict(k=k, size=size, B=b, kind=kind, anchors=anchors, scores=nms_scores(seed, b, kind, anchors),
                          index=z[f'n{k}_index'], boxes=z[f'n{k}_boxes']))
    return cases


def load_crop_cases(z=None):
    z = z or load()
    cases = []
    for k, c in enumerate(CROP_CASES):
        seed = int(z[f'c{k}_recipe'][0])
        cases.append(dict(c, k=k, images=crop_images(seed, c['B'], c['C'], c['H'], c['W']), boxes=np.array(CROP_BOXES, dtype=np.int32),
                          out_f32=z[f'c{k}_out_f32'], out_f64=z[f'c{k}_out_f64']))
    return cases


LOSS_RESULTS = ('loss', 'draw', 'dconcat', 'dpart', 'dprob')          # loss [5] = total, raw CE, concat CE, part-class CE, rank


def load_loss_cases(z=None):
    z = z or load()
    cases = []
    for k, (b, n, c) in enumerate(LOSS_CASES):
        seed, zb, zn, zc = (int(v) for v in z[f'l{k}_recipe'])
        assert (zb, zn, zc) == (b, n, c)
        raw, cat, part, prob, y = loss_inputs(seed, b, n, c)
        case = dict(k=k, B=b, N=n, C=c, raw=raw, concat=cat, part=part, prob=prob, y=y, indicator=z[f'l{k}_indicator'])
        for prec in ('f32', 'f64'):
            for name in LOSS_RESULTS:
                case[f'{name}_{prec}'] = z[f'l{k}_{name}_{prec}']
        cases.append(case)
    return cases


def load_model_case(z=None):
    z = z or load()
    seed, b, size, init_seed = (int(v) for v in z['model_recipe'])
    case = dict(MODEL_CASE, seed=seed, images=model_images(seed, b, size), top_n_index=z['model_top_n_index'])
    for prec in ('f32', 'f64'):
        for name in ('raw_logits', 'concat_logits', 'part_logits', 'top_n_prob'):
            case[f'{name}_{prec}'] = z[f'model_{name}_{prec}']
    return case


def nms_case_id(case):
    return f"{case['k']}-{case['size']}-B{case['B']}-{case['kind']}"


def loss_case_id(case):
    return f"{case['k']}-B{case['B']}-N{case['N']}-C{case['C']}"


# Tolerance - the rule of tests/golden/apinet_inputs.py and peer_inputs.py: a result's distance from the float64 reference
# may be at most FACTOR x the float32 reference's own distance from it, with a floor of FLOOR; norm-wise relative distance
# for tensors, relative distance for scalars.
FACTOR, FLOOR = 4.0, 1e-6


def distance(got, ref64):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    den = np.linalg.norm(np.atleast_1d(ref64))
    num = np.linalg.norm(np.atleast_1d(got - ref64))
    return float(num) if den == 0 else float(num / den)


def judge_value(label, name, got, ref32, ref64):
    """Asserts the rule for one tensor or scalar; prints and returns the ratio distance / allowed."""
    d, d32 = distance(got, ref64), distance(ref32, ref64)
    allowed = max(FACTOR * d32, FLOOR)
    print(f'nts {label} {name}: distance {d:.3e}, reference fp32 {d32:.3e}, allowed {allowed:.3e}, ratio {d / allowed:.3f}')
    assert d <= allowed, (label, name, d, d32)
    return d / allowed


LOSS_TERMS = ('total', 'raw', 'concat', 'partcls', 'rank')


def judge_loss(case, loss, draw, dconcat, dpart, dprob, label=''):
    """Values by the rule above; a term that is exactly zero in float64 must be exactly zero.  numpy inputs."""
    label = f'{label} loss case {loss_case_id(case)}'
    worst = 0.0
    for i, name in enumerate(LOSS_TERMS):
        if case['loss_f64'][i] == 0:
            assert loss[i] == 0, (label, name, loss[i])
            continue
        worst = max(worst, judge_value(label, name, loss[i], case['loss_f32'][i], case['loss_f64'][i]))
    for name, got in (('draw', draw), ('dconcat', dconcat), ('dpart', dpart), ('dprob', dprob)):
        if not np.any(case[f'{name}_f64']):
            assert not np.any(got), (label, name)
            continue
        worst = max(worst, judge_value(label, name, got, case[f'{name}_f32'], case[f'{name}_f64']))
    return worst
