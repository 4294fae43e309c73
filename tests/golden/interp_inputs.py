"""Inputs of the InterpParts cases (tests/golden/interp_*.npz store only their recipe - seed and sizes - and the reference's
results) and the rule by which results are judged (that of tests/golden/crossx_inputs.py).

numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions.  The grouping unit and the shaping
loss are not differentiable everywhere - the clamp of the logits at 0, the clamp of the assignment sums at 1e-5, the maximum
of a blurred map, the sort of the maxima, the absolute value - so a seed is accepted only if the inputs, evaluated here in
float64, keep away from every such place (the margins below): the reference alone is then well defined.  Computed from the
inputs, never from the code under test."""
import os

import numpy as np

from crossx_inputs import FACTOR, FLOOR, distance, judge_value  # noqa: F401  (the project's rule, one definition)

FILES = ('interp_ops.npz', 'interp_model.npz')
L_MARGIN = 1e-3                                          # no pre-clamp logit this close to 0 (the clamp case apart)
S_FACTOR = 10.0                                          # no assignment sum within this factor of 1e-5
TOP_MARGIN = 1e-3                                        # the two largest blurred values of a map
RANK_MARGIN = 1e-4                                       # two maxima of one part
ABS_MARGIN = 1e-3                                        # |log emp - log prior|
EPS = 1e-5

# (N, C, K, H, W): 63 pixels (no multiple of a tile); one part; the largest K; one pixel; the plugin's own tile
GROUP_CASES = [(3, 64, 5, 7, 9), (2, 128, 1, 4, 4), (2, 64, 32, 5, 5), (1, 64, 3, 1, 1), (2, 1024, 5, 28, 28)]
CLAMP_CASE = (2, 64, 4, 3, 5)                            # pixel CLAMP_AT of sample 0 is set equal to centre CLAMP_PART
CLAMP_AT, CLAMP_PART = 7, 1


def group_case_id(case):
    return 'N{}-C{}-K{}-{}x{}'.format(*case)


def group_arrays(seed, case):
    """The logits are -|x_p - c_k|^2 / beta_k: with |x|^2 of the order of C, as a trunk's map has it, unequal beta_k alone would
    saturate the softmax.  So x is noise of squared norm about 2 plus 0.8 times the centre of a part drawn per pixel, and the smooth
    factors stay near 0: assignments between 1e-3 and 1, every part present."""
    n, c, k, h, w = case
    rs = np.random.RandomState(int(seed))
    f = lambda *s: rs.randn(*s).astype(np.float32)
    centres = np.maximum(f(k, c) * np.float32(np.sqrt(2.0 / c)), np.float32(1e-5))        # the reference's clamped MSRA centres
    own = rs.randint(0, k, (n, h, w))
    x = f(n, c, h, w) * np.float32(1.5 / np.sqrt(c)) + np.float32(0.8) * centres[own].transpose(0, 3, 1, 2)
    return dict(x=np.ascontiguousarray(x), weight=centres, smooth=f(k) * np.float32(0.3), d_outputs_t=f(n, c, k), d_assign=f(n, k, h, w))


def group_margins(a):
    """-> (the largest pre-clamp logit numerator, the assignment sums [N,K]) in float64."""
    x, cw, s = (a[key].astype(np.float64) for key in ('x', 'weight', 'smooth'))
    n, c = x.shape[:2]
    xf = x.reshape(n, c, -1)
    raw = 2 * np.einsum('kc,ncm->nkm', cw, xf) - (xf ** 2).sum(1)[:, None] - (cw ** 2).sum(1)[None, :, None]
    beta = 1 / (1 + np.exp(-s))
    l = np.minimum(raw, 0) / beta[None, :, None]
    e = np.exp(l - l.max(1, keepdims=True))
    return raw, (e / e.sum(1, keepdims=True)).sum(2)


def group_seed_ok(a):
    raw, sums = group_margins(a)
    return float(np.abs(raw).min()) >= L_MARGIN and not ((sums > EPS / S_FACTOR) & (sums < EPS * S_FACTOR)).any()


def group_inputs(case):
    """-> float32 arrays x [N,C,H,W], weight [K,C], smooth [K], d_outputs_t [N,C,K], d_assign [N,K,H,W]."""
    case = tuple(case)
    base = 9800 + 20 * (GROUP_CASES.index(case) if case in GROUP_CASES else len(GROUP_CASES))
    for seed in range(base, base + 20):
        a = group_arrays(seed, case)
        if group_seed_ok(a):
            return a
    raise RuntimeError(f'grouping case {case}: no seed keeps away from the clamps')


def clamp_inputs():
    a = group_inputs(CLAMP_CASE)
    n, c, k, h, w = CLAMP_CASE
    a['x'].reshape(n, c, h * w)[0, :, CLAMP_AT] = a['weight'][CLAMP_PART]
    return a


# ------------------------------------------------------------------------------------------------------------- loss
# (N, K, H, W, classes), radius, std, alpha, beta, coeff: two at radius 2 (the second with a 1 x 1 blurred map), radius 0, the
# yaml's parameters, and a prior that is not constant (at beta = 0.001 every grid point rounds to 1.0f: a wrong pairing of rank
# and prior would go unnoticed)
LOSS_CASES = [((8, 5, 12, 12, 10), 2, 0.4, 1.0, 0.001, 0.5), ((4, 3, 5, 5, 7), 2, 0.4, 1.0, 0.001, 0.5), ((5, 2, 6, 7, 4), 0, 0.4, 1.0, 0.001, 0.5),
              ((16, 5, 28, 28, 200), 2, 0.4, 1.0, 0.001, 0.5), ((8, 5, 12, 12, 10), 2, 0.4, 1.0, 2.0, 0.25)]
LOSS_INPUTS = ('logits', 'assign', 'y')
LOSS_RESULTS = ('loss', 'd_logits', 'd_assign')
LOSS_TERMS = ('total', 'ce', 'shaping')


WINDOWS = ((2, 0.4), (1, 1.0), (3, 0.8))                 # (radius, std)
PRIORS = tuple((n, 1.0, b) for n in (4, 8, 16) for b in (0.001, 2.0)) + ((8, 2.0, 1.0), (8, 2.0, 3.0))      # (N, alpha, beta)


def window64(radius, std):
    r = np.arange(-radius, radius + 1)
    w = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2 * std * std))
    return w / w.sum()


def prior64(n, alpha, beta):
    """Closed forms only (the cases use alpha == 1): 1 - (1 - p)^(1 / beta) at p = (2 i + 1) / (2 N)."""
    assert alpha == 1.0
    p = (np.arange(1.0, 2 * n, 2.0).astype(np.float32) / np.float32(2 * n)).astype(np.float64)
    return 1.0 - np.power(1.0 - p, 1.0 / beta)


def blurred64(assign, radius, std):
    a = assign.astype(np.float64)
    n, k, h, w = a.shape
    win = window64(radius, std)
    out = np.zeros((n, k, h - 2 * radius, w - 2 * radius))
    for u in range(2 * radius + 1):
        for v in range(2 * radius + 1):
            out += win[u, v] * a[:, :, u:u + h - 2 * radius, v:v + w - 2 * radius]
    return out


def loss_arrays(seed, shape, radius):
    n, k, h, w, classes = shape
    rs = np.random.RandomState(int(seed))
    y = rs.randint(0, classes, n)
    logits = rs.randn(n, classes)
    logits[np.arange(n), y] += float(round(np.log(classes) + 0.7)) * (0.5 + rs.rand(n))
    # a map: noise below 0.6 u and one peak of height u at a random pixel that a window is centred on, u in [0.15, 0.95] per
    # (sample, part) - the maximum of the blurred map is then decided by a clear margin, and the maxima of a part are spread
    u = 0.15 + 0.8 * rs.rand(n, k, 1, 1)
    assign = 0.6 * u * rs.rand(n, k, h, w)
    peak = rs.randint(radius, h - radius, (n, k)) * w + rs.randint(radius, w - radius, (n, k))
    flat = assign.reshape(n, k, h * w)
    np.put_along_axis(flat, peak[:, :, None], u.reshape(n, k, 1), axis=2)
    return logits.astype(np.float32), assign.astype(np.float32), y.astype(np.int64)


def loss_seed_ok(assign, radius, std, alpha, beta):
    b = blurred64(assign, radius, std)
    n, k = b.shape[:2]
    flat = np.sort(b.reshape(n, k, -1), axis=2)
    if flat.shape[2] > 1 and float((flat[:, :, -1] - flat[:, :, -2]).min()) < TOP_MARGIN:
        return False
    emp = np.sort(flat[:, :, -1], axis=0)
    if n > 1 and float(np.diff(emp, axis=0).min()) < RANK_MARGIN:
        return False
    gap = np.abs(np.log(emp + EPS) - np.log(prior64(n, alpha, beta) + EPS)[:, None])
    return float(gap.min()) >= ABS_MARGIN


def loss_inputs(k_case, seed=None):
    """-> (logits [N,classes], assign [N,K,H,W], labels [N], the accepted seed)."""
    shape, radius, std, alpha, beta, _ = LOSS_CASES[k_case]
    base = 9900 + 200 * k_case
    for cand in ([int(seed)] if seed is not None else range(base, base + 200)):
        arrays = loss_arrays(cand, shape, radius)
        if loss_seed_ok(arrays[1], radius, std, alpha, beta):
            return arrays + (cand,)
    raise RuntimeError(f'loss case {k_case}: no seed keeps the maxima apart')


# the whole model with short `layers`: one block per stage, a 4 x 4 layer-3 map
MODEL_CASE = dict(B=2, size=64, layers=(1, 1, 1), classes=7, parts=5, init_seed=1277)
MODEL_OUTPUTS = ('logits', 'att', 'assign')
MODEL_MODES = ('eval', 'train')


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


def load_loss_cases(z=None):
    z = z or load()
    cases = []
    for k, (shape, radius, std, alpha, beta, coeff) in enumerate(LOSS_CASES):
        recipe = [int(v) for v in z[f'l{k}_recipe']]
        assert recipe[1:] == list(shape) + [radius], recipe
        case = dict(zip(LOSS_INPUTS, loss_inputs(k, recipe[0])[:3]), k=k, shape=shape, radius=radius, std=std, alpha=alpha, beta=beta,
                    coeff=coeff)
        for prec in ('f32', 'f64'):
            for name in LOSS_RESULTS:
                case[f'{name}_{prec}'] = z[f'l{k}_{name}_{prec}']
        cases.append(case)
    return cases


def load_model_case(z=None):
    z = z or load()
    seed, b, size, init_seed = (int(v) for v in z['model_recipe'])
    assert dict(MODEL_CASE, B=b, size=size, init_seed=init_seed) == MODEL_CASE
    case = dict(MODEL_CASE, seed=seed, images=model_images(seed, b, size))
    for key in z:
        if key.startswith('model_') and key != 'model_recipe':
            case[key[len('model_'):]] = z[key]
    return case


def loss_case_id(case):
    return '{}-N{}-K{}-{}x{}-r{}-b{}'.format(case['k'], *case['shape'][:4], case['radius'], case['beta'])


def judge_loss(case, got, label=''):
    """got: dict of numpy arrays named as LOSS_RESULTS."""
    label = f'{label} loss case {loss_case_id(case)}'
    worst = 0.0
    for i, name in enumerate(LOSS_TERMS):
        worst = max(worst, judge_value(label, name, got['loss'][i], case['loss_f32'][i], case['loss_f64'][i]))
    for name in LOSS_RESULTS[1:]:
        worst = max(worst, judge_value(label, name, got[name], case[f'{name}_f32'], case[f'{name}_f64']))
    return worst
