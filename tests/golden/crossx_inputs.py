"""Inputs of the CrossX cases (tests/golden/crossx_*.npz store only their recipe - seed and sizes - and the reference's
results) and the rule by which results are judged.

numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions.  A multi-excitation case takes
the first seed from its base at which (1) no nonzero ReLU argument - `out * gate + res` for every part, `out + res` - is
closer to zero than RELU_MARGIN in float64 and (2) float32 and float64 arithmetic pick the same arg-max position in every
part row; both are computed here from the inputs, never from the code under test."""
import os

import numpy as np

CLASSES = 200
FILES = ('crossx_ops.npz', 'crossx_model.npz')
RELU_MARGIN = 1e-5

# (P, N, C, HW, pool).  196 and 784 are the model's rows; 49, 7 and 1 are no multiple of 4; 1000 is longer than a workgroup
ME_CASES = [(2, 2, 8, 196, 'avg'), (2, 1, 6, 784, 'max'), (3, 1, 5, 49, 'max'), (1, 2, 3, 7, 'avg'), (3, 2, 2, 1, 'max'), (2, 1, 3, 1000, 'max')]
# (N, C, Hi, Wi, Ho, Wo)
UP_CASES = [(2, 3, 14, 14, 28, 28), (1, 2, 7, 7, 28, 28), (1, 5, 28, 28, 28, 28), (1, 1, 3, 5, 6, 5)]
UP_REFUSED = (1, 1, 5, 5, 28, 28)
# (B, K, P, (C_ulti, C_plty, C_cmbn)); the last one is the yaml's
LOSS_CASES = [(2, 3, 2, (8, 4, 4)), (3, 200, 3, (70, 33, 33)), (8, 200, 2, (2048, 1024, 1024))]
GAMMA = (0.5, 0.25, 0.5)
MODEL_CASE = dict(P=2, B=2, size=448, init_seed=977)


def me_arguments(out, res, gates, dtype):
    """-> main argument [N,C,HW], part arguments [P,N,C,HW] in `dtype` arithmetic (the product rounded, then the sum)."""
    o, r, g = out.astype(dtype), res.astype(dtype), gates.astype(dtype)
    return o + r, o[None] * g[..., None] + r[None]


def me_seed_ok(out, res, gates):
    m64, p64 = me_arguments(out, res, gates, np.float64)
    m32, p32 = me_arguments(out, res, gates, np.float32)
    for a in (m64, p64):
        nz = np.abs(a[a != 0])
        if nz.size and nz.min() < RELU_MARGIN:
            return False
    if not (np.array_equal(m32 > 0, m64 > 0) and np.array_equal(p32 > 0, p64 > 0)):
        return False
    return np.array_equal(np.maximum(p32, 0).argmax(-1), np.maximum(p64, 0).argmax(-1))


def me_inputs(case, base_seed=None):
    """-> dict of float32 arrays: out, res [N,C,HW], gates [P,N,C] (sigmoids), the upstream gradients d_main [N,C,HW],
    d_parts [P,N,C,HW], d_pooled [P,N,C], dz [N,C], and the seed that was accepted."""
    p, n, c, hw, _ = case
    base = 7000 + 100 * ME_CASES.index(tuple(case)) if base_seed is None else base_seed
    for seed in range(base, base + 100):
        rs = np.random.RandomState(seed)
        out, res = rs.randn(n, c, hw).astype(np.float32), rs.randn(n, c, hw).astype(np.float32)
        gates = (1 / (1 + np.exp(-rs.randn(p, n, c)))).astype(np.float32)
        if me_seed_ok(out, res, gates):
            break
    else:
        raise RuntimeError(f'ME case {case}: no seed meets the margins')
    f = lambda *s: rs.randn(*s).astype(np.float32)
    return dict(out=out, res=res, gates=gates, d_main=f(n, c, hw), d_parts=f(p, n, c, hw), d_pooled=f(p, n, c), dz=f(n, c), seed=seed)


def up_inputs(case):
    n, c, hi, wi, ho, wo = case
    rs = np.random.RandomState(7900 + hi * wo)
    return rs.randn(n, c, ho, wo).astype(np.float32), rs.randn(n, c, hi, wi).astype(np.float32), rs.randn(n, c, ho, wo).astype(np.float32)


def loss_inputs(seed, b, k, p, widths):
    """-> ulti, plty, cmbn [b,k] float32, labels [b] int64, three feature arrays [p,b,C_l] float32.  The label's logit is
    raised so that its probability is of the order of a half; the features are pooled ReLU outputs: non-negative, a
    part-specific profile plus noise, so the parts correlate neither fully nor not at all."""
    rs = np.random.RandomState(int(seed))
    y = rs.randint(0, k, b)
    plant = float(round(np.log(k) + 0.7))
    logits = []
    for _ in range(3):
        l = rs.randn(b, k)
        l[np.arange(b), y] += plant * (0.5 + rs.rand(b))
        logits.append(l.astype(np.float32))
    feats = []
    for c in widths:
        profile = np.abs(rs.randn(p, 1, c))
        feats.append((profile + 0.7 * np.abs(rs.randn(p, b, c))).astype(np.float32))
    return logits[0], logits[1], logits[2], y.astype(np.int64), feats[0], feats[1], feats[2]


def regulariser_closed_form(x, gamma):
    """float64 value of gamma / B^2 [sum_i (B^2 - |s_i|^2) + sum_{i<j} s_i . s_j], s_i = sum_b x_i[b] / |x_i[b]|, x [P,B,C]."""
    x = np.asarray(x, dtype=np.float64)
    p, b, _ = x.shape
    s = (x / np.linalg.norm(x, axis=2, keepdims=True)).sum(1)
    total = sum(b * b - s[i] @ s[i] for i in range(p)) + sum(s[i] @ s[j] for i in range(p) for j in range(i + 1, p))
    return gamma * total / (b * b)


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


LOSS_RESULTS = ('loss', 'd_ulti', 'd_plty', 'd_cmbn', 'df_ulti', 'df_plty', 'df_cmbn')
LOSS_TERMS = ('total', 'cls', 'kl', 'reg_ulti', 'reg_plty', 'reg_cmbn')
LOSS_INPUTS = ('ulti', 'plty', 'cmbn', 'y', 'f_ulti', 'f_plty', 'f_cmbn')


def load_loss_cases(z=None):
    z = z or load()
    cases = []
    for k, (b, kk, p, widths) in enumerate(LOSS_CASES):
        recipe = [int(v) for v in z[f'l{k}_recipe']]
        assert recipe[1:] == [b, kk, p, *widths], recipe
        case = dict(zip(LOSS_INPUTS, loss_inputs(recipe[0], b, kk, p, widths)), k=k, B=b, K=kk, P=p, widths=widths)
        for prec in ('f32', 'f64'):
            for name in LOSS_RESULTS:
                case[f'{name}_{prec}'] = z[f'l{k}_{name}_{prec}']
        cases.append(case)
    return cases


MODEL_OUTPUTS = ('ulti_logits', 'plty_logits', 'cmbn_logits', 'ulti_ftrs', 'plty_ftrs', 'cmbn_ftrs')


def load_model_case(z=None):
    z = z or load()
    seed, p, b, size, init_seed = (int(v) for v in z['model_recipe'])
    assert dict(P=p, B=b, size=size, init_seed=init_seed) == MODEL_CASE
    case = dict(MODEL_CASE, seed=seed, images=model_images(seed, b, size))
    for prec in ('f32', 'f64'):
        for name in MODEL_OUTPUTS:
            case[f'{name}_{prec}'] = z[f'model_{name}_{prec}']
    return case


def me_case_id(case):
    return 'P{}-N{}-C{}-HW{}-{}'.format(*case)


def loss_case_id(case):
    return f"{case['k']}-B{case['B']}-K{case['K']}-P{case['P']}-C{case['widths'][0]}"


# Tolerance - the rule of tests/golden/nts_inputs.py: a result's distance from the float64 reference may be at most
# FACTOR x the float32 reference's own distance from it, with a floor of FLOOR; norm-wise relative distance for tensors,
# relative distance for scalars.  A quantity that is exactly zero in float64 must be exactly zero.
FACTOR, FLOOR = 4.0, 1e-6


def distance(got, ref64):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    den = np.linalg.norm(np.atleast_1d(ref64))
    num = np.linalg.norm(np.atleast_1d(got - ref64))
    return float(num) if den == 0 else float(num / den)


def judge_value(label, name, got, ref32, ref64):
    """Asserts the rule for one tensor or scalar; prints and returns the ratio distance / allowed."""
    assert np.shape(got) == np.shape(ref64), (label, name, np.shape(got), np.shape(ref64))
    if not np.any(ref64):
        assert not np.any(got), (label, name)
        return 0.0
    d, d32 = distance(got, ref64), distance(ref32, ref64)
    allowed = max(FACTOR * d32, FLOOR)
    print(f'crossx {label} {name}: distance {d:.3e}, reference fp32 {d32:.3e}, allowed {allowed:.3e}, ratio {d / allowed:.3f}')
    assert d <= allowed, (label, name, d, d32)
    return d / allowed


def judge_loss(case, got, label=''):
    """got: dict of numpy arrays named as LOSS_RESULTS."""
    label = f'{label} loss case {loss_case_id(case)}'
    worst = 0.0
    for i, name in enumerate(LOSS_TERMS):
        worst = max(worst, judge_value(label, name, got['loss'][i], case['loss_f32'][i], case['loss_f64'][i]))
    for name in LOSS_RESULTS[1:]:
        worst = max(worst, judge_value(label, name, got[name], case[f'{name}_f32'], case[f'{name}_f64']))
    return worst
