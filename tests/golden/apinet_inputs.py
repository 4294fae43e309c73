"""Inputs of the APINet cases (tests/golden/apinet_*.npz store only their recipe - seed and sizes - and the reference's
results) and the rule by which results are judged.

Purely random rows concentrate their pairwise distances, so that rounding could flip a nearest neighbour and the
partners could not be compared exactly.  Every row is therefore its class's centre plus noise; the 7 x 7 map is the
pooled value plus per-pixel noise, ReLU'd like a trunk's output, and the rows are permuted so that classes are not
contiguous.  numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions."""
import os

import numpy as np

MAP = 7
CLASSES = 200            # the reference's head hard-codes 200 logits (model/methods/APINet.py:63-64)

# (classes, samples per class, D, hidden width)
HEAD_CASES = [
    (2, 2, 64, 32),
    (3, 2, 72, 40),          # D no multiple of 64
    (3, 3, 256, 64),         # odd B
    (5, 1, 64, 32),          # no intra candidate anywhere: every intra partner is 0
    (1, 4, 64, 32),          # no inter candidate anywhere: every inter partner is 0
    (10, 4, 2048, 512),      # the yaml's batch and the model's widths
]
MODEL_CASE = dict(classes=2, samples=2, size=224, init_seed=950)
FILES = ('apinet_head.npz', 'apinet_head_yaml.npz', 'apinet_head_yaml_grad.npz', 'apinet_model.npz')


def head_inputs(seed, n_classes, n_samples, d):
    """-> x [B,d,7,7] float32, labels [B] int64: a pure function of its arguments."""
    rs = np.random.RandomState(int(seed))
    b = n_classes * n_samples
    centres = 0.5 + 0.6 * rs.randn(n_classes, d)
    ids = np.sort(rs.choice(CLASSES, n_classes, replace=False))
    lab = np.repeat(np.arange(n_classes), n_samples)
    pooled = centres[lab] + 0.35 * rs.randn(b, d)
    perm = rs.permutation(b)
    pooled, lab = pooled[perm], lab[perm]
    x = np.maximum(pooled[:, :, None, None] + 0.3 * rs.randn(b, d, MAP, MAP), 0.0)
    return x.astype(np.float32), ids[lab].astype(np.int64)


PLANT = 4.0              # see head_weights


def head_weights(seed, d, hidden, x=None, y=None):
    """-> dict of float32 arrays under the head's state_dict keys (map1, map2, fc).  With the case's inputs given, the
    classifier is the one of a trained head rather than a random one: each present class's row of fc gets PLANT x the
    direction from the batch mean to that class's mean pooled vector (over its squared length), which puts the target's
    probability near a third instead of 1 / 200, and map2 is three times wider than its fan-in rule so that the two gates of
    a pair differ.  Only then do p_self and p_other differ by about the margin and the rank term has rows on both sides."""
    rs = np.random.RandomState(int(seed) + 100003)
    w = {}
    for name, (out_f, in_f), gain in (('map1', (hidden, 2 * d), 1.0), ('map2', (d, hidden), 1.0 if x is None else 9.0),
                                      ('fc', (CLASSES, d), 2.0)):
        w[name + '.weight'] = (rs.randn(out_f, in_f) * np.sqrt(gain / in_f)).astype(np.float32)
        w[name + '.bias'] = (0.1 * rs.randn(out_f)).astype(np.float32)
    if x is not None:
        pool = x.astype(np.float64).mean((2, 3))
        fc = w['fc.weight'].astype(np.float64)
        for c in np.unique(y):
            direction = pool[y == c].mean(0) - pool.mean(0)
            if (direction ** 2).sum() > 0:                       # a batch of one class has no direction: fc stays random
                fc[c] += PLANT * direction / (direction ** 2).sum()
        w['fc.weight'] = fc.astype(np.float32)
    return w


def model_images(seed, n_classes, n_samples, size):
    """-> images [B,3,size,size] float32, labels [B] int64 for the whole-model case."""
    rs = np.random.RandomState(int(seed))
    b = n_classes * n_samples
    ids = np.sort(rs.choice(CLASSES, n_classes, replace=False))
    lab = np.repeat(np.arange(n_classes), n_samples)[rs.permutation(b)]
    return rs.randn(b, 3, size, size).astype(np.float32), ids[lab].astype(np.int64)


def load(path=None):
    """Every array of the APINet golden files in one dict."""
    here = path or os.path.dirname(os.path.abspath(__file__))
    out = {}
    for name in FILES:
        with np.load(os.path.join(here, name)) as z:
            for k in z.files:
                assert k not in out, k
                out[k] = z[k]
    return out


RESULTS = ('self_logits', 'other_logits', 'loss', 'dpool')       # loss [3] = total, CE, rank


def load_head_cases(path=None):
    """The head cases as dicts: inputs and weights rebuilt from the recipe; the reference's partners, labels1 / labels2,
    active rank rows and, in float32 and float64, both logit matrices, the three loss terms and d loss / d pool
    (d loss / d x is dpool / 49 at each of the map's 49 positions - the generator checks that on the reference)."""
    z = load(path)
    cases = []
    for k in range(int(z['head_cases'])):
        seed, n_classes, n_samples, d, hidden = (int(v) for v in z[f'h{k}_recipe'])
        assert (n_classes, n_samples, d, hidden) == HEAD_CASES[k]
        x, y = head_inputs(seed, n_classes, n_samples, d)
        case = dict(k=k, seed=seed, n_classes=n_classes, n_samples=n_samples, B=n_classes * n_samples, D=d, hidden=hidden, x=x, y=y,
                    weights=head_weights(seed, d, hidden, x, y))
        for name in ('partner', 'labels1', 'labels2', 'active'):
            case[name] = z[f'h{k}_{name}']
        for prec in ('f32', 'f64'):
            for name in RESULTS:
                case[f'{name}_{prec}'] = z[f'h{k}_{name}_{prec}']
        cases.append(case)
    return cases


def head_case_id(case):
    return f"{case['k']}-{case['n_classes']}x{case['n_samples']}-D{case['D']}-H{case['hidden']}"


# Tolerance - the rule of tests/golden/peer_inputs.py: a result's distance from the float64 reference may be at most
# FACTOR x the float32 reference's own distance from it, with a floor of FLOOR; norm-wise relative distance for tensors,
# relative distance for scalars.
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
    print(f'apinet {label} {name}: distance {d:.3e}, reference fp32 {d32:.3e}, allowed {allowed:.3e}, ratio {d / allowed:.3f}')
    assert d <= allowed, (label, name, d, d32)
    return d / allowed


def judge_head(case, partner, labels1, labels2, self_logits, other_logits, loss, dpool, label=''):
    """Partners and labels exactly, values by the rule above (loss [3] = total, CE, rank; a rank term that is exactly
    zero in float64 must be exactly zero).  numpy inputs.  Returns the worst ratio."""
    label = f'{label} case {head_case_id(case)}'
    assert np.array_equal(np.asarray(partner, dtype=np.int64), case['partner']), (label, partner, case['partner'])
    assert np.array_equal(np.asarray(labels1), case['labels1']) and np.array_equal(np.asarray(labels2), case['labels2']), label
    worst = 0.0
    for name, got in (('self_logits', self_logits), ('other_logits', other_logits), ('dpool', dpool)):
        worst = max(worst, judge_value(label, name, got, case[f'{name}_f32'], case[f'{name}_f64']))
    for i, name in enumerate(('total', 'CE', 'rank')):
        if case['loss_f64'][i] == 0:
            assert loss[i] == 0, (label, name, loss[i])
            continue
        worst = max(worst, judge_value(label, name, loss[i], case['loss_f32'][i], case['loss_f64'][i]))
    return worst


def active_rows(self_logits, other_logits, labels1, labels2, margin=0.05):
    """The rows whose rank term is active, from float64 softmaxes of the given logits (numpy)."""
    y = np.concatenate([labels1, labels2])
    p = []
    for l in (self_logits, other_logits):
        l = np.asarray(l, dtype=np.float64)
        e = np.exp(l - l.max(1, keepdims=True))
        p.append((e / e.sum(1, keepdims=True))[np.arange(len(y)), y])
    return (p[1] - p[0] + margin) > 0
