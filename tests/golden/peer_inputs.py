"""Inputs of the peer-learning loss cases (tests/golden/peer_loss.npz stores only their recipe: seed and parameters).

Plain randn logits disagree on almost every row and would leave the selection untested, so every row gets a planted
class: logits = randn + 4 onehot(t).  The second net's planted class is re-drawn for about a quarter of the rows and
the label for about 30 %.  numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions."""
import numpy as np

PLANT = 4.0

# (N, C, drop_rate, mode); mode: 'mixed' as above, 'agree': both nets plant the same class in every row,
# 'disagree': never the same class
CASES = [
    (8, 200, 0.35, 'mixed'),        # yaml batch; resident form
    (64, 200, 0.35, 'mixed'),       # benchmark batch; 102 KB resident
    (7, 13, 0.2, 'mixed'),          # odd C; scalar loads; partial wave
    (65, 37, 0.5, 'mixed'),         # N not a multiple of the rows per block
    (130, 200, 0.1, 'mixed'),       # too big for the resident form; general only
    (8, 200, 0.0, 'mixed'),         # m = n, nothing dropped
    (8, 200, 0.35, 'disagree'),     # n = 0
    (8, 200, 0.35, 'agree'),        # every row agrees
    (4, 5, 1.0, 'agree'),           # every row agrees and m = 0: NaN losses, zero gradients
]


def peer_inputs(seed, n, c, mode='mixed'):
    """-> logits_1 [n,c] float32, logits_2 [n,c] float32, labels [n] int64 (numpy arrays), a pure function of its arguments."""
    rs = np.random.RandomState(int(seed))
    t1 = rs.randint(0, c, n)
    t2_new = rs.randint(0, c, n)
    t2_pick = rs.rand(n) < 0.25
    y_new = rs.randint(0, c, n)
    y_pick = rs.rand(n) < 0.30
    shift = rs.randint(1, c, n)
    if mode == 'mixed':
        t2 = np.where(t2_pick, t2_new, t1)
    elif mode == 'agree':
        t2 = t1.copy()
    elif mode == 'disagree':
        t2 = (t1 + shift) % c
    else:
        raise ValueError(mode)
    y = np.where(y_pick, y_new, t1)
    l1 = rs.randn(n, c)
    l2 = rs.randn(n, c)
    l1[np.arange(n), t1] += PLANT
    l2[np.arange(n), t2] += PLANT
    return l1.astype(np.float32), l2.astype(np.float32), y.astype(np.int64)


def load_cases(path=None):
    """The cases of peer_loss.npz as dicts: inputs rebuilt from the recipe, the reference's float32 / float64 results,
    n, m and the keep masks."""
    import os
    z = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'peer_loss.npz'))
    cases = []
    for k in range(int(z['cases'])):
        seed, n, c = (int(v) for v in z[f'c{k}_recipe'])
        mode, drop_rate = str(z[f'c{k}_mode']), float(z[f'c{k}_drop_rate'])
        assert (n, c, drop_rate, mode) == CASES[k]
        l1, l2, y = peer_inputs(seed, n, c, mode)
        case = dict(k=k, N=n, C=c, drop_rate=drop_rate, mode=mode, l1=l1, l2=l2, y=y, n=int(z[f'c{k}_n']), m=int(z[f'c{k}_m']),
                    keep1=z[f'c{k}_keep1'], keep2=z[f'c{k}_keep2'])
        for prec in ('f32', 'f64'):
            for name in ('loss', 'dl1', 'dl2'):
                case[f'{name}_{prec}'] = z[f'c{k}_{name}_{prec}']
        cases.append(case)
    return cases


def case_id(case):
    return f"{case['k']}-{case['N']}x{case['C']}-{case['drop_rate']}-{case['mode']}"


# Tolerance (tied to the reference's own rounding): a result's distance from the float64 reference may be at most
# FACTOR x the float32 reference's distance from that same float64 result, with a floor of FLOOR (relative).  Distance:
# relative error of a loss, norm-wise relative error of a gradient.
FACTOR, FLOOR = 4.0, 1e-6


def distances(case, loss, dl1, dl2):
    """[(name, distance of the given result from float64, distance of the float32 reference from float64)] - numpy inputs."""
    out = []
    for name, got in (('loss_1', loss[0]), ('loss_2', loss[1]), ('dl1', dl1), ('dl2', dl2)):
        key = {'loss_1': ('loss', 0), 'loss_2': ('loss', 1)}.get(name)
        ref64 = case['loss_f64'][key[1]] if key else case[f'{name}_f64']
        ref32 = case['loss_f32'][key[1]] if key else case[f'{name}_f32']
        got = np.asarray(got, dtype=np.float64)
        den = np.linalg.norm(np.atleast_1d(ref64))
        if den == 0:                                    # an all-zero gradient: nothing may differ
            out.append((name, float(np.abs(got).max()), 0.0))
            continue
        out.append((name, float(np.linalg.norm(np.atleast_1d(got - ref64)) / den),
                    float(np.linalg.norm(np.atleast_1d(ref32.astype(np.float64) - ref64)) / den)))
    return out


def judge(case, loss, dl1, dl2, stats, label=''):
    """Masks, n, m and the counts exactly; values within the tolerance above.  Prints the measured ratios.  Returns the
    worst ratio distance / allowed."""
    n_rows = case['N']
    assert list(stats[:2]) == [case['n'], case['m']], (list(stats), case['n'], case['m'])
    assert int(stats[2]) == int(case['keep1'].sum()) and int(stats[3]) == int(case['keep2'].sum()), list(stats)
    assert np.array_equal((dl1 != 0).any(1), case['keep1']) and np.array_equal((dl2 != 0).any(1), case['keep2'])
    for g, keep in ((dl1, case['keep1']), (dl2, case['keep2'])):
        assert not g[~keep].any() and g.shape == (n_rows, case['C'])          # dropped rows are exactly zero
    worst = 0.0
    if np.isnan(case['loss_f64']).any():
        assert np.isnan(case['loss_f64']).all() and np.isnan(loss).all()
        assert not dl1.any() and not dl2.any()
        print(f'peer {label} case {case_id(case)}: NaN losses, zero gradients')
        return worst
    for name, d, d32 in distances(case, loss, dl1, dl2):
        allowed = max(FACTOR * d32, FLOOR)
        worst = max(worst, d / allowed)
        print(f'peer {label} case {case_id(case)} {name}: distance {d:.3e}, reference fp32 {d32:.3e}, allowed {allowed:.3e}, '
              f'ratio {d / allowed:.3f}')
        assert d <= allowed, (name, d, d32)
    return worst
