"""Inputs of the DCL cases (tests/golden/dcl_*.npz store only their recipe - seed and sizes - and the reference's
results) and the rule by which results are judged (that of tests/golden/crossx_inputs.py).

numpy's RandomState (a frozen stream) keeps the tensors identical across torch versions.  The L1 term is not
differentiable where the mask meets the law, so a loss case takes the first seed from its base at which no mask element
is closer to its law than L1_MARGIN in float64 - computed here from the inputs, never from the code under test.  The
tie case then sets chosen mask elements bit-equal to the law; those must get a gradient of exactly zero."""
import os

import numpy as np

from crossx_inputs import FACTOR, FLOOR, distance, judge_value  # noqa: F401  (the project's rule, one definition)

CLASSES = 200
FILES = ('dcl_ops.npz', 'dcl_model.npz')
L1_MARGIN = 1e-3
SMOOTHING = 0.1
COEF = (1.0, 0.5, 2.0)                                   # alpha, beta, gamma: each term weighted differently

# (B, C, H, W): the plugin's own map at two samples; odd sides with HW % 4 != 0 and a channel count that fills no whole
# chunk; mixed parity; one mask value; 130 channels on a 4 x 4 map
HEAD_CASES = [(2, 2048, 14, 14), (2, 70, 7, 7), (3, 5, 5, 6), (1, 1, 2, 2), (2, 130, 4, 4)]
# (N, K, S, M): the yaml's doubled batch; cls_2xmul; tiny; one class; the exact-tie case
LOSS_CASES = [(16, 200, 2, 49), (4, 200, 400, 49), (2, 3, 2, 1), (1, 1, 2, 9), (3, 5, 2, 9)]
TIE_CASE = 4
TIES = ((0, 0), (1, 4), (2, 8))                          # (sample, mask element) set bit-equal to the law in TIE_CASE
MODEL_CASE = dict(B=2, size=448, init_seed=1177, cls_2=True, cls_2xmul=False)


def head_case_id(case):
    return 'B{}-C{}-{}x{}'.format(*case)


def head_inputs(case):
    """-> float32 arrays x [B,C,H,W], w [C], bias [1], d_pooled [B,C], d_mask [B,(H/2)(W/2)].  w is scaled so that the
    1 x 1 convolution's output is of the order of one and the tanh is not saturated."""
    b, c, h, w = case
    rs = np.random.RandomState(9000 + 10 * HEAD_CASES.index(tuple(case)))
    f = lambda *s: rs.randn(*s).astype(np.float32)
    return dict(x=f(b, c, h, w), w=(rs.randn(c) / np.sqrt(c)).astype(np.float32), bias=f(1) * np.float32(0.3), d_pooled=f(b, c),
                d_mask=f(b, (h // 2) * (w // 2)))


def law_values(index, parts):
    """(index - parts // 2) / parts in float64, then float32: what the reference's collate makes of a law."""
    return ((np.asarray(index, dtype=np.int64) - parts // 2) / float(parts)).astype(np.float32)


def loss_arrays(seed, n, k, s, m):
    rs = np.random.RandomState(int(seed))
    y, ys = rs.randint(0, k, n), rs.randint(0, s, n)
    logits, swap = rs.randn(n, k), rs.randn(n, s)
    logits[np.arange(n), y] += float(round(np.log(k) + 0.7)) * (0.5 + rs.rand(n))
    mask = np.tanh(0.6 * rs.randn(n, m)).astype(np.float32)
    law = law_values(rs.randint(0, m, (n, m)), m)
    return logits.astype(np.float32), swap.astype(np.float32), mask, y.astype(np.int64), ys.astype(np.int64), law


def loss_seed_ok(mask, law):
    return float(np.abs(mask.astype(np.float64) - law.astype(np.float64)).min()) >= L1_MARGIN


def loss_inputs(k_case, seed=None):
    """-> (logits [N,K], swap logits [N,S], mask [N,M], labels [N], swap labels [N], law [N,M], the accepted seed)."""
    n, k, s, m = LOSS_CASES[k_case]
    base = 9300 + 20 * k_case
    for cand in ([int(seed)] if seed is not None else range(base, base + 20)):
        arrays = loss_arrays(cand, n, k, s, m)
        if loss_seed_ok(arrays[2], arrays[5]):
            break
    else:
        raise RuntimeError(f'loss case {k_case}: no seed keeps the mask {L1_MARGIN} away from the law')
    if k_case == TIE_CASE:
        for b, e in TIES:
            arrays[2][b, e] = arrays[5][b, e]
    return arrays + (cand,)


LOSS_INPUTS = ('logits', 'swap', 'mask', 'y', 'ys', 'law')
LOSS_RESULTS = ('loss', 'd_logits', 'd_swap', 'd_mask')
LOSS_TERMS = ('total', 'ce', 'swap', 'law')


# ------------------------------------------------------------------------------------------------------- swap law
def patch_bounds(size, parts):
    return [int((size / parts) * i) for i in range(parts + 1)]


def patch_totals(img, grid):
    """Integer band totals [gy gx, 3] and pixel counts [gy gx] of the patches of a uint8 image [H,W,3]."""
    gx, gy = grid
    h, w, _ = img.shape
    xs, ys = patch_bounds(w, gx), patch_bounds(h, gy)
    tot, cnt = [], []
    for j in range(gy):
        for i in range(gx):
            p = img[ys[j]:min(ys[j + 1], h), xs[i]:min(xs[i + 1], w)].astype(np.int64)
            tot.append(p.reshape(-1, 3).sum(0))
            cnt.append(p.shape[0] * p.shape[1])
    return np.array(tot), np.array(cnt)


def permute_patches(img, perm, grid):
    """Whole-patch moves on the array: position k (row-major) takes patch perm[k].  Every patch must have one size."""
    gx, gy = grid
    h, w, _ = img.shape
    ph, pw = h // gy, w // gx
    assert ph * gy == h and pw * gx == w
    out = np.empty_like(img)
    for k, src in enumerate(perm):
        dj, di, sj, si = k // gx, k % gx, int(src) // gx, int(src) % gx
        out[dj * ph:(dj + 1) * ph, di * pw:(di + 1) * pw] = img[sj * ph:(sj + 1) * ph, si * pw:(si + 1) * pw]
    return out


def smooth_image(rs, h, w, cells=9):
    """A seeded uint8 image [h,w,3] with structure at the patch scale: a coarse random grid, enlarged, plus fine noise."""
    coarse = rs.randint(0, 256, (cells, cells, 3)).astype(np.float64)
    big = np.repeat(np.repeat(coarse, -(-h // cells), 0), -(-w // cells), 1)[:h, :w]
    return np.clip(0.7 * big + 0.3 * rs.randint(0, 256, (h, w, 3)), 0, 255).astype(np.uint8)


def law_permutation_case():
    """14 x 14, grid 7 x 7 (2 x 2 pixels per patch): the 49 patch totals pairwise distinct (asserted), the swapped image a
    patch permutation -> (unswapped, swapped, the permutation)."""
    rs = np.random.RandomState(9501)
    for _ in range(50):
        img = rs.randint(0, 256, (14, 14, 3)).astype(np.uint8)
        tot, _ = patch_totals(img, (7, 7))
        if len(set(tot.sum(1).tolist())) == 49:
            break
    else:
        raise RuntimeError('no image with 49 distinct patch totals')
    perm = rs.permutation(49)
    return img, permute_patches(img, perm, (7, 7)), perm.astype(np.int32)


def law_ragged_case():
    """50 x 45 (height x width), grid 7 x 7: patches of unequal sizes; the swapped image is the unswapped one turned by
    180 degrees plus fresh noise in one corner."""
    rs = np.random.RandomState(9502)
    img = smooth_image(rs, 50, 45)
    sw = img[::-1, ::-1].copy()
    sw[:9, :9] = rs.randint(0, 256, (9, 9, 3))
    return img, sw


def law_constant_case():
    img = np.full((28, 35, 3), 117, dtype=np.uint8)
    return img, img.copy()


EQUAL_TOTAL_BANDS = ((0, 0, 6), (0, 1, 5))              # band totals of the two special patches: 6 either way


def law_equal_total_case():
    """21 x 21, grid 7 x 7 (9 pixels per patch).  Patches 5 and 30 of the unswapped image have the band totals (0, 0, 6)
    and (0, 1, 5): one integer total, but ((0 + 0/9) + 0/9) + 6/9 != ((0 + 0/9) + 1/9) + 5/9 in float64 (asserted).  Patch
    12 of the swapped image is a copy of patch 30: the reference finds 30, at distance 0; a search on integer totals would
    stop at 5."""
    a, b = (((0.0 + r / 9) + g / 9) + bl / 9 for r, g, bl in EQUAL_TOTAL_BANDS)
    assert a != b and sum(EQUAL_TOTAL_BANDS[0]) == sum(EQUAL_TOTAL_BANDS[1])
    rs = np.random.RandomState(9504)
    img = rs.randint(40, 256, (21, 21, 3)).astype(np.uint8)            # every other patch total is far above 6

    def fill(image, patch, bands):
        j, i = patch // 7, patch % 7
        block = np.zeros((3, 3, 3), dtype=np.uint8)
        for band, total in enumerate(bands):
            for t in range(total):
                block[t // 3, t % 3, band] += 1
        image[3 * j:3 * j + 3, 3 * i:3 * i + 3] = block
    fill(img, 5, EQUAL_TOTAL_BANDS[0])
    fill(img, 30, EQUAL_TOTAL_BANDS[1])
    sw = rs.randint(40, 256, (21, 21, 3)).astype(np.uint8)
    fill(sw, 12, EQUAL_TOTAL_BANDS[1])
    tot, cnt = patch_totals(img, (7, 7))
    assert (tot[5].tolist(), tot[30].tolist()) == tuple(list(v) for v in EQUAL_TOTAL_BANDS) and (cnt == 9).all()
    return img, sw


def law_large_case():
    """One 448 x 448 pair: a smooth image and a patch permutation of its 7 x 7 patches of 64 x 64 pixels, plus noise of
    +-2 grey levels so that no swapped patch equals its source."""
    rs = np.random.RandomState(9505)
    img = smooth_image(rs, 448, 448, cells=14)
    sw = permute_patches(img, rs.permutation(49), (7, 7)).astype(np.int16) + rs.randint(-2, 3, (448, 448, 3))
    return img, np.clip(sw, 0, 255).astype(np.uint8)


LAW_CASES = {'permutation': lambda: law_permutation_case()[:2], 'ragged': law_ragged_case, 'constant': law_constant_case,
             'equal_total': law_equal_total_case, 'large': law_large_case}
LAW_GRID = (7, 7)


# ------------------------------------------------------------------------------- transforms and collate fixtures
SWAP_SEED = 20240
SWAP_IMAGE = (76, 90)                                    # height, width of the image RandomSwap is run on
PERM_SIDE = 16                                           # the permutation probe: 7 x 7 flat patches of 16 x 16 pixels + the border


def swap_image():
    return smooth_image(np.random.RandomState(9601), *SWAP_IMAGE)


def probe_image():
    """An image whose patches (after RandomSwap's 10-pixel border cut) are flat, patch k in the grey level 5 k + 5: the
    permutation a swap drew can be read off the centres of the result's patches."""
    side = 7 * PERM_SIDE + 20
    img = np.zeros((side, side, 3), dtype=np.uint8)
    for k in range(49):
        j, i = k // 7, k % 7
        img[10 + j * PERM_SIDE:10 + (j + 1) * PERM_SIDE, 10 + i * PERM_SIDE:10 + (i + 1) * PERM_SIDE] = 5 * k + 5
    return img


def read_probe(swapped):
    """-> the permutation: entry k is the source patch found at position k of a swapped probe image."""
    side = swapped.shape[0]
    perm = []
    for k in range(49):
        j, i = k // 7, k % 7
        v = float(swapped[int((j + 0.5) * side / 7), int((i + 0.5) * side / 7)].astype(np.float64).mean())
        perm.append(int(round((v - 5) / 5)))
    return perm


def collate_samples():
    """Four training samples and four validation samples in the reference's formats, with small integer images:
    (img_unswap, img_swap, label, label_swap, law1, law2, name) and (img, label, label_swap, law1, law2, name)."""
    rs = np.random.RandomState(9701)
    ramp = [(i - 2) / 4 for i in range(4)]
    train, val = [], []
    for n, (label, label_swap) in enumerate(((3, -1), (0, -1), (7, 207), (5, 205))):
        law2 = [(int(v) - 2) / 4 for v in rs.randint(0, 4, 4)]
        train.append((rs.randint(0, 256, (2, 3, 3)), rs.randint(0, 256, (2, 3, 3)), label, label_swap, ramp, law2, f'a/{n}.jpg'))
        val.append((rs.randint(0, 256, (2, 3, 3)), label, label, ramp, ramp, f'b/{n}.jpg'))
    return train, val


# ------------------------------------------------------------------------------------------------------- fixtures
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
    for k, (n, kk, s, m) in enumerate(LOSS_CASES):
        recipe = [int(v) for v in z[f'l{k}_recipe']]
        assert recipe[1:] == [n, kk, s, m], recipe
        case = dict(zip(LOSS_INPUTS, loss_inputs(k, recipe[0])[:6]), k=k, N=n, K=kk, S=s, M=m)
        for prec in ('f32', 'f64'):
            for name in LOSS_RESULTS:
                case[f'{name}_{prec}'] = z[f'l{k}_{name}_{prec}']
        cases.append(case)
    return cases


MODEL_OUTPUTS = ('logits', 'swap_logits', 'mask')


def load_model_case(z=None):
    z = z or load()
    seed, b, size, init_seed = (int(v) for v in z['model_recipe'])
    assert dict(MODEL_CASE, B=b, size=size, init_seed=init_seed) == MODEL_CASE
    case = dict(MODEL_CASE, seed=seed, images=model_images(seed, b, size))
    for prec in ('f32', 'f64'):
        for name in MODEL_OUTPUTS:
            case[f'{name}_{prec}'] = z[f'model_{name}_{prec}']
    return case


def loss_case_id(case):
    return f"{case['k']}-N{case['N']}-K{case['K']}-S{case['S']}-M{case['M']}"


def judge_loss(case, got, label=''):
    """got: dict of numpy arrays named as LOSS_RESULTS."""
    label = f'{label} loss case {loss_case_id(case)}'
    worst = 0.0
    for i, name in enumerate(LOSS_TERMS):
        worst = max(worst, judge_value(label, name, got['loss'][i], case['loss_f32'][i], case['loss_f64'][i]))
    for name in LOSS_RESULTS[1:]:
        worst = max(worst, judge_value(label, name, got[name], case[f'{name}_f32'], case[f'{name}_f64']))
    return worst
