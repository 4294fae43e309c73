"""The APINet checks that the emulated tier (test_emu_apinet.py) and the GPU tier (test_gpu_apinet.py) share: each takes
the device to run on.  Values are judged by the rule of tests/golden/apinet_inputs.py - at most 4 x the float32
reference's own distance from the float64 result, floor 1e-6 - where the float32 reference of an op case is the same
torch restatement run in float32 on the CPU.  Not a test module itself."""
import numpy as np
import torch

import apinet_inputs as A


def F():
    import hawkeye_amd.functional as HF
    return HF


def np_(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------- head cases
def head_forward(case, device, x=None):
    """-> dict of tensors; the whole head on the kernels, from the 7 x 7 map to the loss."""
    HF = F()
    w = {k: torch.from_numpy(v).to(device) for k, v in case['weights'].items()}
    x = torch.from_numpy(case['x']).to(device).requires_grad_(True) if x is None else x
    y = torch.from_numpy(case['y']).to(device)
    b = case['B']
    pool = HF.osme_gap(x)
    pool.retain_grad()
    feed = pool
    partner = HF.api_pairs(feed, y)
    labels1 = torch.cat([y, y])
    labels2 = y.index_select(0, partner.long())
    mutual = HF.api_pair_features(feed, partner)
    m = HF.linear(HF.linear(mutual, w['map1.weight'], w['map1.bias']), w['map2.weight'], w['map2.bias'])
    feats = HF.api_interact(feed, partner, m)
    logits = HF.linear(feats, w['fc.weight'], w['fc.bias'])
    self_logits, other_logits = logits[:4 * b], logits[4 * b:]
    loss, parts = HF.apinet_loss_with_parts(self_logits, other_logits, labels1, labels2)
    return dict(x=x, pool=pool, partner=partner, labels1=labels1, labels2=labels2, self_logits=self_logits, other_logits=other_logits,
                loss=loss, parts=parts, m=m, feats=feats)


def run_head(case, device, weight=1.0):
    t = head_forward(case, device)
    (t['loss'] * weight).backward()
    loss = np.concatenate([np_(t['loss']).reshape(1), np_(t['parts'])])
    sl, ol, l1, l2 = np_(t['self_logits']), np_(t['other_logits']), np_(t['labels1']), np_(t['labels2'])
    dpool = np_(t['pool'].grad)
    return dict(judged=(np_(t['partner']), l1, l2, sl, ol, loss, dpool), dpool=dpool, dx=np_(t['x'].grad),
                active=A.active_rows(sl, ol, l1, l2))


def check_dx(got):
    """d loss / d x is d loss / d pool / 49 at each of the 49 positions (the goldens store dpool; their generator checks
    the same on the reference): equal across the map, and within a rounding of the division."""
    dx, dpool = got['dx'], got['dpool']
    assert np.array_equal(dx, np.broadcast_to(dx[:, :, :1, :1], dx.shape))
    np.testing.assert_allclose(dx[:, :, 0, 0], dpool / np.float32(49), rtol=3e-7, atol=0)


# ----------------------------------------------------------------------------------------------------- pair selection
def check_pairs_ties(device):
    HF = F()
    rs = np.random.RandomState(5)
    base = rs.randn(3, 70).astype(np.float32)
    # rows 1, 3 and 5 are copies of one vector, rows 2 and 4 of another: every distance between copies is exactly equal
    pool = torch.from_numpy(np.stack([base[0], base[1], base[2], base[1], base[2], base[1]])).to(device)
    y = torch.tensor([7, 7, 9, 7, 9, 7], device=device)
    got = np_(HF.api_pairs(pool, y)).tolist()
    d = ((base[:, None] - base[None]) ** 2).sum(-1)
    near0 = 1 if d[0, 1] < d[0, 2] else 2                                    # row 0's nearest vector
    assert got[:6] == [1, 3, 4, 1, 2, 1]                                     # intra: of the equal copies the lowest index, never itself
    assert got[6] == near0 if near0 == 2 else got[6] == 2                    # inter of row 0: label 9 only (rows 2, 4): the lower one
    assert got[7:] == [2, 0 if d[2, 0] < d[2, 1] else 1, 2, 0 if d[2, 0] < d[2, 1] else 1, 2]
    assert got == np_(HF.api_pairs(pool, y.int())).tolist() and HF.api_pairs(pool, y).dtype == torch.int32
    # an exact tie between two different candidates at equal distance on either side of the anchor
    line = torch.tensor([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 2.0], [0.0, -2.0]], device=device)
    got = np_(HF.api_pairs(line, torch.tensor([1, 1, 1, 2, 2], device=device))).tolist()
    assert got[0] == 1 and got[5] == 3                                       # (1, 2) tie -> 1 ; (3, 4) tie -> 3
    # a NaN row is nobody's partner and is itself paired with row 0 (a NaN distance counts as +inf)
    bad = line.clone()
    bad[1, 0] = float('nan')
    got = np_(HF.api_pairs(bad, torch.tensor([1, 1, 1, 2, 2], device=device))).tolist()
    assert got[0] == 2 and got[1] == 0 and got[6] == 0


def check_pairs_no_candidates(device):
    HF = F()
    rs = np.random.RandomState(6)
    pool = torch.from_numpy(rs.randn(5, 33).astype(np.float32)).to(device)
    got = np_(HF.api_pairs(pool, torch.arange(5, device=device))).tolist()
    assert got[:5] == [0] * 5 and all(g != i for i, g in enumerate(got[5:]))           # all labels differ: no intra candidate
    got = np_(HF.api_pairs(pool, torch.full((5,), 3, device=device))).tolist()
    assert got[5:] == [0] * 5 and all(g != i for i, g in enumerate(got[:5]))           # all labels equal: no inter candidate
    d = ((pool[:, None].double() - pool[None].double()) ** 2).sum(-1).cpu()
    d.fill_diagonal_(float('inf'))
    assert got[:5] == d.argmin(1).tolist()
    one = HF.api_pairs(pool[:1], torch.tensor([4], device=device))
    assert np_(one).tolist() == [0, 0]                                                 # B = 1
    # B = 1 through the gather and the interaction: the row is paired with itself
    p1 = pool[:1].clone().requires_grad_(True)
    mutual = HF.api_pair_features(p1, one)
    assert torch.equal(mutual.detach(), torch.cat([p1.detach(), p1.detach()], 1).repeat(2, 1))
    mutual.sum().backward()
    assert torch.equal(p1.grad, torch.full_like(p1, 4.0))


def check_pairs_unaligned(device):
    """D % 4 == 0 behind a base pointer that is not 16-byte aligned (a dense view one float into a buffer): the quads are
    fetched element by element, in the same order - the same partners as the aligned call, and the hand-checked ones."""
    HF = F()
    rs = np.random.RandomState(9)
    b, d = 7, 72
    pool = rs.randn(b, d).astype(np.float32)
    y = torch.tensor([1, 2, 1, 2, 3, 1, 3], device=device)
    buf = torch.zeros(b * d + 5, device=device)
    view = buf[1:1 + b * d].view(b, d)
    view.copy_(torch.from_numpy(pool))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    aligned = torch.from_numpy(pool).to(device)
    assert aligned.data_ptr() % 16 == 0
    got = HF.api_pairs(view, y)
    assert torch.equal(got, HF.api_pairs(aligned, y))
    dist = ((pool[:, None].astype(np.float64) - pool[None]) ** 2).sum(-1)
    yn = np_(y)
    want = []
    for same in (True, False):
        for i in range(b):
            cand = [j for j in range(b) if j != i and (yn[j] == yn[i]) == same]
            want.append(min(cand, key=lambda j: dist[i, j]))
    assert np_(got).tolist() == want


# ----------------------------------------------------------------------------------------------------- interaction
def interact_ref(pool, partner, m, masks, scale):
    b = pool.shape[0]
    f1, f2 = pool[torch.arange(2 * b) % b], pool[partner]
    g1, g2 = torch.sigmoid(m * f1), torch.sigmoid(m * f2)
    feats = torch.cat([f1 * g1 + f1, f2 * g2 + f2, f1 * g2 + f1, f2 * g1 + f2])
    return feats if masks is None else feats * (masks.to(pool.dtype) * scale)


def check_interact(device, b, d, use_masks=True):
    HF = F()
    rs = np.random.RandomState(100 + b)
    partner = np.zeros(2 * b, dtype=np.int64)           # row 0 is chosen by many rows, row 1 by one, row 2 by two, the rest by none
    partner[0], partner[3], partner[b + 1] = 1, 2, 2
    pool = rs.randn(b, d).astype(np.float32)
    m = rs.randn(2 * b, d).astype(np.float32)
    masks = rs.rand(8 * b, d) < 0.5 if use_masks else None
    wgt = rs.randn(8 * b, d).astype(np.float32)
    counts = np.bincount(partner, minlength=b)
    assert counts[1] == 1 and counts[2] == 2 and counts[0] == 2 * b - 3 and not counts[3:].any()
    ref = {}
    for dt in (torch.float32, torch.float64):
        pp, mm = torch.from_numpy(pool).to(dt).requires_grad_(True), torch.from_numpy(m).to(dt).requires_grad_(True)
        feats = interact_ref(pp, torch.from_numpy(partner), mm, None if masks is None else torch.from_numpy(masks), 2.0)
        (feats * torch.from_numpy(wgt).to(dt)).sum().backward()
        ref[dt] = dict(feats=np_(feats), dpool=np_(pp.grad), dm=np_(mm.grad))
    pp, mm = torch.from_numpy(pool).to(device).requires_grad_(True), torch.from_numpy(m).to(device).requires_grad_(True)
    part = torch.from_numpy(partner).to(device)
    mk = None if masks is None else torch.from_numpy(masks).to(device)
    feats = HF.api_interact(pp, part, mm, mk, 0.5)
    (feats * torch.from_numpy(wgt).to(device)).sum().backward()
    got = dict(feats=np_(feats), dpool=np_(pp.grad), dm=np_(mm.grad))
    for name in ('feats', 'dpool', 'dm'):
        A.judge_value(f'interact B {b} D {d}', name, got[name], ref[torch.float32][name], ref[torch.float64][name])
    if masks is not None:
        assert not got['feats'][~masks].any()                                          # dropped elements are exactly zero
        assert torch.equal(HF.api_interact(pp, part, mm, mk.to(torch.uint8), 0.5), feats)
    # the pair gather with the same scatter counts
    pp.grad = None
    mutual = HF.api_pair_features(pp, part)
    assert torch.equal(mutual.detach(), torch.cat([pp.detach().repeat(2, 1), pp.detach()[part]], 1))
    w2 = torch.from_numpy(rs.randn(2 * b, 2 * d).astype(np.float32))
    (mutual * w2.to(device)).sum().backward()
    want = w2[:b, :d].double() + w2[b:, :d].double()
    want.index_add_(0, torch.from_numpy(partner), w2[:, d:].double())
    want32 = (w2[:b, :d] + w2[b:, :d]).index_add_(0, torch.from_numpy(partner), w2[:, d:])
    A.judge_value(f'gather B {b} D {d}', 'dpool', np_(pp.grad), np_(want32), np_(want))
    return got


# ----------------------------------------------------------------------------------------------------- loss
LOSS_CASES = [(4, 7, 'mixed'), (36, 200, 'mixed'), (160, 200, 'mixed'), (8, 257, 'mixed'), (36, 200, 'inactive'), (36, 200, 'active')]


ROUNDINGS = 4            # per float32 probability: the exponential, the row sum, the division and the stored result


def loss_inputs(r, c, mode):
    """self = randn + plant onehot(y) with plant = round(log c + 0.7) - 6 at 200 and 257 classes, 3 at 7 - so that the
    target's probability is near a half at every width; mixed: other = another randn + plant onehot(y); inactive / active:
    other = self scaled down (x 0.1) / up (x 2).  The seed is the first one whose inputs allow the rule to be applied to the
    rank term as it stands: the active set is what the mode says (mixed: rows on both sides), every |rank term| >= 1e-4 in float64 (the set can be
    compared exactly), and the term is
    not a near-cancellation for float32.  The second asks that ROUNDINGS roundings of 2^-24 in each probability, added over
    the rows as independent errors, stay within the rule's floor of 1e-6 x rank:
        ROUNDINGS 2^-24 sqrt(sum_r p_self^2 + p_other^2) / R <= 1e-6 rank.
    With probabilities near 1 and a rank of a few hundredths over four rows no float32 computation can promise 1e-6."""
    plant = float(round(np.log(c) + 0.7))
    for seed in range(1000):
        rs = np.random.RandomState(7000 + 31 * r + c + 977 * seed)
        y = rs.randint(0, c, r)
        ls = rs.randn(r, c)
        ls[np.arange(r), y] += plant
        if mode == 'mixed':
            lo = rs.randn(r, c)
            lo[np.arange(r), y] += plant
        else:
            lo = ls * (0.1 if mode == 'inactive' else 2.0)
        ls, lo = ls.astype(np.float32), lo.astype(np.float32)
        p = [torch.softmax(torch.from_numpy(v).double(), 1)[torch.arange(r), torch.from_numpy(y)].numpy() for v in (ls, lo)]
        hinge = p[1] - p[0] + 0.05
        rank = np.maximum(hinge, 0).mean()
        noise = ROUNDINGS * 2.0 ** -24 * np.sqrt((p[0] ** 2 + p[1] ** 2).sum()) / r
        active = hinge > 0
        sides = active.all() if mode == 'active' else (not active.any() if mode == 'inactive' else (active.any() and not active.all()))
        if sides and np.abs(hinge).min() >= 1e-4 and (rank == 0 or noise <= 1e-6 * rank):
            return ls, lo, y[:r // 2], y[r // 2:], hinge > 0
    raise RuntimeError('no seed')


def loss_ref(ls, lo, y1, y2, smoothing=0.1, margin=0.05):
    y = torch.cat([y1, y2])
    ce = torch.nn.functional.cross_entropy(torch.cat([ls, lo]), torch.cat([y, y]), label_smoothing=smoothing)
    rows = torch.arange(y.numel())
    s, o = torch.softmax(ls, 1)[rows, y], torch.softmax(lo, 1)[rows, y]
    rank = torch.nn.functional.margin_ranking_loss(s, o, torch.ones_like(s), margin=margin)
    return ce + rank, ce, rank


def check_loss(device, r, c, mode, weight=1.0):
    HF = F()
    ls, lo, y1, y2, active = loss_inputs(r, c, mode)
    assert active.all() if mode == 'active' else (not active.any() if mode == 'inactive' else (active.any() and not active.all()))
    ref = {}
    for dt in (torch.float32, torch.float64):
        a, b = torch.from_numpy(ls).to(dt).requires_grad_(True), torch.from_numpy(lo).to(dt).requires_grad_(True)
        total, ce, rank = loss_ref(a, b, torch.from_numpy(y1), torch.from_numpy(y2))
        total.backward()
        ref[dt] = dict(total=total.item(), ce=ce.item(), rank=rank.item(), ds=np_(a.grad), do=np_(b.grad))
    a, b = torch.from_numpy(ls).to(device).requires_grad_(True), torch.from_numpy(lo).to(device).requires_grad_(True)
    l1, l2 = torch.from_numpy(y1).to(device), torch.from_numpy(y2).to(device)
    total, parts = HF.apinet_loss_with_parts(a, b, l1, l2)
    assert total.dim() == 0 and parts.shape == (2,) and not parts.requires_grad
    (total * weight).backward()
    got = dict(total=total.item(), ce=parts[0].item(), rank=parts[1].item(), ds=np_(a.grad) / weight, do=np_(b.grad) / weight)
    label = f'loss R {r} C {c} {mode}'
    for name in ('total', 'ce', 'ds', 'do') + (() if mode == 'inactive' else ('rank',)):
        A.judge_value(label, name, got[name], ref[torch.float32][name], ref[torch.float64][name])
    # the rows whose rank term the kernel took as active, exactly: with margin -2 no row can be active, so a row of dself
    # that differs from that run's is a row with a rank gradient
    a0 = a.detach().clone().requires_grad_(True)
    HF.apinet_loss(a0, b.detach(), l1, l2, margin=-2.0).backward()
    assert np.array_equal((np_(a0.grad) != np_(a.grad) / weight).any(1), active), label
    if mode == 'inactive':
        assert got['rank'] == 0.0 and ref[torch.float64]['rank'] == 0.0 and got['total'] == got['ce']
    assert torch.equal(HF.apinet_loss(a, b, l1, l2), total)
    assert torch.equal(HF.apinet_loss(a, b, l1.int(), l2.int()), total)
    return got, (a, b, l1, l2)


def check_loss_bad_labels(device):
    HF = F()
    ls, lo, y1, y2, _ = loss_inputs(8, 257, 'mixed')
    a, b = torch.from_numpy(ls).to(device).requires_grad_(True), torch.from_numpy(lo).to(device)
    l1, l2 = torch.from_numpy(y1).to(device).clone(), torch.from_numpy(y2).to(device).clone()
    l1[1], l2[2] = 257 + 1000000, -5
    total, parts = HF.apinet_loss_with_parts(a, b, l1, l2)
    assert torch.isnan(total) and torch.isnan(parts).all()
    total.backward()
    g = np_(a.grad)
    assert np.isfinite(g[[0, 2, 3, 4, 5, 7]]).all()                    # the rows with valid labels keep their gradients
