"""The same bits under memory pressure, for every kernel that waits for its own loads by count: the ones that issue untracked loads
(HK_LOAD16_ASYNC / HK_LOAD4_ASYNC), wait with s_waitcnt vmcnt(n) (HK_VMCNT_IMM, HK_VM_BARRIER) or stage through LDS-DMA (glds16 /
glds4).  On an
idle device the tiles of a small test shape come out of L2 and a value consumed one wait too early can still have landed; in a
training step it has not.  So each case is launched twenty times, every odd launch while a side stream saturates HBM with copies
(memory latency several times the quiet one) - as test_classifier_backward_full_shape_is_reproducible_under_memory_pressure does for
the 64-row classifier backward (tests/test_gpu_full_shapes.py).  The first, quiet launch meets the check of the test that owns the
kernel against float64 or the oracle - its inputs, its bound; no tolerance is introduced here - and every later launch gives the bits of the first: no
kernel in csrc/ uses atomics, their sums run in a fixed order.  A difference between launches means a value was consumed before it
arrived: a wait count that is short.  Outputs and workspaces the test allocates hold NaN before each launch; where the wrapper
allocates them, the results are overwritten with NaN once compared, so that a block the allocator hands out again holds no answer.
Nothing here runs under emulation: its loads are synchronous."""
import functools

import pytest
import torch

import hawkeye_oracle as O
from conv_fwd_cases import bound, case as conv_case, within
from test_gpu_conv_wrw_wide import _case as wrw_case, _within as wrw_within
from test_gpu_kernels import _fill_batches, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LAUNCHES = 20                                              # a condition, not a measurement (the precedent: 40)
NAN = float('nan')


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


@pytest.fixture(scope='module')
def pressure():
    """-> run(op, check_first): LAUNCHES launches of op() -> list of tensors; the first result goes to check_first, every later one
    must equal it bit for bit.  Two junk buffers of 64 Mi floats and one side stream, shared by the module's cases."""
    junk_a, junk_b = torch.empty(64 * 1024 * 1024, device=DEV), torch.empty(64 * 1024 * 1024, device=DEV)
    side = torch.cuda.Stream()

    def run(op, check_first):
        first = None
        for it in range(LAUNCHES):
            if it % 2:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(6):
                        junk_b.copy_(junk_a)
            outs = op()
            torch.cuda.synchronize()
            if first is None:
                first = [o.detach().clone() for o in outs]
                check_first(first)
            else:
                assert len(outs) == len(first)
                for i, (p, q) in enumerate(zip(first, outs)):
                    assert torch.equal(p, q.detach()), (it, i)
            for o in outs:
                o.detach().fill_(NAN)
        torch.cuda.synchronize()
    yield run
    del junk_a, junk_b
    torch.cuda.empty_cache()


def _nan_bytes(n):
    return torch.full((max(int(n), 16),), 0xFF, dtype=torch.uint8, device=DEV)           # (four 0xFF bytes are a NaN)


# ------------------------------------------------------------------------------------------------ csrc/conv_fwd.hip
CONV = (4, 28, 28, 256, 128)          # 8 K chunks forward, 4 backward: the chain restarts every 3; 28 pixel tiles x 2 Cout tiles


@pytest.mark.parametrize('direction', ['forward', 'input_gradient'])
def test_conv3x3_forward_and_input_gradient(F, tune, pressure, direction):
    from hawkeye_amd import _lib
    from hawkeye_amd.functional import ptr, stream
    lib = _lib.load()
    n, h, w, cin, cout = CONV
    x, wt, dy, y64, sy, dx64, sdx = conv_case(CONV, 'relu')
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    fwd = direction == 'forward'
    src, wg = (x if fwd else dy).to(DEV), wt.to(DEV)
    fn = lib.hk_conv3x3_fwd if fwd else lib.hk_conv3x3_bwd_data
    nws = lib.hk_conv3x3_ws_bytes(cin, cout)

    def op():
        out = torch.full((n, cout if fwd else cin, h, w), NAN, device=DEV).contiguous(memory_format=torch.channels_last)
        ws = _nan_bytes(nws)
        assert fn(ptr(src), ptr(wg), ptr(out), n, h, w, cin, cout, ptr(ws), nws, stream()) == 0
        return [out]

    def check(first):
        if fwd:
            within(first[0], y64, sy, bound(cin), f'forward {CONV}')
        else:
            within(first[0], dx64, sdx, bound(cout), f'input gradient {CONV}')
    pressure(op, check)


# ------------------------------------------------------------------------------------------------ csrc/conv_wrw.hip
WRW = {'fp32': ((8, 28, 28, 64, 128), 0), 'split': ((8, 28, 28, 64, 128), 1), 'wide': ((8, 28, 28, 128, 128), 1)}     # shape, wrw_split


@pytest.mark.parametrize('form', list(WRW))
def test_conv3x3_weight_gradient(F, tune, pressure, form):
    """`wrw_wgs` at 4: 56 row steps per workgroup, past the 32 after which the split forms add their accumulators to the partial."""
    from hawkeye_amd import _lib
    from hawkeye_amd.functional import ptr, stream
    lib = _lib.load()
    shape, split = WRW[form]
    n, h, w, cin, cout = shape
    x, dy, ref, scale = wrw_case(*shape)
    xg, dyg = x.to(DEV), dy.to(DEV)
    tune('wrw_wgs', 4)
    tune('wrw_split', split)
    nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)

    def op():
        buf = torch.full((cout, 3, 3, cin), NAN, device=DEV)
        ws = _nan_bytes(nws)
        assert lib.hk_conv3x3_wrw(ptr(dyg), ptr(xg), ptr(buf), n, h, w, cin, cout, ptr(ws), nws, stream()) == 0
        return [buf.permute(0, 3, 1, 2)]
    assert n * h * w > 1024
    pressure(op, lambda first: wrw_within(first[0], ref, scale, 1.5e-6, f'{form} {shape}'))


# ------------------------------------------------------------------------------------------------ csrc/cin.hip
@functools.lru_cache(maxsize=None)
def _cin_case(b, c, hw):
    """The inputs and the float64 results of test_cin_channel_interaction_ops, once per shape."""
    gen = torch.Generator().manual_seed(b * 100 + c)
    x = torch.relu(torch.randn(b, c, hw, generator=gen))
    wt = torch.randn(b, generator=gen) * 0.7
    g1, g2 = torch.randn(b, c, hw, generator=gen), torch.randn(b, c, hw, generator=gen)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    w_ref = torch.softmax(-torch.bmm(xr, xr.transpose(1, 2)) / hw, dim=2)
    y_ref = torch.bmm(w_ref, xr)
    w_ba = torch.cat((w_ref[b // 2:], w_ref[:b // 2]), 0)
    yc_ref = torch.bmm(torch.abs(w_ref - wr.view(-1, 1, 1) * w_ba), xr)
    ((y_ref * g1.double()).sum() + (yc_ref * g2.double()).sum()).backward()
    x3 = x.double().requires_grad_(True)
    (torch.bmm(torch.softmax(-torch.bmm(x3, x3.transpose(1, 2)) / hw, dim=2), x3) * g1.double()).sum().backward()
    return x, wt, g1, g2, [v.detach() for v in (w_ref, y_ref, yc_ref, xr.grad, wr.grad, x3.grad)]


@pytest.mark.parametrize('b,c,hw', [(2, 384, 196), (2, 256, 144)])
def test_cin_stored_score_forms(F, pressure, b, c, hw):
    """cin_ax_kernel: softmax . X, W^T dY and (dG + dG^T) X of the stored-score forms (14 x 14 and 12 x 12 maps, C % 128 == 0)."""
    x, wt, g1, g2, ref = _cin_case(b, c, hw)
    xd, wd, g1d, g2d = (v.to(DEV) for v in (x, wt, g1, g2))

    def op():
        xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
        y, w = F.cin_sci(xg)
        yc = F.cin_cci(w, xg, wg)
        ((y * g1d).sum() + (yc * g2d).sum()).backward()
        x2 = xd.clone().requires_grad_(True)                                             # SCI alone: the gradient without the extra term
        (F.cin_sci(x2)[0] * g1d).sum().backward()
        return [w, y, yc, xg.grad, wg.grad, x2.grad]

    def check(first):
        w, y, yc, dx, dw, dx2 = first
        assert rel(w, ref[0]) < 2e-6 and rel(y, ref[1]) < 2e-6 and rel(yc, ref[2]) < 5e-6
        assert rel(dx, ref[3]) < 2e-5 and rel(dw, ref[4]) < 2e-5
        assert rel(dx2, ref[5]) < 2e-5
    pressure(op, check)


# ------------------------------------------------------------------------------------------------ csrc/linear.hip
@functools.lru_cache(maxsize=None)
def _linear_case(b, j, k, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(b, j, generator=gen)
    w = torch.randn(k, j, generator=gen) / j ** 0.5
    bias = torch.randn(k, generator=gen)
    g = torch.randn(b, k, generator=gen)
    out = torch.nn.functional.linear(y.double(), w.double(), bias.double())
    return y, w, bias, g, out, g.double() @ w.double(), g.double().t() @ y.double(), g.double().sum(0)


@pytest.mark.parametrize('b,j,k,seed', [(64, 4096, 200, 64 * 1000 + 4096), (64, 32896, 200, 64 + 32896 + 200)], ids=['2-chunk-slabs', '5-chunk-slabs'])
def test_classifier_forward(F, pressure, b, j, k, seed):
    """hk_linear_fwd -> linear_skinny_kernel, four LDS-DMA stages.  (64, 4096) -> 200, judged as test_linear_split_k (its inputs, the
    automatic slab count): 128 chunks over 256 wanted slabs, two chunks per slab - fewer than the stages, so every barrier of this
    shape waits for all loads; it is here for the prologue and the drain.  (64, 32896) -> 200, MPN's width, inputs and bound as
    test_linear_wide_classifier_kernel: 1028 chunks, five per slab - chunks 3 and 4 are issued inside the loop and the barriers
    that end chunks 0 and 1 wait with vmcnt(n) for everything but the pieces just issued: the counted wait."""
    from hawkeye_amd import _lib
    from hawkeye_amd.functional import ptr, stream
    lib = _lib.load()
    y, w, bias, _, o64 = _linear_case(b, j, k, seed)[:5]
    yg, wg, bg = y.to(DEV), w.to(DEV), bias.to(DEV)
    nws = lib.hk_linear_ws_bytes(b, j, k)

    def op():
        out = torch.full((b, k), NAN, device=DEV)
        ws = _nan_bytes(nws)
        assert lib.hk_linear_fwd(ptr(yg), ptr(wg), ptr(bg), ptr(out), b, j, k, ptr(ws), nws, stream()) == 0
        return [out]

    def check(first):
        assert rel(first[0], o64) < 2e-6
    pressure(op, check)


@pytest.mark.parametrize('b,j,k', [(2, 32896, 200), (16, 20032, 1000)], ids=['bwd64-two-samples', 'bwd16'])
def test_classifier_backward(F, pressure, b, j, k):
    """hk_linear_bwd, judged as test_linear_bwd_direct_at_classifier_shapes (both shapes are cases of it).
    (2, 32896) -> 200: B <= 64, K <= 208, J >= 4096 is linear_bwd64_kernel<50, 0> - the kernel with the LDS-DMA stages and the
    counted HK_VM_BARRIER(n) - at a two-sample batch: one ragged sample tile, 514 chunks, three per workgroup, where the test at the
    metric's shape (tests/test_gpu_full_shapes.py) has 64 samples and 16 chunks per workgroup.
    (16, 20032) -> 1000: K >= 256 is linear_bwd16_kernel.  It has no untracked load and no counted wait - it waits by the
    compiler's counts - so it is outside this file's criterion; the case is here so that the kernel is not taken for covered by the
    first one."""
    from hawkeye_amd import _lib
    from hawkeye_amd.functional import ptr, stream
    lib = _lib.load()
    y, w, _, g, _, dy64, dw64, db64 = _linear_case(b, j, k, j + k)
    yg, wg, gg = y.to(DEV), w.to(DEV), g.to(DEV)

    def op():
        dy, dw, db = torch.full((b, j), NAN, device=DEV), torch.full((k, j), NAN, device=DEV), torch.full((k,), NAN, device=DEV)
        assert lib.hk_linear_bwd(ptr(yg), ptr(wg), ptr(gg), ptr(dy), ptr(dw), ptr(db), b, j, k, stream()) == 0
        return [dy, dw, db]

    def check(first):
        dy, dw, db = first
        assert rel(dy, dy64) < 2e-6 and rel(dw, dw64) < 2e-6 and rel(db, db64) < 2e-6
        assert float((dy.double().cpu() - dy64).abs().max()) < 1e-5 * float(dy64.abs().max())
        assert float((dw.double().cpu() - dw64).abs().max()) < 1e-5 * float(dw64.abs().max())
    pressure(op, check)


# ------------------------------------------------------------------------------------------------ hk_bwd3.h, hk_bwd3c.h
@functools.lru_cache(maxsize=None)
def _gram_case(b, c, hw):
    """The inputs of test_backward_bwd3_kernel (the BCNN mode) and the oracle's gradient."""
    x = torch.relu(torch.randn(b, c, hw, hw, generator=torch.Generator().manual_seed(c + hw)))
    wt = torch.randn(b, c * c, generator=torch.Generator().manual_seed(1))
    xo = x.clone().requires_grad_(True)
    (O.bilinear_pool(xo) * wt).sum().backward()
    return x, wt, xo.grad


@pytest.mark.parametrize('rows', ['rows128', 'rows64'])
def test_gram_backward_bwd3_kernel(F, tune, pressure, rows):
    """gram_bwd3_kernel (LDS-DMA staging) in its 128-row and 64-row form, judged as test_backward_bwd3_kernel: against the four-wave
    panel kernel (bwd_v 1) and the oracle."""
    b, c, hw = 2, 128, 14
    x, wt, ref = _gram_case(b, c, hw)
    xd, wd = x.to(DEV), wt.to(DEV)

    def grad():
        xg = xd.clone().requires_grad_(True)
        (F.bilinear_pool(xg) * wd).sum().backward()
        return [xg.grad]
    tune('bwd_v', 1)
    tune('sched_b', 0)
    panel = grad()[0].clone()
    tune('bwd_v', 0)
    tune('sched_b', _fill_batches(c)[rows])

    def check(first):
        assert rel(first[0], panel) < 2e-6 and rel(first[0], ref) < 2e-5
    assert rel(panel, ref) < 2e-5
    pressure(grad, check)


@functools.lru_cache(maxsize=None)
def _cbp_case(b, c, hw, d):
    """The inputs of test_cbp_backward_bwd3c_kernel and the oracle's float64 gradient."""
    gen = torch.Generator().manual_seed(c + hw + d)
    x = torch.relu(torch.randn(b, c, hw, hw, generator=gen))
    wt = torch.randn(b, d, generator=gen)
    xo = x.clone().double().requires_grad_(True)
    (O.compact_bilinear_pool_gram(xo, d) * wt.double()).sum().backward()
    return x, wt, xo.grad


@pytest.mark.parametrize('rows', ['rows128', 'rows64', 'colsplit'])
def test_cbp_backward_bwd3c_kernel(F, tune, pressure, rows):
    """cbp_bwd3_kernel at (2, 128, 14 x 14) -> D 2048, judged as test_cbp_backward_bwd3c_kernel: against the 64-row panel kernel
    behind cbp_dc1_kernel (bwd_v 1) and, through it, against the oracle in float64 (its bound: 1e-4 + 50 x the panel kernel's own
    distance).  The kernel has three shapes - 128-row blocks, 64-row blocks, column tiles divided between two workgroups - with their
    own staging loops, so each gets its launches."""
    b, c, hw, d = 2, 128, 14, 2048
    x, wt, ref64 = _cbp_case(b, c, hw, d)
    x, wt = x.to(DEV), wt.to(DEV)
    plan = F.CbpPlan(*F.sketch_hashes(c, c, d), d, torch.device('cuda', torch.cuda.current_device()))

    def grad(v, sb):
        tune('bwd_v', v)
        tune('sched_b', 0)                      # (the forward's work split sees the real batch: the same y for every form)
        xg = x.clone().requires_grad_(True)
        loss = (F.compact_bilinear_pool(xg, plan) * wt).sum()
        tune('sched_b', sb)
        loss.backward()
        return [xg.grad]
    panel = grad(1, 0)[0].clone()
    sb = _fill_batches(c)[rows]

    def check(first):
        assert rel(first[0], panel) < 2e-6
        assert rel(first[0], ref64) < 1e-4 + 50 * rel(panel, ref64)
    pressure(lambda: grad(0, sb), check)
