"""hk_conv3x3_wrw_pooled (csrc/conv_wrw.hip, "Pooled") through the CPU emulation, with no GPU: the cases of tests/wrw_pool_cases.py.
What the emulation shows: the window image of wrp_aoff, the k order of wrp_kpix against the sparse instruction's operand and index
layout (tests/emu/shim/hk_smfmac_bf16.h, the layout measured on the device), the five-slot ring with its two barriers, the even row
blocks and the flush.  That the device's transposing reads and its instruction agree with both is tests/test_gpu_wrw_pool.py's."""
import pytest
import torch

import wrw_pool_cases as C

CPU = torch.device('cpu')
EACH = pytest.mark.parametrize('shape,wgs', C.CASES, ids=C.IDS)


@pytest.fixture(scope='module')
def lib():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    from emu.harness import load_emu
    return load_emu()


def _run(lib, c, wgs=0, **kw):
    x, dp, p, am = c[:4]
    return C.run(lib, CPU, x, dp, p, am, wgs, **kw)


@EACH
def test_small_integers_give_the_float64_gradient_exactly(lib, monkeypatch, shape, wgs):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    c = C.case(shape, 'int')
    dw = _run(lib, c, wgs)
    assert torch.equal(dw.double(), c[5]), (shape, int((dw.double() != c[5]).sum()))


@EACH
def test_randn_within_the_bound_beside_the_dense_kernel(lib, monkeypatch, shape, wgs):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    c = C.case(shape, 'randn')
    dw = _run(lib, c, wgs)
    ratio, diff = C.M.worst(dw, c[5], c[6])
    dense, _ = C.M.worst(C.run_dense(lib, CPU, c[0], c[4], wgs), c[5], c[6])
    print(f'{shape}: max |dW - dW64| / S = {ratio:.3e} pooled, {dense:.3e} dense on g (bound {C.bound(shape):.1e})')
    assert bool((diff <= C.bound(shape) * c[6]).all()), (shape, ratio)
    assert torch.equal(_run(lib, c, wgs, guarded=False), dw), shape                 # a second launch: the same bits


@pytest.mark.parametrize('order', ('rev', 'rand:11'))
@EACH
def test_any_work_item_order_gives_the_same_integers(lib, monkeypatch, shape, wgs, order):
    monkeypatch.setenv('HK_EMU_ORDER', order)
    c = C.case(shape, 'int')
    assert torch.equal(_run(lib, c, wgs).double(), c[5]), (shape, order)


@pytest.mark.parametrize('kind', ('codes 0', 'codes 3', 'one window column'))
def test_every_code_and_one_column_of_windows(lib, monkeypatch, kind):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    c = C.case(C.SMALL, kind)
    ratio, diff = C.M.worst(_run(lib, c), c[5], c[6])
    print(f'{kind}: max |dW - dW64| / S = {ratio:.3e} (bound {C.bound(C.SMALL):.1e})')
    assert bool((diff <= C.bound(C.SMALL) * c[6]).all()), (kind, ratio)


def test_every_value_masked_gives_exact_zeros(lib, monkeypatch):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    c = C.case(C.SMALL, 'all masked')
    assert float(c[4].abs().max()) == 0.0
    assert float(_run(lib, c).abs().max()) == 0.0


@pytest.mark.parametrize('kind', C.M.STRESS_KINDS)
def test_inputs_that_stress_the_split(lib, monkeypatch, kind):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    c = C.stress(kind)
    ratio, diff = C.M.worst(_run(lib, c), c[5], c[6])
    bound = C.bound(C.M.STRESS_SHAPE)                                               # the stress inputs' own shape: dp is their dy
    print(f'{kind}: max |dW - dW64| / S = {ratio:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * c[6]).all()), (kind, ratio)


def test_the_images_add_up_and_a_wide_call_is_its_64_channel_slices(lib, monkeypatch):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    x, dp, p, am, _, ref, scale = C.case(C.SMALL, 'randn')                          # (2, 6, 28, 256, 64)
    dw = C.run(lib, CPU, x, dp, p, am, 2)
    one = sum(C.run(lib, CPU, x[i:i + 1], dp[i:i + 1], p[i:i + 1], am[i:i + 1], 2).double() for i in range(2))
    assert bool(((one - dw.double()).abs() <= 1e-6 * scale).all())
    cl = torch.channels_last
    for s in range(4):                                                              # the same workgroups per slice: the same jobs, the same bits
        xs = x[:, 64 * s:64 * s + 64].contiguous(memory_format=cl)
        assert torch.equal(C.run(lib, CPU, xs, dp, p, am, 2), dw[:, 64 * s:64 * s + 64]), s


def test_knob_round_trip_and_who_is_served(lib):
    for v in (0, 1, -1):
        with C.M.Knobs(lib, wrw_pool=v):
            assert C.M.knob(lib, 'wrw_pool') == v
            assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 256, 64) == (1 if v == 1 else 0)         # below what the rule was measured on
            assert lib.hk_conv3x3_wrw_pooled_served(16, 28, 28, 512, 512) == (0 if v == 0 else 1)      # conv5_3 at batch 16: the rule's smallest map
            assert lib.hk_conv3x3_wrw_pooled_served(64, 448, 448, 64, 64) == (0 if v == 0 else 1)      # conv1_2 at batch 64
    with C.M.Knobs(lib, wrw_pool=1):
        assert lib.hk_conv3x3_wrw_pooled_served(2, 7, 28, 256, 64) == 0             # odd H
        assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 27, 256, 64) == 0             # odd W
        assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 96, 64) == 0              # Cin no multiple of 64
        with C.M.Knobs(lib, wrw_split=0):
            assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 256, 64) == 0
        # the kernel's lane offsets are 32-bit bytes into a row: a row of x, or a window row of dp, of 2^31 bytes or more is refused
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, (1 << 20) - 2, 512, 64) == 1
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, 1 << 20, 512, 64) == 0
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, 1 << 21, 64, 512) == 0
    x, dp, p, am = C.case((1, 2, 2, 64, 64), 'int')[:4]
    ws = torch.empty(lib.hk_conv3x3_wrw_ws_bytes(64, 64), dtype=torch.uint8)
    dw = torch.empty(64 * 9 * 64)
    q = C._p
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 3, 2, 64, 64, q(ws), ws.numel(), None) == -3       # odd H: unsupported
    ws2 = torch.empty(lib.hk_conv3x3_wrw_ws_bytes(512, 64), dtype=torch.uint8)
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 2, 1 << 20, 512, 64, q(ws2), ws2.numel(), None) == -3   # a 2^31-byte row: refused before any launch
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 2, 2, 64, 64, q(ws), ws.numel() - 1, None) == -2   # workspace
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), None, q(x), q(dw), 1, 2, 2, 64, 64, q(ws), ws.numel(), None) == -1        # null


@pytest.mark.parametrize('wgs', (0, 1, 3, 7))
def test_row_blocks_start_on_even_rows_and_cover_the_map(lib, wgs):
    with C.M.Knobs(lib, wrw_wgs=wgs):
        for h in range(2, 71, 2):
            for n, w in ((1, 32), (3, 70)):
                rc, (nstrips, nrb, rpb, njobs, nwg) = C.plan(lib, n, h, w, 64, 64)
                assert rc == 0
                assert rpb % 2 == 0 and rpb >= 2, (h, rpb)
                assert (nrb - 1) * rpb < h <= nrb * rpb, (h, nrb, rpb)                # every block has rows, the last one ends at H
                assert nstrips == (w + 31) // 32 and njobs == n * nstrips * nrb and 1 <= nwg <= njobs
                if wgs:
                    assert nwg <= wgs
        assert C.plan(lib, 1, 7, 32, 64, 64)[0] == -3
