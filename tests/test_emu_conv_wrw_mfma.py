"""conv3x3_wrw_split_kernel on either bf16 MFMA (csrc/conv_wrw.hip, MF; knob `wrw_mfma`: 0 = 32 x 32 x 16, 1 = 16 x 16 x 32) through the
CPU emulation, with no GPU: the plane image of wrs16_off, the permuted k of wrs16_kpix, the kw offsets, the 16 x 16 C layout at the
flush, and `MF = 0` held to the bits of the commit before (tests/golden/wrw_mfma_emu.json, tools/gen_wrw_mfma_golden.py emu).

The emulation reads the fragments through wrs16_frag's host twin and the model of the instruction in tests/emu/shim/hk_mfma_bf16.h:
that the device's transposing reads and its MFMA agree with both is tests/test_gpu_conv_wrw_mfma.py's to show."""
import pytest
import torch

import wrw_mfma_cases as C

CPU = torch.device('cpu')
MFS = pytest.mark.parametrize('mf', (1, 0), ids=('mfma16', 'mfma32'))
EACH = pytest.mark.parametrize('shape,wgs', C.CASES, ids=C.IDS)


@pytest.fixture(scope='module')
def lib():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    from emu.harness import load_emu
    return load_emu()


@pytest.fixture(scope='module')
def results(lib):
    """dW on the 'randn' inputs in the emulator's own work-item order: made once per (case, MFMA shape), shared, never written to."""
    memo = {}

    def get(shape, wgs, mf):
        if (shape, wgs, mf) not in memo:
            x, dy, _, _ = C.case(shape, 'randn')
            memo[shape, wgs, mf] = C.run(lib, CPU, x, dy, mf, wgs)
        return memo[shape, wgs, mf]
    return get


@MFS
@EACH
def test_small_integers_give_the_float64_gradient_exactly(lib, monkeypatch, shape, wgs, mf):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    x, dy, ref, _ = C.case(shape, 'int')
    dw = C.run(lib, CPU, x, dy, mf, wgs)
    assert torch.equal(dw.double(), ref), (shape, mf, int((dw.double() != ref).sum()))


@EACH
def test_randn_within_the_bound_on_both_shapes_and_mfma32_keeps_its_bits(lib, results, monkeypatch, shape, wgs):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    x, dy, ref, scale = C.case(shape, 'randn')
    got = {mf: results(shape, wgs, mf) for mf in (1, 0)}
    ratio = {mf: C.worst(got[mf], ref, scale) for mf in (1, 0)}
    print(f'{shape}: max |dW - dW64| / S = {ratio[1][0]:.3e} on 16x16x32, {ratio[0][0]:.3e} on 32x32x16 (bound {C.bound(shape):.1e})')
    for mf in (1, 0):
        assert bool((ratio[mf][1] <= C.bound(shape) * scale).all()), (shape, mf, ratio[mf][0])
    name = C.IDS[C.CASES.index((shape, wgs))]
    assert C.digest(got[0]) == C.golden('emu')[name], (name, 'wrw_mfma 0 no longer gives the bits of the commit before')
    # a second call, on buffers without guard rows: the same bits
    for mf in (1, 0):
        assert torch.equal(C.run(lib, CPU, x, dy, mf, wgs, guarded=False), got[mf]), (shape, mf)


@pytest.mark.parametrize('order', ('rev', 'rand:11'))
@MFS
@EACH
def test_the_bits_do_not_depend_on_the_order_of_the_work_items(lib, results, monkeypatch, shape, wgs, mf, order):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    base = results(shape, wgs, mf)
    monkeypatch.setenv('HK_EMU_ORDER', order)
    x, dy, _, _ = C.case(shape, 'randn')
    assert torch.equal(C.run(lib, CPU, x, dy, mf, wgs), base), (shape, mf, order)


@pytest.mark.parametrize('kind', C.STRESS_KINDS)
def test_inputs_that_stress_the_split(lib, monkeypatch, kind):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    x, dy, ref, scale = C.stress(kind)
    ratio = {mf: C.worst(C.run(lib, CPU, x, dy, mf), ref, scale) for mf in (1, 0)}
    print(f'{kind}: max |dW - dW64| / S = {ratio[1][0]:.3e} on 16x16x32, {ratio[0][0]:.3e} on 32x32x16 (bound 1.0e-06)')
    for mf in (1, 0):
        assert bool((ratio[mf][1] <= 1e-6 * scale).all()), (kind, mf, ratio[mf][0])


@MFS
def test_the_images_add_up_and_a_wide_call_is_its_64_channel_slices(lib, results, monkeypatch, mf):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    shape, wgs = C.CASES[3]                                            # (2, 6, 28, 256, 64)
    x, dy, _, _ = C.case(shape, 'randn')
    dw = results(shape, wgs, mf)
    parts = sum(C.run(lib, CPU, x[i:i + 1], dy[i:i + 1], mf, wgs).double() for i in range(shape[0]))
    assert float((dw.double() - parts).norm() / parts.norm()) < 1e-6
    # a Cin slice is what the same MFMA shape gives for those 64 channels alone (same jobs, same workgroups), bit for bit
    for s in range(shape[3] // 64):
        alone = C.run(lib, CPU, x[:, 64 * s:64 * s + 64].contiguous(memory_format=torch.channels_last), dy, mf, wgs)
        assert torch.equal(dw[:, 64 * s:64 * s + 64], alone), (mf, s)


def test_the_knob_and_the_rule_behind_its_default(lib, results, monkeypatch):
    """`wrw_mfma` round-trips through hk_tuning_get (C.Knobs asserts it at every value); at -1 the rule of conv_wrw.hip decides: every
    call runs on 16 x 16 x 32 - seen here by its bits, which are not the other shape's."""
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    assert C.knob(lib, 'wrw_mfma') == -1
    for shape, wgs in (C.CASES[2], C.CASES[4]):                        # a wide call and a 64-channel one
        x, dy, _, _ = C.case(shape, 'randn')
        by_rule = C.run(lib, CPU, x, dy, -1, wgs)
        assert torch.equal(by_rule, results(shape, wgs, 1)) and not torch.equal(by_rule, results(shape, wgs, 0)), shape
    assert C.knob(lib, 'wrw_mfma') == -1
