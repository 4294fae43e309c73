"""conv3x3_wrw_split_kernel on either bf16 MFMA (csrc/conv_wrw.hip, MF; knob `wrw_mfma`: 0 = 32 x 32 x 16, 1 = 16 x 16 x 32) on the GPU:
the cases of tests/wrw_mfma_cases.py.  What only the device shows: that ds_read_b64_tr_b16 over the image of wrs16_off hands each lane
the pixels wrs16_kpix names, and that v_mfma_f32_16x16x32_bf16 takes and returns the layouts the kernel assumes - on small integers any
disagreement gives a wrong integer, and the result has to equal the float64 gradient exactly.

`wrw_mfma` 0 is held to the bits of the commit before (tests/golden/wrw_mfma_gpu.json, tools/gen_wrw_mfma_golden.py gpu on that build)."""
import pytest
import torch

import wrw_mfma_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
MFS = pytest.mark.parametrize('mf', (1, 0), ids=('mfma16', 'mfma32'))
EACH = pytest.mark.parametrize('shape,wgs', C.CASES, ids=C.IDS)


@pytest.fixture(scope='module')
def lib():
    from hawkeye_amd import _lib
    lib_ = _lib.load()
    assert b'gfx950' in lib_.hk_version()
    return lib_


def _run(lib, x, dy, mf, wgs=0, guarded=True):
    from hawkeye_amd import _lib
    return C.run(lib, DEV, x, dy, mf, wgs, _lib.stream(), guarded)


@pytest.fixture(scope='module')
def results(lib):
    """dW on the 'randn' inputs: made once per (case, MFMA shape), shared, never written to."""
    memo = {}

    def get(shape, wgs, mf):
        if (shape, wgs, mf) not in memo:
            x, dy, _, _ = C.case(shape, 'randn')
            memo[shape, wgs, mf] = _run(lib, x, dy, mf, wgs)
        return memo[shape, wgs, mf]
    return get


@MFS
@EACH
def test_small_integers_give_the_float64_gradient_exactly(lib, shape, wgs, mf):
    x, dy, ref, _ = C.case(shape, 'int')
    dw = _run(lib, x, dy, mf, wgs)
    assert torch.equal(dw.double(), ref), (shape, mf, int((dw.double() != ref).sum()))


@EACH
def test_randn_within_the_bound_on_both_shapes_and_mfma32_keeps_its_bits(lib, results, shape, wgs):
    x, dy, ref, scale = C.case(shape, 'randn')
    got = {mf: results(shape, wgs, mf) for mf in (1, 0)}
    ratio = {mf: C.worst(got[mf], ref, scale) for mf in (1, 0)}
    print(f'{shape}: max |dW - dW64| / S = {ratio[1][0]:.3e} on 16x16x32, {ratio[0][0]:.3e} on 32x32x16 (bound {C.bound(shape):.1e})')
    for mf in (1, 0):
        assert bool((ratio[mf][1] <= C.bound(shape) * scale).all()), (shape, mf, ratio[mf][0])
    name = C.IDS[C.CASES.index((shape, wgs))]
    assert C.digest(got[0]) == C.golden('gpu')[name], (name, 'wrw_mfma 0 no longer gives the bits of the commit before')
    # a second call, on buffers without guard rows: the same bits
    for mf in (1, 0):
        assert torch.equal(_run(lib, x, dy, mf, wgs, guarded=False), got[mf]), (shape, mf)


@pytest.mark.parametrize('kind', C.STRESS_KINDS)
def test_inputs_that_stress_the_split(lib, kind):
    x, dy, ref, scale = C.stress(kind)
    ratio = {mf: C.worst(_run(lib, x, dy, mf), ref, scale) for mf in (1, 0)}
    print(f'{kind}: max |dW - dW64| / S = {ratio[1][0]:.3e} on 16x16x32, {ratio[0][0]:.3e} on 32x32x16 (bound 1.0e-06)')
    for mf in (1, 0):
        assert bool((ratio[mf][1] <= 1e-6 * scale).all()), (kind, mf, ratio[mf][0])


@MFS
def test_the_images_add_up_and_a_wide_call_is_its_64_channel_slices(lib, results, mf):
    shape, wgs = C.CASES[3]                                            # (2, 6, 28, 256, 64)
    x, dy, _, _ = C.case(shape, 'randn')
    dw = results(shape, wgs, mf)
    parts = sum(_run(lib, x[i:i + 1], dy[i:i + 1], mf, wgs).double() for i in range(shape[0]))
    assert float((dw.double() - parts).norm() / parts.norm()) < 1e-6
    # a Cin slice is what the same MFMA shape gives for those 64 channels alone (same jobs, same workgroups), bit for bit
    for s in range(shape[3] // 64):
        alone = _run(lib, x[:, 64 * s:64 * s + 64].contiguous(memory_format=torch.channels_last), dy, mf, wgs)
        assert torch.equal(dw[:, 64 * s:64 * s + 64], alone), (mf, s)


def test_the_knob_and_the_rule_behind_its_default(lib, results):
    """`wrw_mfma` round-trips through hk_tuning_get (C.Knobs asserts it at every value); at -1 the rule of conv_wrw.hip decides: every
    call runs on 16 x 16 x 32 - seen here by its bits, which are not the other shape's."""
    assert C.knob(lib, 'wrw_mfma') == -1
    for shape, wgs in (C.CASES[2], C.CASES[4]):                        # a wide call and a 64-channel one
        x, dy, _, _ = C.case(shape, 'randn')
        by_rule = _run(lib, x, dy, -1, wgs)
        assert torch.equal(by_rule, results(shape, wgs, 1)) and not torch.equal(by_rule, results(shape, wgs, 0)), shape
    assert C.knob(lib, 'wrw_mfma') == -1
