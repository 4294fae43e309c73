"""conv3x3_split_kernel on either bf16 MFMA (csrc/conv_fwd.hip, MF; knob `conv_mfma`: 0 = 32 x 32 x 16, 1 = 16 x 16 x 32) on the GPU.

Both shapes: forward and input gradient against float64 within tests/conv_fwd_cases.py's bound (|y - y64| <= c S, c = 1e-6 for
9 Cin <= 1024 and 1.5e-6 above - the project's own, the same for either shape), the worst ratio printed beside the other shape's on
the same input; the input gradient bit-equal to the forward of dy with flipped, transposed weights; two launches bit-equal; guard
rows intact; one inf in exactly its window.  The 16 x 16 x 32 shape alone: its four epilogues, re-derived for an accumulator layout
that spreads a pixel's channel quads over four lanes, bit for bit against the two-kernel paths run under the same knob
(tests/conv_epilogue_cases.py's checks, inputs and bias-gradient bound)."""
import pytest
import torch

import conv_epilogue_cases as C
from conv_fwd_cases import IDS, SHAPES, bound, case, nhwc, within
from test_gpu_conv_fwd import _guarded, _raw

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


@pytest.fixture
def on(tune):
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    tune('conv_epi', 2)
    return tune


@pytest.fixture
def lib16(F, on):
    from hawkeye_amd import _lib
    on('conv_mfma', 1)
    return _lib.load()


def _ratio(got, ref, scale):
    return float(((got.double().cpu() - ref).abs() / scale.clamp_min(1e-300)).max())


@pytest.mark.parametrize('mfma', [0, 1])
@pytest.mark.parametrize('kind', ['relu', 'stress'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_and_input_gradient_against_float64(F, on, shape, kind, mfma):
    n, h, w, cin, cout = shape
    x, wt, dy, y64, sy, dx64, sdx = case(shape, kind)
    xg, wg, dyg = x.to(DEV), wt.to(DEV), dy.to(DEV)
    on('conv_mfma', 1 - mfma)
    other = _ratio(F.conv3x3_fwd_raw(xg, wg), y64, sy), _ratio(F.conv3x3_bwd_data_raw(dyg, wg), dx64, sdx)
    on('conv_mfma', mfma)
    y = F.conv3x3_fwd_raw(xg, wg)
    dx = F.conv3x3_bwd_data_raw(dyg, wg)
    assert tuple(y.shape) == (n, cout, h, w) and y.is_contiguous(memory_format=torch.channels_last)
    assert tuple(dx.shape) == (n, cin, h, w) and dx.is_contiguous(memory_format=torch.channels_last)
    print(f'conv_mfma {1 - mfma} {shape} {kind}: forward {other[0]:.3e}, input gradient {other[1]:.3e}')
    within(y, y64, sy, bound(cin), f'conv_mfma {mfma} forward {shape} {kind}')
    within(dx, dx64, sdx, bound(cout), f'conv_mfma {mfma} input gradient {shape} {kind}')
    wflip = nhwc(wg.flip(2, 3).transpose(0, 1))
    assert torch.equal(dx, F.conv3x3_fwd_raw(dyg, wflip))


@pytest.mark.parametrize('mfma', [0, 1])
def test_isolation_guards_and_run_to_run_bits(F, on, mfma):
    on('conv_mfma', mfma)
    shape = SHAPES[3]                                                      # ragged tiles in both directions, two images
    x, wt, dy = case(shape)[:3]
    xg, wg, dyg = x.to(DEV), wt.to(DEV), dy.to(DEV)
    for fn, src, call in (('hk_conv3x3_fwd', xg, F.conv3x3_fwd_raw), ('hk_conv3x3_bwd_data', dyg, F.conv3x3_bwd_data_raw)):
        plain = call(src, wg)
        assert torch.equal(call(src, wg), plain)                           # the same bits from run to run
        gsrc = _guarded(src)[0]
        wbig = torch.full((wg.numel() + 2048,), 1e30, device=DEV)
        gw = wbig[1024:1024 + wg.numel()].view(wg.shape[0], 3, 3, wg.shape[1])
        gw.copy_(wg.permute(0, 2, 3, 1))
        gw = gw.permute(0, 3, 1, 2)
        gout, big, pad = _guarded(torch.zeros_like(plain))
        assert _raw(F, fn, gsrc, gw, gout) == 0
        assert torch.equal(gout, plain)
        assert bool((big[:pad] == 1e30).all()) and bool((big[pad + plain.numel():] == 1e30).all())      # no store past a ragged tile


@pytest.mark.parametrize('mfma', [0, 1])
def test_one_inf_reaches_exactly_its_window(F, on, mfma):
    on('conv_mfma', mfma)
    shape = SHAPES[3]
    n, h, w, cin, cout = shape
    x, wt = case(shape)[:2]
    xg, wg = x.to(DEV), wt.to(DEV)
    clean = F.conv3x3_fwd_raw(xg, wg)
    xi = xg.clone()
    xi[1, 70, 3, 32] = float('inf')                                         # row 3, column 32: the first column of the second strip
    y = F.conv3x3_fwd_raw(xi, wg)
    hit = torch.zeros(n, 1, h, w, dtype=torch.bool, device=DEV)
    hit[1, 0, 2:5, 31:34] = True
    hit = hit.expand(n, cout, h, w)
    assert torch.equal(~torch.isfinite(y), hit)
    assert torch.equal(y[~hit], clean[~hit])


def test_the_knob_switches_kernels(F, on):
    x, wt = case(SHAPES[4])[:2]                                             # 192 channels: chains long enough to round differently
    xg, wg = x.to(DEV), wt.to(DEV)
    on('conv_mfma', 0)
    a = F.conv3x3_fwd_raw(xg, wg)
    on('conv_mfma', 1)
    assert not torch.equal(a, F.conv3x3_fwd_raw(xg, wg))


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', C.SHAPES_A, ids=C.ids(C.SHAPES_A))
def test_bias_relu_forward_equals_the_two_kernels(F, lib16, shape, variant):
    C.check_bias_relu(F, lib16, DEV, shape, variant)


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', C.SHAPES_B, ids=C.ids(C.SHAPES_B))
def test_bias_relu_pool_forward_equals_the_two_kernels(F, lib16, shape, variant):
    C.check_bias_relu_pool(F, lib16, DEV, shape, variant)


@pytest.mark.parametrize('variant', ['random', 'set'])
@pytest.mark.parametrize('shape', C.SHAPES_A, ids=C.ids(C.SHAPES_A))
def test_masked_input_gradient_equals_the_two_kernels(F, lib16, shape, variant):
    C.check_masked_bwd_data(F, lib16, DEV, shape, variant)


def test_stack_with_the_epilogues_inside_against_the_passes(F, lib16, on, monkeypatch):
    C.check_stack(F, lib16, DEV, on, monkeypatch)
