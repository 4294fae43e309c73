"""The weight tiles of conv3x3_split_kernel by LDS-DMA (csrc/conv_fwd.hip, load_w) on the GPU: forward, input gradient and the four
epilogues on both MFMA shapes at the shapes of tests/conv_wdma_cases.py, every output bit-equal to what the register-staged kernel of the
commit before gave on the MI355X (tests/golden/conv_wdma_gpu.json, SHA-256 digests recorded with tools/gen_conv_wdma_golden.py gpu on that
commit's build), the same bits from a second launch, and the 1e30 guard rows around x, w, the workspace and the outputs intact."""
import pytest
import torch

import conv_wdma_cases as W
from conv_fwd_cases import case
from test_gpu_conv_fwd import _guarded, _raw

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


@pytest.fixture(scope='module')
def recorded():
    return W.golden('gpu')


@pytest.mark.parametrize('mf', (0, 1), ids=('mfma32', 'mfma16'))
@pytest.mark.parametrize('shape', W.SHAPES, ids=W.IDS)
def test_every_output_keeps_the_bits_of_the_register_staged_kernel(F, recorded, shape, mf):
    from hawkeye_amd import _lib
    want = recorded['x'.join(map(str, shape))][f'mf{mf}']
    first = W.digests(_lib.load(), torch.device(DEV), shape, mf, _lib.stream())         # (asserts the guard rows of every buffer)
    again = W.digests(_lib.load(), torch.device(DEV), shape, mf, _lib.stream())
    assert first == again, (shape, mf, 'two launches', [k for k in first if first[k] != again[k]])
    differ = [k for k in want if first.get(k) != want[k]]
    assert sorted(first) == sorted(want) and not differ, (shape, mf, differ)


@pytest.mark.parametrize('mf', (0, 1), ids=('mfma32', 'mfma16'))
def test_guard_rows_with_the_helpers_of_the_forward_tests(F, tune, mf):
    """The entry points themselves on buffers between guard rows (test_gpu_conv_fwd's helpers): ragged tiles in both directions, two
    images, the workspace exactly as large as hk_conv3x3_ws_bytes says and guarded as well."""
    from hawkeye_amd import _lib
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    tune('conv_mfma', mf)
    shape = W.SHAPES[1]
    x, wt, dy = case(shape)[:3]
    xg, wg, dyg = x.to(DEV), wt.to(DEV), dy.to(DEV)
    need = _lib.load().hk_conv3x3_ws_bytes(shape[3], shape[4])
    for fn, src, call in (('hk_conv3x3_fwd', xg, F.conv3x3_fwd_raw), ('hk_conv3x3_bwd_data', dyg, F.conv3x3_bwd_data_raw)):
        plain = call(src, wg)
        gsrc, sbig, spad = _guarded(src)
        gw, wbig, wpad = _guarded(wg)
        gout, big, pad = _guarded(torch.zeros_like(plain))
        wsbig = torch.full((need + 8192,), 0xA5, dtype=torch.uint8, device=DEV)
        assert _raw(F, fn, gsrc, gw, gout, ws=wsbig[4096:4096 + need]) == 0
        assert torch.equal(gout, plain)
        assert bool((big[:pad] == 1e30).all()) and bool((big[pad + plain.numel():] == 1e30).all())
        assert bool((sbig[:spad] == 1e30).all()) and bool((sbig[spad + src.numel():] == 1e30).all())
        assert bool((wbig[:wpad] == 1e30).all()) and bool((wbig[wpad + wg.numel():] == 1e30).all())
        assert bool((wsbig[:4096] == 0xA5).all()) and bool((wsbig[4096 + need:] == 0xA5).all())
