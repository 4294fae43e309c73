"""The tile geometries of conv3x3_split_kernel (csrc/conv_fwd.hip, G: 8 x 16 and 16 x 8 besides 4 x 32) on the GPU: forward, input gradient
and the four epilogues on both MFMA shapes at the shapes of tests/conv_tile_cases.py, every output with the planned tiling bit-equal to
4 x 32 everywhere (the bias gradient as that module says), the same bits from a second launch, the plan itself asserted through
hk_conv3x3_tile_plan and the 1e30 guard rows around x, w, the workspace and the outputs intact."""
import pytest
import torch

import conv_tile_cases as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return _lib.load()


@pytest.mark.parametrize('mf', (0, 1), ids=('mfma32', 'mfma16'))
@pytest.mark.parametrize('shape', T.SHAPES, ids=T.IDS)
def test_every_output_keeps_the_bits_of_4x32(lib, shape, mf):
    from hawkeye_amd import _lib
    T.check_against_4x32(lib, torch.device(DEV), shape, mf, _lib.stream(), twice=True)
