"""The tile geometries of conv3x3_split_kernel (csrc/conv_fwd.hip, G: 8 x 16 and 16 x 8 besides 4 x 32) through the CPU emulation, with no
GPU: forward, input gradient and the four epilogues on both MFMA shapes at the shapes of tests/conv_tile_cases.py, every output with the
planned tiling bit-equal to 4 x 32 everywhere, the plan itself asserted through hk_conv3x3_tile_plan, the guard rows intact.  The shape
with two regions in one launch also with the work-items of a workgroup resumed in reverse.  HK_EMU_FULL=1 adds the largest shape."""
import os

import pytest
import torch

import conv_tile_cases as T

CPU = torch.device('cpu')
FULL = os.environ.get('HK_EMU_FULL') == '1'
LARGEST = T.SHAPES[1]


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    from emu.harness import emulated
    with emulated() as f:
        yield f


@pytest.mark.parametrize('mf', (0, 1), ids=('mfma32', 'mfma16'))
@pytest.mark.parametrize('shape', T.SHAPES, ids=T.IDS)
def test_every_output_keeps_the_bits_of_4x32(F, shape, mf):
    from hawkeye_amd import _lib
    if shape == LARGEST and not FULL:
        pytest.skip('the largest shape takes the emulation longer than a few seconds: HK_EMU_FULL=1')
    T.check_against_4x32(_lib.load(), CPU, shape, mf)


def test_two_regions_in_one_launch_in_reverse_order(F, monkeypatch):
    from hawkeye_amd import _lib
    monkeypatch.setenv('HK_EMU_ORDER', 'rev')
    T.check_against_4x32(_lib.load(), CPU, T.MIXED, 1)
