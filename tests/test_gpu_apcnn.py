"""GPU tier: csrc/apcnn.hip, apcnn_roi2.hip, osme.hip and mamc.hip of the gfx950 build - the cases of the emulated tier
(test_emu_apcnn.py) on the device: the ROI crop + resize on both sides of every dispatch threshold against float64, the
attention ROI selection on non-square maps and above 64 KB of LDS, the attention pooling's edges, OSME with and without dz,
the n-pairs loss with two trips of the row kernel's loops.  The two refusals return before any launch."""
import pytest
import torch

import apcnn_ops as A

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
MODES = ('eval', 'train')
SMALL_MAPS = [m for m in A.ROI_MAPS if max(m) <= 64]


def map_id(m):
    return '{}x{}'.format(*m)


def shape_id(case):
    return '-'.join(str(v) for v in case).replace(' ', '')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('hw', A.ROI_MAPS, ids=map_id)
def test_roi_crop_against_float64(hw, mode):
    print(f"worst ratio {A.check_roi_case(*hw, mode == 'train', DEV):.3f}")


@pytest.mark.parametrize('shape', A.ROI_CPB_CASES, ids=shape_id)
def test_roi_crop_ragged_last_group_of_maps(shape):
    print(f'worst ratio {A.check_roi_cpb(shape, DEV):.3f}')


@pytest.mark.parametrize('hw', SMALL_MAPS, ids=map_id)
def test_roi_crop_staged_and_table_kernels_give_the_same_bits(hw, tune):
    A.check_roi_kernel_pairs(*hw, DEV, tune)


@pytest.mark.parametrize('ncls', [200, 8142])
@pytest.mark.parametrize('case', A.SELECT_CASES, ids=A.select_case_id)
def test_att_roi_select_bit_exact(case, ncls):
    A.check_select_case(case, ncls, DEV)


@pytest.mark.parametrize('ncls', [200, 8142])
def test_att_roi_select_three_non_square_levels_in_one_launch(ncls):
    A.check_select_levels(ncls, DEV)


def test_att_roi_select_refuses_a_140x140_map():
    A.check_select_refused(DEV)


@pytest.mark.parametrize('att', [True, False], ids=['attention', 'plain'])
@pytest.mark.parametrize('case', A.POOL_CASES, ids=shape_id)
def test_att_pool_against_float64(case, att):
    print(f'worst ratio {A.check_pool_case(case, att, DEV):.3f}')


@pytest.mark.parametrize('case', A.POOL_LEVEL_CASES, ids=shape_id)
def test_att_pool_levels_give_the_bits_of_three_calls(case):
    print(f'worst ratio {A.check_pool_levels(case, DEV):.3f}')


def test_att_pool_backward_refuses_8193_channels():
    print(f'worst ratio {A.check_pool_refused(DEV):.3f}')


@pytest.mark.parametrize('case', A.OSME_CASES, ids=shape_id)
def test_osme_against_float64(case):
    print(f'worst ratio {A.check_osme_case(case, DEV):.3f}')


@pytest.mark.parametrize('case', A.NPAIRS_CASES, ids=shape_id)
def test_npairs_loss_against_float64(case):
    print(f'worst ratio {A.check_npairs_case(case, DEV):.3f}')
