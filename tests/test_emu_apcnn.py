"""CPU tier: csrc/apcnn.hip, apcnn_roi2.hip, osme.hip and mamc.hip compiled for the host (tests/emu) - every kernel form of the
first-generation heads against the reference's op sequence in float64: the ROI crop + resize on maps on both sides of every
dispatch threshold in eval and train mode, the attention ROI selection on non-square maps, the attention pooling's edges,
OSME with and without dz, the n-pairs loss with two trips of the row kernel's loops.  Test infrastructure only."""
import pytest
import torch

from emu.harness import emulated

import apcnn_ops as A

CPU = torch.device('cpu')
MODES = ('eval', 'train')
SMALL_MAPS = [m for m in A.ROI_MAPS if max(m) <= 64]        # (no case here takes more than about a second when emulated)


@pytest.fixture(autouse=True, scope='module')
def _emulated_kernels():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated():
        yield


def map_id(m):
    return '{}x{}'.format(*m)


def shape_id(case):
    return '-'.join(str(v) for v in case).replace(' ', '')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('hw', A.ROI_MAPS, ids=map_id)
def test_roi_crop_against_float64(hw, mode):
    print(f"worst ratio {A.check_roi_case(*hw, mode == 'train', CPU):.3f}")


@pytest.mark.parametrize('shape', A.ROI_CPB_CASES, ids=shape_id)
def test_roi_crop_ragged_last_group_of_maps(shape):
    print(f'worst ratio {A.check_roi_cpb(shape, CPU):.3f}')


@pytest.mark.parametrize('hw', SMALL_MAPS, ids=map_id)
def test_roi_crop_staged_and_table_kernels_give_the_same_bits(hw, tune):
    A.check_roi_kernel_pairs(*hw, CPU, tune)


def test_roi_crop_cases_reach_every_branch_of_the_backward():
    A.check_roi_branch_coverage()


@pytest.mark.parametrize('ncls', [200, 8142])
@pytest.mark.parametrize('case', A.SELECT_CASES, ids=A.select_case_id)
def test_att_roi_select_bit_exact(case, ncls):
    A.check_select_case(case, ncls, CPU)


@pytest.mark.parametrize('ncls', [200, 8142])
def test_att_roi_select_three_non_square_levels_in_one_launch(ncls):
    A.check_select_levels(ncls, CPU)


def test_att_roi_select_refuses_a_140x140_map():
    A.check_select_refused(CPU)


@pytest.mark.parametrize('att', [True, False], ids=['attention', 'plain'])
@pytest.mark.parametrize('case', A.POOL_CASES, ids=shape_id)
def test_att_pool_against_float64(case, att):
    print(f'worst ratio {A.check_pool_case(case, att, CPU):.3f}')


@pytest.mark.parametrize('case', A.POOL_LEVEL_CASES, ids=shape_id)
def test_att_pool_levels_give_the_bits_of_three_calls(case):
    print(f'worst ratio {A.check_pool_levels(case, CPU):.3f}')


def test_att_pool_backward_refuses_8193_channels():
    print(f'worst ratio {A.check_pool_refused(CPU):.3f}')


@pytest.mark.parametrize('case', A.OSME_CASES, ids=shape_id)
def test_osme_against_float64(case):
    print(f'worst ratio {A.check_osme_case(case, CPU):.3f}')


@pytest.mark.parametrize('case', A.NPAIRS_CASES, ids=shape_id)
def test_npairs_loss_against_float64(case):
    print(f'worst ratio {A.check_npairs_case(case, CPU):.3f}')
