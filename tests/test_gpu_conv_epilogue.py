"""The epilogues inside conv3x3_split_kernel (csrc/conv_fwd.hip, EPI) on the GPU against the two-kernel paths they replace, bit for
bit: bias + ReLU + sign mask and bias + ReLU + pool + argmax in the forward, the producer's mask and bias gradient in the input
gradient, and a ConvStack with `conv_epi` at 1 and 2 against 0.  The checks, their inputs and the bound on the bias gradient are
tests/conv_epilogue_cases.py's; the routes are forced with the knobs."""
import pytest
import torch

import conv_epilogue_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


@pytest.fixture
def lib(F, tune):
    from hawkeye_amd import _lib
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    tune('conv_epi', 2)
    return _lib.load()


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', C.SHAPES_A, ids=C.ids(C.SHAPES_A))
def test_bias_relu_forward_equals_the_two_kernels(F, lib, shape, variant):
    C.check_bias_relu(F, lib, DEV, shape, variant)


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', C.SHAPES_B, ids=C.ids(C.SHAPES_B))
def test_bias_relu_pool_forward_equals_the_two_kernels(F, lib, shape, variant):
    C.check_bias_relu_pool(F, lib, DEV, shape, variant)


@pytest.mark.parametrize('variant', ['random', 'set'])
@pytest.mark.parametrize('shape', C.SHAPES_A, ids=C.ids(C.SHAPES_A))
def test_masked_input_gradient_equals_the_two_kernels(F, lib, shape, variant):
    C.check_masked_bwd_data(F, lib, DEV, shape, variant)


def test_masked_input_gradient_with_two_reduction_stages(F, lib):
    """More tiles than one reduction group holds (CF_DB_RPG = 128): 2 x 40 x 200 pixels are 140 tiles, so both stages of the column sums
    run, the second group ragged."""
    C.check_masked_bwd_data(F, lib, DEV, (2, 40, 200, 64, 64), 'random')


def test_stack_with_the_epilogues_inside_against_the_passes(F, lib, tune, monkeypatch):
    C.check_stack(F, lib, DEV, tune, monkeypatch)
