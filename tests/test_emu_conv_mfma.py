"""conv3x3_split_kernel on the 16 x 16 x 32 bf16 MFMA (csrc/conv_fwd.hip, MF; knob `conv_mfma` 1) through the CPU emulation, with no
GPU: the image of cf16_off in the pre-pass, the staging stores and the fragment reads, the eight accumulators and their C layout,
against float64 at the four smallest shapes of tests/conv_fwd_cases.py with its bound; and the two epilogues that add barrier
intervals - the pooled forward and the masked input gradient with its partial sums - with the work-items of a workgroup resumed in
another order, bit-equal to the two-kernel paths under the same knob.  (The emulation's model of the instruction is
tests/emu/shim/hk_mfma_bf16.h: its A/B layout is an assumption that tests/test_gpu_conv_mfma.py confirms on the device.)"""
import pytest
import torch

import conv_epilogue_cases as C
from conv_fwd_cases import IDS, SHAPES, bound, case, within
from emu.harness import emulated

ORDERS = ('rev', 'rand:11')
CPU = torch.device('cpu')
SMALL_A, SMALL_B = C.SHAPES_A[:4], C.SHAPES_B[:3]


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated() as f:
        yield f


@pytest.fixture
def lib(F, tune):
    from hawkeye_amd import _lib
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    tune('conv_epi', 2)
    tune('conv_mfma', 1)
    return _lib.load()


@pytest.mark.parametrize('shape', SHAPES[:4], ids=IDS[:4])
def test_emulated_forward_and_input_gradient_against_float64(F, lib, tune, shape):
    n, h, w, cin, cout = shape
    x, wt, dy, y64, sy, dx64, sdx = case(shape)
    y = F.conv3x3_fwd_raw(x, wt)
    dx = F.conv3x3_bwd_data_raw(dy, wt)
    wflip = wt.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)
    assert torch.equal(dx, F.conv3x3_fwd_raw(dy, wflip))
    within(y, y64, sy, bound(cin), f'forward {shape}')
    within(dx, dx64, sdx, bound(cout), f'input gradient {shape}')


ORDER_CASES = [('pool', shape) for shape in SMALL_B] + [('masked', shape) for shape in SMALL_A]


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('which,shape', ORDER_CASES, ids=[w + '-' + i for (w, _), i in zip(ORDER_CASES, C.ids(SMALL_B) + C.ids(SMALL_A))])
def test_emulated_epilogues_in_another_work_item_order(F, lib, which, shape, order, monkeypatch):
    monkeypatch.setenv('HK_EMU_ORDER', order)
    if which == 'pool':
        C.check_bias_relu_pool(F, lib, CPU, shape, 'signed')
    else:
        C.check_masked_bwd_data(F, lib, CPU, shape, 'random')


@pytest.mark.parametrize('shape', SMALL_A[:2], ids=C.ids(SMALL_A[:2]))
def test_emulated_bias_relu_forward_equals_the_two_kernels(F, lib, shape):
    C.check_bias_relu(F, lib, CPU, shape, 'signed')
