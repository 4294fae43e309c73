"""hk_conv3x3_fwd and hk_conv3x3_bwd_data (csrc/conv_fwd.hip) through the CPU emulation, against float64, with no GPU: the weight
pre-pass in both orientations, the halo tile with its borders, the tap offsets, the chunk walk and the C layout of the stores, at
the four smallest shapes of tests/conv_fwd_cases.py and with its bound."""
import pytest
import torch

from conv_fwd_cases import IDS, SHAPES, bound, case, within
from emu.harness import emulated


@pytest.mark.parametrize('shape', SHAPES[:4], ids=IDS[:4])
def test_emulated_forward_and_input_gradient_against_float64(shape, tune):
    n, h, w, cin, cout = shape
    x, wt, dy, y64, sy, dx64, sdx = case(shape)
    with emulated() as f:
        tune('conv_fwd', 1)
        tune('conv_bwd_data', 1)
        y = f.conv3x3_fwd_raw(x, wt)
        dx = f.conv3x3_bwd_data_raw(dy, wt)
        # the input gradient IS the forward of dy with the flipped, transposed weights: the same kernel behind the other pre-pass
        wflip = wt.flip(2, 3).transpose(0, 1).contiguous(memory_format=torch.channels_last)
        assert torch.equal(dx, f.conv3x3_fwd_raw(dy, wflip))
    assert tuple(y.shape) == (n, cout, h, w) and y.is_contiguous(memory_format=torch.channels_last)
    assert tuple(dx.shape) == (n, cin, h, w) and dx.is_contiguous(memory_format=torch.channels_last)
    within(y, y64, sy, bound(cin), f'forward {shape}')
    within(dx, dx64, sdx, bound(cout), f'input gradient {shape}')


def test_emulated_entry_points_refuse_what_they_do_not_serve(tune):
    from hawkeye_amd._lib import HawkeyeHipError
    x, wt, dy = case(SHAPES[0])[:3]
    with emulated() as f:
        for knob, call, src in (('conv_fwd', f.conv3x3_fwd_raw, x), ('conv_bwd_data', f.conv3x3_bwd_data_raw, dy)):
            tune(knob, 0)
            with pytest.raises(HawkeyeHipError):
                call(src, wt)
            tune(knob, 1)
            call(src, wt)
        with pytest.raises(HawkeyeHipError):                                     # 96 channels
            f.conv3x3_fwd_raw(torch.randn(1, 96, 2, 2).contiguous(memory_format=torch.channels_last),
                              torch.randn(64, 96, 3, 3).contiguous(memory_format=torch.channels_last))
