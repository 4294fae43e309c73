"""hk_conv3x3_wrw with more than 64 input channels (csrc/conv_wrw.hip: the split form reads its 64-channel slice of `x` out of
Cin-wide pixels, a workgroup owns one (Cout slice, Cin slice) block of dW) through the CPU emulation, against float64: the pixel
stride and channel offset of `x`, the row pitch 9 Cin of the partial result and the finish over [workgroup][Cout][9][Cin], with no
GPU.  Bound as for 64 input channels (tests/test_emu_conv_wrw_split.py): |dW - dW64| <= 1e-6 S elementwise, S = the same sum over
|x| and |dy|, 1.5e-6 S above 1024 pixels - an element of dW is the same sum over the same pixels whatever Cin is."""
import pytest
import torch

from emu.harness import emulated

# (N, H, W, Cin, Cout): two Cin slices, all border | both slice indices, a ragged second strip
CASES = [(1, 2, 2, 128, 64), (1, 5, 33, 128, 128)]
ONE_WG = (2, 9, 70, 128, 64)          # 12 jobs, 54 row steps: the accumulators go to the partial on the way, at a Cin offset of 64


def _inputs(n, h, w, cin, cout, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    return x, dy


def _within(dw, x, dy, bound, what):
    cin, cout = x.shape[1], dy.shape[1]
    assert tuple(dw.shape) == (cout, cin, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, cin, 3, 3), dy.double().abs(), padding=1)
    diff = (dw.double() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())             # (S = 0: a tap that only ever sees the border; dW is 0 there)
    print(f'{what}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), (what, worst)


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_emulated_wide_weight_gradient_against_float64(shape, tune):
    n, h, w, cin, cout = shape
    x, dy = _inputs(*shape)
    with emulated() as f:
        dw = f.conv3x3_wrw_raw(x, dy)
        # a Cin slice is what the split form gives for those 64 channels alone (same jobs, same workgroups), bit for bit: no slice
        # reads its neighbour's channels
        tune('wrw_split', 1)
        for s in range(cin // 64):
            alone = f.conv3x3_wrw_raw(x[:, 64 * s:64 * s + 64].contiguous(memory_format=torch.channels_last), dy)
            assert torch.equal(dw[:, 64 * s:64 * s + 64], alone), s
    _within(dw, x, dy, 1e-6 if n * h * w <= 1024 else 1.5e-6, shape)


def test_emulated_wide_one_workgroup_adds_its_accumulators_to_the_partial_on_the_way(tune):
    x, dy = _inputs(*ONE_WG)
    with emulated() as f:
        tune('wrw_wgs', 1)
        dw = f.conv3x3_wrw_raw(x, dy)
    _within(dw, x, dy, 1.5e-6, 'one workgroup')


def test_emulated_entry_point_refuses_wide_calls_without_the_split_form_or_with_the_knob_off(tune):
    from hawkeye_amd._lib import HawkeyeHipError
    x, dy = _inputs(*CASES[0])
    with emulated() as f:
        for knob in ('wrw_split', 'wrw_wide'):
            tune(knob, 0)
            with pytest.raises(HawkeyeHipError):
                f.conv3x3_wrw_raw(x, dy)
            tune(knob, 1)
        f.conv3x3_wrw_raw(x, dy)
