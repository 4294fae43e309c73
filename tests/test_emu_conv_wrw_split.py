"""The split form of hk_conv3x3_wrw (csrc/conv_wrw.hip, knob `wrw_split` at 1: three bf16 pieces per value, six bf16 MFMAs per
tap) through the CPU emulation, against float64: the piece planes in LDS, the transposing operand read's plain C++ form, the
job / strip / row-block walk and the zeros of the borders, with no GPU.  Shapes and bound are those of the fp32 form
(tests/test_emu_conv_wrw.py): |dW - dW64| <= 1e-6 S elementwise, 1.5e-6 S for the case with 1260 pixels - the split itself adds
at most 3.9e-8 S (the pieces drop terms of 2^-24 |x| |dy| and below), the fp32 accumulation of the six products is the rest."""
import pytest
import torch

from emu.harness import emulated
from test_emu_conv_wrw import CASES, _inputs, _ref64


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_emulated_split_weight_gradient_against_float64(shape, tune):
    n, h, w, cout = shape
    x, dy = _inputs(n, h, w, cout)
    with emulated() as f:
        tune('wrw_split', 1)
        dw = f.conv3x3_wrw_raw(x, dy)
        if shape == CASES[0]:
            tune('wrw_split', 0)
            assert not torch.equal(f.conv3x3_wrw_raw(x, dy), dw)       # the knob switches kernels
    assert tuple(dw.shape) == (cout, 64, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    ref, scale = _ref64(x, dy)
    bound = 1e-6 if n * h * w <= 1024 else 1.5e-6
    diff = (dw.double() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())
    print(f'{shape}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), worst


def test_emulated_split_one_workgroup_adds_its_accumulators_to_the_partial_on_the_way(tune):
    """`wrw_wgs` at 1: one workgroup walks all 12 jobs, 54 row steps - past the 32 after which the accumulators go to the partial."""
    shape = CASES[4]
    x, dy = _inputs(*shape)
    with emulated() as f:
        tune('wrw_split', 1)
        tune('wrw_wgs', 1)
        dw = f.conv3x3_wrw_raw(x, dy)
    ref, scale = _ref64(x, dy)
    diff = (dw.double() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())
    print(f'{shape}, one workgroup: max |dW - dW64| / S = {worst:.3e}')
    assert bool((diff <= 1.5e-6 * scale).all()), worst
