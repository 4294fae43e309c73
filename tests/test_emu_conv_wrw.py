"""hk_conv3x3_wrw (csrc/conv_wrw.hip) through the CPU emulation of the kernel sources, against float64: the file builds
under the shim as it stands, and the job / strip / row-block walk, the LDS ring and the zeros of the borders are exercised
with no GPU.  Bound as on the GPU tier (tests/test_gpu_conv_wrw.py): |dW - dW64| <= 1e-6 S elementwise, S = the same sum
over |x| and |dy| - an fp32 MFMA chain is at 0.75 - 1.5e-7 sum |a b| for K <= 1024, which leaves about 7x for the fixed-order
sum of the workgroups' partial results; 1.5e-6 for the one case with 1260 pixels."""
import pytest
import torch

from emu.harness import emulated

# (N, H, W, Cout): two images and a ragged second strip, fewer jobs than workgroups | odd width, a one-pixel last strip, two
# Cout slices | all border | all border | two row blocks (rows 0-4 and 5-8: a block is at least four rows high)
CASES = [(2, 6, 40, 64), (1, 5, 33, 128), (3, 1, 1, 64), (1, 2, 2, 64), (2, 9, 70, 64)]


def _inputs(n, h, w, cout, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 64, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    return x, dy


def _ref64(x, dy):
    cout = dy.shape[1]
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, 64, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 64, 3, 3), dy.double().abs(), padding=1)
    return ref, scale


@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_emulated_weight_gradient_against_float64(shape):
    n, h, w, cout = shape
    x, dy = _inputs(n, h, w, cout)
    with emulated() as f:
        dw = f.conv3x3_wrw_raw(x, dy)
    assert tuple(dw.shape) == (cout, 64, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    ref, scale = _ref64(x, dy)
    bound = 1e-6 if n * h * w <= 1024 else 1.5e-6
    diff = (dw.double() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())             # (S = 0: a tap that only ever sees the border; dW is 0 there)
    print(f'{shape}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), worst


def test_emulated_entry_point_refuses_what_it_does_not_serve():
    import ctypes
    from hawkeye_amd import _lib
    from emu.harness import load_emu
    lib = load_emu()
    x, dy = _inputs(1, 2, 2, 64)
    dw = torch.empty(64, 3, 3, 64)
    nws = lib.hk_conv3x3_wrw_ws_bytes(64, 64)
    assert nws >= 64 * 576 * 4
    ws = torch.empty(nws, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda cin, cout, xs=x, nb=nws: lib.hk_conv3x3_wrw(p(dy), p(xs), p(dw), 1, 2, 2, cin, cout, p(ws), nb, None)
    assert call(64, 64) == _lib.HK_OK
    assert call(64, 64, nb=nws - 1) == _lib.HK_ERR_WORKSPACE
    big = torch.empty(max(nws, lib.hk_conv3x3_wrw_ws_bytes(32, 96), lib.hk_conv3x3_wrw_ws_bytes(64, 96)), dtype=torch.uint8)
    ws = big
    assert lib.hk_conv3x3_wrw(p(dy), p(x), p(dw), 1, 2, 2, 32, 64, p(ws), ws.numel(), None) == _lib.HK_ERR_UNSUPPORTED
    assert lib.hk_conv3x3_wrw(p(dy), p(x), p(dw), 1, 2, 2, 64, 96, p(ws), ws.numel(), None) == _lib.HK_ERR_UNSUPPORTED
    off = ctypes.c_void_p(x.data_ptr() + 4)
    assert lib.hk_conv3x3_wrw(p(dy), off, p(dw), 1, 2, 2, 64, 64, p(ws), ws.numel(), None) == _lib.HK_ERR_UNSUPPORTED
    assert lib.hk_conv3x3_wrw(p(dy), p(x), p(dw), 0, 2, 2, 64, 64, p(ws), ws.numel(), None) == _lib.HK_ERR_BAD_ARG
