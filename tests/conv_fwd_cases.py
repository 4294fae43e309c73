"""Shapes, inputs, float64 references and the bound shared by tests/test_emu_conv_fwd.py and tests/test_gpu_conv_fwd.py
(hk_conv3x3_fwd / hk_conv3x3_bwd_data, csrc/conv_fwd.hip).  Not a test module.

Bound, elementwise as for the weight gradient: |y - y64| <= c S with S = float64 conv2d(|x|, |w|) at that element, c = 1e-6 for
chains of 9 Cin <= 1024 products and 1.5e-6 above - the project's figures for v_mfma_f32_32x32x16_bf16 chains."""
import functools

import torch

TILE_ROWS = 4                                   # CF_R of csrc/conv_fwd.hip: output rows of a workgroup's tile
# (N, H, W, Cin, Cout), the smallest at which each mechanism can break
SHAPES = [
    (1, 1, 1, 64, 64),                          # every tap but the centre is outside the image
    (2, 3, 5, 64, 64),                          # both borders in every row, a tile mostly empty, a batch offset
    (1, 5, 33, 64, 128),                        # one column past a 32-column strip, two output slices
    (2, 7, 34, 128, 64),                        # two K chunks per slice pair, the halo across a strip boundary, output narrower than input
    (1, 4, 28, 192, 192),                       # odd counts of chunks and slices at W = 28
    (1, 2 * TILE_ROWS + 2, 40, 64, 64),         # H > twice the tile height plus one: row-tile boundaries and a ragged last tile
    (1, 4, 28, 512, 64),                        # the longest chain, 4608
]
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def bound(k_channels):
    return 1e-6 if 9 * k_channels <= 1024 else 1.5e-6


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _stress_values(shape, g):
    """Values that stress the pieces: 1 + 2^-9-like patterns (the mid piece carries the information), residuals of both signs, and
    magnitudes across 2^+-40 - one scale per input channel, so that the sum of an output element keeps terms of every size."""
    base = 1.0 + torch.randint(-3, 4, shape, generator=g).float() * 2.0 ** -9 + torch.randint(-3, 4, shape, generator=g).float() * 2.0 ** -17
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    scale = torch.exp2(torch.randint(-40, 41, (shape[1],), generator=g).float()).view(1, -1, 1, 1)
    return base * sign * scale


@functools.lru_cache(maxsize=None)
def case(shape, kind='relu'):
    """x, w, dy (channels_last fp32) and the float64 y, S_y, dx, S_dx of one shape: computed once, never modified."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    if kind == 'relu':
        x = torch.relu(torch.randn(n, cin, h, w, generator=g))
        wt = torch.randn(cout, cin, 3, 3, generator=g)
        dy = torch.randn(n, cout, h, w, generator=g)
    else:
        x = _stress_values((n, cin, h, w), g)
        wt = _stress_values((cout, cin, 3, 3), g)
        dy = _stress_values((n, cout, h, w), g)
    x, wt, dy = nhwc(x), nhwc(wt), nhwc(dy)
    conv = torch.nn.functional.conv2d
    y64, sy = conv(x.double(), wt.double(), padding=1), conv(x.double().abs(), wt.double().abs(), padding=1)
    wflip = wt.double().flip(2, 3).transpose(0, 1)                       # w'[ci][co][kh][kw] = w[co][ci][2 - kh][2 - kw]
    dx64, sdx = conv(dy.double(), wflip, padding=1), conv(dy.double().abs(), wflip.abs(), padding=1)
    return x, wt, dy, y64, sy, dx64, sdx


def within(got, ref, scale, c, what):
    diff = (got.detach().double().cpu() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())
    print(f'{what}: max |y - y64| / S = {worst:.3e} (bound {c:.1e})')
    assert bool((diff <= c * scale).all()), (what, worst)
    return worst
