"""Shapes and checks shared by tests/test_emu_conv_mf16_rule.py (CPU emulation) and tests/test_gpu_conv_mf16_rule.py (MI355X): the MFMA
shape of conv3x3_split_kernel chosen in the library (csrc/conv_fwd.hip, conv3x3_mfma16_wins; knob `conv_mfma` at its default, -1).
Not a test module.

Every entry point - forward, input gradient and the four epilogues - runs once per (shape, knob value) through
tests/conv_wdma_cases.py's `outputs`, which puts x, w, bias, mask, workspace and every output between 1e30 (bytes: 0xA5) guard rows and
asserts them.  The rule is "always 16 x 16 x 32", so at every shape the default knob has to give the bits of `conv_mfma` 1 and not those
of `conv_mfma` 0.

What the default knob's result is held to:
  forward, input gradient   |y - y64| <= c S elementwise, c = 1e-6 (1.5e-6 where the chain has more than 1024 products): the bound of
                            tests/conv_fwd_cases.py, as tests/test_gpu_conv_mfma.py uses it
  bias + ReLU               the bits of relu(forward + bias) - one fp32 addition per element, so one rounding, whoever does it - and the
                            sign bytes of that map
  bias + ReLU + pool        the bits of max_pool2d of that map (even H and W; the entry point refuses the others)
  masked input gradient     the plain input gradient where the mask's bit is set, +0 elsewhere, bit for bit; the bias gradient within
                            tests/conv_epilogue_cases.py's bound (n_pixels 2^-24 sum |masked dx| per channel)
  a second launch           the same bits, every output"""
import torch

import conv_wdma_cases as W
from conv_epilogue_cases import db_bound
from conv_fwd_cases import bound, case, within

# (N, H, W, Cin, Cout)
SHAPES = [
    (1, 1, 1, 64, 64),                          # the smallest: one tile, every tap but the centre outside the image
    (2, 7, 34, 128, 64),                        # 8 x 16 tiles (3 an image against 4 of 4 x 32), ragged both ways, two images, four chunks
    (1, 16, 24, 64, 64),                        # 8 x 16 over columns 0 - 15 and the 16 x 8 remainder strip over 16 - 23: one mixed launch
    (1, 4, 28, 192, 192),                       # six chunks: one restart of the accumulator chains (CF_FLUSH = 3), three Cout tiles
]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
FLOATS = ('fwd', 'bwd_data', 'bias_relu', 'pool', 'masked_bwd_data')


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes()


class Runs:
    """outputs(shape, knob): every entry point at `shape` under `conv_mfma` = knob, made once and never written to."""

    def __init__(self, lib, dev, stream=None):
        self.lib, self.dev, self.stream, self.memo = lib, dev, stream, {}

    def fresh(self, shape, knob):
        return W.outputs(self.lib, self.dev, shape, knob, self.stream)

    def __call__(self, shape, knob):
        if (shape, knob) not in self.memo:
            self.memo[shape, knob] = self.fresh(shape, knob)
        return self.memo[shape, knob]


def names(shape):
    n = ['fwd', 'bwd_data', 'bias_relu', 'bias_relu_mask', 'masked_bwd_data', 'masked_bwd_data_db']
    return sorted(n + (['pool', 'pool_argmax'] if shape[1] % 2 == 0 and shape[2] % 2 == 0 else []))


def check_rule(runs, shape):
    """The default knob runs what `conv_mfma` 1 runs, at every entry point, and not what `conv_mfma` 0 runs."""
    by_rule, mf16, mf32 = runs(shape, -1), runs(shape, 1), runs(shape, 0)
    assert sorted(by_rule) == names(shape)
    differ = [k for k in by_rule if not same(by_rule[k], mf16[k])]
    assert not differ, (shape, 'the default knob does not give the bits of conv_mfma 1', differ)
    equal = [k for k in FLOATS if k in by_rule and same(by_rule[k], mf32[k])]
    assert not equal, (shape, 'the default knob gives the bits of conv_mfma 0', equal)


def check_default(runs, shape):
    """The default knob's result against float64, against the passes the epilogues replace, and against a second launch."""
    n, h, w, cin, cout = shape
    out = runs(shape, -1)
    x, wt, dy, y64, sy, dx64, sdx = case(shape)
    nchw = lambda flat, c: flat.view(n, h, w, c).permute(0, 3, 1, 2)
    y, dx = nchw(out['fwd'], cout), nchw(out['bwd_data'], cin)
    within(y, y64, sy, bound(cin), f'default knob forward {shape}')
    within(dx, dx64, sdx, bound(cout), f'default knob input gradient {shape}')
    # the inputs of W.outputs, made again from its seed
    g = torch.Generator().manual_seed(4242 + sum(shape))
    bias = torch.randn(cout, generator=g)
    mask = torch.randint(0, 16, (n, h, w, cin // 4), generator=g, dtype=torch.uint8)
    act = torch.relu(out['fwd'].view(n, h, w, cout) + bias)
    assert same(out['bias_relu'], act.reshape(-1)), (shape, 'bias + ReLU')
    signs = (~(act <= 0)).view(n, h, w, cout // 4, 4).to(torch.uint8)
    assert same(out['bias_relu_mask'], (signs[..., 0] | signs[..., 1] << 1 | signs[..., 2] << 2 | signs[..., 3] << 3).reshape(-1)), (shape, 'sign mask')
    if 'pool' in out:
        pooled = torch.nn.functional.max_pool2d(act.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert same(out['pool'], pooled.reshape(-1)), (shape, 'bias + ReLU + pool')
    keep = ((mask.unsqueeze(-1) >> torch.arange(4, dtype=torch.uint8)) & 1).bool().view(n, h, w, cin)
    masked = torch.where(keep, out['bwd_data'].view(n, h, w, cin), torch.zeros(()))
    assert same(out['masked_bwd_data'], masked.reshape(-1)), (shape, 'masked input gradient')
    db64, allowed = db_bound(masked.permute(0, 3, 1, 2))
    err = (out['masked_bwd_data_db'].double() - db64).abs()
    print(f'default knob bias gradient {shape}: max |db - db64| = {float(err.max()):.3e} (allowed at that channel {float(allowed[err.argmax()]):.3e})')
    assert bool((err <= allowed).all()), (shape, 'bias gradient', float((err - allowed).max()))
    again = runs.fresh(shape, -1)                                        # (asserts the guard rows of every buffer, as the first did)
    differ = [k for k in out if not same(out[k], again[k])]
    assert not differ, (shape, 'two launches', differ)
