"""Shapes, inputs, references and the recorded bits shared by tests/test_emu_conv_wrw_mfma.py (CPU emulation),
tests/test_gpu_conv_wrw_mfma.py (MI355X) and tools/gen_wrw_mfma_golden.py: the split form of hk_conv3x3_wrw (csrc/conv_wrw.hip) on
either bf16 MFMA - knob `wrw_mfma` 0 = v_mfma_f32_32x32x16_bf16, 1 = v_mfma_f32_16x16x32_bf16.  Not a test module.

Two kinds of input per shape:
  'int'    small integers, |v| <= 8: exact in the high bf16 piece (the other two pieces are zero), every product an integer and every
           sum below 2^24 (asserted here from S = sum |x| |dy|), so dW has to equal the float64 weight gradient EXACTLY on either
           MFMA, whatever the order of the additions - any disagreement between the k order of dy and x, the plane layout, the kw
           offsets or the C layout shows with no tolerance
  'randn'  the project's bound: |dW - dW64| <= 1e-6 S elementwise, 1.5e-6 S above 1024 pixels (tests/test_gpu_conv_wrw_split.py)
The fixtures tests/golden/wrw_mfma_{emu,gpu}.json hold SHA-256 digests of the `wrw_mfma` 0 results on the 'randn' inputs, recorded on the
commit BEFORE the second MFMA shape (which has no such knob: its only kernel is what 0 selects now)."""
import ctypes
import functools
import hashlib
import json
import os

import torch

from conv_epilogue_cases import Guarded

# ((N, H, W, Cin, Cout), wrw_wgs)
CASES = [
    ((1, 1, 1, 64, 64), 0),                     # all border
    ((1, 2, 2, 128, 64), 0),                    # wide, all border
    ((1, 5, 33, 128, 128), 0),                  # a ragged second strip of one pixel under the permuted k
    ((2, 6, 28, 256, 64), 0),                   # one short strip, four Cin slices
    ((1, 3, 64, 64, 128), 0),                   # two full strips: the column halo across pixel 31 | 32, two Cout slices
    ((3, 1, 1, 192, 64), 0),                    # an odd slice count
    ((2, 9, 70, 128, 64), 1),                   # one workgroup, 54 row steps: the flush added to the partial at a channel offset
    ((1, 64, 32, 64, 64), 1),                   # one workgroup, 64 row steps: two full chains
]
IDS = ['x'.join(map(str, s)) + (f'-wgs{g}' if g else '') for s, g in CASES]
STRESS_SHAPE = (2, 6, 40, 64, 64)               # the shape of tests/test_gpu_conv_wrw_split.py's stress inputs
STRESS_KINDS = ['dy 1e-6', 'dy 1e-30', 'relu', 'bf16 values', 'negative residuals', 'spread 2^+-6']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def bound(shape):
    n, h, w = shape[:3]
    return 1e-6 if n * h * w <= 1024 else 1.5e-6


def _ref64(x, dy):
    cout, cin = dy.shape[1], x.shape[1]
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, cin, 3, 3), dy.double().abs(), padding=1)
    return ref, scale


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """x, dy (CPU, channels_last), the float64 weight gradient and its scale S - made once per (shape, kind), never written to."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cin + cout + (7 if kind == 'int' else 0))
    if kind == 'int':
        x = torch.randint(-8, 9, (n, cin, h, w), generator=g).float()
        dy = torch.randint(-8, 9, (n, cout, h, w), generator=g).float()
    else:
        x = torch.randn(n, cin, h, w, generator=g)
        dy = torch.randn(n, cout, h, w, generator=g)
    x, dy = x.contiguous(memory_format=torch.channels_last), dy.contiguous(memory_format=torch.channels_last)
    ref, scale = _ref64(x, dy)
    if kind == 'int':
        assert float(scale.max()) < 2.0 ** 24, (shape, float(scale.max()))          # every partial sum in any order is an exact fp32 integer
    return x, dy, ref, scale


@functools.lru_cache(maxsize=None)
def stress(kind):
    """The stress inputs of tests/test_gpu_conv_wrw_split.py (64 input channels) with their float64 reference and scale."""
    from test_gpu_conv_wrw_split import _stress
    return _stress(kind)


def worst(dw, ref, scale):
    """max |dW - dW64| / S, and whether the elementwise bound holds is the caller's: (ratio, diff, scale)."""
    diff = (dw.double().cpu() - ref).abs()
    return float((diff / scale.clamp_min(1e-300)).max()), diff          # (S = 0: a tap that only ever sees the border; dW is 0 there)


def golden(which):
    """The recorded digests: `which` = 'emu' or 'gpu' -> {case id: digest of the `wrw_mfma` 0 result on the 'randn' inputs}."""
    with open(os.path.join(GOLDEN, f'wrw_mfma_{which}.json')) as f:
        return json.load(f)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def knob(lib, name):
    v = ctypes.c_int(0)
    assert lib.hk_tuning_get(name.encode(), ctypes.byref(v)) == 0, name
    return v.value


class Knobs:
    """The library's knobs for the length of a block, on the handle the caller uses (the emulated build or the device's).
    `optional`: names a build may not have (the recording of the fixtures on the commit before `wrw_mfma`); their value must be 0."""

    def __init__(self, lib, optional=(), **knobs):
        self.lib, self.knobs, self.optional, self.saved = lib, knobs, optional, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            old = ctypes.c_int(0)
            if self.lib.hk_tuning_get(k.encode(), ctypes.byref(old)) != 0:
                assert k in self.optional and v == 0, k
                continue
            self.saved[k] = old.value
            assert self.lib.hk_tuning_set(k.encode(), v) == 0
            assert knob(self.lib, k) == v                                          # (the knob round-trips)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.hk_tuning_set(k.encode(), v)
        return False


def run(lib, dev, x, dy, mf, wgs=0, stream=None, guarded=True, optional=()):
    """hk_conv3x3_wrw's split form on MFMA shape `mf` (0, 1, or -1: the library's rule) -> dW [Cout, Cin, 3, 3] on the CPU.  guarded: x,
    dy, the workspace (exactly hk_conv3x3_wrw_ws_bytes) and dW lie between guard rows (1e30, bytes 0xA5) that have to survive."""
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)
    assert nws > 0
    xf, dyf = x.permute(0, 2, 3, 1).reshape(-1), dy.permute(0, 2, 3, 1).reshape(-1)
    if guarded:
        gx, gdy = Guarded(xf.numel(), torch.float32, dev, 4 * ((3 * w * cin + 3) // 4)), Guarded(dyf.numel(), torch.float32, dev, 4 * ((3 * w * cout + 3) // 4))
        gx.inner.copy_(xf.to(dev))
        gdy.inner.copy_(dyf.to(dev))
        gws, gdw = Guarded(nws, torch.uint8, dev, 4096), Guarded(cout * 9 * cin, torch.float32, dev, 9 * cin)
        bufs = [gx, gdy, gws, gdw]
        px, pdy, pws, dw = gx.inner, gdy.inner, gws.inner, gdw.inner
    else:
        bufs = []
        px, pdy = xf.to(dev).contiguous(), dyf.to(dev).contiguous()
        pws, dw = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(cout * 9 * cin, dtype=torch.float32, device=dev)
    with Knobs(lib, optional=optional, wrw_split=1, wrw_wide=1, wrw_wgs=wgs, wrw_mfma=mf):
        rc = lib.hk_conv3x3_wrw(_p(pdy), _p(px), _p(dw), n, h, w, cin, cout, _p(pws), nws, stream)
    assert rc == 0, rc
    out = dw.cpu().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    bad = [i for i, b in enumerate(bufs) if not b.intact()]
    assert not bad, ('guard rows of x, dy, workspace, dW', bad)
    return out
