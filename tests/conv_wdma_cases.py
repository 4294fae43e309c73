"""Shapes, inputs and the recorded bits shared by tests/test_emu_conv_wdma.py (CPU emulation), tests/test_gpu_conv_wdma.py (MI355X) and
tools/gen_conv_wdma_golden.py: every entry point of csrc/conv_fwd.hip - forward, input gradient and the four epilogues of
conv3x3_split_kernel - on both MFMA shapes, as SHA-256 digests of the outputs' bytes.  Not a test module.

The fixtures under tests/golden/ were recorded from the commit BEFORE the weight tiles went into LDS by DMA (the kernel that staged
them through registers): how a weight tile reaches LDS changes no operand and no order of additions, so every output keeps its bits.
The emulation and the device have fixtures of their own (the emulation's MFMA adds in another order than the device's).

Every buffer a call touches - x, w, bias, mask, workspace, outputs - lies between guard rows (1e30, bytes 0xA5) that have to survive."""
import ctypes
import hashlib
import json
import os

import torch

from conv_epilogue_cases import Guarded
from conv_fwd_cases import case

# (N, H, W, Cin, Cout) of tests/conv_fwd_cases.py: the smallest that reach the weight pipeline's cases
SHAPES = [
    (1, 1, 1, 64, 64),                          # 18 tiles, one workgroup
    (2, 7, 34, 128, 64),                        # four chunks, two strips, two images
    (1, 4, 28, 192, 192),                       # three Cout tiles - the offset of a Cout tile into the workspace - and an odd chunk count
    (1, 4, 28, 512, 64),                        # 144 tiles: every chain restart
]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KNOBS = {'conv_fwd': 1, 'conv_bwd_data': 1, 'conv_epi': 2}


def golden(which):
    """The recorded digests: `which` = 'emu' or 'gpu' -> {shape id: {'mf0' | 'mf1': {output name: digest}}}."""
    with open(os.path.join(GOLDEN, f'conv_wdma_{which}.json')) as f:
        return json.load(f)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class _Knobs:
    """The library's knobs for the length of a block, on the handle the caller uses (the emulated build or the device's)."""

    def __init__(self, lib, **knobs):
        self.lib, self.knobs, self.saved = lib, knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            old = ctypes.c_int(0)
            assert self.lib.hk_tuning_get(k.encode(), ctypes.byref(old)) == 0
            self.saved[k] = old.value
            assert self.lib.hk_tuning_set(k.encode(), v) == 0
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.hk_tuning_set(k.encode(), v)
        return False


def _guard(t, dev, pad):
    """A copy of the flat tensor `t` on `dev` between guard rows."""
    g = Guarded(t.numel(), t.dtype, dev, pad)
    g.inner.copy_(t.to(dev))
    return g


def outputs(lib, dev, shape, mf, stream=None):
    """Every entry point once at `shape` on MFMA shape `mf` (0: 32 x 32 x 16, 1: 16 x 16 x 32) -> {name: CPU tensor}.  The pooled forward
    wants even H and W and is left out elsewhere.  Asserts the return codes and the guard rows."""
    n, h, w, cin, cout = shape
    x, wt, dy = case(shape)[:3]
    g = torch.Generator().manual_seed(4242 + sum(shape))
    bias = torch.randn(cout, generator=g)
    mask = torch.randint(0, 16, (n, h, w, cin // 4), generator=g, dtype=torch.uint8)
    f32, u8 = torch.float32, torch.uint8
    rx, ry = 4 * ((3 * w * cin + 3) // 4), 4 * ((3 * w * cout + 3) // 4)
    gx = _guard(x.permute(0, 2, 3, 1).reshape(-1), dev, rx)
    gdy = _guard(dy.permute(0, 2, 3, 1).reshape(-1), dev, ry)
    gw = _guard(wt.permute(0, 2, 3, 1).reshape(-1), dev, 1024)
    gb = _guard(bias, dev, 64)
    gm = _guard(mask.reshape(-1), dev, 16 * (w * cin // 4))
    nws = lib.hk_conv3x3_ws_bytes(cin, cout)
    nmws = lib.hk_conv3x3_masked_ws_bytes(n, h, w, cin, cout)
    assert nmws >= nws > 0
    out, guards = {}, [gx, gdy, gw, gb, gm]

    def buf(numel, dtype, pad):
        b = Guarded(numel, dtype, dev, pad)
        guards.append(b)
        return b

    with _Knobs(lib, conv_mfma=mf, **KNOBS):
        ws = buf(nmws, u8, 4096)
        y = buf(n * h * w * cout, f32, ry)
        assert lib.hk_conv3x3_fwd(_p(gx.inner), _p(gw.inner), _p(y.inner), n, h, w, cin, cout, _p(ws.inner), nws, stream) == 0
        out['fwd'] = y.inner.cpu()
        dx = buf(n * h * w * cin, f32, rx)
        assert lib.hk_conv3x3_bwd_data(_p(gdy.inner), _p(gw.inner), _p(dx.inner), n, h, w, cin, cout, _p(ws.inner), nws, stream) == 0
        out['bwd_data'] = dx.inner.cpu()
        yr, mk = buf(n * h * w * cout, f32, ry), buf(n * h * w * cout // 4, u8, 16 * (w * cout // 4))
        assert lib.hk_conv3x3_bias_relu_fwd(_p(gx.inner), _p(gw.inner), _p(gb.inner), _p(yr.inner), _p(mk.inner), n, h, w, cin, cout,
                                            _p(ws.inner), nws, stream) == 0
        out['bias_relu'], out['bias_relu_mask'] = yr.inner.cpu(), mk.inner.cpu()
        if h % 2 == 0 and w % 2 == 0:
            ho, wo = h // 2, w // 2
            p, am = buf(n * ho * wo * cout, f32, 3 * wo * cout), buf(n * ho * wo * cout // 4, u8, 16 * (wo * cout // 4))
            assert lib.hk_conv3x3_bias_relu_pool_fwd(_p(gx.inner), _p(gw.inner), _p(gb.inner), _p(p.inner), _p(am.inner), n, h, w, cin, cout,
                                                     _p(ws.inner), nws, stream) == 0
            out['pool'], out['pool_argmax'] = p.inner.cpu(), am.inner.cpu()
        mdx, db = buf(n * h * w * cin, f32, rx), buf(cin, f32, 64)
        assert lib.hk_conv3x3_masked_bwd_data(_p(gdy.inner), _p(gw.inner), _p(gm.inner), _p(mdx.inner), _p(db.inner), n, h, w, cin, cout,
                                              _p(ws.inner), nmws, stream) == 0
        out['masked_bwd_data'], out['masked_bwd_data_db'] = mdx.inner.cpu(), db.inner.cpu()
    bad = [i for i, b in enumerate(guards) if not b.intact()]
    assert not bad, (shape, mf, 'guard rows of buffers', bad)
    return out


def digests(lib, dev, shape, mf, stream=None):
    return {k: digest(v) for k, v in outputs(lib, dev, shape, mf, stream).items()}
