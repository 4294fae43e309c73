"""Shapes, inputs and references shared by tests/test_emu_wrw_pool.py (CPU emulation) and tests/test_gpu_wrw_pool.py (MI355X):
hk_conv3x3_wrw_pooled (csrc/conv_wrw.hip, "Pooled"; include/hawkeye_conv_pool.h), the weight gradient of a layer that ends in a 2 x 2
max-pool, from the pooled gradient dp, the pooled output p and the argmax codes on the 2:4 sparse bf16 MFMA.  Not a test module.

Reference: the full-resolution gradient g spelled in torch by bias_relu_pool_bwd_kernel's rule - the value !(p <= 0) ? dp : 0 at the
window position the code names, zeros elsewhere - then the float64 weight gradient of conv2d on the CPU; S = the same gradient of
(|x|, |g|).  Bound: wrw_mfma_cases.bound(shape) S, the project's, imported."""
import ctypes
import functools

import torch

from conv_epilogue_cases import Guarded
import wrw_mfma_cases as M

# ((N, H, W, Cin, Cout), wrw_wgs): H, W the full-resolution sizes
CASES = [
    ((1, 2, 2, 64, 64), 0),                     # one window, all border
    ((1, 2, 34, 64, 64), 0),                    # a second strip with two live columns
    ((2, 6, 28, 256, 64), 0),                   # wide Cin, ragged strip, two images
    ((1, 8, 16, 128, 192), 0),                  # three Cout slices, two Cin slices
    ((1, 70, 32, 64, 64), 1),                   # one workgroup, 35 two-row steps: a chain across a flush, and a last step after it
    ((1, 70, 32, 64, 64), 3),                   # several even row blocks
]
IDS = ['x'.join(map(str, s)) + (f'-wgs{g}' if g else '') for s, g in CASES]
KINDS = ['int', 'randn', 'codes 0', 'codes 3', 'all masked', 'one window column']
SMALL = (2, 6, 28, 256, 64)                     # the shape of the input kinds that do not need every case
bound = M.bound


def full_gradient(dp, p, codes):
    """g [N, Cout, 2 Ho, 2 Wo] of dp, p [N, Cout, Ho, Wo] and per-channel codes [N, Cout, Ho, Wo] (0 .. 3 = 2 dh + dw)."""
    n, c, ho, wo = dp.shape
    d = torch.where(~(p <= 0), dp, torch.zeros_like(dp))
    g = torch.zeros(n, c, 2 * ho, 2 * wo, dtype=dp.dtype)
    for k in range(4):
        g[:, :, (k >> 1)::2, (k & 1)::2] = torch.where(codes == k, d, torch.zeros_like(d))
    return g


def pack_codes(codes):
    """Per-channel codes [N, C, Ho, Wo] -> bias_relu_pool_fwd's bytes [N, Ho, Wo, C / 4]: channel 4 q + t in bits 2 t, 2 t + 1 of byte q."""
    n, c, ho, wo = codes.shape
    q = codes.permute(0, 2, 3, 1).reshape(n, ho, wo, c // 4, 4).to(torch.int32)
    return (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).to(torch.uint8).contiguous()


def _finish(x, dp, p, codes, exact=False):
    cl = torch.channels_last
    x, dp, p = x.contiguous(memory_format=cl), dp.contiguous(memory_format=cl), p.contiguous(memory_format=cl)
    g = full_gradient(dp, p, codes).contiguous(memory_format=cl)
    ref, scale = M._ref64(x, g)
    if exact:
        assert float(scale.max()) < 2.0 ** 24, float(scale.max())         # every partial sum in any order is an exact fp32 integer
    return x, dp, p, pack_codes(codes), g, ref, scale


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """x, dp, p, code bytes, g (CPU), the float64 weight gradient and its scale S - made once per (shape, kind), never written to."""
    n, h, w, cin, cout = shape
    ho, wo = h // 2, w // 2
    gen = torch.Generator().manual_seed(1000 * n + 10 * h + w + cin + cout + 13 * KINDS.index(kind))
    codes = torch.randint(0, 4, (n, cout, ho, wo), generator=gen)
    if kind == 'int':
        x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).float()
        dp = torch.randint(-8, 9, (n, cout, ho, wo), generator=gen).float()
        p = torch.randint(-1, 3, (n, cout, ho, wo), generator=gen).float()      # half of them <= 0
        return _finish(x, dp, p, codes, exact=True)
    x = torch.randn(n, cin, h, w, generator=gen)
    dp = torch.randn(n, cout, ho, wo, generator=gen)
    p = torch.randn(n, cout, ho, wo, generator=gen).clamp_min(0.0)               # a ReLU's output: half of it zero
    if kind == 'codes 0':
        codes = torch.zeros_like(codes)
    elif kind == 'codes 3':
        codes = torch.full_like(codes, 3)
    elif kind == 'all masked':
        p = -p
    elif kind == 'one window column':
        keep = torch.zeros(wo, dtype=torch.bool)
        keep[wo // 2] = True
        dp = dp * keep
    return _finish(x, dp, p, codes)


@functools.lru_cache(maxsize=None)
def stress(kind):
    """tests/wrw_mfma_cases.py's stress inputs (x, dy at 6 x 40, 64 channels) with dy taken as the pooled gradient of a 12 x 80 map: x is
    tiled to the full resolution; p positive, random codes."""
    x, dy, _, _ = M.stress(kind)
    gen = torch.Generator().manual_seed(5 + M.STRESS_KINDS.index(kind))
    xf = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) * (1.0 + 0.25 * torch.rand(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], generator=gen))
    codes = torch.randint(0, 4, tuple(dy.shape), generator=gen)
    return _finish(xf, dy, torch.ones_like(dy), codes)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _flat(t):
    return t.permute(0, 2, 3, 1).reshape(-1)


def run(lib, dev, x, dp, p, code_bytes, wgs=0, stream=None, guarded=True, knobs=None):
    """hk_conv3x3_wrw_pooled -> dW [Cout, Cin, 3, 3] on the CPU.  guarded: dp, p, the codes, x, the workspace (exactly
    hk_conv3x3_wrw_ws_bytes) and dW lie between guard rows (1e30, bytes 0xA5) that have to survive."""
    n, cin, h, w = x.shape
    cout = dp.shape[1]
    nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)
    assert nws > 0
    srcs = [(_flat(x), torch.float32, 4 * ((3 * w * cin + 3) // 4)), (_flat(dp), torch.float32, 2 * w * cout), (_flat(p), torch.float32, 2 * w * cout),
            (code_bytes.reshape(-1), torch.uint8, 16 * ((w * cout + 15) // 16))]
    bufs = []
    if guarded:
        ins = []
        for flat, dt, pad in srcs:
            gb = Guarded(flat.numel(), dt, dev, pad)
            gb.inner.copy_(flat.to(dev))
            bufs.append(gb)
            ins.append(gb.inner)
        gws, gdw = Guarded(nws, torch.uint8, dev, 4096), Guarded(cout * 9 * cin, torch.float32, dev, 9 * cin)
        bufs += [gws, gdw]
        pws, dw = gws.inner, gdw.inner
    else:
        ins = [flat.to(dev).contiguous() for flat, _, _ in srcs]
        pws, dw = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(cout * 9 * cin, dtype=torch.float32, device=dev)
    px, pdp, pp, pam = ins
    with M.Knobs(lib, wrw_split=1, wrw_wide=1, wrw_wgs=wgs, **(knobs or {})):
        rc = lib.hk_conv3x3_wrw_pooled(_p(pdp), _p(pp), _p(pam), _p(px), _p(dw), n, h, w, cin, cout, _p(pws), nws, stream)
    assert rc == 0, rc
    out = dw.cpu().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    bad = [i for i, b in enumerate(bufs) if not b.intact()]
    assert not bad, ('guard rows of x, dp, p, codes, workspace, dW', bad)
    return out


def run_dense(lib, dev, x, g, wgs=0, stream=None):
    """hk_conv3x3_wrw's split form on the 16 x 16 x 32 MFMA on the full-resolution g: the kernel the pooled form stands in for."""
    return M.run(lib, dev, x, g, 1, wgs, stream, guarded=False)


def plan(lib, n, h, w, cin, cout):
    out = (ctypes.c_int * 5)()
    rc = lib.hk_conv3x3_wrw_pooled_plan(n, h, w, cin, cout, ctypes.cast(out, ctypes.c_void_p))
    return rc, list(out)
