"""torch.autograd.Function wrappers over the C ABI (include/hawkeye_hip.h).

Same pattern the reference already uses for MPN-COV (model/methods/MPNCOV.py:105-230:
hand-written forward/backward `Function`s), applied to every op on the hot path.
Outputs and workspaces are allocated through torch's caching allocator; kernels
are enqueued on torch's current HIP stream; nothing synchronises the host.
fp32 only, HIP tensors only - there is no CPU fallback (see hawkeye_amd/_lib.py).
"""
import contextlib
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream


def _f32c(t):
    if t.dtype != torch.float32:
        raise _lib.HawkeyeHipError(f'hawkeye_amd ops are fp32 (reference parity target); got {t.dtype}')
    return t.contiguous()


def _f32_shaped(t, shape, what, name):
    if tuple(t.shape) != tuple(shape):
        raise _lib.HawkeyeHipError(f'{what}: {name} must have the shape {tuple(shape)}, got {tuple(t.shape)}')
    return _f32c(t)


def _int_tensor(t, shape, dtype, device, what, name, same_device=False):
    """An integer argument (labels, indices, boxes) of the given shape -> contiguous `dtype` on `device`, converted there
    (no host round trip).  same_device: a tensor that lives elsewhere is refused instead of moved."""
    if t.is_floating_point() or t.dtype == torch.bool:
        raise _lib.HawkeyeHipError(f'{what}: {name} must be integers; got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise _lib.HawkeyeHipError(f'{what}: {name} must have the shape {tuple(shape)}, got {name} of shape {tuple(t.shape)}')
    if same_device and t.device != device:
        raise _lib.HawkeyeHipError(f'{what}: {name} on {t.device} but the data on {device}')
    return t.to(device=device, dtype=dtype).contiguous()


def _one_device(what, device, *tensors):
    for t in tensors:
        if t.device != device:
            raise _lib.HawkeyeHipError(f'{what}: tensors on {device} and {t.device}')


def _loss_forward(ctx, loss, grads):
    """The end of a fused loss's forward.  loss = [total, terms ..]; grads: the gradients of the total, which backward only
    scales -> (total, terms), the terms not differentiable."""
    ctx.save_for_backward(*grads)
    terms = loss[1:]
    ctx.mark_non_differentiable(terms)
    return loss[0], terms


def _loss_backward(ctx, g, rest):
    """Every saved gradient times the incoming one, then a None for each of the `rest` inputs that take none."""
    return tuple(t * g for t in ctx.saved_tensors) + (None,) * rest


def _on(device):
    """Make `device` the current HIP device for a host-side ABI call (memcpy + stream of that device)."""
    return torch.cuda.device(device)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------- BCNN
class _BilinearPool(torch.autograd.Function):
    """replaces BilinearPooling.forward, model/methods/BCNN.py:13-27."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        b, c, h, w = x.shape
        hw = h * w
        y = torch.empty(b, c * c, dtype=torch.float32, device=x.device)
        inv_norm = torch.empty(b, dtype=torch.float32, device=x.device)
        colsum = torch.empty(b, hw, dtype=torch.float32, device=x.device)
        nws = lib.hk_bcnn_pool_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        check(lib.hk_bcnn_pool_fwd(ptr(x), ptr(y), ptr(inv_norm), ptr(colsum), b, c, hw, ptr(ws), nws, stream()),
              'hk_bcnn_pool_fwd')
        ctx.save_for_backward(x, y, inv_norm, colsum)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, inv_norm, colsum = ctx.saved_tensors
        b, c, h, w = x.shape
        hw = h * w
        dy = _f32c(dy)
        dx = torch.empty_like(x)
        nws = lib.hk_bcnn_pool_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        check(lib.hk_bcnn_pool_bwd(ptr(x), ptr(y), ptr(dy), ptr(inv_norm), ptr(colsum), ptr(dx), b, c, hw,
                                   ptr(ws), nws, stream()), 'hk_bcnn_pool_bwd')
        return dx


class _BilinearPoolSignedSqrt(torch.autograd.Function):
    """The reference's alternative normalisation (commented out at model/methods/BCNN.py:23-24):
    sign(G) sqrt(|G| + 1e-10), l2-normalised."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        b, c, h, w = x.shape
        hw = h * w
        y = torch.empty(b, c * c, dtype=torch.float32, device=x.device)
        inv_norm = torch.empty(b, dtype=torch.float32, device=x.device)
        nws = lib.hk_bcnn_ssqrt_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        check(lib.hk_bcnn_ssqrt_pool_fwd(ptr(x), ptr(y), ptr(inv_norm), b, c, hw, ptr(ws), nws, stream()),
              'hk_bcnn_ssqrt_pool_fwd')
        ctx.save_for_backward(x, y, inv_norm)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, inv_norm = ctx.saved_tensors
        b, c, h, w = x.shape
        hw = h * w
        dy = _f32c(dy)
        dx = torch.empty_like(x)
        nws = lib.hk_bcnn_ssqrt_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        check(lib.hk_bcnn_ssqrt_pool_bwd(ptr(x), ptr(y), ptr(dy), ptr(inv_norm), ptr(dx), b, c, hw, ptr(ws), nws,
                                         stream()), 'hk_bcnn_ssqrt_pool_bwd')
        return dx


def bilinear_pool(x, signed_sqrt=False):
    """[B,C,H,W] -> [B,C*C]:  sqrt(X X^T / HW + 1e-5), l2-normalised (what the reference runs, BCNN.py:21);
    signed_sqrt=True: sign(G) sqrt(|G| + 1e-10) instead (its commented alternative, BCNN.py:23-24)."""
    return _BilinearPoolSignedSqrt.apply(x) if signed_sqrt else _BilinearPool.apply(x)


# --------------------------------------------------------------------- MPN-COV
class _Covpool(torch.autograd.Function):
    """replaces Covpool, model/methods/MPNCOV.py:105-134."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        b, c, h, w = x.shape
        m = h * w
        cov = torch.empty(b, c, c, dtype=torch.float32, device=x.device)
        mu = torch.empty(b, c, dtype=torch.float32, device=x.device)
        check(lib.hk_cov_pool_fwd(ptr(x), ptr(cov), ptr(mu), b, c, m, stream()), 'hk_cov_pool_fwd')
        ctx.save_for_backward(x, mu)
        return cov

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, mu = ctx.saved_tensors
        b, c, h, w = x.shape
        g = _f32c(g)
        dx = torch.empty_like(x)
        check(lib.hk_cov_pool_bwd(ptr(x), ptr(mu), ptr(g), ptr(dx), b, c, h * w, stream()), 'hk_cov_pool_bwd')
        return dx


class _Sqrtm(torch.autograd.Function):
    """replaces Sqrtm, model/methods/MPNCOV.py:137-202."""

    @staticmethod
    def forward(ctx, a, iter_n, symmetric=False, literal_backward=False):
        lib = _lib.load()
        a = _f32c(a)
        b, d, _ = a.shape
        out = torch.empty_like(a)
        norm_a = torch.empty(b, dtype=torch.float32, device=a.device)
        slots = max(iter_n - 1, 1)
        ysave = torch.empty(b, slots, d, d, dtype=torch.float32, device=a.device)
        zsave = torch.empty(b, slots, d, d, dtype=torch.float32, device=a.device)
        nws = lib.hk_ns_sqrtm_ws_bytes(b, d, iter_n, 0)
        ws = _ws(nws, a.device)
        fwd = lib.hk_ns_sqrtm_fwd_sym if symmetric else lib.hk_ns_sqrtm_fwd
        check(fwd(ptr(a), ptr(out), ptr(norm_a), ptr(ysave), ptr(zsave), b, d, iter_n, ptr(ws), nws, stream()),
              'hk_ns_sqrtm_fwd')
        ctx.iter_n = iter_n
        ctx.literal_backward = bool(literal_backward)
        ctx.save_for_backward(a, out, norm_a, ysave, zsave)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, out, norm_a, ysave, zsave = ctx.saved_tensors
        b, d, _ = a.shape
        g = _f32c(g)
        da = torch.empty_like(a)
        nws = lib.hk_ns_sqrtm_ws_bytes(b, d, ctx.iter_n, 1)
        ws = _ws(nws, a.device)
        # 34 products (exact for any input) or, on request, the reference's 38 literally (include/hawkeye_hip.h)
        fn = lib.hk_ns_sqrtm_bwd_general if ctx.literal_backward else lib.hk_ns_sqrtm_bwd
        check(fn(ptr(a), ptr(out), ptr(norm_a), ptr(ysave), ptr(zsave), ptr(g), ptr(da),
                 b, d, ctx.iter_n, ptr(ws), nws, stream()), 'hk_ns_sqrtm_bwd')
        return da, None, None, None


class _SqrtmTriuvec(torch.autograd.Function):
    """Sqrtm followed by Triuvec (MPNCOV.py:88-92) with the packed upper triangle written by the chain's last product
    (hk_ns_sqrtm_triu_fwd); backward = Triuvec's scatter, then Sqrtm.backward."""

    @staticmethod
    def forward(ctx, a, iter_n, symmetric=False):
        lib = _lib.load()
        a = _f32c(a)
        b, d, _ = a.shape
        out = torch.empty_like(a)
        tv = torch.empty(b, d * (d + 1) // 2, 1, dtype=torch.float32, device=a.device)
        norm_a = torch.empty(b, dtype=torch.float32, device=a.device)
        slots = max(iter_n - 1, 1)
        ysave = torch.empty(b, slots, d, d, dtype=torch.float32, device=a.device)
        zsave = torch.empty(b, slots, d, d, dtype=torch.float32, device=a.device)
        nws = lib.hk_ns_sqrtm_ws_bytes(b, d, iter_n, 0)
        ws = _ws(nws, a.device)
        check(lib.hk_ns_sqrtm_triu_fwd(ptr(a), ptr(out), ptr(tv), ptr(norm_a), ptr(ysave), ptr(zsave), b, d, iter_n,
                                       1 if symmetric else 0, ptr(ws), nws, stream()), 'hk_ns_sqrtm_triu_fwd')
        ctx.iter_n = iter_n
        ctx.save_for_backward(a, out, norm_a, ysave, zsave)
        return tv

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, out, norm_a, ysave, zsave = ctx.saved_tensors
        b, d, _ = a.shape
        g = _f32c(g)
        dsq = torch.empty_like(a)
        check(lib.hk_triu_vec_bwd(ptr(g), ptr(dsq), b, d, stream()), 'hk_triu_vec_bwd')
        da = torch.empty_like(a)
        nws = lib.hk_ns_sqrtm_ws_bytes(b, d, ctx.iter_n, 1)
        ws = _ws(nws, a.device)
        check(lib.hk_ns_sqrtm_bwd(ptr(a), ptr(out), ptr(norm_a), ptr(ysave), ptr(zsave), ptr(dsq), ptr(da),
                                  b, d, ctx.iter_n, ptr(ws), nws, stream()), 'hk_ns_sqrtm_bwd')
        return da, None, None


class _Triuvec(torch.autograd.Function):
    """replaces Triuvec, model/methods/MPNCOV.py:205-230 (keeps its [B, L, 1] output shape)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        b, d, _ = x.shape
        y = torch.empty(b, d * (d + 1) // 2, 1, dtype=torch.float32, device=x.device)
        check(lib.hk_triu_vec_fwd(ptr(x), ptr(y), b, d, stream()), 'hk_triu_vec_fwd')
        ctx.dims = (b, d)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        b, d = ctx.dims
        g = _f32c(g)
        dx = torch.empty(b, d, d, dtype=torch.float32, device=g.device)
        check(lib.hk_triu_vec_bwd(ptr(g), ptr(dx), b, d, stream()), 'hk_triu_vec_bwd')
        return dx


def covpool(x):
    return _Covpool.apply(x)


def sqrtm(x, iter_n, symmetric=False, literal_backward=False):
    """Newton-Schulz square root of x [B,d,d] (MPNCOV.py:137-202; any square matrices).
    symmetric=True: the caller guarantees x == x^T (a covariance: what MPNCOV feeds it) - the forward then computes only
    the tiles on or above the diagonal blocks of every product (hk_ns_sqrtm_fwd_sym; wrong for other inputs).
    The backward shares one product between Y_i Z_i and Z_i Y_i (the iterates are polynomials in one matrix: they commute
    for every input); literal_backward=True runs the reference's 38 products literally (A/B checks)."""
    return _Sqrtm.apply(x, int(iter_n), bool(symmetric), bool(literal_backward))


def triuvec(x):
    return _Triuvec.apply(x)


def sqrtm_triuvec(x, iter_n, symmetric=False):
    """triuvec(sqrtm(x, iter_n, symmetric)) in one chain of launches: the last Newton-Schulz product writes the packed
    upper triangle itself (same bits as the two calls)."""
    return _SqrtmTriuvec.apply(x, int(iter_n), bool(symmetric))


# --------------------------------------------------------------------- CBP
def sketch_hashes(input_dim1, input_dim2, output_dim):
    """The reference's fixed count-sketch hashes (CBCNN.py:76-91): legacy numpy
    RandomState seeds 1/3 (h1/s1) and 5/7 (h2/s2).  Saves and restores the
    global numpy RNG state so constructing a model does not disturb user code."""
    state = np.random.get_state()
    try:
        np.random.seed(1)
        h1 = np.random.randint(output_dim, size=input_dim1)
        np.random.seed(3)
        s1 = 2 * np.random.randint(2, size=input_dim1) - 1
        np.random.seed(5)
        h2 = np.random.randint(output_dim, size=input_dim2)
        np.random.seed(7)
        s2 = 2 * np.random.randint(2, size=input_dim2) - 1
    finally:
        np.random.set_state(state)
    return h1.astype(np.int32), s1.astype(np.float32), h2.astype(np.int32), s2.astype(np.float32)


class CbpPlan:
    """Device-side CSR plan (bin -> signed entries of the C1 x C2 cross Gram) built once per device.  One width (C1 = C2):
    the hk_cbp_plan_build blob the one-input route (compact_bilinear_pool) needs; two widths (CBCNN.py:68-94): the
    hk_cbp_rect_plan_build blob.  The two-input forms (compact_bilinear_sketch) take either."""

    def __init__(self, h1, s1, h2, s2, output_dim, device):
        lib = _lib.load()
        assert h1.ndim == 1 and s1.ndim == 1 and len(h1) == len(s1)            # CBCNN.py:151-152
        assert h2.ndim == 1 and s2.ndim == 1 and len(h2) == len(s2)
        assert np.all(h1 >= 0) and np.all(h1 < output_dim)                      # CBCNN.py:153
        assert np.all(h2 >= 0) and np.all(h2 < output_dim)
        self.C1, self.C2, self.D, self.device = len(h1), len(h2), int(output_dim), device
        h1 = np.ascontiguousarray(h1, dtype=np.int32)
        h2 = np.ascontiguousarray(h2, dtype=np.int32)
        s1 = np.ascontiguousarray(s1, dtype=np.float32)
        s2 = np.ascontiguousarray(s2, dtype=np.float32)
        if self.C1 == self.C2:
            self.blob = torch.empty(lib.hk_cbp_plan_bytes(self.C1, self.D), dtype=torch.uint8, device=device)
            with _on(device):
                check(lib.hk_cbp_plan_build(h1.ctypes.data, s1.ctypes.data, h2.ctypes.data, s2.ctypes.data,
                                            self.C1, self.D, ptr(self.blob), stream()), 'hk_cbp_plan_build')
        else:
            self.blob = torch.empty(lib.hk_cbp_rect_plan_bytes(self.C1, self.C2, self.D), dtype=torch.uint8, device=device)
            with _on(device):
                check(lib.hk_cbp_rect_plan_build(h1.ctypes.data, s1.ctypes.data, self.C1, h2.ctypes.data, s2.ctypes.data,
                                                 self.C2, self.D, ptr(self.blob), stream()), 'hk_cbp_rect_plan_build')

    def __del__(self):
        # the library keeps a host-side note per plan ADDRESS: forget it before torch can hand the memory to someone else
        try:
            if getattr(self, 'blob', None) is not None:
                _lib.load().hk_cbp_plan_destroy(ptr(self.blob))
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class _CompactBilinearPool(torch.autograd.Function):
    """replaces CompactBilinearPooling.forward, model/methods/CBCNN.py:96-135."""

    @staticmethod
    def forward(ctx, x, plan):
        lib = _lib.load()
        x = _f32c(x)
        b, c, h, w = x.shape
        hw, d = h * w, plan.D
        if (plan.C1, plan.C2) != (c, c):
            raise _lib.HawkeyeHipError(f'compact_bilinear_pool: the plan was built for {plan.C1} x {plan.C2} channels, input has {c}')
        y = torch.empty(b, d, dtype=torch.float32, device=x.device)
        c_raw = torch.empty(b, d, dtype=torch.float32, device=x.device)
        inv_norm = torch.empty(b, dtype=torch.float32, device=x.device)
        nws = lib.hk_cbp_ws_bytes(b, c, hw, d)
        ws = _ws(nws, x.device)
        check(lib.hk_cbp_fwd(ptr(x), ptr(plan.blob), ptr(y), ptr(c_raw), ptr(inv_norm), b, c, hw, d,
                             ptr(ws), nws, stream()), 'hk_cbp_fwd')
        ctx.plan = plan
        ctx.save_for_backward(x, y, c_raw, inv_norm)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, c_raw, inv_norm = ctx.saved_tensors
        plan = ctx.plan
        b, c, h, w = x.shape
        hw, d = h * w, plan.D
        dy = _f32c(dy)
        dx = torch.empty_like(x)
        nws = lib.hk_cbp_ws_bytes(b, c, hw, d)
        ws = _ws(nws, x.device)
        check(lib.hk_cbp_bwd(ptr(x), ptr(plan.blob), ptr(y), ptr(c_raw), ptr(inv_norm), ptr(dy), ptr(dx),
                             b, c, hw, d, ptr(ws), nws, stream()), 'hk_cbp_bwd')
        return dx, None


def compact_bilinear_pool(x, plan):
    return _CompactBilinearPool.apply(x, plan)


def _bgemm_raw(lib, a, b, out, trans_a, trans_b, m, n, k, nb):
    check(lib.hk_bgemm_f32(ptr(a), a.shape[2], a.shape[1] * a.shape[2], int(trans_a), ptr(b), b.shape[2], b.shape[1] * b.shape[2],
                           int(trans_b), ptr(out), n, m * n, m, n, k, nb, 1.0, 0.0, 0.0, stream()), 'hk_bgemm_f32')


def _rect_shapes(x1, x2, plan, what):
    b, c1, h, w = x1.shape
    if x2.shape[0] != b or tuple(x2.shape[2:]) != (h, w) or (c1, x2.shape[1]) != (plan.C1, plan.C2):
        raise _lib.HawkeyeHipError(f'{what}: inputs {tuple(x1.shape)} / {tuple(x2.shape)}, plan for {plan.C1} x {plan.C2} channels')
    return b, c1, x2.shape[1], h, w


class _CbpCrossSum(torch.autograd.Function):
    """Count sketch of the summed outer product of TWO different maps (CompactBilinearPooling.forward with bottom2 given,
    CBCNN.py:96-130, before its signed sqrt): c[b,k] = sum_{(i,j) -> k} s1_i s2_j (X1 X2^T)[b,i,j] - the C1 x C2 cross Gram
    on the generic MFMA tiles (hk_bgemm_f32), the plan's CSR gather over it (hk_cbp_rect_bin_matrix); backward: dG from dc
    (hk_cbp_rect_unbin_matrix), dX1 = dG X2, dX2 = dG^T X1."""

    @staticmethod
    def forward(ctx, x1, x2, plan):
        lib = _lib.load()
        x1, x2 = _f32c(x1), _f32c(x2)
        b, c1, c2, h, w = _rect_shapes(x1, x2, plan, 'compact_bilinear_pool')
        hw, d = h * w, plan.D
        g = torch.empty(b, c1, c2, dtype=torch.float32, device=x1.device)
        _bgemm_raw(lib, x1.view(b, c1, hw), x2.view(b, c2, hw), g, False, True, c1, c2, hw, b)
        c_raw = torch.empty(b, d, dtype=torch.float32, device=x1.device)
        check(lib.hk_cbp_rect_bin_matrix(ptr(g), ptr(plan.blob), ptr(c_raw), b, c1, c2, d, stream()), 'hk_cbp_rect_bin_matrix')
        ctx.plan = plan
        ctx.save_for_backward(x1, x2)
        return c_raw

    @staticmethod
    def backward(ctx, dc):
        lib = _lib.load()
        x1, x2 = ctx.saved_tensors
        plan = ctx.plan
        b, c1, h, w = x1.shape
        c2, hw, d = x2.shape[1], h * w, plan.D
        dc = _f32c(dc)
        dg = torch.empty(b, c1, c2, dtype=torch.float32, device=x1.device)
        check(lib.hk_cbp_rect_unbin_matrix(ptr(dc), ptr(plan.blob), ptr(dg), b, c1, c2, d, stream()), 'hk_cbp_rect_unbin_matrix')
        dx1 = dx2 = None
        if ctx.needs_input_grad[0]:
            dx1 = torch.empty_like(x1)
            _bgemm_raw(lib, dg, x2.view(b, c2, hw), dx1.view(b, c1, hw), False, False, c1, hw, c2, b)
        if ctx.needs_input_grad[1]:
            dx2 = torch.empty_like(x2)
            _bgemm_raw(lib, dg, x1.view(b, c1, hw), dx2.view(b, c2, hw), True, False, c2, hw, c1, b)
        return dx1, dx2, None


def _loc_bwd_fits(ctx, c1, c2, d):
    """hk_cbp_rect_loc_bwd keeps dc[b,p,:], both channel columns and both hash tables of a location in LDS (144 KB of the CU's 160):
    say so in the FORWARD of a pass that will need it, not in the middle of backward()."""
    if any(ctx.needs_input_grad[:2]) and (d + 2 * (c1 + c2)) * 4 > 144 * 1024:
        raise _lib.HawkeyeHipError(f'compact_bilinear_pool(sum_pool=False): the backward holds D + 2 (C1 + C2) = {d + 2 * (c1 + c2)} '
                                   f'floats per location in LDS (limit {144 * 256}); run this shape under torch.no_grad() or reduce D')


class _CbpPerLocation(torch.autograd.Function):
    """The tensor sketch of every location on its own (CompactBilinearPooling.forward with sum_pool = False, CBCNN.py:117-128
    before its signed sqrt): c[b,h,w,k] = sum_{(i,j) -> k} s1_i s2_j x1[b,i,h,w] x2[b,j,h,w]  ->  [B,H,W,D]."""

    @staticmethod
    def forward(ctx, x1, x2, plan):
        lib = _lib.load()
        x1, x2 = _f32c(x1), _f32c(x2)
        b, c1, c2, h, w = _rect_shapes(x1, x2, plan, 'compact_bilinear_pool')
        _loc_bwd_fits(ctx, c1, c2, plan.D)
        out = torch.empty(b, h, w, plan.D, dtype=torch.float32, device=x1.device)
        check(lib.hk_cbp_rect_loc_fwd(ptr(x1), ptr(x2), ptr(plan.blob), ptr(out), b, c1, c2, h * w, plan.D, stream()),
              'hk_cbp_rect_loc_fwd')
        ctx.plan = plan
        ctx.save_for_backward(x1, x2)
        return out

    @staticmethod
    def backward(ctx, dc):
        lib = _lib.load()
        x1, x2 = ctx.saved_tensors
        plan = ctx.plan
        b, c1, h, w = x1.shape
        dc = _f32c(dc)
        dx1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
        dx2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        check(lib.hk_cbp_rect_loc_bwd(ptr(x1), ptr(x2), ptr(dc), ptr(plan.blob), ptr(dx1), ptr(dx2), b, c1, x2.shape[1], h * w,
                                      plan.D, stream()), 'hk_cbp_rect_loc_bwd')
        return dx1, dx2, None


def compact_bilinear_sketch(x1, x2, plan, sum_pool=True):
    """The count sketch BEFORE the signed square root, for the forms Hawkeye's own CBCNN does not take: two different inputs
    ([B,D]) or no sum over the map ([B,H,W,D]); x2 may be x1.  Any widths C1, C2 of the plan."""
    return _CbpCrossSum.apply(x1, x2, plan) if sum_pool else _CbpPerLocation.apply(x1, x2, plan)


# --------------------------------------------------------------------- AP-CNN
class _AttPool(torch.autograd.Function):
    """gap = mean_hw F ; sgap = mean_hw a_s F  (one pass over F).
    replaces APCNN.py:256-266 + the AdaptiveAvgPool2d(1) heads :377-405,:533-538."""

    @staticmethod
    def forward(ctx, f, a_s):
        lib = _lib.load()
        f = _f32c(f)
        b, c, h, w = f.shape
        gap = torch.empty(b, c, dtype=torch.float32, device=f.device)
        if a_s is None:
            check(lib.hk_att_pool_fwd(ptr(f), None, ptr(gap), None, b, c, h * w, stream()), 'hk_att_pool_fwd')
            ctx.save_for_backward(f)
            ctx.has_att = False
            return gap, None
        a_s = _f32c(a_s)
        if a_s.numel() != b * h * w:
            raise _lib.HawkeyeHipError(f'att_pool: spatial attention must have {b} x {h} x {w} elements, got {tuple(a_s.shape)}')
        sgap = torch.empty(b, c, dtype=torch.float32, device=f.device)
        check(lib.hk_att_pool_fwd(ptr(f), ptr(a_s), ptr(gap), ptr(sgap), b, c, h * w, stream()), 'hk_att_pool_fwd')
        ctx.save_for_backward(f, a_s)
        ctx.has_att = True
        return gap, sgap

    @staticmethod
    def backward(ctx, dgap, dsgap):
        lib = _lib.load()
        f = ctx.saved_tensors[0]
        b, c, h, w = f.shape
        df = torch.empty_like(f)
        if dgap is None:
            dgap = torch.zeros(b, c, dtype=torch.float32, device=f.device)
        dgap = _f32c(dgap)
        if not ctx.has_att:
            check(lib.hk_att_pool_bwd(ptr(f), None, ptr(dgap), None, ptr(df), None, b, c, h * w, stream()),
                  'hk_att_pool_bwd')
            return df, None
        a_s = ctx.saved_tensors[1]
        if dsgap is None:
            dsgap = torch.zeros(b, c, dtype=torch.float32, device=f.device)
        dsgap = _f32c(dsgap)
        da = torch.empty_like(a_s)
        check(lib.hk_att_pool_bwd(ptr(f), ptr(a_s), ptr(dgap), ptr(dsgap), ptr(df), ptr(da), b, c, h * w,
                                  stream()), 'hk_att_pool_bwd')
        return df, da


def att_pool(f, a_s=None):
    """-> (gap [B,C], sgap [B,C] or None)"""
    return _AttPool.apply(f, a_s)


class _AttPool3(torch.autograd.Function):
    """The three pyramid levels of PyramidAttentions (APCNN.py:256-266) in one launch per direction:
    (f3, f4, f5, a3, a4, a5) -> gap [3,B,C], sgap [3,B,C]."""

    @staticmethod
    def forward(ctx, f0, f1, f2, a0, a1, a2):
        lib = _lib.load()
        fs = [_f32c(f) for f in (f0, f1, f2)]
        as_ = [_f32c(a) for a in (a0, a1, a2)]
        b, c = fs[0].shape[:2]
        hws = [f.shape[2] * f.shape[3] for f in fs]
        for f, a, hw in zip(fs, as_, hws):
            if f.shape[:2] != (b, c) or a.numel() != b * hw:
                raise _lib.HawkeyeHipError(f'att_pool_levels: level shapes {tuple(f.shape)} / {tuple(a.shape)} do not match [{b},{c},h,w] / [{b},1,h,w]')
        gap = torch.empty(3, b, c, dtype=torch.float32, device=fs[0].device)
        sgap = torch.empty_like(gap)
        check(lib.hk_att_pool3_fwd(ptr(fs[0]), ptr(fs[1]), ptr(fs[2]), ptr(as_[0]), ptr(as_[1]), ptr(as_[2]), ptr(gap), ptr(sgap),
                                   b, c, hws[0], hws[1], hws[2], stream()), 'hk_att_pool3_fwd')
        ctx.save_for_backward(*fs, *as_)
        return gap, sgap

    @staticmethod
    def backward(ctx, dgap, dsgap):
        lib = _lib.load()
        fs, as_ = ctx.saved_tensors[:3], ctx.saved_tensors[3:]
        b, c = fs[0].shape[:2]
        hws = [f.shape[2] * f.shape[3] for f in fs]
        dgap = _f32c(dgap) if dgap is not None else torch.zeros(3, b, c, dtype=torch.float32, device=fs[0].device)
        dsgap = _f32c(dsgap) if dsgap is not None else torch.zeros(3, b, c, dtype=torch.float32, device=fs[0].device)
        dfs = [torch.empty_like(f) for f in fs]
        das = [torch.empty_like(a) for a in as_]
        check(lib.hk_att_pool3_bwd(ptr(fs[0]), ptr(fs[1]), ptr(fs[2]), ptr(as_[0]), ptr(as_[1]), ptr(as_[2]), ptr(dgap), ptr(dsgap),
                                   ptr(dfs[0]), ptr(dfs[1]), ptr(dfs[2]), ptr(das[0]), ptr(das[1]), ptr(das[2]),
                                   b, c, hws[0], hws[1], hws[2], stream()), 'hk_att_pool3_bwd')
        return (*dfs, *das)


def att_pool_levels(feats, atts):
    """feats: three [B,C,h,w] pyramid levels, atts: their spatial attentions [B,1,h,w] -> (gap [3,B,C], sgap [3,B,C])."""
    return _AttPool3.apply(*feats, *atts)


def att_roi_select(att_mask, feature_stride, anchor_size, img_h, img_w, num_classes, iou_thred, topk):
    """Device-side get_att_roi (APCNN.py:444-476).  -> (rois [B,topk,5], count [B] int32),
    rows beyond count are zero.  No gradient (reference: torch.no_grad, :447)."""
    lib = _lib.load()
    with torch.no_grad():
        a = _f32c(att_mask.detach())
        n, _, h, w = a.shape
        lo, hi = (0.2, 0.8) if num_classes == 200 else (0.1, 0.9)     # APCNN.py:451-455
        r0, r1, c0, c1 = int(lo * h), int(hi * h), int(lo * w), int(hi * w)
        rois = torch.empty(n, topk, 5, dtype=torch.float32, device=a.device)
        cnt = torch.empty(n, dtype=torch.int32, device=a.device)
        check(lib.hk_att_roi_select(ptr(a), ptr(rois), ptr(cnt), n, h, w, int(feature_stride), float(anchor_size),
                                    int(img_h), int(img_w), r0, r1, c0, c1, float(iou_thred), int(topk), stream()),
              'hk_att_roi_select')
    return rois, cnt


def att_roi_select_levels(att_masks, levels, img_h, img_w, num_classes, iou_thred):
    """The three pyramid levels of one forward in one launch (hk_att_roi_select3): att_masks = (a3, a4, a5),
    levels = ((feature_stride, anchor_size, topk), ...).  -> [(rois, count)] * 3, the results of three att_roi_select
    calls bit for bit."""
    import ctypes
    lib = _lib.load()
    assert len(att_masks) == 3 and len(levels) == 3
    with torch.no_grad():
        a = [_f32c(m.detach()) for m in att_masks]
        n = a[0].shape[0]
        lo, hi = (0.2, 0.8) if num_classes == 200 else (0.1, 0.9)     # APCNN.py:451-455
        hs, ws = [m.shape[2] for m in a], [m.shape[3] for m in a]
        keep = []
        for h, w in zip(hs, ws):
            keep += [int(lo * h), int(hi * h), int(lo * w), int(hi * w)]
        rois = [torch.empty(n, int(k), 5, dtype=torch.float32, device=a[0].device) for _, _, k in levels]
        cnt = [torch.empty(n, dtype=torch.int32, device=a[0].device) for _ in levels]
        P3, I3, F3, I12 = ctypes.c_void_p * 3, ctypes.c_int * 3, ctypes.c_float * 3, ctypes.c_int * 12
        arrs = (P3(*[ptr(m) for m in a]), P3(*[ptr(r) for r in rois]), P3(*[ptr(c) for c in cnt]), I3(*hs), I3(*ws),
                I3(*[int(s) for s, _, _ in levels]), F3(*[float(z) for _, z, _ in levels]), I12(*keep),
                I3(*[int(k) for _, _, k in levels]))               # host arrays, read by the entry point before it returns
        ad = [ctypes.addressof(x) for x in arrs]
        check(lib.hk_att_roi_select3(ad[0], ad[1], ad[2], n, ad[3], ad[4], ad[5], ad[6], int(img_h), int(img_w), ad[7],
                                     float(iou_thred), ad[8], stream()), 'hk_att_roi_select3')
    return list(zip(rois, cnt))


def roi_boxes(tables, u01, scale):
    """Union / drop boxes on device from three (rois, count) tables.  -> box [B,4], drop [B,4]"""
    lib = _lib.load()
    (r3, n3), (r4, n4), (r5, n5) = tables
    b = r3.shape[0]
    box = torch.empty(b, 4, dtype=torch.float32, device=r3.device)
    drop = torch.empty(b, 4, dtype=torch.float32, device=r3.device)
    check(lib.hk_roi_boxes(ptr(r3), ptr(n3), r3.shape[1], ptr(r4), ptr(n4), r4.shape[1], ptr(r5), ptr(n5),
                           r5.shape[1], ptr(u01) if u01 is not None else None, float(scale), ptr(box), ptr(drop),
                           b, stream()), 'hk_roi_boxes')
    return box, drop


class _RoiCropResize(torch.autograd.Function):
    """replaces get_roi_crop_feat's per-image python loop, APCNN.py:478-531."""

    @staticmethod
    def forward(ctx, x, box, drop, training):
        lib = _lib.load()
        x = _f32c(x)
        b, c, h, w = x.shape
        box, drop = _f32c(box), _f32c(drop)
        if tuple(box.shape) != (b, 4) or tuple(drop.shape) != (b, 4):
            raise _lib.HawkeyeHipError(f'roi_crop_resize: box and drop must be [{b}, 4], got {tuple(box.shape)} and {tuple(drop.shape)}')
        y = torch.empty_like(x)
        check(lib.hk_roi_crop_resize_fwd(ptr(x), ptr(box), ptr(drop), ptr(y), b, c, h, w, int(training), stream()),
              'hk_roi_crop_resize_fwd')
        ctx.save_for_backward(box, drop)
        ctx.training = int(training)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        box, drop = ctx.saved_tensors
        dy = _f32c(dy)
        b, c, h, w = dy.shape
        dx = torch.empty_like(dy)
        check(lib.hk_roi_crop_resize_bwd(ptr(dy), ptr(box), ptr(drop), ptr(dx), b, c, h, w, ctx.training, stream()),
              'hk_roi_crop_resize_bwd')
        return dx, None, None, None


def roi_crop_resize(x, box, drop, training):
    return _RoiCropResize.apply(x, box, drop, training)


# --------------------------------------------------------------------- OSME
class _OsmeGap(torch.autograd.Function):
    """z = GAP(x).  replaces OSME.py:21 (avg_pool + squeeze)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        n, c, h, w = x.shape
        z = torch.empty(n, c, dtype=torch.float32, device=x.device)
        check(lib.hk_osme_gap(ptr(x), ptr(z), n, c, h * w, stream()), 'hk_osme_gap')
        ctx.shape = x.shape
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.load()
        n, c, h, w = ctx.shape
        dz = _f32c(dz)
        dx = torch.empty(n, c, h, w, dtype=torch.float32, device=dz.device)
        # dx[b,c,:] = dz[b,c] / HW: the row-parallel GAP backward of the attention pooling (one launch; without a gate
        # the entry point takes no F)
        check(lib.hk_att_pool_bwd(None, None, ptr(dz), None, ptr(dx), None, n, c, h * w, stream()), 'hk_att_pool_bwd')
        return dx


class _OsmeScale(torch.autograd.Function):
    """s[p] = m[p] (.) x for all P gates in one pass.  replaces OSME.py:23."""

    @staticmethod
    def forward(ctx, x, m):
        lib = _lib.load()
        x, m = _f32c(x), _f32c(m)
        n, c, h, w = x.shape
        if m.dim() != 3 or tuple(m.shape[1:]) != (n, c):
            raise _lib.HawkeyeHipError(f'osme_scale: gates must be [P, N, C] = [P, {n}, {c}], got {tuple(m.shape)}')
        p = m.shape[0]
        s = torch.empty(p, n, c, h, w, dtype=torch.float32, device=x.device)
        check(lib.hk_osme_scale_fwd(ptr(x), ptr(m), ptr(s), p, n, c, h * w, stream()), 'hk_osme_scale_fwd')
        ctx.save_for_backward(x, m)
        return s

    @staticmethod
    def backward(ctx, ds):
        lib = _lib.load()
        x, m = ctx.saved_tensors
        n, c, h, w = x.shape
        p = m.shape[0]
        ds = _f32c(ds)
        dx = torch.empty_like(x)
        dm = torch.empty_like(m)
        check(lib.hk_osme_scale_bwd(ptr(x), ptr(m), ptr(ds), None, ptr(dx), ptr(dm), p, n, c, h * w, stream()),
              'hk_osme_scale_bwd')
        return dx, dm


def osme_gap(x):
    return _OsmeGap.apply(x)


def osme_scale(x, m):
    """x [N,C,H,W], m [P,N,C] -> s [P,N,C,H,W]"""
    return _OsmeScale.apply(x, m)


# --------------------------------------------------------------------- generic
# --------------------------------------------------------------------- CIN channel interaction
# hk_cin_sci_fwd: for C % 64 == 0 and 7x7 / 8x8 / 6x6 maps ONE kernel (cin.hip: two passes over the column blocks, softmax
# statistics first, then W written once and consumed from registers by the second product) - 297 us at the plugin's shape
# (B = 20, C = 2048, HW = 49) against 486 us for rocBLAS bmm + softmax + bmm.  14x14 / 12x12 / 10x10 maps (a 448^2 input):
# the scores are materialised by the Gram panel kernel, then row statistics, then ONE kernel that applies the softmax on the
# way into the second product and writes W once, in place (631 us at B = 20, C = 2048, HW = 196; library 937).  Other shapes
# run the three-kernel chain on the generic MFMA tile inside the same entry point - there is no library branch.


class _CinSci(torch.autograd.Function):
    """W = softmax_rows(-X X^T / HW), Y = W X.  replaces model/methods/CIN.py:31-34.  W is an output too: the
    contrastive branch (cin_cci) consumes it and sends a gradient back into it."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib.load()
        x = _f32c(x)
        b, c, hw = x.shape
        w = torch.empty(b, c, c, dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        check(lib.hk_cin_sci_fwd(ptr(x), ptr(w), ptr(y), b, c, hw, stream()), 'hk_cin_sci_fwd')
        ctx.save_for_backward(x, w)
        ctx.set_materialize_grads(False)
        return y, w

    @staticmethod
    def backward(ctx, dy, dw):
        lib = _lib.load()
        x, w = ctx.saved_tensors
        b, c, hw = x.shape
        dy = _f32c(dy) if dy is not None else torch.zeros_like(x)
        dwbuf = _f32c(dw).clone() if dw is not None else torch.empty_like(w)     # overwritten by the kernel chain
        dx = torch.empty_like(x)
        check(lib.hk_cin_sci_bwd(ptr(x), ptr(w), ptr(dy), ptr(dwbuf), int(dw is not None), ptr(dx), b, c, hw, stream()),
              'hk_cin_sci_bwd')
        return dx


class _CinCci(torch.autograd.Function):
    """Yc[b] = |W[b] - w_b W[(b + B/2) % B]| X[b].  replaces model/methods/CIN.py:51-54."""

    @staticmethod
    def forward(ctx, w, x, wt):
        lib = _lib.load()
        w, x, wt = _f32c(w), _f32c(x), _f32c(wt)
        b, c, hw = x.shape
        if b % 2 or wt.shape != (b,):
            raise _lib.HawkeyeHipError(f'cin_cci: batch {b} must be even and weights [B], got {tuple(wt.shape)}')
        y = torch.empty_like(x)
        check(lib.hk_cin_cci_fwd(ptr(x), ptr(w), ptr(wt), ptr(y), b, c, hw, stream()), 'hk_cin_cci_fwd')
        ctx.save_for_backward(w, x, wt)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        w, x, wt = ctx.saved_tensors
        b, c, hw = x.shape
        dy = _f32c(dy)
        dx, dw, dwt = torch.empty_like(x), torch.empty_like(w), torch.empty_like(wt)
        nws = lib.hk_cin_cci_ws_bytes(b, c)
        ws = _ws(nws, x.device)
        check(lib.hk_cin_cci_bwd(ptr(x), ptr(w), ptr(wt), ptr(dy), ptr(dx), ptr(dw), ptr(dwt), b, c, hw, ptr(ws), nws,
                                 stream()), 'hk_cin_cci_bwd')
        return dw, dx, dwt


def cin_sci(x):
    """x [B,C,HW] -> (Y [B,C,HW], W_SCI [B,C,C])."""
    return _CinSci.apply(x)


def cin_cci(w_sci, x, weight):
    """W_SCI [B,C,C], x [B,C,HW], weight [B] (eta for the first half of the batch, gamma for the second) -> Y_CCI."""
    return _CinCci.apply(w_sci, x, weight)


# --------------------------------------------------------------------- MAMC n-pairs loss
class _NPairsLoss(torch.autograd.Function):
    """replaces NPairsLoss.forward, model/loss/MAMC_loss.py:34-90.  The kernel returns the loss and its gradient
    with respect to the parts in one pass; backward only scales it."""

    @staticmethod
    def forward(ctx, parts, targets):
        lib = _lib.load()
        parts = _f32c(parts)
        b, p, d = parts.shape
        labels = _int_tensor(targets, (b,), torch.int32, parts.device, 'npairs_loss', 'targets')
        loss = torch.empty(1, dtype=torch.float32, device=parts.device)
        dx = torch.empty_like(parts)
        nws = lib.hk_npairs_ws_bytes(b * p, d)
        ws = _ws(nws, parts.device)
        check(lib.hk_npairs_loss(ptr(parts), ptr(labels), ptr(loss), ptr(dx), b, p, d, ptr(ws), nws, stream()),
              'hk_npairs_loss')
        ctx.save_for_backward(dx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        return _loss_backward(ctx, g, 1)


def npairs_loss(parts, targets):
    """parts [B,P,D] (OSMENet's second output), targets [B] -> scalar n-pairs loss (MAMC eq. 11)."""
    return _NPairsLoss.apply(parts, targets)


# --------------------------------------------------------------------- peer-learning loss
def _peer_args(logits_1, logits_2, labels, drop_rate):
    if logits_1.dim() != 2 or logits_1.shape != logits_2.shape:
        raise _lib.HawkeyeHipError(f'peer_learning_loss: logits of shapes {tuple(logits_1.shape)} and {tuple(logits_2.shape)}; '
                                   f'two [N, C] matrices of one shape are needed')
    _one_device('peer_learning_loss', logits_1.device, logits_2)
    l1, l2 = _f32c(logits_1), _f32c(logits_2)          # dense copies of views; the kernels read rows of C floats
    y = _int_tensor(labels, (l1.shape[0],), torch.int32, l1.device, 'peer_learning_loss', 'labels')
    return l1, l2, y, float(drop_rate)


def _peer_call(l1, l2, y, drop_rate):
    lib = _lib.load()
    n, c = l1.shape
    loss = torch.empty(2, dtype=torch.float32, device=l1.device)
    dl1, dl2 = torch.empty_like(l1), torch.empty_like(l2)
    stats = torch.empty(4, dtype=torch.int32, device=l1.device)
    nws = lib.hk_peer_loss_ws_bytes(n, c)
    ws = _ws(nws, l1.device)
    check(lib.hk_peer_loss(ptr(l1), ptr(l2), ptr(y), drop_rate, ptr(loss), ptr(dl1), ptr(dl2), ptr(stats), n, c, ptr(ws),
                           nws, stream()), 'hk_peer_loss')
    return loss, dl1, dl2, stats


class _PeerLearningLoss(torch.autograd.Function):
    """replaces PeerLearningLoss, model/loss/peer_learning_loss.py:5-65.  The kernel returns both losses and both
    gradients in one pass; backward only scales them.  loss_1 depends on logits_1 alone and loss_2 on logits_2 alone
    (the selection is not differentiated: the reference sorts `.data`)."""

    @staticmethod
    def forward(ctx, logits_1, logits_2, labels, drop_rate):
        l1, l2, y, drop_rate = _peer_args(logits_1, logits_2, labels, drop_rate)
        loss, dl1, dl2, stats = _peer_call(l1, l2, y, drop_rate)
        ctx.save_for_backward(dl1, dl2)
        ctx.mark_non_differentiable(stats)
        return loss[0], loss[1], stats

    @staticmethod
    def backward(ctx, g1, g2, _g_stats):
        dl1, dl2 = ctx.saved_tensors
        return dl1 * g1, dl2 * g2, None, None


def peer_learning_loss(logits_1, logits_2, labels, drop_rate):
    """logits_1, logits_2 [N,C], labels [N], drop_rate (host float in [0, 1]) -> (loss_1, loss_2), each net's mean cross
    entropy over the rows it keeps: every row on which the two argmaxes disagree, and of the n agreeing rows the
    int((1 - drop_rate) n) its PEER ranks lowest in cross entropy."""
    loss_1, loss_2, _ = _PeerLearningLoss.apply(logits_1, logits_2, labels, drop_rate)
    return loss_1, loss_2


def peer_learning_loss_with_stats(logits_1, logits_2, labels, drop_rate):
    """peer_learning_loss plus the int32 device tensor [n, m, count_1, count_2] (agreeing rows, agreeing rows kept, rows in
    each net's mean) - for tests and logging; nothing is read back to the host here."""
    return _PeerLearningLoss.apply(logits_1, logits_2, labels, drop_rate)


def peer_learning_stats(logits_1, logits_2, labels, drop_rate):
    """Only the [n, m, count_1, count_2] device tensor of peer_learning_loss (no autograd)."""
    with torch.no_grad():
        return _peer_call(*_peer_args(logits_1, logits_2, labels, drop_rate))[3]


# --------------------------------------------------------------------- APINet pairwise interaction
def _api_pool(pool, what):
    if pool.dim() != 2 or pool.shape[0] < 1 or pool.shape[1] < 1:
        raise _lib.HawkeyeHipError(f'{what}: pool must be [B, D] pooled vectors, got {tuple(pool.shape)}')
    return _f32c(pool)


def _api_partner(partner, pool, what):
    return _int_tensor(partner, (2 * pool.shape[0],), torch.int32, pool.device, what, 'partner', same_device=True)


def api_pairs(pool, labels):
    """pool [B,D], labels [B] -> partner int32 [2B] on the device (no autograd, no host round trip): partner[i] the
    nearest row of the same label (j != i), partner[B+i] the nearest row of another label; squared Euclidean distance,
    ties to the lowest index, 0 where a row has no candidate.  replaces get_pairs, model/methods/APINet.py:76-91."""
    pool = _api_pool(pool.detach(), 'api_pairs')
    b, d = pool.shape
    y = _int_tensor(labels, (b,), torch.int32, pool.device, 'api_pairs', 'labels')
    lib = _lib.load()
    partner = torch.empty(2 * b, dtype=torch.int32, device=pool.device)
    check(lib.hk_api_pairs(ptr(pool), ptr(y), ptr(partner), b, d, stream()), 'hk_api_pairs')
    return partner


class _ApiPairFeatures(torch.autograd.Function):
    """mutual = [pool[r mod B] | pool[partner[r]]].  replaces APINet.py:36-37,41 (four index gathers and three cats);
    the backward is the deterministic scatter of hk_api_gather_bwd."""

    @staticmethod
    def forward(ctx, pool, partner):
        lib = _lib.load()
        pool = _api_pool(pool, 'api_pair_features')
        partner = _api_partner(partner, pool, 'api_pair_features')
        b, d = pool.shape
        mutual = torch.empty(2 * b, 2 * d, dtype=torch.float32, device=pool.device)
        check(lib.hk_api_gather_fwd(ptr(pool), ptr(partner), ptr(mutual), b, d, stream()), 'hk_api_gather_fwd')
        ctx.save_for_backward(partner)
        ctx.shape = (b, d)
        return mutual

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (partner,) = ctx.saved_tensors
        b, d = ctx.shape
        g = _f32c(g)
        dpool = torch.empty(b, d, dtype=torch.float32, device=g.device)
        check(lib.hk_api_gather_bwd(ptr(g), ptr(partner), ptr(dpool), b, d, stream()), 'hk_api_gather_bwd')
        return dpool, None


def api_pair_features(pool, partner):
    """pool [B,D], partner [2B] (api_pairs) -> mutual [2B,2D]: each row next to its partner, intra pairs first."""
    return _ApiPairFeatures.apply(pool, partner)


class _ApiInteract(torch.autograd.Function):
    """The gates and the four gated feature blocks in one launch each way.  replaces APINet.py:46-61 (and, through the
    row order of `feats`, the zeros + slice copies of :63-68)."""

    @staticmethod
    def forward(ctx, pool, partner, m, masks, drop_p):
        lib = _lib.load()
        pool = _api_pool(pool, 'api_interact')
        partner = _api_partner(partner, pool, 'api_interact')
        b, d = pool.shape
        if tuple(m.shape) != (2 * b, d):
            raise _lib.HawkeyeHipError(f'api_interact: m must be [2B, D] = [{2 * b}, {d}], got {tuple(m.shape)}')
        _one_device('api_interact', pool.device, m)
        m = _f32c(m)
        scale = 1.0
        if masks is not None:
            if masks.dtype not in (torch.bool, torch.uint8):
                raise _lib.HawkeyeHipError(f'api_interact: keep-masks must be bool or uint8; got {masks.dtype}')
            if tuple(masks.shape) != (8 * b, d):
                raise _lib.HawkeyeHipError(f'api_interact: keep-masks must be [8B, D] = [{8 * b}, {d}], got {tuple(masks.shape)}')
            _one_device('api_interact', pool.device, masks)
            if not 0.0 <= drop_p < 1.0:
                raise _lib.HawkeyeHipError(f'api_interact: drop_p must lie in [0, 1); got {drop_p}')
            masks = masks.contiguous().view(torch.uint8)
            scale = 1.0 / (1.0 - drop_p)
        feats = torch.empty(8 * b, d, dtype=torch.float32, device=pool.device)
        check(lib.hk_api_interact_fwd(ptr(pool), ptr(partner), ptr(m), ptr(masks), scale, ptr(feats), b, d, stream()),
              'hk_api_interact_fwd')
        ctx.save_for_backward(pool, partner, m, masks)
        ctx.scale = scale
        return feats

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        pool, partner, m, masks = ctx.saved_tensors
        b, d = pool.shape
        g = _f32c(g)
        dm, dpool = torch.empty_like(m), torch.empty_like(pool)
        check(lib.hk_api_interact_bwd(ptr(pool), ptr(partner), ptr(m), ptr(masks), ctx.scale, ptr(g), ptr(dm), ptr(dpool), b, d,
                                      stream()), 'hk_api_interact_bwd')
        return dpool, None, dm, None, None


def api_interact(pool, partner, m, masks=None, drop_p=0.5):
    """pool [B,D], partner [2B], m [2B,D] (= map2(drop(map1(mutual)))) -> feats [8B,D] in the row order 1-self, 2-self,
    1-other, 2-other, so that fc(feats) split in half is (self_logits, other_logits).  masks: bool / uint8 [8B,D]
    keep-masks of the four dropouts (kept elements are scaled by 1 / (1 - drop_p)); None: no dropout."""
    return _ApiInteract.apply(pool, partner, m, masks, float(drop_p))


def _apinet_loss_args(self_logits, other_logits, labels1, labels2, what='apinet_loss'):
    if self_logits.dim() != 2 or self_logits.shape != other_logits.shape:
        raise _lib.HawkeyeHipError(f'{what}: logits of shapes {tuple(self_logits.shape)} and {tuple(other_logits.shape)}; '
                                   f'two [R, C] matrices of one shape are needed')
    _one_device(what, self_logits.device, other_logits)
    ls, lo = _f32c(self_logits), _f32c(other_logits)
    r = ls.shape[0]
    if labels1.dim() != 1 or labels1.shape != labels2.shape or 2 * labels1.shape[0] != r:
        raise _lib.HawkeyeHipError(f'{what}: {r} rows need labels1 and labels2 of shape ({r // 2},) each, got '
                                   f'{tuple(labels1.shape)} and {tuple(labels2.shape)}')
    return ls, lo, _int_tensor(torch.cat([labels1, labels2]), (r,), torch.int32, ls.device, what, 'labels')     # one cat, one cast


class _APINetLoss(torch.autograd.Function):
    """replaces APINetLoss.__call__, model/loss/APINet_loss.py:29-39.  The kernel returns the three loss terms and both
    logit gradients of the total in one call; backward only scales them."""

    @staticmethod
    def forward(ctx, self_logits, other_logits, labels1, labels2, label_smoothing, margin):
        ls, lo, y = _apinet_loss_args(self_logits, other_logits, labels1, labels2)
        lib = _lib.load()
        r, c = ls.shape
        loss = torch.empty(3, dtype=torch.float32, device=ls.device)
        ds, do = torch.empty_like(ls), torch.empty_like(lo)
        nws = lib.hk_apinet_loss_ws_bytes(r, c)
        ws = _ws(nws, ls.device)
        check(lib.hk_apinet_loss(ptr(ls), ptr(lo), ptr(y), label_smoothing, margin, ptr(loss), ptr(ds), ptr(do), r, c, ptr(ws),
                                 nws, stream()), 'hk_apinet_loss')
        return _loss_forward(ctx, loss, (ds, do))

    @staticmethod
    def backward(ctx, g, _g_parts):
        return _loss_backward(ctx, g, 4)


def apinet_loss(self_logits, other_logits, labels1, labels2, label_smoothing=0.1, margin=0.05):
    """self_logits, other_logits [4B,C], labels1, labels2 [2B] (APINet's training outputs) -> the scalar loss: cross
    entropy with label smoothing over cat(self, other) against the fourfold targets, plus the mean hinge
    max(0, p_other[y] - p_self[y] + margin)."""
    return _APINetLoss.apply(self_logits, other_logits, labels1, labels2, float(label_smoothing), float(margin))[0]


def apinet_loss_with_parts(self_logits, other_logits, labels1, labels2, label_smoothing=0.1, margin=0.05):
    """apinet_loss plus the device tensor [CE, rank] of its two terms (not differentiable) - for logging and tests."""
    return _APINetLoss.apply(self_logits, other_logits, labels1, labels2, float(label_smoothing), float(margin))


# --------------------------------------------------------------------- NTS-Net proposals, part crops, loss
def nts_nms(scores, anchors, topn, iou_thresh=0.25):
    """scores [B,A], anchors integer [A,4] = y0, x0, y1, x1 -> (index int64 [B,topn], boxes int32 [B,topn,4]) on the
    device, no autograd, no host round trip.  replaces hard_nms (model/methods/NTS_Net/anchors.py:63-90) and the numpy
    plumbing around it (NTSNet.py:35-41): greedy, highest live score first, a live anchor survives a pick only with
    IoU < iou_thresh (strictly; corner differences without + 1, evaluated in float64 as the reference does).  Equal
    scores go to the highest index - what a stable ascending sort read from its end gives; the reference's argsort is
    not stable there.  A slot that no live anchor can fill repeats the last chosen anchor: the reference builds a ragged
    array and fails on it; with the default anchor set (426 or 1614 anchors, topn 6) that cannot happen.  hard_nms also
    stops when every remaining row is all zeros (`res.any()`); that quirk is not reproduced.  A <= 2048."""
    if scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise _lib.HawkeyeHipError(f'nts_nms: scores must be [B, A], got {tuple(scores.shape)}')
    scores = _f32c(scores.detach())
    b, a = scores.shape
    topn = int(topn)
    if topn < 1:
        raise _lib.HawkeyeHipError(f'nts_nms: topn must be positive; got {topn}')
    anchors = _int_tensor(anchors, (a, 4), torch.int32, scores.device, 'nts_nms', 'anchors', same_device=True)
    lib = _lib.load()
    index = torch.empty(b, topn, dtype=torch.int32, device=scores.device)
    boxes = torch.empty(b, topn, 4, dtype=torch.int32, device=scores.device)
    check(lib.hk_nts_nms(ptr(scores), ptr(anchors), ptr(index), ptr(boxes), b, a, topn, float(iou_thresh), stream()), 'hk_nts_nms')
    return index.long(), boxes


def nts_crop_resize(images, boxes, pad, size):
    """images [B,C,H,W], boxes integer [B,N,4] = y0, x0, y1, x1 in image coordinates -> [B N,C,size_h,size_w]: each box
    cut out of its image as if the image were zero-padded by `pad` on every side (the box is clipped to the padded
    extent) and resized bilinearly with align_corners=True.  replaces F.pad and the double loop of F.interpolate,
    NTSNet.py:31,43-47.  No autograd: the reference detaches the crops."""
    if images.dim() != 4 or min(images.shape) < 1:
        raise _lib.HawkeyeHipError(f'nts_crop_resize: images must be [B, C, H, W], got {tuple(images.shape)}')
    images = _f32c(images.detach())
    b, c, h, w = images.shape
    if boxes.dim() != 3 or boxes.shape[1] < 1:
        raise _lib.HawkeyeHipError(f'nts_crop_resize: boxes must be [B, N, 4], got {tuple(boxes.shape)}')
    n = boxes.shape[1]
    boxes = _int_tensor(boxes, (b, n, 4), torch.int32, images.device, 'nts_crop_resize', 'boxes', same_device=True)
    oh, ow = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1 or int(pad) < 0:
        raise _lib.HawkeyeHipError(f'nts_crop_resize: size {size} and pad {pad} must be positive / non-negative')
    lib = _lib.load()
    out = torch.empty(b * n, c, oh, ow, dtype=torch.float32, device=images.device)
    check(lib.hk_nts_crop_resize(ptr(images), ptr(boxes), ptr(out), b, n, c, h, w, int(pad), oh, ow, stream()), 'hk_nts_crop_resize')
    return out


def _nts_loss_args(raw_logits, concat_logits, part_logits, top_n_prob, labels, what='nts_loss'):
    if raw_logits.dim() != 2 or raw_logits.shape != concat_logits.shape:
        raise _lib.HawkeyeHipError(f'{what}: raw and concat logits of shapes {tuple(raw_logits.shape)} and '
                                   f'{tuple(concat_logits.shape)}; two [B, C] matrices of one shape are needed')
    b, c = raw_logits.shape
    if part_logits.dim() != 3 or part_logits.shape[0] != b or part_logits.shape[2] != c or part_logits.shape[1] < 1:
        raise _lib.HawkeyeHipError(f'{what}: part_logits must be [{b}, N, {c}], got {tuple(part_logits.shape)}')
    n = part_logits.shape[1]
    if tuple(top_n_prob.shape) != (b, n):
        raise _lib.HawkeyeHipError(f'{what}: top_n_prob must be [{b}, {n}], got {tuple(top_n_prob.shape)}')
    _one_device(what, raw_logits.device, concat_logits, part_logits, top_n_prob)
    y = _int_tensor(labels, (b,), torch.int32, raw_logits.device, what, 'labels')
    return _f32c(raw_logits), _f32c(concat_logits), _f32c(part_logits), _f32c(top_n_prob), y


class _NTSLoss(torch.autograd.Function):
    """replaces NTSLoss.__call__, list_loss and ranking_loss, model/loss/NTS_loss.py:15-47.  The kernel returns the five
    loss terms and all four gradients of the total in one launch; backward only scales them."""

    @staticmethod
    def forward(ctx, raw_logits, concat_logits, part_logits, top_n_prob, labels, label_smoothing):
        raw, cat, part, prob, y = _nts_loss_args(raw_logits, concat_logits, part_logits, top_n_prob, labels)
        lib = _lib.load()
        b, n, c = part.shape
        loss = torch.empty(5, dtype=torch.float32, device=raw.device)
        grads = [torch.empty_like(t) for t in (raw, cat, part, prob)]
        nws = lib.hk_nts_loss_ws_bytes(b, n, c)
        ws = _ws(nws, raw.device)
        check(lib.hk_nts_loss(ptr(raw), ptr(cat), ptr(part), ptr(prob), ptr(y), label_smoothing, ptr(loss), *[ptr(g) for g in grads],
                              b, n, c, ptr(ws), nws, stream()), 'hk_nts_loss')
        return _loss_forward(ctx, loss, grads)

    @staticmethod
    def backward(ctx, g, _g_parts):
        return _loss_backward(ctx, g, 2)


def nts_loss(raw_logits, concat_logits, part_logits, top_n_prob, labels, label_smoothing=0.1):
    """NTS-Net's loss on raw_logits, concat_logits [B,C], part_logits [B,N,C], top_n_prob [B,N], labels [B] -> the scalar
    raw CE + concat CE + part-class CE (label-smoothed means) + the ranking hinge over the proposals' scores gated by
    their unsmoothed part losses.  part_logits receives gradient from the part-class CE only (the gate has none),
    top_n_prob from the ranking term only."""
    return _NTSLoss.apply(raw_logits, concat_logits, part_logits, top_n_prob, labels, float(label_smoothing))[0]


def nts_loss_with_parts(raw_logits, concat_logits, part_logits, top_n_prob, labels, label_smoothing=0.1):
    """nts_loss plus the device tensor [raw CE, concat CE, part-class CE, rank] (not differentiable)."""
    return _NTSLoss.apply(raw_logits, concat_logits, part_logits, top_n_prob, labels, float(label_smoothing))


# --------------------------------------------------------------------- CrossX multi-excitation block, upsample + add, loss
ME_POOLS = {'max': 0, 'avg': 1}


def crossx_me_bwd(d_main, d_parts, d_pooled, argmax, dz, out, gates, main, parts, pool):
    """The raw backward of `crossx_me` (hk_crossx_me_bwd): d_main [N,C,H,W], d_parts [P,N,C,H,W], d_pooled [P,N,C] and
    dz [N,C] - the gradient that reaches the squeeze GAP(out) - may each be None, meaning zero -> (d_out, d_res, d_gates).
    No autograd."""
    lib = _lib.load()
    mode = ME_POOLS[pool]
    p, n, c, h, w = parts.shape
    out, main, parts, gates = _f32_shaped(out, (n, c, h, w), 'crossx_me_bwd', 'out'), _f32_shaped(main, (n, c, h, w), 'crossx_me_bwd', 'main'), \
        _f32c(parts), _f32_shaped(gates, (p, n, c), 'crossx_me_bwd', 'gates')
    d_main = None if d_main is None else _f32_shaped(d_main, (n, c, h, w), 'crossx_me_bwd', 'd_main')
    d_parts = None if d_parts is None else _f32_shaped(d_parts, (p, n, c, h, w), 'crossx_me_bwd', 'd_parts')
    d_pooled = None if d_pooled is None else _f32_shaped(d_pooled, (p, n, c), 'crossx_me_bwd', 'd_pooled')
    dz = None if dz is None else _f32_shaped(dz, (n, c), 'crossx_me_bwd', 'dz')
    d_out, d_res, d_gates = torch.empty_like(out), torch.empty_like(out), torch.empty_like(gates)
    check(lib.hk_crossx_me_bwd(ptr(d_main), ptr(d_parts), ptr(d_pooled), ptr(argmax), ptr(dz), ptr(out), ptr(gates), ptr(main), ptr(parts),
                               ptr(d_out), ptr(d_res), ptr(d_gates), p, n, c, h * w, mode, stream()), 'hk_crossx_me_bwd')
    return d_out, d_res, d_gates


class _CrossXME(torch.autograd.Function):
    """replaces the tail of Bottleneck.forward with MELayer's multiplies (model/methods/CrossX.py:62-70,109-119) and the
    adaptive pools of ResNet.forward (:225-226)."""

    @staticmethod
    def forward(ctx, out, res, gates, pool):
        lib = _lib.load()
        mode = ME_POOLS[pool]
        out = _f32c(out)
        if out.dim() != 4 or min(out.shape) < 1:
            raise _lib.HawkeyeHipError(f'crossx_me: out must be [N, C, H, W], got {tuple(out.shape)}')
        n, c, h, w = out.shape
        res = _f32_shaped(res, (n, c, h, w), 'crossx_me', 'res')
        if gates.dim() != 3 or tuple(gates.shape[1:]) != (n, c) or not 1 <= gates.shape[0] <= 3:
            raise _lib.HawkeyeHipError(f'crossx_me: gates must be [P, N, C] = [1..3, {n}, {c}], got {tuple(gates.shape)}')
        gates = _f32c(gates)
        p = gates.shape[0]
        main = torch.empty_like(out)
        parts = torch.empty(p, n, c, h, w, dtype=torch.float32, device=out.device)
        pooled = torch.empty(p, n, c, dtype=torch.float32, device=out.device)
        argmax = torch.empty(p, n, c, dtype=torch.int32, device=out.device) if mode == 0 else None
        check(lib.hk_crossx_me_fwd(ptr(out), ptr(res), ptr(gates), ptr(main), ptr(parts), ptr(pooled), ptr(argmax), p, n, c, h * w, mode,
                                   stream()), 'hk_crossx_me_fwd')
        ctx.pool = pool
        ctx.save_for_backward(out, gates, main, parts, argmax)
        ctx.set_materialize_grads(False)                   # an unused output costs no read of a map of zeros
        return main, parts, pooled

    @staticmethod
    def backward(ctx, d_main, d_parts, d_pooled):
        out, gates, main, parts, argmax = ctx.saved_tensors
        return crossx_me_bwd(d_main, d_parts, d_pooled, argmax, None, out, gates, main, parts, ctx.pool) + (None,)


def crossx_me(out, res, gates, pool):
    """The end of a multi-excitation bottleneck in one pass: out, res [N,C,H,W] (the block's bn3 output and its residual),
    gates [P,N,C] (after the sigmoid), pool 'max' or 'avg' -> main [N,C,H,W] = relu(out + res), parts [P,N,C,H,W] =
    relu(out * gates[p] + res), pooled [P,N,C] = each part's spatial max (ties: the lowest index) or mean.  The backward
    is one pass too; the pooled gradient is never a map."""
    if pool not in ME_POOLS:
        raise _lib.HawkeyeHipError(f"crossx_me: pool must be 'max' or 'avg', got {pool!r}")
    return _CrossXME.apply(out, res, gates, pool)


class _CrossXUpAdd(torch.autograd.Function):
    """replaces F.interpolate(b, 28) + torch.add, model/methods/CrossX.py:213-223."""

    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        a, b = _f32c(a), _f32c(b)
        n, c, ho, wo = a.shape
        hi, wi = b.shape[2:]
        y = torch.empty_like(a)
        check(lib.hk_crossx_up_add_fwd(ptr(a), ptr(b), ptr(y), n, c, hi, wi, ho, wo, stream()), 'hk_crossx_up_add_fwd')
        ctx.dims = (n, c, hi, wi, ho, wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        n, c, hi, wi, ho, wo = ctx.dims
        db = None
        if ctx.needs_input_grad[1]:
            g = _f32c(dy)
            db = torch.empty(n, c, hi, wi, dtype=torch.float32, device=dy.device)
            check(lib.hk_crossx_up_add_bwd(ptr(g), ptr(db), n, c, hi, wi, ho, wo, stream()), 'hk_crossx_up_add_bwd')
        return dy, db                                      # a's gradient is the incoming one itself


def crossx_up_add(a, b):
    """a [N,C,Ho,Wo] + nearest_upsample(b [N,C,Hi,Wi]) with Ho % Hi == 0 and Wo % Wi == 0; the upsampled map is never
    written."""
    if a.dim() != 4 or b.dim() != 4 or tuple(a.shape[:2]) != tuple(b.shape[:2]) or min(a.shape) < 1 or min(b.shape) < 1:
        raise _lib.HawkeyeHipError(f'crossx_up_add: two [N, C, H, W] maps of one N and C are needed, got {tuple(a.shape)} and {tuple(b.shape)}')
    if a.shape[2] % b.shape[2] or a.shape[3] % b.shape[3]:
        raise _lib.HawkeyeHipError(f'crossx_up_add: the size {tuple(a.shape[2:])} is no whole multiple of {tuple(b.shape[2:])}')
    _one_device('crossx_up_add', a.device, b)
    return _CrossXUpAdd.apply(a, b)


def _cx_features(feats, b, device, what, name):
    """A list of P tensors [B,C,1,1] / [B,C], or one [P,B,C] tensor -> [P,B,C] dense."""
    t = torch.stack([f.reshape(f.shape[0], -1) for f in feats]) if isinstance(feats, (list, tuple)) else feats
    if t.dim() != 3 or t.shape[1] != b or not 1 <= t.shape[0] <= 3 or t.shape[2] < 1:
        raise _lib.HawkeyeHipError(f'{what}: {name} must be 1 to 3 parts of [{b}, C] features, got {tuple(t.shape)}')
    _one_device(what, device, t)
    return t


class _CrossXLoss(torch.autograd.Function):
    """replaces CrossXLoss.__call__ and RegularLoss.forward, model/loss/CrossX_loss.py:13-64: six loss terms and all six
    gradients from one launch; backward only scales them."""

    @staticmethod
    def forward(ctx, ulti, plty, cmbn, f_ulti, f_plty, f_cmbn, labels, gamma):
        lib = _lib.load()
        ulti, plty, cmbn, f_ulti, f_plty, f_cmbn = (_f32c(t) for t in (ulti, plty, cmbn, f_ulti, f_plty, f_cmbn))
        b, k = ulti.shape
        p = f_ulti.shape[0]
        cs = [f.shape[2] for f in (f_ulti, f_plty, f_cmbn)]
        loss = torch.empty(6, dtype=torch.float32, device=ulti.device)
        grads = [torch.empty_like(t) for t in (ulti, plty, cmbn, f_ulti, f_plty, f_cmbn)]
        nws = lib.hk_crossx_loss_ws_bytes(b, k, p, *cs)
        ws = _ws(nws, ulti.device)
        check(lib.hk_crossx_loss(ptr(ulti), ptr(plty), ptr(cmbn), ptr(labels), ptr(f_ulti), ptr(f_plty), ptr(f_cmbn), gamma[0], gamma[1],
                                 gamma[2], 1.0, ptr(loss), *[ptr(g) for g in grads], b, k, p, *cs, ptr(ws), nws, stream()), 'hk_crossx_loss')
        return _loss_forward(ctx, loss, grads)

    @staticmethod
    def backward(ctx, g, _g_terms):
        return _loss_backward(ctx, g, 2)


def _crossx_loss_args(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, labels, gamma, what='crossx_loss'):
    if ulti.dim() != 2 or ulti.shape != plty.shape or ulti.shape != cmbn.shape:
        raise _lib.HawkeyeHipError(f'{what}: three [B, K] logit matrices of one shape are needed, got {tuple(ulti.shape)}, '
                                   f'{tuple(plty.shape)} and {tuple(cmbn.shape)}')
    b = ulti.shape[0]
    if b < 2:                                              # the reference's squeeze() drops the batch axis at B = 1 and fails
        raise _lib.HawkeyeHipError(f'{what}: the batch must hold at least 2 samples, got {b}')
    _one_device(what, ulti.device, plty, cmbn)
    feats = [_cx_features(f, b, ulti.device, what, n) for f, n in ((ulti_ftrs, 'ulti_ftrs'), (plty_ftrs, 'plty_ftrs'), (cmbn_ftrs, 'cmbn_ftrs'))]
    if len({f.shape[0] for f in feats}) != 1:
        raise _lib.HawkeyeHipError(f'{what}: the three feature lists hold {[f.shape[0] for f in feats]} parts')
    y = _int_tensor(labels, (b,), torch.int64, ulti.device, what, 'labels')
    gamma = tuple(float(v) for v in gamma)
    if len(gamma) != 3:
        raise _lib.HawkeyeHipError(f'{what}: gamma must hold three values (ulti, plty, cmbn), got {gamma}')
    return feats, y, gamma


def crossx_loss_with_terms(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, labels, gamma):
    """CrossX's loss on the three logit matrices [B,K], the three feature lists (P tensors [B,C,1,1] or [B,C] each, or one
    [P,B,C] tensor; the width may differ per list) and labels [B] -> (total, the device tensor [cls, kl, reg_ulti, reg_plty,
    reg_cmbn], not differentiable).  cls: the label-smoothed (0.1) cross entropy of the summed logits; kl: KL(softmax(ulti) |
    softmax(plty)) + KL(softmax(ulti) | softmax(cmbn)) over B, the target carrying gradient too; reg: gamma x the upper
    triangle of each list's part-correlation matrix."""
    feats, y, gamma = _crossx_loss_args(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, labels, gamma)
    return _CrossXLoss.apply(ulti, plty, cmbn, *feats, y, gamma)


def crossx_loss(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, labels, gamma):
    return crossx_loss_with_terms(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, labels, gamma)[0]


# --------------------------------------------------------------------- DCL head, loss and swap law
def _dcl_head_args(x, weight, bias, what):
    if x.dim() != 4 or min(x.shape) < 1:
        raise _lib.HawkeyeHipError(f'{what}: x must be [B, C, H, W], got {tuple(x.shape)}')
    b, c, h, w = x.shape
    if h < 2 or w < 2:                                     # the reference's AvgPool2d(2) has no output there and fails
        raise _lib.HawkeyeHipError(f'{what}: the map must be at least 2 x 2, got {h} x {w}')
    if weight.numel() != c:
        raise _lib.HawkeyeHipError(f'{what}: weight must hold {c} values ([1, {c}, 1, 1] or [{c}]), got {tuple(weight.shape)}')
    if bias.numel() != 1:
        raise _lib.HawkeyeHipError(f'{what}: bias must hold one value, got {tuple(bias.shape)}')
    _one_device(what, x.device, weight, bias)
    return _f32c(x), _f32c(weight).reshape(c), _f32c(bias).reshape(1)


def dcl_head_bwd(x, weight, mask, d_pooled, d_mask, need=(True, True, True)):
    """The raw backward of `dcl_head` (hk_dcl_head_bwd): x [B,C,H,W], weight [C], the saved mask [B,M]; d_pooled [B,C] and
    d_mask [B,M] may each be None, meaning zero -> (dx, dw [C], dbias [1]), None where `need` says so.  No autograd."""
    lib = _lib.load()
    x, weight, mask = _f32c(x), _f32c(weight).reshape(-1), _f32c(mask)
    b, c, h, w = x.shape
    m = (h // 2) * (w // 2)
    if tuple(mask.shape) != (b, m):
        raise _lib.HawkeyeHipError(f'dcl_head_bwd: mask must have the shape {(b, m)}, got {tuple(mask.shape)}')
    d_pooled = None if d_pooled is None else _f32_shaped(d_pooled, (b, c), 'dcl_head_bwd', 'd_pooled')
    d_mask = None if d_mask is None else _f32_shaped(d_mask, (b, m), 'dcl_head_bwd', 'd_mask')
    dx = torch.empty_like(x) if need[0] else None
    dw = torch.empty(c, dtype=torch.float32, device=x.device) if need[1] else None
    dbias = torch.empty(1, dtype=torch.float32, device=x.device) if need[2] else None
    nws = lib.hk_dcl_head_bwd_ws_bytes(b, c, h, w)
    ws = _ws(nws, x.device)
    check(lib.hk_dcl_head_bwd(ptr(x), ptr(weight), ptr(mask), ptr(d_pooled), ptr(d_mask), ptr(dx), ptr(dw), ptr(dbias), b, c, h, w, ptr(ws),
                              nws, stream()), 'hk_dcl_head_bwd')
    return dx, dw, dbias


class _DCLHead(torch.autograd.Function):
    """replaces Convmask, avgpool2, tanh, the view and avgpool of DCL.forward, model/methods/DCL.py:33-39."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        ctx.wshape, ctx.bshape = weight.shape, bias.shape
        x, weight, bias = _dcl_head_args(x, weight, bias, 'dcl_head')
        b, c, h, w = x.shape
        pooled = torch.empty(b, c, dtype=torch.float32, device=x.device)
        mask = torch.empty(b, (h // 2) * (w // 2), dtype=torch.float32, device=x.device)
        nws = lib.hk_dcl_head_fwd_ws_bytes(b, c, h, w)
        ws = _ws(nws, x.device)
        check(lib.hk_dcl_head_fwd(ptr(x), ptr(weight), ptr(bias), ptr(pooled), ptr(mask), b, c, h, w, ptr(ws), nws, stream()),
              'hk_dcl_head_fwd')
        ctx.save_for_backward(x, weight, mask)
        ctx.set_materialize_grads(False)                   # an unused output reaches the kernel as a null gradient
        return pooled, mask

    @staticmethod
    def backward(ctx, d_pooled, d_mask):
        x, weight, mask = ctx.saved_tensors
        dx, dw, dbias = dcl_head_bwd(x, weight, mask, d_pooled, d_mask, ctx.needs_input_grad)
        return dx, None if dw is None else dw.view(ctx.wshape), None if dbias is None else dbias.view(ctx.bshape)


def dcl_head(x, weight, bias):
    """DCL's two readers of the last map in one read: x [B,C,H,W], weight [1,C,1,1] or [C] and bias [1] (Convmask's) ->
    pooled [B,C] = the spatial mean, mask [B,(H/2)(W/2)] = tanh(avgpool2x2(sum_c weight[c] x[:,c] + bias)).  One autograd
    node; its backward reads x once and writes dx once."""
    return _DCLHead.apply(x, weight, bias)


class _DCLLoss(torch.autograd.Function):
    """replaces DCLLoss.__call__, model/loss/DCL_loss.py:16-21: the four loss terms and the three gradients from one
    launch; backward only scales them."""

    @staticmethod
    def forward(ctx, logits, swap_logits, mask, labels, labels_swap, law, coef, smoothing):
        lib = _lib.load()
        logits, swap_logits, mask = _f32c(logits), _f32c(swap_logits), _f32c(mask)
        n, k = logits.shape
        loss = torch.empty(4, dtype=torch.float32, device=logits.device)
        grads = [torch.empty_like(t) for t in (logits, swap_logits, mask)]
        check(lib.hk_dcl_loss(ptr(logits), ptr(swap_logits), ptr(mask), ptr(labels), ptr(labels_swap), ptr(law), coef[0], coef[1], coef[2],
                              smoothing, 1.0, ptr(loss), *[ptr(g) for g in grads], n, k, swap_logits.shape[1], mask.shape[1], stream()),
              'hk_dcl_loss')
        return _loss_forward(ctx, loss, grads)

    @staticmethod
    def backward(ctx, g, _g_terms):
        return _loss_backward(ctx, g, 5)


def _dcl_loss_args(logits, swap_logits, mask, labels, labels_swap, swap_law, alpha, beta, gamma, what='dcl_loss'):
    if logits.dim() != 2 or swap_logits.dim() != 2 or mask.dim() != 2 or min(logits.shape) < 1 or min(swap_logits.shape) < 1 or \
            min(mask.shape) < 1 or not logits.shape[0] == swap_logits.shape[0] == mask.shape[0]:
        raise _lib.HawkeyeHipError(f'{what}: logits [N, K], swap logits [N, S] and a mask [N, M] of one N are needed, got '
                                   f'{tuple(logits.shape)}, {tuple(swap_logits.shape)} and {tuple(mask.shape)}')
    n = logits.shape[0]
    dev = logits.device
    _one_device(what, dev, swap_logits, mask)
    y, ys = (_int_tensor(t, (n,), torch.int64, dev, what, name) for t, name in ((labels, 'labels'), (labels_swap, 'labels_swap')))
    if tuple(swap_law.shape) != tuple(mask.shape):
        raise _lib.HawkeyeHipError(f'{what}: swap_law must have the mask\'s shape {tuple(mask.shape)}, got {tuple(swap_law.shape)}')
    if not swap_law.is_floating_point():
        raise _lib.HawkeyeHipError(f'{what}: swap_law must be floating point; got {swap_law.dtype}')
    return y, ys, swap_law.to(device=dev, dtype=torch.float32).contiguous(), (float(alpha), float(beta), float(gamma))


def dcl_loss_with_terms(logits, swap_logits, mask, labels, labels_swap, swap_law, alpha=1.0, beta=1.0, gamma=1.0, label_smoothing=0.1):
    """DCL's loss on the class logits [N,K], the swap logits [N,S], the mask [N,M], labels and labels_swap [N] and the swap
    law [N,M] -> (total, the device tensor [ce, swap, law], not differentiable).  ce, swap: label-smoothed cross entropies;
    law: mean |mask - swap_law| (its gradient exactly 0 where they are equal); total = alpha ce + beta swap + gamma law."""
    y, ys, law, coef = _dcl_loss_args(logits, swap_logits, mask, labels, labels_swap, swap_law, alpha, beta, gamma)
    return _DCLLoss.apply(logits, swap_logits, mask, y, ys, law, coef, float(label_smoothing))


def dcl_loss(logits, swap_logits, mask, labels, labels_swap, swap_law, alpha=1.0, beta=1.0, gamma=1.0, label_smoothing=0.1):
    return dcl_loss_with_terms(logits, swap_logits, mask, labels, labels_swap, swap_law, alpha, beta, gamma, label_smoothing)[0]


_DCL_BOUNDS = {}


def _dcl_bounds(h, w, gx, gy, device):
    from .transforms import patch_bounds                   # the reference's crop_image bounds, in Python floats
    key = (h, w, gx, gy, str(device))
    if key not in _DCL_BOUNDS:                             # made once per shape; the upload is the only copy
        _DCL_BOUNDS[key] = tuple(torch.tensor(patch_bounds(s, g), dtype=torch.int32).to(device) for s, g in ((w, gx), (h, gy)))
    return _DCL_BOUNDS[key]


def dcl_swap_law(u8_unswap, u8_swap, grid=(7, 7)):
    """The swap law of DCL's data pipeline on the device: two uint8 batches [N,H,W,3] (an image and its patch-shuffled
    version) and grid = (columns, rows) -> (law float32 [N, columns rows], index int32 of the same shape).  For each patch
    of the swapped image (row-major) `index` names the patch of the unswapped image with the nearest sum of band means -
    every decision as the reference takes it in float64, the lowest index on ties - and law = (index - P // 2) / P.  No
    gradient."""
    lib = _lib.load()
    gx, gy = (int(g) for g in grid)
    for name, t in (('u8_unswap', u8_unswap), ('u8_swap', u8_swap)):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or min(t.shape) < 1:
            raise _lib.HawkeyeHipError(f'dcl_swap_law: {name} must be uint8 [N, H, W, 3], got {t.dtype} {tuple(t.shape)}')
    if u8_unswap.shape != u8_swap.shape:
        raise _lib.HawkeyeHipError(f'dcl_swap_law: two batches of one shape are needed, got {tuple(u8_unswap.shape)} and {tuple(u8_swap.shape)}')
    _one_device('dcl_swap_law', u8_unswap.device, u8_swap)
    n, h, w, _ = u8_unswap.shape
    if gx < 1 or gy < 1:
        raise _lib.HawkeyeHipError(f'dcl_swap_law: grid must hold two positive counts, got {grid}')
    if w < gx or h < gy:                                   # the reference divides by the pixel count of an empty patch
        raise _lib.HawkeyeHipError(f'dcl_swap_law: a {h} x {w} image has no {gy} x {gx} patches: a patch would be empty')
    a, s = u8_unswap.contiguous(), u8_swap.contiguous()
    bx, by = _dcl_bounds(h, w, gx, gy, a.device)
    index = torch.empty(n, gx * gy, dtype=torch.int32, device=a.device)
    law = torch.empty(n, gx * gy, dtype=torch.float32, device=a.device)
    check(lib.hk_dcl_swap_law(ptr(a), ptr(s), ptr(bx), ptr(by), ptr(index), ptr(law), n, h, w, gx, gy, stream()), 'hk_dcl_swap_law')
    return law, index


# --------------------------------------------------------------------- InterpParts: region grouping and shaping loss
IP_MAX_PARTS, IP_MAX_CHANNELS = 32, 1024


def _ip_group_args(x, weight, smooth_factor, what):
    if x.dim() != 4 or min(x.shape) < 1:
        raise _lib.HawkeyeHipError(f'{what}: x must be [N, C, H, W], got {tuple(x.shape)}')
    c = x.shape[1]
    if weight.dim() not in (2, 4) or weight.shape[1] != c or weight.numel() != weight.shape[0] * c:
        raise _lib.HawkeyeHipError(f'{what}: weight must be [K, {c}, 1, 1] or [K, {c}], got {tuple(weight.shape)}')
    k = weight.shape[0]
    if smooth_factor.numel() != k:
        raise _lib.HawkeyeHipError(f'{what}: smooth_factor must hold {k} values, got {tuple(smooth_factor.shape)}')
    if not 1 <= k <= IP_MAX_PARTS:
        raise _lib.HawkeyeHipError(f'{what}: 1 to {IP_MAX_PARTS} parts are served, got {k}')
    if c % 64 or c > IP_MAX_CHANNELS:
        raise _lib.HawkeyeHipError(f'{what}: the channel count must be a multiple of 64 up to {IP_MAX_CHANNELS} (the tile is held in LDS), got {c}')
    _one_device(what, x.device, weight, smooth_factor)
    return _f32c(x), _f32c(weight).reshape(k, c), _f32c(smooth_factor).reshape(k)


def ip_group_bwd(x, weight, smooth_factor, outputs_t, s, nrm, d_outputs_t, d_assign, need=(True, True, True)):
    """The raw backward of `ip_group` (hk_ip_group_bwd): x [N,C,H,W], weight [K,C], smooth_factor [K], the forward's outputs_t
    [N,C,K], s and nrm [N,K]; d_outputs_t [N,C,K] and d_assign [N,K,H,W] may each be None, meaning zeros ->
    (dx, d_weight [K,C], d_smooth_factor [K]), None where `need` says so.  No autograd."""
    lib = _lib.load()
    x, weight, smooth_factor = _ip_group_args(x, weight, smooth_factor, 'ip_group_bwd')
    n, c, h, w = x.shape
    k = weight.shape[0]
    outputs_t, s, nrm = (_f32_shaped(t, shape, 'ip_group_bwd', name) for t, shape, name in
                         ((outputs_t, (n, c, k), 'outputs_t'), (s, (n, k), 's'), (nrm, (n, k), 'nrm')))
    d_outputs_t = None if d_outputs_t is None else _f32_shaped(d_outputs_t, (n, c, k), 'ip_group_bwd', 'd_outputs_t')
    d_assign = None if d_assign is None else _f32_shaped(d_assign, (n, k, h, w), 'ip_group_bwd', 'd_assign')
    dx = torch.empty_like(x) if need[0] else None
    dwt = torch.empty(k, c, dtype=torch.float32, device=x.device) if need[1] else None
    dsm = torch.empty(k, dtype=torch.float32, device=x.device) if need[2] else None
    nws = lib.hk_ip_group_bwd_ws_bytes(n, c, k, h, w)
    ws = _ws(nws, x.device)
    check(lib.hk_ip_group_bwd(ptr(x), ptr(weight), ptr(smooth_factor), ptr(outputs_t), ptr(s), ptr(nrm), ptr(d_outputs_t), ptr(d_assign),
                              ptr(dx), ptr(dwt), ptr(dsm), n, c, k, h, w, ptr(ws), nws, stream()), 'hk_ip_group_bwd')
    return dx, dwt, dsm


class _IPGroup(torch.autograd.Function):
    """replaces GroupingUnit.forward, model/methods/Interp_Parts.py:56-122."""

    @staticmethod
    def forward(ctx, x, weight, smooth_factor):
        lib = _lib.load()
        ctx.wshape, ctx.sshape = weight.shape, smooth_factor.shape
        x, weight, smooth_factor = _ip_group_args(x, weight, smooth_factor, 'ip_group')
        n, c, h, w = x.shape
        k = weight.shape[0]
        outputs_t = torch.empty(n, c, k, dtype=torch.float32, device=x.device)
        assign = torch.empty(n, k, h, w, dtype=torch.float32, device=x.device)
        s, nrm = (torch.empty(n, k, dtype=torch.float32, device=x.device) for _ in range(2))
        nws = lib.hk_ip_group_fwd_ws_bytes(n, c, k, h, w)
        ws = _ws(nws, x.device)
        check(lib.hk_ip_group_fwd(ptr(x), ptr(weight), ptr(smooth_factor), ptr(outputs_t), ptr(assign), ptr(s), ptr(nrm), n, c, k, h, w,
                                  ptr(ws), nws, stream()), 'hk_ip_group_fwd')
        ctx.save_for_backward(x, weight, smooth_factor, outputs_t, s, nrm)
        ctx.set_materialize_grads(False)                   # an unused output reaches the kernel as a null gradient
        return outputs_t, assign

    @staticmethod
    def backward(ctx, d_outputs_t, d_assign):
        dx, dwt, dsm = ip_group_bwd(*ctx.saved_tensors, d_outputs_t, d_assign, ctx.needs_input_grad)
        return dx, None if dwt is None else dwt.view(ctx.wshape), None if dsm is None else dsm.view(ctx.sshape)


def ip_group(x, weight, smooth_factor):
    """InterpParts' grouping unit in one read of the map: x [N,C,H,W], weight [K,C,1,1] or [K,C] (the part centres) and
    smooth_factor [K] (before the sigmoid) -> (outputs_t [N,C,K], assign [N,K,H,W]) as GroupingUnit.forward returns them:
    assign = softmax_k(min(0, 2 <c_k, x_p> - |x_p|^2 - |c_k|^2) / beta_k), outputs_t the normalised residual coding of the
    assignment-weighted features, transposed.  1 <= K <= 32, C a multiple of 64 up to 1024.  One autograd node; its backward
    reads x once and writes dx once; gradients come back in the parameters' own shapes."""
    return _IPGroup.apply(x, weight, smooth_factor)


_IP_CACHE = {}


def ip_gaussian_window(radius, std):
    """The reference's GaussianKernel(radius, std) as a float32 tensor [(2 radius + 1), (2 radius + 1)], bit-equal to it:
    np.exp per element in float64, stored to float32, then normalised by the float32 sum.  radius 0: [[1.]]."""
    radius = int(radius)
    if radius < 0:
        raise _lib.HawkeyeHipError(f'ip_gaussian_window: radius must not be negative, got {radius}')
    size = 2 * radius + 1
    weight = torch.ones(size, size)
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            weight[i + radius][j + radius] = np.exp(-((i * i) + (j * j)) / (2 * std * std))
    return weight / weight.sum()


def ip_beta_prior(batch_size, alpha, beta, device=None):
    """The reference's update_prior_dist: the inverse CDF of Beta(alpha, beta) at the grid points (2 i + 1) / (2 N) - formed in
    float32 as the reference does, the inverse taken in float64, rounded to float32 -> [N] on `device`.  alpha == 1:
    1 - (1 - p)^(1 / beta); beta == 1: p^(1 / alpha); anything else needs scipy.  It depends on the arguments alone: made once
    per (N, alpha, beta, device) and kept."""
    n = int(batch_size)
    if n < 1 or not alpha > 0 or not beta > 0:
        raise _lib.HawkeyeHipError(f'ip_beta_prior: a positive batch size, alpha and beta are needed, got {batch_size}, {alpha}, {beta}')
    key = ('prior', n, float(alpha), float(beta), str(device))
    if key not in _IP_CACHE:
        grid = (torch.arange(1., 2 * n, 2.).float() / (2 * n)).numpy().astype(np.float64)
        if float(alpha) == 1.0:
            icdf = 1.0 - np.power(1.0 - grid, 1.0 / float(beta))
        elif float(beta) == 1.0:
            icdf = np.power(grid, 1.0 / float(alpha))
        else:
            try:
                from scipy import stats
            except ImportError as e:
                raise _lib.HawkeyeHipError(f'ip_beta_prior: Beta({alpha}, {beta}) has no closed-form inverse CDF here (alpha == 1 or '
                                           f'beta == 1 have): scipy is needed and is not installed') from e
            icdf = stats.beta.ppf(grid, a=alpha, b=beta)
        _IP_CACHE[key] = torch.tensor(icdf).float().to(device) if device is not None else torch.tensor(icdf).float()
    return _IP_CACHE[key]


def _ip_window_on(radius, std, device):
    key = ('window', int(radius), float(std), str(device))
    if key not in _IP_CACHE:
        _IP_CACHE[key] = ip_gaussian_window(radius, std).reshape(-1).to(device)
    return _IP_CACHE[key]


class _IPLoss(torch.autograd.Function):
    """replaces InterpPartsLoss.__call__ and ShapingLoss, model/loss/InterpParts_loss.py:24-138: the three terms and both
    gradients from two launches; backward only scales them."""

    @staticmethod
    def forward(ctx, logits, assign, labels, window, prior, coeff, radius):
        lib = _lib.load()
        logits, assign = _f32c(logits), _f32c(assign)
        n, classes = logits.shape
        _, k, h, w = assign.shape
        loss = torch.empty(3, dtype=torch.float32, device=logits.device)
        grads = [torch.empty_like(t) for t in (logits, assign)]
        nws = lib.hk_ip_loss_ws_bytes(n, k)
        ws = _ws(nws, logits.device)
        check(lib.hk_ip_loss(ptr(logits), ptr(labels), ptr(assign), ptr(window), ptr(prior), coeff, ptr(loss), ptr(grads[0]), ptr(grads[1]),
                             n, classes, k, h, w, radius, ptr(ws), nws, stream()), 'hk_ip_loss')
        return _loss_forward(ctx, loss, grads)

    @staticmethod
    def backward(ctx, g, _g_terms):
        return _loss_backward(ctx, g, 5)


def ip_loss_with_terms(logits, assign, labels, radius=2, std=0.4, alpha=1.0, beta=0.001, coeff=0.5, window=None, prior=None):
    """InterpParts' criterion on the logits [N,classes], the assignment maps [N,K,H,W] and labels [N] -> (total, the device
    tensor [cross entropy, shaping], not differentiable).  shaping: each map blurred with the Gaussian window ("valid"), its
    maximum, the N maxima of a part sorted and compared in log space with the Beta(alpha, beta) prior's inverse CDF; total =
    cross entropy + coeff shaping.  The gradient reaches `assign` at the window around each argmax only.  Ties: the lowest
    flat index, the lower sample first.  No host synchronisation: the window and the prior are made once per configuration
    (`window` [(2 radius + 1)^2] and `prior` [N] on the device override them)."""
    what = 'ip_loss'
    if logits.dim() != 2 or assign.dim() != 4 or min(logits.shape) < 1 or min(assign.shape) < 1 or logits.shape[0] != assign.shape[0]:
        raise _lib.HawkeyeHipError(f'{what}: logits [N, classes] and assign [N, K, H, W] of one N are needed, got {tuple(logits.shape)} and '
                                   f'{tuple(assign.shape)}')
    n, dev, radius = logits.shape[0], logits.device, int(radius)
    _one_device(what, dev, assign)
    size = 2 * radius + 1
    if radius < 0 or assign.shape[2] < size or assign.shape[3] < size:                       # the reference's conv2d raises there
        raise _lib.HawkeyeHipError(f'{what}: a {assign.shape[2]} x {assign.shape[3]} map is smaller than the {size} x {size} window')
    y = _int_tensor(labels, (n,), torch.int64, dev, what, 'labels')
    window = _ip_window_on(radius, std, dev) if window is None else _f32_shaped(window.reshape(-1), (size * size,), what, 'window')
    prior = ip_beta_prior(n, alpha, beta, dev) if prior is None else _f32_shaped(prior, (n,), what, 'prior')
    _one_device(what, dev, window, prior)
    return _IPLoss.apply(logits, assign, y, window, prior, float(coeff), radius)


def ip_loss(logits, assign, labels, radius=2, std=0.4, alpha=1.0, beta=0.001, coeff=0.5, window=None, prior=None):
    return ip_loss_with_terms(logits, assign, labels, radius, std, alpha, beta, coeff, window, prior)[0]


# --------------------------------------------------------------------- MGE-CNN part pool, Grad-CAM box, loss
MGE_MAX_LOGITS = 16


def _mge_partpool_args(x, weight, bias, what):
    if x.dim() != 4 or min(x.shape) < 1:
        raise _lib.HawkeyeHipError(f'{what}: x must be [B, Cin, H, W], got {tuple(x.shape)}')
    cin = x.shape[1]
    if cin % 32:
        raise _lib.HawkeyeHipError(f'{what}: Cin must be a multiple of 32, got {cin}')
    if weight.dim() not in (2, 4) or weight.shape[0] < 1 or weight.numel() != weight.shape[0] * cin:
        raise _lib.HawkeyeHipError(f'{what}: weight must be [Cout, {cin}] or [Cout, {cin}, 1, 1], got {tuple(weight.shape)}')
    cout = weight.shape[0]
    if tuple(bias.shape) != (cout,):
        raise _lib.HawkeyeHipError(f'{what}: bias must hold {cout} values, got {tuple(bias.shape)}')
    _one_device(what, x.device, weight, bias)
    return _f32c(x), _f32c(weight).reshape(cout, cin), _f32c(bias)


def mge_partpool_fwd(x, weight, bias):
    """The raw forward (hk_mge_partpool_fwd): -> (pooled [B,Cout], argmax int32 [B,Cout]).  No autograd."""
    x, weight, bias = _mge_partpool_args(x.detach(), weight.detach(), bias.detach(), 'mge_partpool')
    lib = _lib.load()
    b, cin, h, w = x.shape
    cout = weight.shape[0]
    pooled = torch.empty(b, cout, dtype=torch.float32, device=x.device)
    argmax = torch.empty(b, cout, dtype=torch.int32, device=x.device)
    nws = lib.hk_mge_partpool_fwd_ws_bytes(b, cin, cout, h, w)
    ws = _ws(nws, x.device)
    check(lib.hk_mge_partpool_fwd(ptr(x), ptr(weight), ptr(bias), ptr(pooled), ptr(argmax), b, cin, cout, h, w, ptr(ws), nws, stream()),
          'hk_mge_partpool_fwd')
    return pooled, argmax


def mge_partpool_bwd(x, g, pooled, argmax, need=(True, True)):
    """The raw backward (hk_mge_partpool_bwd): x [B,Cin,H,W], g and pooled [B,Cout], argmax int32 [B,Cout] -> (dw [Cout,Cin],
    db [Cout]), None where `need` says so.  No autograd."""
    lib = _lib.load()
    x = _f32c(x)
    b, cin, h, w = x.shape
    cout = pooled.shape[1]
    g, pooled = _f32_shaped(g, (b, cout), 'mge_partpool_bwd', 'g'), _f32_shaped(pooled, (b, cout), 'mge_partpool_bwd', 'pooled')
    argmax = _int_tensor(argmax, (b, cout), torch.int32, x.device, 'mge_partpool_bwd', 'argmax', same_device=True)
    dw = torch.empty(cout, cin, dtype=torch.float32, device=x.device) if need[0] else None
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if need[1] else None
    check(lib.hk_mge_partpool_bwd(ptr(x), ptr(g), ptr(pooled), ptr(argmax), ptr(dw), ptr(db), b, cin, cout, h, w, stream()),
          'hk_mge_partpool_bwd')
    return dw, db


class _MGEPartPool(torch.autograd.Function):
    """replaces pool_max(relu(conv6(x.detach()))) of LocalCamNet.forward, model/methods/MGE_CNN/MGE.py:135,166,197."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.wshape = weight.shape
        pooled, argmax = mge_partpool_fwd(x, weight, bias)
        ctx.save_for_backward(x, pooled, argmax)
        ctx.mark_non_differentiable(argmax)
        return pooled, argmax

    @staticmethod
    def backward(ctx, g, _g_argmax):
        x, pooled, argmax = ctx.saved_tensors
        dw, db = mge_partpool_bwd(x, g, pooled, argmax, ctx.needs_input_grad[1:])
        return None, None if dw is None else dw.view(ctx.wshape), db


def mge_partpool(x, weight, bias):
    """MGE-CNN's part pool: x [B,Cin,H,W] (no gradient reaches it: the reference detaches it), weight [Cout,Cin] or
    [Cout,Cin,1,1] and bias [Cout] of a Conv2d(Cin, Cout, 1, 1, padding=1) -> [B,Cout] = the global maximum of relu(conv(x)) over
    the padded (H + 2) x (W + 2) map, which is never written.  One autograd node; its backward is a gather of one pixel per
    (image, channel).  Cin a multiple of 32."""
    return _MGEPartPool.apply(x, weight, bias)[0]


def mge_cam_weights(cls_weight, index, hw):
    """The Grad-CAM channel weights in closed form: relu(W[index]) / hw [B,C] - what the reference's autograd run through the last
    block, AdaptiveAvgPool2d(1) and the classifier returns (grad_cam.py:82-86).  Plain torch ops; hk_mge_cam_bbox does the same inside."""
    return torch.relu(cls_weight.detach()[index.long()]) / float(hw)


def mge_cam_bbox(conv5, cls_weight, index, rate, image_size):
    """conv5 [B,C,h,w], cls_weight [classes,C], index integer [B] on the device -> boxes int32 [B,1,4] = y0, x0, y1, x1 (exclusive
    ends) of the region whose normalised, bilinearly upsampled (align_corners) class activation map is >= rate, as get_bbox
    (MGE.py:48-72) slices it; the whole image 0, 0, S, S where that slice is empty, the map is constant or `index` is out of
    range.  No autograd, no host round trip; feed the boxes to nts_crop_resize(images, boxes, 0, S)."""
    what = 'mge_cam_bbox'
    if conv5.dim() != 4 or min(conv5.shape) < 1:
        raise _lib.HawkeyeHipError(f'{what}: conv5 must be [B, C, h, w], got {tuple(conv5.shape)}')
    conv5 = _f32c(conv5.detach())
    b, c, h, w = conv5.shape
    if cls_weight.dim() != 2 or cls_weight.shape[1] != c or cls_weight.shape[0] < 1:
        raise _lib.HawkeyeHipError(f'{what}: cls_weight must be [classes, {c}], got {tuple(cls_weight.shape)}')
    _one_device(what, conv5.device, cls_weight)
    cls_weight = _f32c(cls_weight.detach())
    index = _int_tensor(index, (b,), torch.int32, conv5.device, what, 'index', same_device=True)
    s = int(image_size)
    if h * w > 512 or not 1 <= s <= 2048:
        raise _lib.HawkeyeHipError(f'{what}: a map of at most 512 pixels and an image side of 1 .. 2048 are served, got {h} x {w} and {s}')
    lib = _lib.load()
    boxes = torch.empty(b, 1, 4, dtype=torch.int32, device=conv5.device)
    check(lib.hk_mge_cam_bbox(ptr(conv5), ptr(cls_weight), ptr(index), ptr(boxes), b, c, h, w, cls_weight.shape[0], float(rate), s,
                              stream()), 'hk_mge_cam_bbox')
    return boxes


class _MGELoss(torch.autograd.Function):
    """replaces the ten criterion calls and their mean, Examples/MGE_CNN.py:43-45: the mean, the K terms and the K gradients of
    the mean from one launch; backward only scales them."""

    @staticmethod
    def forward(ctx, labels, label_smoothing, *logits):
        import ctypes
        lib = _lib.load()
        k = len(logits)
        b, c = logits[0].shape
        grads = [torch.empty_like(t) for t in logits]
        loss = torch.empty(1 + k, dtype=torch.float32, device=logits[0].device)
        table = ctypes.c_void_p * k
        nws = lib.hk_mge_loss_ws_bytes(k, b)
        ws = _ws(nws, logits[0].device)
        check(lib.hk_mge_loss(table(*[ptr(t).value for t in logits]), ptr(labels), label_smoothing, ptr(loss),
                              table(*[ptr(t).value for t in grads]), k, b, c, ptr(ws), nws, stream()), 'hk_mge_loss')
        return _loss_forward(ctx, loss, grads)

    @staticmethod
    def backward(ctx, g, _g_terms):
        return (None, None) + _loss_backward(ctx, g, 0)


def mge_loss_with_terms(logits, labels, label_smoothing=0.1):
    """MGE-CNN's criterion on a list of K <= 16 logits tensors [B,C] (the model's ten) and labels [B] -> (the mean of the K
    label-smoothed cross entropies, the device tensor of the K terms, not differentiable).  One launch for the loss and every
    gradient; the reference calls CrossEntropyLoss once per tensor."""
    what = 'mge_loss'
    logits = list(logits)
    if not 1 <= len(logits) <= MGE_MAX_LOGITS:
        raise _lib.HawkeyeHipError(f'{what}: 1 .. {MGE_MAX_LOGITS} logits tensors are served, got {len(logits)}')
    if logits[0].dim() != 2 or min(logits[0].shape) < 1 or any(t.shape != logits[0].shape for t in logits):
        raise _lib.HawkeyeHipError(f'{what}: every logits tensor must be [B, C] of one shape, got {[tuple(t.shape) for t in logits]}')
    _one_device(what, logits[0].device, *logits)
    y = _int_tensor(labels, (logits[0].shape[0],), torch.int32, logits[0].device, what, 'labels')
    return _MGELoss.apply(y, float(label_smoothing), *[_f32c(t) for t in logits])


def mge_loss(logits, labels, label_smoothing=0.1):
    return mge_loss_with_terms(logits, labels, label_smoothing)[0]


# --------------------------------------------------------------------- classifier
class _Linear(torch.autograd.Function):
    """replaces nn.Linear on the pooled vector (model/methods/BCNN.py:42,54 and the other heads' classifiers)."""

    @staticmethod
    def forward(ctx, y, weight, bias):
        lib = _lib.load()
        y, weight = _f32c(y), _f32c(weight)
        b, j = y.shape
        k = weight.shape[0]
        if weight.shape[1] != j:
            raise _lib.HawkeyeHipError(f'linear: weight {tuple(weight.shape)} does not match input {tuple(y.shape)}')
        bias_c = _f32c(bias) if bias is not None else None
        out = torch.empty(b, k, dtype=torch.float32, device=y.device)
        nws = lib.hk_linear_ws_bytes(b, j, k)
        ws = _ws(nws, y.device)
        check(lib.hk_linear_fwd(ptr(y), ptr(weight), ptr(bias_c), ptr(out), b, j, k, ptr(ws), nws, stream()),
              'hk_linear_fwd')
        ctx.save_for_backward(y, weight)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        y, weight = ctx.saved_tensors
        g = _f32c(g)
        b, j = y.shape
        k = weight.shape[0]
        dy = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        db = torch.empty(k, dtype=torch.float32, device=y.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        check(lib.hk_linear_bwd(ptr(y), ptr(weight), ptr(g), ptr(dy), ptr(dw), ptr(db), b, j, k, stream()),
              'hk_linear_bwd')
        return dy, dw, db


class _SsqrtPoolLinear(torch.autograd.Function):
    """Signed-sqrt bilinear pooling (the reference's commented alternative, BCNN.py:23-24) + the classifier on it with the
    l2 scale folded into the classifier: the pooled vector is handed over as u = sign(G) sqrt(|G| + 1e-10),
    unnormalised - the scale pass over B x C^2 floats is not launched - and logits = inv_norm[b] (u W^T) + bias."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        x, weight = _f32c(x), _f32c(weight)
        b, c, h, w = x.shape
        hw, j, k = h * w, c * c, weight.shape[0]
        if weight.shape[1] != j:
            raise _lib.HawkeyeHipError(f'ssqrt_pool_linear: weight {tuple(weight.shape)} does not match {c} x {c} pooled features')
        u = torch.empty(b, j, dtype=torch.float32, device=x.device)
        inv_norm = torch.empty(b, dtype=torch.float32, device=x.device)
        nws = lib.hk_bcnn_ssqrt_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        # the kernels write the PRE-BIAS product `pre` = inv_norm (u W^T); it stays private to this node (the backward's
        # <y, dy> = sum_k g_k pre_k needs it exact, whatever the bias is and whatever the caller does to the logits in place)
        pre = torch.empty(b, k, dtype=torch.float32, device=x.device)
        nwl = lib.hk_linear_ws_bytes(b, j, k)
        wsl = _ws(nwl, x.device)
        # two launches + the classifier's reduce: the Gram kernel leaves partial sums of u^2 and the reduce launch forms 1 / |u|
        import ctypes
        nparts = ctypes.c_int(0)
        rc = lib.hk_bcnn_ssqrt_pool_fwd_parts(ptr(x), ptr(u), ptr(ws), ctypes.byref(nparts), b, c, hw, stream())
        if rc == _lib.HK_OK:
            check(lib.hk_linear_fwd_ssq(ptr(u), ptr(weight), None, ptr(ws), nparts.value, ptr(inv_norm), ptr(pre), b, j, k,
                                        ptr(wsl), nwl, stream()), 'hk_linear_fwd_ssq')
        else:
            if rc != _lib.HK_ERR_UNSUPPORTED:
                check(rc, 'hk_bcnn_ssqrt_pool_fwd_parts')
            check(lib.hk_bcnn_ssqrt_pool_fwd_unscaled(ptr(x), ptr(u), ptr(inv_norm), b, c, hw, ptr(ws), nws, stream()),
                  'hk_bcnn_ssqrt_pool_fwd_unscaled')
            check(lib.hk_linear_fwd_scaled(ptr(u), ptr(weight), None, ptr(inv_norm), ptr(pre), b, j, k, ptr(wsl), nwl,
                                           stream()), 'hk_linear_fwd_scaled')
        ctx.save_for_backward(x, u, inv_norm, weight, pre)
        ctx.has_bias = bias is not None
        return pre + _f32c(bias) if bias is not None else pre.clone()

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, u, inv_norm, weight, pre = ctx.saved_tensors
        g = _f32c(g)
        b, c, h, w = x.shape
        hw, j, k = h * w, c * c, weight.shape[0]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy = torch.empty_like(u) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(k, dtype=torch.float32, device=x.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        rc = lib.hk_linear_bwd_scaled(ptr(u), ptr(weight), ptr(g), ptr(inv_norm), ptr(dy), ptr(dw), ptr(db), b, j, k, stream())
        if rc == _lib.HK_ERR_UNSUPPORTED:      # shapes the one-launch kernel does not serve: dW from the scaled g explicitly
            gs = g * inv_norm[:, None]
            check(lib.hk_linear_bwd(ptr(u), ptr(weight), ptr(g), ptr(dy), None, ptr(db), b, j, k, stream()), 'hk_linear_bwd')
            if need_w:
                check(lib.hk_linear_bwd(ptr(u), ptr(weight), ptr(gs), None, ptr(dw), None, b, j, k, stream()), 'hk_linear_bwd')
        else:
            check(rc, 'hk_linear_bwd_scaled')
        dx = None
        if need_x:
            dx = torch.empty_like(x)
            nws = lib.hk_bcnn_ssqrt_ws_bytes(b, c, hw)
            ws = _ws(nws, x.device)
            # <y, dy> = sum_k g_k pre_k (the pre-bias product): the classifier's operands instead of a pass over u and dy
            check(lib.hk_bcnn_ssqrt_pool_bwd_tdot(ptr(x), ptr(u), ptr(dy), ptr(inv_norm), ptr(g), ptr(pre), None, k, 1, ptr(dx),
                                                  b, c, hw, ptr(ws), nws, stream()), 'hk_bcnn_ssqrt_pool_bwd_tdot')
        return dx, dw, db


class _BilinearPoolLinear(torch.autograd.Function):
    """BilinearPooling + the classifier on it (model/methods/BCNN.py:13-27 + :54) as ONE autograd node.  Forward: the two
    entry points back to back (the l2 scale is already free in the Gram epilogue: nothing to fold).  Backward: because
    dy = g W is produced here, the inner product <y, dy> that F.normalize's backward needs is known in closed form,
        t[b] = sum_j y[b,j] sum_k g[b,k] W[k,j] = sum_k g[b,k] (y W^T)[b,k]      (the pre-bias product, kept by this node),
    so hk_bcnn_pool_bwd_tdot runs the Gram backward as one launch with the rank-1 term applied while dX is written -
    no partial sums of y * dy, no second pass over dX."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        x, weight = _f32c(x), _f32c(weight)
        b, c, h, w = x.shape
        hw, j, k = h * w, c * c, weight.shape[0]
        if weight.shape[1] != j:
            raise _lib.HawkeyeHipError(f'bilinear_pool_linear: weight {tuple(weight.shape)} does not match {c} x {c} pooled features')
        y = torch.empty(b, j, dtype=torch.float32, device=x.device)
        inv_norm = torch.empty(b, dtype=torch.float32, device=x.device)
        colsum = torch.empty(b, hw, dtype=torch.float32, device=x.device)
        nws = lib.hk_bcnn_pool_ws_bytes(b, c, hw)
        ws = _ws(nws, x.device)
        check(lib.hk_bcnn_pool_fwd(ptr(x), ptr(y), ptr(inv_norm), ptr(colsum), b, c, hw, ptr(ws), nws, stream()),
              'hk_bcnn_pool_fwd')
        # the kernel writes the PRE-BIAS product y W^T, which stays private to this node: the backward's closed form
        # t = sum_k g_k (y W^T)_k then neither cancels against a large bias nor breaks when the caller modifies the logits in
        # place (nn.Linear does not save its output either); the bias is added by one [B,K] elementwise op - the same bits
        # as the kernel's own `sum + bias`
        pre = torch.empty(b, k, dtype=torch.float32, device=x.device)
        nwl = lib.hk_linear_ws_bytes(b, j, k)
        wsl = _ws(nwl, x.device)
        check(lib.hk_linear_fwd(ptr(y), ptr(weight), None, ptr(pre), b, j, k, ptr(wsl), nwl, stream()), 'hk_linear_fwd')
        ctx.save_for_backward(x, y, inv_norm, colsum, weight, pre)
        ctx.has_bias = bias is not None
        return pre + _f32c(bias) if bias is not None else pre.clone()

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, y, inv_norm, colsum, weight, pre = ctx.saved_tensors
        g = _f32c(g)
        b, c, h, w = x.shape
        hw, j, k = h * w, c * c, weight.shape[0]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy = torch.empty_like(y) if need_x else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(k, dtype=torch.float32, device=x.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if dy is not None or dw is not None or db is not None:
            check(lib.hk_linear_bwd(ptr(y), ptr(weight), ptr(g), ptr(dy), ptr(dw), ptr(db), b, j, k, stream()), 'hk_linear_bwd')
        dx = None
        if need_x:
            dx = torch.empty_like(x)
            nws = lib.hk_bcnn_pool_ws_bytes(b, c, hw)
            ws = _ws(nws, x.device)
            check(lib.hk_bcnn_pool_bwd_tdot(ptr(x), ptr(y), ptr(dy), ptr(inv_norm), ptr(colsum), ptr(g), ptr(pre), None, k,
                                            ptr(dx), b, c, hw, ptr(ws), nws, stream()), 'hk_bcnn_pool_bwd_tdot')
        return dx, dw, db


def bilinear_pool_linear(x, weight, bias=None):
    """x [B,C,h,w] -> logits [B,K] = Linear(BilinearPooling(x)) (BCNN.py:13-27,54) as one node: see _BilinearPoolLinear."""
    return _BilinearPoolLinear.apply(x, weight, bias)


def ssqrt_pool_linear(x, weight, bias=None):
    """x [B,C,h,w] -> logits [B,K] = Linear(normalize(sign(G) sqrt(|G| + 1e-10))) with the normalisation folded into the
    classifier's epilogue (the pooled vector is never rescaled in memory)."""
    return _SsqrtPoolLinear.apply(x, weight, bias)


def linear(y, weight, bias=None):
    """y [B,J] @ weight[K,J]^T + bias[K] -> [B,K] on the split-K f32-MFMA path."""
    return _Linear.apply(y, weight, bias)


# --------------------------------------------------------------------- VGG trunk epilogues
def _nhwc(t, what):
    """A [N,C,H,W] fp32 tensor whose memory is NHWC (channels_last) - the layout the trunk runs in."""
    if t.dtype != torch.float32:
        raise _lib.HawkeyeHipError(f'{what}: fp32 only, got {t.dtype}')
    if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
        raise _lib.HawkeyeHipError(f'{what}: needs a channels_last [N,C,H,W] tensor, got shape {tuple(t.shape)} strides {t.stride()}')
    return t


def trunk_epilogue_ok(x, pool=False):
    """Whether hk_bias_relu_* serve this convolution output: an fp32 channels_last map on a HIP device, C / 4 a divisor of 256
    (VGG: 64 .. 512), even H and W for the pooled form.  Anything else stays on the framework's own ops (model/backbone/vgg.py)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    n, c, h, w = x.shape
    ok = n > 0 and c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0 and x.is_contiguous(memory_format=torch.channels_last)
    return ok and (not pool or (h % 2 == 0 and w % 2 == 0 and h > 0 and w > 0)) and x.data_ptr() % 16 == 0


class _BiasReLU(torch.autograd.Function):
    """y = relu(conv_out + bias) IN PLACE on the convolution's output; backward: dx = dy where y > 0, dbias = sum dx in one
    pass.  replaces nn.Conv2d's bias add + nn.ReLU(inplace=True) of the VGG trunk (model/backbone/vgg.py:24-57)."""

    @staticmethod
    def forward(ctx, x, bias):
        lib = _lib.load()
        _nhwc(x, 'bias_relu')
        n, c, h, w = x.shape
        b = _f32c(bias)
        # a pass that will run backward keeps the SIGN of the output as one byte per channel quad (1/16 of the map): the backward
        # then reads that instead of the map (which stays alive anyway - it is the next convolution's input)
        mask = torch.empty(n, h, w, c // 4, dtype=torch.uint8, device=x.device) if any(ctx.needs_input_grad) else None
        check(lib.hk_bias_relu_fwd(ptr(x), ptr(b), ptr(mask), n * h * w, c, stream()), 'hk_bias_relu_fwd')
        ctx.mark_dirty(x)
        ctx.save_for_backward(mask)
        ctx.in_shape = (n, c, h, w)
        return x

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (mask,) = ctx.saved_tensors
        n, c, h, w = ctx.in_shape
        if dy.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'bias_relu backward: fp32 only, got {dy.dtype}')
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(dy, memory_format=torch.channels_last)
        db = torch.empty(c, dtype=torch.float32, device=dy.device)
        nws = lib.hk_trunk_ws_bytes(c)
        ws = _ws(nws, dy.device)
        check(lib.hk_bias_relu_bwd(ptr(dy), None, ptr(mask), ptr(dx), ptr(db), n * h * w, c, ptr(ws), nws, stream()), 'hk_bias_relu_bwd')
        return dx, db


class _BiasReLUPool(torch.autograd.Function):
    """p = maxpool2x2(relu(conv_out + bias)); the full-resolution activation is never written - a 2-bit argmax per element is
    kept instead - and the backward routes dp through pool, ReLU and the bias sum in one pass.  replaces the bias add +
    nn.ReLU + nn.MaxPool2d(2, 2) behind the last convolution of each VGG stage (model/backbone/vgg.py:24-57)."""

    @staticmethod
    def forward(ctx, x, bias):
        lib = _lib.load()
        _nhwc(x, 'bias_relu_pool')
        n, c, h, w = x.shape
        b = _f32c(bias)
        p = torch.empty(n, c, h // 2, w // 2, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        am = torch.empty(n, h // 2, w // 2, c // 4, dtype=torch.uint8, device=x.device)
        check(lib.hk_bias_relu_pool_fwd(ptr(x), ptr(b), ptr(p), ptr(am), n, h, w, c, stream()), 'hk_bias_relu_pool_fwd')
        ctx.save_for_backward(p, am)
        ctx.in_shape = (n, c, h, w)
        return p

    @staticmethod
    def backward(ctx, dp):
        lib = _lib.load()
        p, am = ctx.saved_tensors
        n, c, h, w = ctx.in_shape
        if dp.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'bias_relu_pool backward: fp32 only, got {dp.dtype}')
        dp = dp.contiguous(memory_format=torch.channels_last)
        dx = torch.empty(n, c, h, w, dtype=torch.float32, device=p.device, memory_format=torch.channels_last)
        db = torch.empty(c, dtype=torch.float32, device=p.device)
        nws = lib.hk_trunk_ws_bytes(c)
        ws = _ws(nws, p.device)
        check(lib.hk_bias_relu_pool_bwd(ptr(dp), ptr(p), ptr(am), ptr(dx), ptr(db), n, h, w, c, ptr(ws), nws, stream()),
              'hk_bias_relu_pool_bwd')
        return dx, db


def _same_dense_layout(a, b):
    return (a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype == torch.float32 and a.numel() % 4 == 0 and a.numel() > 0
            and (a.is_contiguous() or (a.dim() == 4 and a.is_contiguous(memory_format=torch.channels_last))))


def add_relu_ok(a, b):
    """Whether hk_add_relu_fwd serves `relu_(a.add_(b))`: two fp32 HIP tensors of one dense layout."""
    return torch.is_tensor(a) and torch.is_tensor(b) and a.is_cuda and b.is_cuda and _same_dense_layout(a, b) and \
        a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0


class _AddReLU(torch.autograd.Function):
    """a = relu(a + b) in place on a (the residual sum that ends a ResNet bottleneck, model/backbone/resnet.py:89-136):
    one pass instead of add_ + relu_; backward: one masked copy that is the gradient of both operands."""

    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        if not _same_dense_layout(a, b):
            raise _lib.HawkeyeHipError(f'add_relu: operands must share one dense fp32 layout, got {tuple(a.shape)} {a.stride()} / '
                                       f'{tuple(b.shape)} {b.stride()}')
        check(lib.hk_add_relu_fwd(ptr(a), ptr(b), a.numel(), stream()), 'hk_add_relu_fwd')
        ctx.mark_dirty(a)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (y,) = ctx.saved_tensors
        if dy.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'add_relu backward: fp32 only, got {dy.dtype}')
        if dy.stride() != y.stride():
            dy = dy.contiguous(memory_format=torch.channels_last) if (y.dim() == 4 and not y.is_contiguous()) else dy.contiguous()
        g = torch.empty_like(y)
        check(lib.hk_relu_mask_bwd(ptr(dy), ptr(y), ptr(g), y.numel(), stream()), 'hk_relu_mask_bwd')
        return g, g


def add_relu(a, b):
    """relu(a + b) in place on a; see _AddReLU."""
    return _AddReLU.apply(a, b)


def conv1_ok(x, conv):
    """Whether hk_conv1_bias_relu_* serve this convolution: the trunk's first layer - Conv2d(Cin <= 3, 64, 3, stride 1, padding 1)
    with a bias on an fp32 channels_last HIP batch that needs no gradient itself."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not x.requires_grad):
        return False
    two = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return (x.shape[1] <= 3 and conv.in_channels == x.shape[1] and conv.out_channels == 64 and conv.bias is not None
            and two(conv.kernel_size) == (3, 3) and two(conv.stride) == (1, 1) and two(conv.padding) == (1, 1)
            and two(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and x.is_contiguous(memory_format=torch.channels_last) and x.numel() > 0)


class _Conv1BiasReLU(torch.autograd.Function):
    """relu(conv2d(x, weight, bias, padding=1)) for the trunk's first layer (Cin <= 3 -> 64 channels) in one kernel per
    direction (Cin <= 3): the output map is written once (with its sign mask), and the backward forms dW and dbias straight from the
    output's gradient without writing the masked gradient map.  replaces the library convolution + its bias / ReLU passes
    (model/backbone/vgg.py:24-57, `features[0:2]`)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        _nhwc(x, 'conv1_bias_relu')
        n, cin, h, w = x.shape
        if tuple(weight.shape) != (64, cin, 3, 3):
            raise _lib.HawkeyeHipError(f'conv1_bias_relu: weight {tuple(weight.shape)} does not match [64, {cin}, 3, 3]')
        wt = weight.detach().permute(2, 3, 1, 0).reshape(9 * cin, 64).contiguous()          # tap-major: (kh, kw, c) x out
        b = _f32c(bias.detach())
        y = torch.empty(n, 64, h, w, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        mask = torch.empty(n, h, w, 16, dtype=torch.uint8, device=x.device) if any(ctx.needs_input_grad[1:]) else None
        check(lib.hk_conv1_bias_relu_fwd(ptr(x), ptr(wt), ptr(b), ptr(y), ptr(mask), n, h, w, cin, 64, stream()), 'hk_conv1_bias_relu_fwd')
        ctx.save_for_backward(x, mask)
        ctx.wfmt = weight.is_contiguous(memory_format=torch.channels_last) and not weight.is_contiguous()
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, mask = ctx.saved_tensors
        n, cin, h, w = x.shape
        if dy.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'conv1_bias_relu backward: fp32 only, got {dy.dtype}')
        dy = dy.contiguous(memory_format=torch.channels_last)
        dwt = torch.empty(9 * cin, 64, dtype=torch.float32, device=x.device)
        db = torch.empty(64, dtype=torch.float32, device=x.device)
        nws = lib.hk_conv1_ws_bytes(cin)
        ws = _ws(nws, x.device)
        check(lib.hk_conv1_bias_relu_bwd(ptr(dy), ptr(mask), ptr(x), ptr(dwt), ptr(db), n, h, w, cin, 64, ptr(ws), nws, stream()),
              'hk_conv1_bias_relu_bwd')
        dw = dwt.view(3, 3, cin, 64).permute(3, 2, 0, 1)                                     # [64, Cin, 3, 3]
        dw = dw.contiguous(memory_format=torch.channels_last) if ctx.wfmt else dw.contiguous()
        return None, dw, db


def conv1_bias_relu(x, weight, bias):
    """relu(conv2d(x, weight, bias, stride=1, padding=1)) for Cin <= 3 -> 64 channels; see _Conv1BiasReLU."""
    return _Conv1BiasReLU.apply(x, weight, bias)


def _two(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# The layers with more than 64 input channels whose weight gradient goes to hk_conv3x3_wrw by default: (Cin, Cout, H, W) -> the batch
# sizes at which the kernel was measured against the library's weight gradient of that layer and won, stand-alone
# (profiles/wrw_wide_timing.json: slowest repeat faster than the library's fastest by more than three times the library's own
# spread) AND inside the training step.  Nothing that was not measured is here.
WRW_WIDE_WINS = {
    (128, 128, 224, 224): (64, 16),                                                                    # conv2_2 of VGG-16 at 448 x 448
    (128, 256, 112, 112): (64, 16), (256, 256, 112, 112): (64, 16),                                    # conv3_1, conv3_2 / conv3_3
    (256, 512, 56, 56): (64, 16), (512, 512, 56, 56): (64, 16),                                        # conv4_1, conv4_2 / conv4_3
    (512, 512, 28, 28): (64, 16),                                                                      # conv5_1 / conv5_2 / conv5_3
}


def _knob(name):
    import ctypes
    v = ctypes.c_int(0)
    check(_lib.load().hk_tuning_get(name, ctypes.byref(v)), f'hk_tuning_get({name.decode()})')
    return v.value


def conv3x3_wrw_route(cout, n, h, w, cin=64):
    """The dispatch rule of hk_conv3x3_wrw, by measurement (in-step kernel times at batch 64 and 16 against the
    library's weight gradient of the same layer).  64 input channels: every supported layer goes to the kernel.  More: the
    layers of WRW_WIDE_WINS at their measured batch sizes (knob `wrw_split` at its default -1), every supported layer with
    `wrw_split` at 1, none with `wrw_split` or `wrw_wide` at 0 (the entry point refuses them then).  None at all with `conv_wrw` at 0."""
    if _knob(b'conv_wrw') == 0:
        return False
    if cin <= 64:
        return True
    split = _knob(b'wrw_split')
    if _knob(b'wrw_wide') == 0 or split == 0:
        return False
    return split > 0 or n in WRW_WIDE_WINS.get((cin, cout, h, w), ())


def _conv3x3_served(x, conv):
    """What all three trunk kernels (hk_conv3x3_wrw, hk_conv3x3_fwd, hk_conv3x3_bwd_data) ask of a layer and its input, their
    dispatch rules aside: Conv2d(Cin, Cout, 3, stride 1, padding 1), Cin and Cout multiples of 64, zeros padding, with a
    channels_last fp32 weight, on a 16-byte aligned fp32 channels_last HIP map."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0):
        return False
    w = conv.weight
    if not (w.dtype == torch.float32 and w.device == x.device and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    return (conv.in_channels > 0 and conv.in_channels % 64 == 0 and x.shape[1] == conv.in_channels and conv.out_channels > 0
            and conv.out_channels % 64 == 0
            and _two(conv.kernel_size) == (3, 3) and _two(conv.stride) == (1, 1) and _two(conv.padding) == (1, 1)
            and _two(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros')


def conv3x3_wrw_ok(x, conv):
    """Whether hk_conv3x3_wrw computes this convolution's weight gradient: the layer and its input are what the trunk kernels serve
    (_conv3x3_served) and the dispatch rule (conv3x3_wrw_route) sends the layer there.  Anything else keeps the library's weight
    gradient (model/backbone/vgg.py)."""
    return _conv3x3_served(x, conv) and conv3x3_wrw_route(conv.out_channels, x.shape[0], x.shape[2], x.shape[3], conv.in_channels)


def conv3x3_wrw_raw(x, dy):
    """dW [Cout, Cin, 3, 3] (channels_last strides over the kernel's [Cout][3][3][Cin] buffer, no copy) of conv2d(x, W, padding=1)
    from the channels_last maps x [N, Cin, H, W] and dy [N, Cout, H, W], Cin and Cout multiples of 64; raises where hk_conv3x3_wrw
    does not serve the call."""
    lib = _lib.load()
    _nhwc(x, 'conv3x3_wrw')
    _nhwc(dy, 'conv3x3_wrw')
    n, cin, h, w = x.shape
    cout = dy.shape[1]
    if tuple(dy.shape) != (n, cout, h, w) or x.numel() == 0 or dy.numel() == 0:
        raise _lib.HawkeyeHipError(f'conv3x3_wrw: dy {tuple(dy.shape)} does not match x {tuple(x.shape)}')
    px, pdy = ptr(x), ptr(dy)                      # (a CPU tensor is refused here, before anything is allocated)
    buf = torch.empty(cout, 3, 3, cin, dtype=torch.float32, device=x.device)
    nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)
    ws = _ws(nws, x.device)
    check(lib.hk_conv3x3_wrw(pdy, px, ptr(buf), n, h, w, cin, cout, ptr(ws), nws, stream()), 'hk_conv3x3_wrw')
    return buf.permute(0, 3, 1, 2)


def conv3x3_wrw_pooled_raw(x, dp, p, aux):
    """dW as conv3x3_wrw_raw(x, g) gives it for the g that hk_bias_relu_pool_bwd makes of the pooled gradient dp [N, Cout, H/2, W/2], the
    pooled output p and the forward's argmax codes aux [N, H/2, W/2, Cout/4] - without g (hk_conv3x3_wrw_pooled: the 2:4 sparse
    MFMA, half the matrix instructions); raises where the entry point does not serve the call."""
    lib = _lib.load()
    _nhwc(x, 'conv3x3_wrw_pooled')
    _nhwc(dp, 'conv3x3_wrw_pooled')
    _nhwc(p, 'conv3x3_wrw_pooled')
    n, cin, h, w = x.shape
    cout = dp.shape[1]
    if (h % 2 or w % 2 or tuple(dp.shape) != (n, cout, h // 2, w // 2) or tuple(p.shape) != tuple(dp.shape) or aux.dtype != torch.uint8
            or tuple(aux.shape) != (n, h // 2, w // 2, cout // 4) or x.numel() == 0 or dp.numel() == 0):
        raise _lib.HawkeyeHipError(f'conv3x3_wrw_pooled: dp {tuple(dp.shape)}, p {tuple(p.shape)}, codes {tuple(aux.shape)} do not match x {tuple(x.shape)}')
    px, pdp, pp, pa = ptr(x), ptr(dp), ptr(p), ptr(aux)
    buf = torch.empty(cout, 3, 3, cin, dtype=torch.float32, device=x.device)
    nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)
    ws = _ws(nws, x.device)
    check(lib.hk_conv3x3_wrw_pooled(pdp, pp, pa, px, ptr(buf), n, h, w, cin, cout, ptr(ws), nws, stream()), 'hk_conv3x3_wrw_pooled')
    return buf.permute(0, 3, 1, 2)


# The layers whose forward goes to hk_conv3x3_fwd, and whose input gradient goes to hk_conv3x3_bwd_data, by default (knobs `conv_fwd` /
# `conv_bwd_data` at -1): (Cin, Cout, H, W) -> the batch sizes at which the kernel was measured against the library's kernel of that
# layer and direction and won, stand-alone (profiles/conv_split_timing.json: slowest repeat faster than the library's fastest by more
# than three times the library's own spread) AND inside the training step.  Nothing that was not measured is here.
CONV_FWD_WINS = {
    (64, 64, 448, 448): (64, 16), (64, 128, 224, 224): (64, 16), (128, 128, 224, 224): (64, 16),       # conv1_2, conv2_1, conv2_2 of VGG-16 at 448 x 448
    (128, 256, 112, 112): (64, 16), (256, 256, 112, 112): (64, 16),                                    # conv3_1, conv3_2 / conv3_3
    (256, 512, 56, 56): (64, 16), (512, 512, 56, 56): (64, 16),                                        # conv4_1, conv4_2 / conv4_3
    (512, 512, 28, 28): (64, 16),                                                                      # conv5_1 / conv5_2 / conv5_3
}
CONV_BWD_DATA_WINS = {
    (64, 64, 448, 448): (64, 16), (64, 128, 224, 224): (64, 16), (128, 128, 224, 224): (64, 16),       # conv1_2, conv2_1, conv2_2 of VGG-16 at 448 x 448
    (128, 256, 112, 112): (64, 16), (256, 256, 112, 112): (64, 16),                                    # conv3_1, conv3_2 / conv3_3
    (256, 512, 56, 56): (64, 16), (512, 512, 56, 56): (64, 16),                                        # conv4_1, conv4_2 / conv4_3
    (512, 512, 28, 28): (64, 16),                                                                      # conv5_1 / conv5_2 / conv5_3
}


def _conv3x3_route(knob, table, cin, cout, n, h, w):
    v = _knob(knob)
    if v == 0:
        return False
    return v > 0 or n in table.get((cin, cout, h, w), ())


def conv3x3_fwd_route(cin, cout, n, h, w):
    """The dispatch rule of hk_conv3x3_fwd: knob `conv_fwd` at -1 (default) the layers of CONV_FWD_WINS at their measured batch
    sizes, at 0 none, at 1 every layer the entry point serves."""
    return _conv3x3_route(b'conv_fwd', CONV_FWD_WINS, cin, cout, n, h, w)


def conv3x3_bwd_data_route(cin, cout, n, h, w):
    """The dispatch rule of hk_conv3x3_bwd_data: as conv3x3_fwd_route, with the knob `conv_bwd_data` and CONV_BWD_DATA_WINS."""
    return _conv3x3_route(b'conv_bwd_data', CONV_BWD_DATA_WINS, cin, cout, n, h, w)


def conv3x3_fwd_ok(x, conv):
    """Whether hk_conv3x3_fwd computes this convolution (conditions as conv3x3_wrw_ok) and conv3x3_fwd_route sends the layer there."""
    return (_conv3x3_served(x, conv) and conv.weight.data_ptr() % 16 == 0          # (these two kernels read the weight itself)
            and conv3x3_fwd_route(conv.in_channels, conv.out_channels, x.shape[0], x.shape[2], x.shape[3]))


def conv3x3_bwd_data_ok(x, conv):
    """Whether hk_conv3x3_bwd_data computes this convolution's input gradient and conv3x3_bwd_data_route sends the layer there."""
    return (_conv3x3_served(x, conv) and conv.weight.data_ptr() % 16 == 0
            and conv3x3_bwd_data_route(conv.in_channels, conv.out_channels, x.shape[0], x.shape[2], x.shape[3]))


# The layers whose forward / input gradient runs conv3x3_split_kernel on v_mfma_f32_16x16x32_bf16 instead of v_mfma_f32_32x32x16_bf16
# by default (knob `conv_mfma` at -1): (Cin, Cout, H, W) -> the batch sizes at which EVERY layer of that shape cleared the stand-alone
# bar (profiles/conv_mfma_timing.json: the 32 x 32 x 16 arm's fastest repeat minus the 16 x 16 x 32 arm's slowest more than three times
# the 32 x 32 x 16 arm's own spread) AND was faster inside the training step (profiles/conv_mfma_step_layers.json; DESIGN 3.10, "The
# MFMA shape").  Nothing that was not measured is here; a shape or batch that is not listed keeps 32 x 32 x 16.
# (Since the library chooses the shape itself at -1 - csrc/conv_fwd.hip, conv3x3_mfma16_wins: always 16 x 16 x 32 - these tables are a subset of what it does anyway.)
CONV_MFMA16_FWD = {
    (256, 256, 112, 112): (64,),                                                                       # conv3_2 / conv3_3
    (256, 512, 56, 56): (64, 16), (512, 512, 56, 56): (64,),                                           # conv4_1, conv4_2 / conv4_3
    (512, 512, 28, 28): (16,),                                                                         # conv5_1 / conv5_2 / conv5_3
}
CONV_MFMA16_BWD_DATA = {
    (64, 64, 448, 448): (64,),                                                                         # conv1_2
    (128, 256, 112, 112): (64, 16), (256, 256, 112, 112): (64, 16),                                    # conv3_1, conv3_2 / conv3_3
    (256, 512, 56, 56): (64, 16), (512, 512, 56, 56): (64, 16),                                        # conv4_1, conv4_2 / conv4_3
    (512, 512, 28, 28): (16,),                                                                         # conv5_1 / conv5_2 / conv5_3
}


def conv3x3_mfma_route(direction, cin, cout, n, h, w):
    """Whether the forward (`direction` 'fwd') or the input gradient ('bwd_data') of the layer (Cin, Cout) on N maps of H x W runs on the
    16 x 16 x 32 bf16 MFMA: knob `conv_mfma` at 1 every call, at 0 none, at -1 (default) the layers of CONV_MFMA16_FWD /
    CONV_MFMA16_BWD_DATA at their measured batch sizes."""
    v = _knob(b'conv_mfma')
    if v >= 0:
        return v == 1
    table = CONV_MFMA16_FWD if direction == 'fwd' else CONV_MFMA16_BWD_DATA
    return n in table.get((cin, cout, h, w), ())


def _conv3x3_mfma(direction, cin, cout, n, h, w):
    """The scope of one entry-point call of csrc/conv_fwd.hip: with the knob at its default the table's choice reaches the library as
    the knob's value for the length of the call (the entry points' signatures carry no shape of the instruction); a forced knob is
    left alone."""
    if _knob(b'conv_mfma') < 0 and conv3x3_mfma_route(direction, cin, cout, n, h, w):
        return _lib.tuning(conv_mfma=1)
    return contextlib.nullcontext()


def _conv3x3_call(fn, what, src, weight, cout_of_result):
    lib = _lib.load()
    _nhwc(src, what)
    if (weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or not weight.is_contiguous(memory_format=torch.channels_last)
            or weight.dtype != torch.float32 or weight.device != src.device):
        raise _lib.HawkeyeHipError(f'{what}: wants a channels_last fp32 [Cout, Cin, 3, 3] weight on {src.device}, got {weight.dtype} {tuple(weight.shape)}')
    n, _, h, w = src.shape
    cout, cin = weight.shape[0], weight.shape[1]
    if src.numel() == 0 or src.shape[1] != (cin if cout_of_result else cout):
        raise _lib.HawkeyeHipError(f'{what}: map {tuple(src.shape)} does not match the weight {tuple(weight.shape)}')
    psrc, pw = ptr(src), ptr(weight)                # (a CPU tensor is refused here, before anything is allocated)
    # (a channels_last tensor of its own, not a permuted view: the trunk's epilogue works in place on it)
    out = torch.empty((n, cout if cout_of_result else cin, h, w), dtype=torch.float32, device=src.device, memory_format=torch.channels_last)
    nws = lib.hk_conv3x3_ws_bytes(cin, cout)
    ws = _ws(nws, src.device)
    with _conv3x3_mfma('fwd' if cout_of_result else 'bwd_data', cin, cout, n, h, w):
        check(getattr(lib, fn)(psrc, pw, ptr(out), n, h, w, cin, cout, ptr(ws), nws, stream()), fn)
    return out


def conv3x3_fwd_raw(x, weight):
    """conv2d(x, weight, None, stride 1, padding 1) on hk_conv3x3_fwd (csrc/conv_fwd.hip): channels_last x [N, Cin, H, W] and weight
    [Cout, Cin, 3, 3] -> a new channels_last [N, Cout, H, W]; raises where the entry point does not serve the call."""
    return _conv3x3_call('hk_conv3x3_fwd', 'conv3x3_fwd', x, weight, True)


def conv3x3_bwd_data_raw(dy, weight):
    """The input gradient of that convolution on hk_conv3x3_bwd_data: channels_last dy [N, Cout, H, W] and the forward's weight ->
    a new channels_last [N, Cin, H, W]."""
    return _conv3x3_call('hk_conv3x3_bwd_data', 'conv3x3_bwd_data', dy, weight, False)


class _Conv3x3(torch.autograd.Function):
    """conv2d(x, weight, None, stride 1, padding 1) for multiples of 64 channels, each of its three GEMMs on the project's kernel or the
    library's, independently: the forward on hk_conv3x3_fwd (`fwd`) or F.conv2d, the input gradient on hk_conv3x3_bwd_data (`bwd`)
    or aten.convolution_backward, the weight gradient on hk_conv3x3_wrw (`wrw`; csrc/conv_wrw.hip) or aten.convolution_backward.
    The library's fp32 kernels stay on the fp32 matrix pipe, which the kernels' split bf16 form leaves (model/backbone/vgg.py:24-57)."""

    @staticmethod
    def forward(ctx, x, weight, fwd, bwd, wrw):
        ctx.save_for_backward(x, weight)
        ctx.routes = (bwd, wrw)
        if fwd:
            return conv3x3_fwd_raw(x, weight)
        return torch.nn.functional.conv2d(x, weight, None, 1, 1, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        bwd, wrw = ctx.routes
        if dy.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'conv3x3 backward: fp32 only, got {dy.dtype}')
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_dx and bwd:
            dx = conv3x3_bwd_data_raw(dy, weight)
        if need_dw and wrw:
            dw = conv3x3_wrw_raw(x, dy)
        mask = (need_dx and not bwd, need_dw and not wrw, False)
        if mask[0] or mask[1]:
            g = torch.ops.aten.convolution_backward(dy, x, weight, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, mask)
            dx = g[0] if mask[0] else dx
            dw = g[1] if mask[1] else dw
        return dx, dw, None, None, None


def conv3x3(x, weight, fwd=False, bwd=False, wrw=True):
    """conv2d(x, weight, None, stride=1, padding=1) with the chosen GEMMs on the project's kernels; see _Conv3x3.  Inside a
    ConvEpilogue context (and with `fwd`): the fused unit it asks for, see _ConvUnit."""
    e = ConvEpilogue.take()
    if e is not None:
        if not fwd:
            raise _lib.HawkeyeHipError('conv3x3: an epilogue inside the kernel needs the forward on the kernel (fwd)')
        return _ConvUnit.apply(x, weight, e.bias, e.pool, bool(bwd), bool(wrw), e.masked, e.link_in, e.link)
    return _Conv3x3.apply(x, weight, bool(fwd), bool(bwd), bool(wrw))


def conv3x3_wrw(x, weight):
    """conv2d(x, weight, None, stride=1, padding=1) with the weight gradient on hk_conv3x3_wrw; see _Conv3x3."""
    return _Conv3x3.apply(x, weight, False, False, True)


# The layers whose forward runs with its epilogue inside the kernel (hk_conv3x3_bias_relu_fwd / hk_conv3x3_bias_relu_pool_fwd) and
# whose input gradient takes the producing layer's mask (hk_conv3x3_masked_bwd_data), knob `conv_epi` at its default 2: the layers of
# CONV_FWD_WINS / CONV_BWD_DATA_WINS for which the fused form was not measured SLOWER than its two-kernel pair inside the training
# step ("Epilogues inside the kernels").  A layer listed here is taken out of the fusion, not out of the kernel.
CONV_EPI_FWD_LOSES = {}
CONV_EPI_MASKED_LOSES = {}


def conv3x3_epi_level():
    """Knob `conv_epi`: 0 the epilogues of the trunk's convolutions as passes of their own, 1 bias + ReLU (+ pool) inside the forward
    kernel, 2 (default) also the producer's ReLU mask and bias-gradient partials inside the input-gradient kernel."""
    return _knob(b'conv_epi')


def conv3x3_epi_fwd_ok(x, conv, fwd):
    """Whether a layer whose forward runs on hk_conv3x3_fwd (`fwd` = conv3x3_fwd_ok) runs it with bias + ReLU (+ pool) inside:
    `conv_epi` >= 1, a bias, and a channel count the epilogues' backward passes serve (trunk_epilogue_ok's rule)."""
    c = conv.out_channels
    return bool(fwd and conv3x3_epi_level() >= 1 and conv.bias is not None and conv.bias.dtype == torch.float32
                and conv.bias.data_ptr() % 16 == 0 and 256 % (c // 4) == 0
                and x.shape[0] not in CONV_EPI_FWD_LOSES.get((conv.in_channels, c, x.shape[2], x.shape[3]), ()))


def conv3x3_epi_masked_ok(x, conv, bwd):
    """Whether a layer whose input gradient runs on hk_conv3x3_bwd_data (`bwd` = conv3x3_bwd_data_ok) applies the mask of the layer
    that produced x inside that kernel, given such a mask: `conv_epi` == 2."""
    return bool(bwd and conv3x3_epi_level() >= 2
                and x.shape[0] not in CONV_EPI_MASKED_LOSES.get((conv.in_channels, conv.out_channels, x.shape[2], x.shape[3]), ()))


class ConvLink:
    """What one fused unit of the trunk hands the next (model/backbone/vgg.py: ConvStack.forward) beside its output: `mask`, the sign
    mask of that output ([N][H][W][C / 4] bytes; None behind a pool and behind an unfused layer).  In the backward pass the CONSUMING
    unit, if its input gradient runs on hk_conv3x3_masked_bwd_data, applies the mask itself and leaves `db`, the producer's bias
    gradient, here; the producer then finds its incoming gradient already masked and skips hk_bias_relu_bwd.  The contract - the
    gradient that travels between two linked units is the MASKED one - holds only where nobody else can see that tensor: inside
    ConvStack.forward."""
    __slots__ = ('mask', 'db')

    def __init__(self, mask=None):
        self.mask, self.db = mask, None


class _ConvUnit(torch.autograd.Function):
    """One layer of the trunk as ONE node: relu(conv2d(x, weight, bias, padding 1)), or its 2 x 2 max-pool, with the epilogue inside the
    forward kernel (csrc/conv_fwd.hip, EPI).  Backward: the epilogue's backward pass (hk_bias_relu_pool_bwd, or hk_bias_relu_bwd
    unless the consumer has applied this layer's mask already: ConvLink), then the two gradients as _Conv3x3 routes them, the input
    gradient with the producer's mask where `link_in` carries one and `masked` says so."""

    @staticmethod
    def forward(ctx, x, weight, bias, pool, bwd, wrw, masked, link_in, link_out):
        lib = _lib.load()
        _nhwc(x, 'conv3x3 unit')
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        if (tuple(weight.shape) != (cout, cin, 3, 3) or not weight.is_contiguous(memory_format=torch.channels_last)
                or weight.dtype != torch.float32 or weight.device != x.device):
            raise _lib.HawkeyeHipError(f'conv3x3 unit: wants a channels_last fp32 [Cout, {cin}, 3, 3] weight on {x.device}, got {weight.dtype} {tuple(weight.shape)}')
        b = _f32c(bias)
        px, pw = ptr(x), ptr(weight)
        nws = lib.hk_conv3x3_ws_bytes(cin, cout)
        ws = _ws(nws, x.device)
        grad = any(ctx.needs_input_grad[:3])
        if pool:
            y = torch.empty((n, cout, h // 2, w // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            aux = torch.empty(n, h // 2, w // 2, cout // 4, dtype=torch.uint8, device=x.device)
            with _conv3x3_mfma('fwd', cin, cout, n, h, w):
                check(lib.hk_conv3x3_bias_relu_pool_fwd(px, pw, ptr(b), ptr(y), ptr(aux), n, h, w, cin, cout, ptr(ws), nws, stream()),
                      'hk_conv3x3_bias_relu_pool_fwd')
        else:
            y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            aux = torch.empty(n, h, w, cout // 4, dtype=torch.uint8, device=x.device) if grad else None
            with _conv3x3_mfma('fwd', cin, cout, n, h, w):
                check(lib.hk_conv3x3_bias_relu_fwd(px, pw, ptr(b), ptr(y), ptr(aux), n, h, w, cin, cout, ptr(ws), nws, stream()),
                      'hk_conv3x3_bias_relu_fwd')
            link_out.mask = aux
        min_ = link_in.mask if (masked and link_in is not None) else None
        ctx.save_for_backward(x, weight, aux, y if pool else None, min_)
        ctx.cfg = (pool, bwd, wrw, (n, cout, h, w))
        ctx.links = (link_in, link_out)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight, aux, p, min_ = ctx.saved_tensors
        pool, bwd, wrw, (n, cout, h, w) = ctx.cfg
        link_in, link_out = ctx.links
        cin = x.shape[1]
        if dy.dtype != torch.float32:
            raise _lib.HawkeyeHipError(f'conv3x3 unit backward: fp32 only, got {dy.dtype}')
        dy = dy.contiguous(memory_format=torch.channels_last)
        db, link_out.db = link_out.db, None
        if pool:
            g = torch.empty(n, cout, h, w, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
            db = torch.empty(cout, dtype=torch.float32, device=x.device)
            nws = lib.hk_trunk_ws_bytes(cout)
            ws = _ws(nws, x.device)
            check(lib.hk_bias_relu_pool_bwd(ptr(dy), ptr(p), ptr(aux), ptr(g), ptr(db), n, h, w, cout, ptr(ws), nws, stream()),
                  'hk_bias_relu_pool_bwd')
        elif db is not None:
            g = dy                                         # the consumer wrote dy o mask and summed its columns (ConvLink)
        else:
            g = torch.empty_like(dy, memory_format=torch.channels_last)
            db = torch.empty(cout, dtype=torch.float32, device=x.device)
            nws = lib.hk_trunk_ws_bytes(cout)
            ws = _ws(nws, x.device)
            check(lib.hk_bias_relu_bwd(ptr(dy), None, ptr(aux), ptr(g), ptr(db), n * h * w, cout, ptr(ws), nws, stream()),
                  'hk_bias_relu_bwd')
        dx = dw = None
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_dx and bwd:
            if min_ is not None:
                dx = torch.empty_like(x, memory_format=torch.channels_last)
                dbp = torch.empty(cin, dtype=torch.float32, device=x.device)
                nws = lib.hk_conv3x3_masked_ws_bytes(n, h, w, cin, cout)
                ws = _ws(nws, x.device)
                with _conv3x3_mfma('bwd_data', cin, cout, n, h, w):
                    check(lib.hk_conv3x3_masked_bwd_data(ptr(g), ptr(weight), ptr(min_), ptr(dx), ptr(dbp), n, h, w, cin, cout, ptr(ws), nws,
                                                         stream()), 'hk_conv3x3_masked_bwd_data')
                link_in.db = dbp
            else:
                dx = conv3x3_bwd_data_raw(g, weight)
        if need_dw and wrw:
            # a pooled layer's g is three quarters zeros by construction: where the library says so (knob `wrw_pool`), dW comes from the
            # pooled gradient itself on the 2:4 sparse MFMA; g stays what the input gradient and db are made of
            if pool and lib.hk_conv3x3_wrw_pooled_served(n, h, w, cin, cout):
                dw = conv3x3_wrw_pooled_raw(x, dy, p, aux)
            else:
                dw = conv3x3_wrw_raw(x, g)
        lib_mask = (need_dx and not bwd, need_dw and not wrw, False)
        if lib_mask[0] or lib_mask[1]:
            r = torch.ops.aten.convolution_backward(g, x, weight, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, lib_mask)
            dx = r[0] if lib_mask[0] else dx
            dw = r[1] if lib_mask[1] else dw
        return dx, dw, (db if ctx.needs_input_grad[2] else None), None, None, None, None, None, None


class ConvEpilogue:
    """`with ConvEpilogue(bias, pool, masked, link_in) as e: y = conv3x3(x, weight, True, bwd, wrw)` - the conv3x3 call inside runs as
    ONE fused unit (_ConvUnit): y is relu(conv + bias), or its 2 x 2 max-pool, and e.link is the ConvLink for the next unit.  (The
    request reaches conv3x3 beside its arguments, per thread, so that the call itself stays the one every routed layer makes.)"""
    _pending = threading.local()

    def __init__(self, bias, pool, masked, link_in):
        self.bias, self.pool, self.masked, self.link_in, self.link = bias, bool(pool), bool(masked), link_in, ConvLink()

    def __enter__(self):
        ConvEpilogue._pending.request = self
        return self

    def __exit__(self, *exc):
        ConvEpilogue._pending.request = None
        return False

    @staticmethod
    def take():
        e = getattr(ConvEpilogue._pending, 'request', None)
        ConvEpilogue._pending.request = None
        return e


def bias_relu(x, bias):
    """relu(x + bias[None,:,None,None]) in place on x (a channels_last convolution output); see _BiasReLU."""
    return _BiasReLU.apply(x, bias)


def bias_relu_pool(x, bias):
    """max_pool2d(relu(x + bias[None,:,None,None]), 2, 2) for a channels_last convolution output; see _BiasReLUPool."""
    return _BiasReLUPool.apply(x, bias)


# --------------------------------------------------------------------- input finalisation
def image_finalize(u8, erase=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels_last=False):
    """uint8 [B,H,W,3] on the device (+ int32 erase boxes [B,4] = top, left, h, w) -> normalised fp32 [B,3,H,W]
    (channels_last storage if asked).  No gradient: it is the end of the data pipeline."""
    import ctypes
    lib = _lib.load()
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise _lib.HawkeyeHipError(f'image_finalize wants uint8 [B,H,W,3], got {u8.dtype} {tuple(u8.shape)}')
    u8 = u8.contiguous()
    b, h, w, _ = u8.shape
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    out = torch.empty(b, 3, h, w, dtype=torch.float32, device=u8.device).contiguous(memory_format=fmt)
    if erase is not None:
        erase = erase.to(device=u8.device, dtype=torch.int32).contiguous()
        if erase.shape != (b, 4):
            raise _lib.HawkeyeHipError(f'image_finalize: erase boxes must be [B,4], got {tuple(erase.shape)}')
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(lib.hk_image_finalize(ptr(u8), ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), ptr(erase),
                                ptr(out.permute(0, 2, 3, 1) if channels_last else out), b, h, w, int(channels_last),
                                stream()), 'hk_image_finalize')
    return out


def bgemm(a, b, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, diag=0.0, out=None):
    """Batched fp32 MFMA GEMM (test / composition helper).  a [B,M,K] (or [B,K,M]), b [B,K,N] (or [B,N,K])."""
    lib = _lib.load()
    a, b = _f32c(a), _f32c(b)
    nb = a.shape[0]
    m, k = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
    n = b.shape[1] if trans_b else b.shape[2]
    if out is None:
        out = torch.zeros(nb, m, n, dtype=torch.float32, device=a.device)
    check(lib.hk_bgemm_f32(ptr(a), a.shape[2], a.shape[1] * a.shape[2], int(trans_a),
                           ptr(b), b.shape[2], b.shape[1] * b.shape[2], int(trans_b),
                           ptr(out), n, m * n, m, n, k, nb, float(alpha), float(beta), float(diag), stream()),
          'hk_bgemm_f32')
    return out
