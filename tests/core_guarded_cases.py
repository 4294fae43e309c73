"""Cases, inputs, float64 references and runners shared by tests/test_emu_core_guarded.py (CPU emulation) and
tests/test_gpu_core_guarded.py (MI355X): the library's original ops - bilinear and signed-sqrt pooling, covariance pooling and the
Newton-Schulz chain, compact bilinear pooling in all its forms, the classifier GEMMs, the CIN interaction and hk_bgemm_f32 - called
through the C ABI the way the trunk kernels are tested (tests/conv_epilogue_cases.py, tests/wrw_pool_cases.py).  Not a test module.

Layout of a call (class Bufs)
  * every input lies in a Guarded buffer whose other elements are 1e30: an over-read that is summed in shows up in the result;
  * every output and the workspace lie in Guarded buffers too; their inner part is filled with NaN (the workspace: bytes 0xFF, a NaN
    in every float) before EVERY call, so an element a form does not write cannot inherit the right value from the form before it;
  * the workspace is exactly hk_*_ws_bytes(...) long;
  * pads: one 64-row tile of the widest kernel, 64 * ld floats (ld = the row length of the matrix the kernels tile), 4096 bytes for
    workspaces; inner pointers stay 16-byte aligned;
  * after the call every guard has to be intact and no NaN may be left in what the header documents as written.

The judge (class Report)
  * sums of products in fp32 - per element: |got - ref64| <= (K + 4) 2^-24 S, ref64 the float64 result, S the same expression over
    absolute values, K the number of terms of the longest sum the element goes through.  Any order of fp32 additions of K terms stays
    within (K - 1) 2^-24 sum |term| of the exact sum; the products, a scale factor and a bias in the epilogue round four times more at
    most.  Derived, not measured; where K is not the obvious inner dimension the case says why.
  * ops with a nonlinearity behind the sum (sqrt, signed sqrt, l2 normalisation, softmax, the Newton-Schulz chain) keep the norm-ratio
    bound of the existing test of the same op, quoted with file and line where it is used (rel(), below, is those tests' rel()).
  * the BCNN backward gets both: as a function of what it is given it is a sum of products, and bcnn_case derives its bound per element.

Every reference is float64 torch on the CPU, made once per case (functools.lru_cache) and never written to; the builders assert that it
is finite and that S > 0 wherever the reference is not 0."""
import ctypes
import functools
import math

import numpy as np
import torch

from conv_epilogue_cases import Guarded

U = 2.0 ** -24
NAN = float('nan')
HK_ERR_WORKSPACE, HK_ERR_UNSUPPORTED = -2, -3


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st(dev):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if torch.device(dev).type == 'cuda' else None


def _gen(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + int(x) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _pad(ld):
    return 4 * ((64 * max(int(ld), 1) + 3) // 4)


class Bufs:
    """The guarded buffers of one call (see the module's docstring)."""

    def __init__(self, dev):
        self.dev, self.guards, self.outs, self.keep, self.ws = dev, [], {}, {}, None

    def inp(self, t, ld=None):
        t = t.contiguous()
        g = Guarded(t.numel(), t.dtype, self.dev, _pad(t.shape[-1] if ld is None else ld) if t.dtype == torch.float32 else 4096)
        g.inner.copy_(t.reshape(-1))
        self.guards.append(g)
        return _p(g.inner)

    def out(self, name, shape, ld=None):
        g = Guarded(math.prod(shape), torch.float32, self.dev, _pad(shape[-1] if ld is None else ld))
        g.inner.fill_(NAN)
        self.guards.append(g)
        self.outs[name] = (g, tuple(shape))
        return _p(g.inner)

    def inout(self, name, t, ld=None):
        """An output that is read too (beta C, the CIN scratch with has_extra): refilled with `t` by poison()."""
        p = self.out(name, tuple(t.shape), ld)
        self.keep[name] = t.contiguous()
        self.outs[name][0].inner.copy_(self.keep[name].reshape(-1))
        return p

    def work(self, nbytes):
        self.ws = Guarded(int(nbytes), torch.uint8, self.dev, 4096)
        self.ws.inner.fill_(0xFF)
        self.guards.append(self.ws)
        return _p(self.ws.inner), int(nbytes)

    def poison(self):
        for name, (g, _) in self.outs.items():
            if name in self.keep:
                g.inner.copy_(self.keep[name].reshape(-1))
            else:
                g.inner.fill_(NAN)
        if self.ws is not None:
            self.ws.inner.fill_(0xFF)

    def broken(self):
        return [i for i, g in enumerate(self.guards) if not g.intact()]

    def get(self, name):
        g, shape = self.outs[name]
        return g.inner.cpu().clone().view(shape)

    def ws_floats(self, n):
        """The first n floats of the workspace (a copy on the CPU)."""
        return self.ws.inner[:4 * n].cpu().clone().view(torch.float32)

    def untouched(self):
        """Nothing written: every output still all NaN (in/out buffers: their input), the workspace still all 0xFF."""
        for name, (g, _) in self.outs.items():
            if name in self.keep:
                if not torch.equal(g.inner.cpu(), self.keep[name].reshape(-1)):
                    return False
            elif not bool(torch.isnan(g.inner).all()):
                return False
        return self.ws is None or bool((self.ws.inner == 0xFF).all())


class Report:
    """Collects the checks of one case; done() prints the worst ratio per output and fails with everything that missed."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def check(self, label, ok, info=None):
        if not ok:
            self.bad.append((label, info))

    def call(self, lib, name, bf, *args, expect=0):
        rc = getattr(lib, name)(*args, _st(bf.dev))
        self.check(f'{name}: return code', rc == expect, rc)
        self.check(f'{name}: guard rows', not bf.broken(), bf.broken())
        return rc

    def elem(self, label, got, ref, S, K):
        """|got - ref| <= (K + 4) 2^-24 S per element (K a number or a tensor like ref); exact where S = 0."""
        K = K.double().reshape(-1) if torch.is_tensor(K) else float(K)
        return self.within(label, got, ref, (K + 4.0) * U * S.reshape(-1))

    def within(self, label, got, ref, allowed):
        """|got - ref| <= allowed per element; exact where allowed = 0."""
        got, ref, allowed = got.double().reshape(-1), ref.reshape(-1), allowed.reshape(-1)
        err = (got - ref).abs()
        ok = err <= allowed                                        # (a NaN fails)
        ratio = float((err / allowed.clamp_min(1e-300))[allowed > 0].max()) if bool((allowed > 0).any()) else 0.0
        self.rows.append(f'{label} {ratio:.3f}')
        self.check(f'{label}: per element', bool(ok.all()), dict(missed=int((~ok).sum()), of=ok.numel(), worst_ratio=ratio,
                                                                 nan=int(torch.isnan(got).sum())))
        return ratio

    def exact(self, label, got, ref):
        ok = torch.equal(got.reshape(-1), ref.reshape(-1).to(got.dtype))
        self.rows.append(f'{label} {"exact" if ok else "DIFFERS"}')
        self.check(f'{label}: exact', ok, int((got.reshape(-1) != ref.reshape(-1).to(got.dtype)).sum()))

    def norm(self, label, got, ref, bound, src):
        """The norm-ratio bound of the existing test named by `src` ('file:line'), unchanged; no NaN may be left."""
        self.check(f'{label}: written', not bool(torch.isnan(got).any()), int(torch.isnan(got).sum()))
        e = rel(got, ref)
        self.rows.append(f'{label} {e / bound:.3f}')
        self.check(f'{label}: rel < {bound:g} ({src})', e < bound, e)
        return e

    def done(self):
        print(f'[{self.tag}] worst error / bound: ' + ', '.join(self.rows))
        assert not self.bad, (self.tag, self.bad)


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all())


def _scaled(ref, S):
    """The builder's check for the per-element rule: finite, and S > 0 wherever the reference is not 0."""
    _finite(ref, S)
    assert bool((S[ref != 0] > 0).all())
    return ref, S


class Case(dict):
    __getattr__ = dict.__getitem__


# ======================================================================================================================= generic GEMM
# hk_bgemm_f32 (csrc/api.hip:70, hk_bgemm.h): 64 x 64 tiles, edge tiles guarded; nb = 9 takes the XCD-affine block map with a ragged
# last group (tests/test_gpu_parity.py:62).  (m, n, k, nb, trans_a, trans_b, variant)
BGEMM_SHAPES = [(70, 45, 33), (1, 1, 1), (130, 196, 64)]
BGEMM_CASES = [(m, n, k, nb, ta, tb, 'plain') for (m, n, k) in BGEMM_SHAPES for nb in (3, 9) for ta in (0, 1) for tb in (0, 1)]
BGEMM_CASES += [(70, 45, 33, 3, 0, 1, 'strided'),        # ldc = n + 3, batch stride > m ldc: the gaps are guard values that must survive
                (70, 45, 33, 3, 1, 0, 'strided'),
                (70, 45, 33, 9, 0, 0, 'epilogue'),       # alpha, beta and diag all non-trivial
                (130, 196, 64, 3, 1, 1, 'epilogue')]
BGEMM_IDS = ['x'.join(map(str, c[:4])) + f'-t{c[4]}{c[5]}-{c[6]}' for c in BGEMM_CASES]


@functools.lru_cache(maxsize=None)
def bgemm_case(case):
    m, n, k, nb, ta, tb, variant = case
    g = _gen(2, m, n, k, nb, ta, tb)
    a = torch.randn((nb, k, m) if ta else (nb, m, k), generator=g)
    b = torch.randn((nb, n, k) if tb else (nb, k, n), generator=g)
    c0 = torch.randn(nb, m, n, generator=g)
    alpha, beta, diag = (-0.5, 0.25, 1.5) if variant == 'epilogue' else (1.0, 0.0, 0.0)
    a64 = a.double().transpose(1, 2) if ta else a.double()
    b64 = b.double().transpose(1, 2) if tb else b.double()
    eye = torch.eye(m, n, dtype=torch.float64)
    ref = alpha * (a64 @ b64) + beta * c0.double() + diag * eye
    S = abs(alpha) * (a64.abs() @ b64.abs()) + abs(beta) * c0.double().abs() + abs(diag) * eye
    _scaled(ref, S)
    return Case(a=a, b=b, c0=c0, alpha=alpha, beta=beta, diag=diag, ref=ref, S=S)


def run_bgemm(lib, dev, case, knobs=None):
    m, n, k, nb, ta, tb, variant = case
    c = bgemm_case(case)
    R = Report(f'bgemm {case}')
    bf = Bufs(dev)
    pa, pb = bf.inp(c.a), bf.inp(c.b)
    ldc, sc = (n + 3, m * (n + 3) + 5 * (n + 3) + 4) if variant == 'strided' else (n, m * n)
    if variant == 'epilogue':
        pc = bf.inout('c', c.c0)
    else:
        pc = bf.out('c', (nb * sc,), ld=ldc)
    cells = (torch.arange(m)[:, None] * ldc + torch.arange(n)[None, :]).reshape(-1)          # where a batch's elements lie
    written = torch.zeros(nb, sc, dtype=torch.bool)
    written[:, cells] = True
    for _ in range(2):                                             # the second call on freshly poisoned buffers: the same checks
        bf.poison()
        if variant == 'strided':                                   # written elements NaN, the gaps 1e30 like the pads
            bf.outs['c'][0].inner.copy_(torch.where(written, torch.tensor(NAN), torch.tensor(1e30)).reshape(-1))
        R.call(lib, 'hk_bgemm_f32', bf, pa, c.a.shape[2], c.a.shape[1] * c.a.shape[2], ta, pb, c.b.shape[2], c.b.shape[1] * c.b.shape[2], tb,
               pc, ldc, sc, m, n, k, nb, c.alpha, c.beta, c.diag)
        got = bf.get('c')
        if variant == 'strided':
            full = got.view(nb, sc)
            got = full[:, cells]
            R.check('gaps between rows and batches', bool((full[~written] == 1e30).all()), int((full[~written] != 1e30).sum()))
        R.elem('c', got.reshape(nb, m, n), c.ref, c.S, k)
    R.done()


# ============================================================================================================================== BCNN
# (B, C, HW) and what each reaches (csrc/bcnn_pool.hip, csrc/bcnn_fast.hip):
BCNN_SHAPES = [
    (2, 128, 64),      # panel kernels: C % 64 == 0 and HW in {196, 144, 100, 64} (bcnn_fast.hip:574-581 HK_HW_SWITCH, :585); G = 2 > 1: the
    (2, 128, 100),     #   one-launch forward (bcnn_pool.hip:373) and with fwd_fold = -1 the two-launch one (:379)
    (2, 192, 144),     #   three row blocks
    (2, 128, 196),
    (2, 64, 196),      # G = 1: no fold (bcnn_pool.hip:373 and :379 need G > 1), one-kernel column sums (:344), panel Gram
    (2, 130, 12),      # C % 64 != 0: generic GEMM; G = 3, HW % 4 == 0, HW / 4 <= 64: bcnn_colsum_partial4_kernel (bcnn_pool.hip:334)
    (2, 70, 35),       # G = 2, HW % 4 != 0: bcnn_colsum_partial_kernel (bcnn_pool.hip:337)
    (1, 3, 1),         # one pixel, G = 1: bcnn_colsum_norm_kernel (bcnn_pool.hip:348)
]
# the backward on gram_bwd3_kernel needs B (C / 128) >= 192 with C % 128 == 0 (128-row blocks) or B (C / 64) >= 192 (64-row blocks)
# (bcnn_fast.hip:546-548, the one-launch form :662-664): the smallest real shapes that pass each, not the sched_b knob
BCNN_FILL = [(96, 128, 64),    # fill1 only: 96 * 2 = 192 row blocks of 64, 96 * 1 < 192 of 128
             (96, 256, 64)]    # fill2: 96 * 2 = 192 row blocks of 128
_PANEL_HW = (196, 144, 100, 64)


def _panel(shape):
    return shape[1] % 64 == 0 and shape[2] in _PANEL_HW


def bcnn_knob_sets(shape):
    """Every knob set a shape runs with: the defaults; fast-form shapes also with bcnn_generic = 1 and with fwd_fold = -1; bwd_v and
    bwd_fold at each value tests/test_gpu_kernels.py uses (bwd_v 0 / 1: :63-66, bwd_fold 0 / -1: :106-107) where they change the
    form - the shapes whose row blocks fill the chip."""
    if shape in BCNN_FILL:
        return [dict(), dict(bwd_v=1), dict(bwd_fold=-1)]
    # sched_b: the work split sees a batch of 200, so gram_bwd3_kernel runs at the other panel sizes too (tests/test_gpu_kernels.py:67)
    return [dict()] + ([dict(bcnn_generic=1), dict(fwd_fold=-1), dict(sched_b=200), dict(sched_b=200, bwd_fold=-1)] if _panel(shape) else [])


BCNN_CASES = [(s, tuple(sorted(k.items()))) for s in BCNN_SHAPES + BCNN_FILL for k in bcnn_knob_sets(s)]
BCNN_IDS = ['x'.join(map(str, s)) + ''.join(f'-{k}{v}' for k, v in ks) for s, ks in BCNN_CASES]


def _tdot_operands(t, B, g):
    """ta [B, 3], tb [B, 3], tc [3] with sum_k ta (tb - tc) = t (hawkeye_hip.h:111-115), as float32."""
    ta = torch.randn(B, 3, generator=g).double()
    tc = 0.1 * torch.randn(3, generator=g).double()
    tb = tc + t[:, None] * ta / (ta * ta).sum(1, keepdim=True)
    return ta.float(), tb.float(), tc.float()


@functools.lru_cache(maxsize=4)
def bcnn_case(shape):
    B, C, HW = shape
    g = _gen(1, *shape)
    x = torch.relu(torch.randn(B, C, HW, generator=g))
    dy = torch.randn(B, C * C, generator=g)
    x64 = x.double()
    gram = x64 @ x64.transpose(1, 2) / HW
    z = (gram + 1e-5).sqrt()
    nrm = z.flatten(1).norm(dim=1).clamp_min(1e-12)
    y, inv, colsum = (z / nrm[:, None, None]).flatten(1), 1.0 / nrm, x64.sum(1)
    _finite(y, inv, colsum)
    _scaled(colsum, x64.abs().sum(1))
    # The backward is a function of what it is GIVEN - y, inv_norm and colsum as float32, dy, x: with z = y / inv_norm,
    #   dG = inv (dy - y t) / 2 z = A - inv^2 t / 2,  A = inv^2 dy / 2 y,  t = <y, dy>
    #   dX = (dG + dG^T) X / HW = (A + A^T) X / HW - (inv^2 t / HW) 1 colsum^T
    # - a sum of C products per element (the GEMM launch) and a rank-1 term whose scalar is a sum of C^2 products.
    y32, inv32, cs32, dy64 = y.float().double(), inv.float().double(), colsum.float().double(), dy.double()
    A = (inv32[:, None] ** 2 * dy64 / (2.0 * y32)).view(B, C, C)
    gemm = (A + A.transpose(1, 2)) @ x64 / HW
    S_gemm = (A.abs() + A.abs().transpose(1, 2)) @ x64.abs() / HW
    t, T = (y32 * dy64).sum(1), (y32 * dy64).abs().sum(1)
    ta, tb, tc = _tdot_operands(t, B, g)
    t3 = (ta.double() * (tb.double() - tc.double())).sum(1)                    # the t hk_bcnn_pool_bwd_tdot is handed
    T3 = (ta.double().abs() * (tb.double().abs() + tc.double().abs())).sum(1)
    rank1 = lambda s, cs=cs32: (inv32 ** 2 * s / HW)[:, None, None] * cs[:, None, :]
    dx, dx3 = gemm - rank1(t), gemm - rank1(t3)
    # allowed: (C + 16) 2^-24 S_gemm + (n + 16) 2^-24 S_rank1, n the terms of t (C^2; 3 through the tdot operands).  16: the roundings
    # outside the two sums - two quotients, inv^2, 1 / 2 HW and its product and the sum of the transposed pair in every entry of the
    # operand (<= 8), the GEMM's scale, and inv^2, 1 / HW, the product with colsum and the subtraction of the rank-1 term (<= 6)
    allowed = (C + 16) * U * S_gemm + (C * C + 16) * U * rank1(T, cs32.abs())
    allowed3 = (C + 16) * U * S_gemm + (3 + 16) * U * rank1(T3, cs32.abs())
    _finite(dx, dx3, allowed, allowed3)
    assert bool((allowed[dx != 0] > 0).all())
    return Case(x=x, dy=dy, y=y, inv=inv, colsum=colsum, dx=dx, allowed=allowed, dx3=dx3, allowed3=allowed3, ta=ta, tb=tb, tc=tc)


def bcnn_forward(lib, dev, shape, R, staged=False, short_ws=False):
    """hk_bcnn_pool_fwd, or its stages hk_bcnn_colsum_norm + hk_bcnn_gram_norm -> y, inv_norm, colsum, the workspace's floats."""
    B, C, HW = shape
    c = bcnn_case(shape)
    bf = Bufs(dev)
    px = bf.inp(c.x)
    py, pinv, pcs = bf.out('y', (B, C * C), C), bf.out('inv', (B,)), bf.out('colsum', (B, HW))
    pws, nws = bf.work(lib.hk_bcnn_pool_ws_bytes(B, C, HW))
    # short_ws: 'short' = one byte less than the column-sum partials [B][G][HW] need (the 256 bytes of slack in hk_bcnn_pool_ws_bytes
    # are not what the two-stage forms test, bcnn_pool.hip:333, :379); 'null' = no workspace at all
    given = B * ((C + 63) // 64) * HW * 4 - 1 if short_ws == 'short' else nws
    if short_ws == 'null':
        pws, given = None, 0
    if staged:
        R.call(lib, 'hk_bcnn_colsum_norm', bf, px, pcs, pinv, B, C, HW, pws, given)
        R.call(lib, 'hk_bcnn_gram_norm', bf, px, pinv, py, B, C, HW)
    else:
        R.call(lib, 'hk_bcnn_pool_fwd', bf, px, py, pinv, pcs, B, C, HW, pws, given)
    if short_ws:
        R.check('optional workspace too short: not touched', bool((bf.ws.inner == 0xFF).all()))
    return bf.get('y'), bf.get('inv'), bf.get('colsum'), bf.ws_floats(B * ((C + 63) // 64) * HW)


def _bcnn_bwd_bufs(dev, c, shape):
    B, C, HW = shape
    bf = Bufs(dev)
    ptrs = Case(x=bf.inp(c.x), y=bf.inp(c.y.float(), C), dy=bf.inp(c.dy, C), inv=bf.inp(c.inv.float()), dx=bf.out('dx', (B, C, HW)))
    return bf, ptrs


def run_bcnn(lib, dev, shape, knobs):
    B, C, HW = shape
    c = bcnn_case(shape)
    G = (C + 63) // 64
    generic = knobs.get('bcnn_generic', 0) == 1
    R = Report(f'bcnn {shape} {knobs}')
    SRC_Y, SRC_DX = 'tests/test_gpu_parity.py:180', 'tests/test_gpu_parity.py:181'
    for staged in (False, True):
        y, inv, colsum, ws = bcnn_forward(lib, dev, shape, R, staged)
        tag = 'stages ' if staged else 'fwd '
        R.norm(tag + 'y', y, c.y, 1e-6, SRC_Y)
        R.norm(tag + 'inv_norm', inv, c.inv, 1e-6, SRC_Y)
        R.elem(tag + 'colsum', colsum, c.colsum, c.x.double().abs().sum(1), C)
        # the forms that go through the workspace have to have run: the two-stage column sums of the stage entry point whenever there
        # is more than one channel group (hawkeye_hip.h:156, bcnn_pool.hip:333), the two-launch forward with fwd_fold = -1
        # (bcnn_pool.hip:379) - a hk_bcnn_pool_ws_bytes that is short for them silently selects the one-launch column sums
        one_launch = _panel(shape) and not generic and knobs.get('fwd_fold', 0) >= 0            # bcnn_pool.hip:373: no workspace
        if G > 1 and (staged or not one_launch):
            R.check(tag + 'column-sum partials in the workspace', not bool(torch.isnan(ws).any()), int(torch.isnan(ws).sum()))
    # backward: the saved tensors are the float64 forward rounded to float32
    bf, p = _bcnn_bwd_bufs(dev, c, shape)
    pcs = bf.inp(c.colsum.float())
    pws, nws = bf.work(lib.hk_bcnn_pool_ws_bytes(B, C, HW))
    R.call(lib, 'hk_bcnn_pool_bwd', bf, p.x, p.y, p.dy, p.inv, pcs, p.dx, B, C, HW, pws, nws)
    # the existing bound, and - the gradient being a sum of products of what the call is given - every element (bcnn_case says how)
    R.norm('bwd dx', bf.get('dx'), c.dx, 2e-5, SRC_DX)
    R.within('bwd dx per element', bf.get('dx'), c.dx, c.allowed)
    pta, ptb, ptc = bf.inp(c.ta), bf.inp(c.tb), bf.inp(c.tc)
    for tc in (ptc, None):
        bf.poison()
        tb = ptb if tc is not None else bf.inp(c.tb - c.tc)
        R.call(lib, 'hk_bcnn_pool_bwd_tdot', bf, p.x, p.y, p.dy, p.inv, pcs, pta, tb, tc, 3, p.dx, B, C, HW, pws, nws)
        R.norm('bwd_tdot dx' + ('' if tc is not None else ' (no tc)'), bf.get('dx'), c.dx3, 2e-5, SRC_DX)
        if tc is not None:
            R.within('bwd_tdot dx per element', bf.get('dx'), c.dx3, c.allowed3)
    # the two stages as a pair: tpart [B, ceil(C / 64)] is written by the first and read by the second
    bf, p = _bcnn_bwd_bufs(dev, c, shape)
    pcs, ptp = bf.inp(c.colsum.float()), bf.out('tpart', (B, G))
    R.call(lib, 'hk_bcnn_bwd_gemm', bf, p.x, p.y, p.dy, p.inv, p.dx, ptp, B, C, HW)
    tpart = bf.get('tpart')
    R.check('bwd_gemm tpart written', not bool(torch.isnan(tpart).any()))
    R.call(lib, 'hk_bcnn_bwd_rank1', bf, p.dx, ptp, p.inv, pcs, B, C, HW)
    R.norm('bwd_gemm + rank1 dx', bf.get('dx'), c.dx, 2e-5, SRC_DX)
    R.within('bwd_gemm + rank1 dx per element', bf.get('dx'), c.dx, c.allowed)
    R.done()


# ======================================================================================================================= signed sqrt
SSQRT_CASES = BCNN_CASES
SSQRT_IDS = BCNN_IDS


@functools.lru_cache(maxsize=4)
def ssqrt_case(shape):
    """Features with a sign per channel, |N(0, 1)| + 0.1: no Gram entry near zero, where the slope of sign(G) sqrt(|G| + eps) blows up
    (tests/golden/inputs.py::rs_signed_channels says why)."""
    B, C, HW = shape
    g = _gen(3, *shape)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    x = (torch.randn(B, C, HW, generator=g).abs() + 0.1) * sign[None, :, None]
    dy = torch.randn(B, C * C, generator=g)
    x64 = x.double()
    gram = (x64 @ x64.transpose(1, 2) / HW).flatten(1)
    mag = (gram.abs() + 1e-10).sqrt()
    u = torch.sign(gram) * mag
    nrm = u.norm(dim=1).clamp_min(1e-12)
    inv, y = 1.0 / nrm, u / nrm[:, None]
    t = (y * dy.double()).sum(1)
    du = inv[:, None] * (dy.double() - y * t[:, None])
    dg = torch.where(gram != 0, du / (2.0 * mag), torch.zeros_like(du)).view(B, C, C)
    dx = (dg + dg.transpose(1, 2)) @ x64 / HW
    _finite(u, y, inv, dx)
    ta, tb, tc = _tdot_operands(t, B, g)
    return Case(x=x, dy=dy, u=u, y=y, inv=inv, dx=dx, ta=ta, tb=tb, tc=tc)


def ssqrt_parts_expected(shape, generic):
    """hk_bcnn_ssqrt_pool_fwd_parts serves the panel shapes only (gram_fast_ssqrt, bcnn_fast.hip:605-614), never with bcnn_generic."""
    return 0 if _panel(shape) and not generic else HK_ERR_UNSUPPORTED


def ssqrt_forward(lib, dev, shape, R, entry, short_ws=False):
    """entry: 'fwd' (y), 'unscaled' (u), 'parts' (u, ss_part [B, 64], nparts; no inv_norm) -> dict of outputs."""
    B, C, HW = shape
    c = ssqrt_case(shape)
    bf = Bufs(dev)
    px, py = bf.inp(c.x), bf.out('y', (B, C * C), C)
    if entry == 'parts':
        pss, nparts = bf.out('ss', (B, 64)), ctypes.c_int(0)
        rc = getattr(lib, 'hk_bcnn_ssqrt_pool_fwd_parts')(px, py, pss, ctypes.byref(nparts), B, C, HW, _st(dev))
        R.check('fwd_parts: guard rows', not bf.broken(), bf.broken())
        return dict(rc=rc, y=bf.get('y'), ss=bf.get('ss'), nparts=nparts.value, untouched=bf.untouched())
    pinv = bf.out('inv', (B,))
    pws, nws = bf.work(lib.hk_bcnn_ssqrt_ws_bytes(B, C, HW))
    name = 'hk_bcnn_ssqrt_pool_fwd' if entry == 'fwd' else 'hk_bcnn_ssqrt_pool_fwd_unscaled'
    R.call(lib, name, bf, px, py, pinv, B, C, HW, pws, nws - 1 if short_ws else nws, expect=HK_ERR_WORKSPACE if short_ws else 0)
    return dict(y=bf.get('y'), inv=bf.get('inv'), untouched=bf.untouched())


def run_ssqrt(lib, dev, shape, knobs):
    B, C, HW = shape
    c = ssqrt_case(shape)
    R = Report(f'ssqrt {shape} {knobs}')
    SRC = 'tests/test_gpu_parity.py:120'
    o = ssqrt_forward(lib, dev, shape, R, 'fwd')
    R.norm('fwd y', o['y'], c.y, 2e-6, SRC)
    R.norm('fwd inv_norm', o['inv'], c.inv, 2e-6, SRC)
    o = ssqrt_forward(lib, dev, shape, R, 'unscaled')
    R.norm('fwd_unscaled u', o['y'], c.u, 2e-6, SRC)
    R.norm('fwd_unscaled inv_norm', o['inv'], c.inv, 2e-6, SRC)
    o = ssqrt_forward(lib, dev, shape, R, 'parts')
    want = ssqrt_parts_expected(shape, knobs.get('bcnn_generic', 0) == 1)
    R.check('fwd_parts: return code', o['rc'] == want, (o['rc'], want))
    if want == 0:
        n = o['nparts']
        R.check('fwd_parts: nparts in 1 .. 64', 1 <= n <= 64, n)
        R.norm('fwd_parts u', o['y'], c.u, 2e-6, SRC)
        R.norm('fwd_parts sum of ss_part', o['ss'][:, :max(n, 1)].double().sum(1), (c.u * c.u).sum(1), 2e-6, SRC)
    else:
        R.check('fwd_parts refused: nothing written', o['untouched'])
    # backward
    bf = Bufs(dev)
    px, pdy, pinv, pdx = bf.inp(c.x), bf.inp(c.dy, C), bf.inp(c.inv.float()), bf.out('dx', (B, C, HW))
    py, pu = bf.inp(c.y.float(), C), bf.inp(c.u.float(), C)
    pws, nws = bf.work(lib.hk_bcnn_ssqrt_ws_bytes(B, C, HW))
    pta, ptb, ptc = bf.inp(c.ta), bf.inp(c.tb), bf.inp(c.tc)
    for label, name, args in (('bwd', 'hk_bcnn_ssqrt_pool_bwd', (px, py, pdy, pinv, pdx)),
                              ('bwd_unscaled', 'hk_bcnn_ssqrt_pool_bwd_unscaled', (px, pu, pdy, pinv, pdx)),
                              ('bwd_tdot', 'hk_bcnn_ssqrt_pool_bwd_tdot', (px, py, pdy, pinv, pta, ptb, ptc, 3, 0, pdx)),
                              ('bwd_tdot unscaled', 'hk_bcnn_ssqrt_pool_bwd_tdot', (px, pu, pdy, pinv, pta, ptb, ptc, 3, 1, pdx))):
        bf.poison()
        R.call(lib, name, bf, *args, B, C, HW, pws, nws)
        R.norm(label + ' dx', bf.get('dx'), c.dx, 5e-5, SRC)
    R.done()


# =============================================================================================================================== MPN
# covariance, (B, C, M): the panel kernel with the means inside (gram_fast_raw with mu, bcnn_fast.hip:618-624: C % 64 == 0, M in the
# panel list) and row_mean_kernel + the generic tiles (mpn.hip:299-306); the backward alike (cov_fast_bwd, bcnn_fast.hip:721)
COV_SHAPES = [(2, 128, 196), (2, 64, 64), (2, 70, 35), (1, 5, 2)]
COV_CASES = [(s, tuple(sorted(k.items()))) for s in COV_SHAPES for k in ([dict()] + ([dict(bcnn_generic=1), dict(sched_b=200)] if _panel(s) else []))]
COV_IDS = ['x'.join(map(str, s)) + ''.join(f'-{k}{v}' for k, v in ks) for s, ks in COV_CASES]


@functools.lru_cache(maxsize=None)
def cov_case(shape):
    B, C, M = shape
    g = _gen(4, *shape)
    x = torch.relu(torch.randn(B, C, M, generator=g)) + 0.02
    dcov = torch.randn(B, C, C, generator=g)
    x64, ax = x.double(), x.double().abs()
    mu = x64.mean(2)
    xc = x64 - mu[:, :, None]
    cov = xc @ x64.transpose(1, 2) / M
    # S: (|x_im| + mean_m |x_im|) |x_jm| / M.  K = 2 M: the mean is a sum of M terms itself, and its error rides through the M-term sum
    # of the products (mu mean|x_j| <= mean|x_i| mean|x_j|, which S holds)
    S_cov = (ax + ax.mean(2, keepdim=True)) @ ax.transpose(1, 2) / M
    p64 = dcov.double() + dcov.double().transpose(1, 2)
    dx = p64 @ xc / M
    S_dx = (dcov.double().abs() + dcov.double().abs().transpose(1, 2)) @ (ax + mu.abs()[:, :, None]) / M
    _scaled(cov, S_cov), _scaled(dx, S_dx), _scaled(mu, ax.mean(2))
    return Case(x=x, dcov=dcov, mu=mu, cov=cov, S_cov=S_cov, dx=dx, S_dx=S_dx)


def run_cov(lib, dev, shape, knobs=None):
    B, C, M = shape
    c = cov_case(shape)
    R = Report(f'cov {shape} {knobs}')
    bf = Bufs(dev)
    px, pcov, pmu = bf.inp(c.x), bf.out('cov', (B, C, C)), bf.out('mu', (B, C))
    R.call(lib, 'hk_cov_pool_fwd', bf, px, pcov, pmu, B, C, M)
    R.elem('cov', bf.get('cov'), c.cov, c.S_cov, 2 * M)
    R.elem('mu', bf.get('mu'), c.mu, c.x.double().abs().mean(2), M)
    bf = Bufs(dev)
    px, pmu, pg, pdx = bf.inp(c.x), bf.inp(c.mu.float()), bf.inp(c.dcov), bf.out('dx', (B, C, M))
    R.call(lib, 'hk_cov_pool_bwd', bf, px, pmu, pg, pdx, B, C, M)
    # K = 2 C: P X and (P mu) 1^T are sums over the C channels each (the panel form subtracts the second from the first)
    R.elem('dx', bf.get('dx'), c.dx, c.S_dx, 2 * C)
    R.done()


# hk_triu_vec_fwd / _bwd: copies, exact
TRIU_CASES = [(3, 1), (2, 33), (2, 128)]


def run_triu(lib, dev, case, knobs=None):
    B, d = case
    R = Report(f'triu {case}')
    L = d * (d + 1) // 2
    x = torch.randn(B, d, d, generator=_gen(5, B, d))
    dy = torch.randn(B, L, generator=_gen(6, B, d))
    iu = torch.triu_indices(d, d)
    bf = Bufs(dev)
    px, py = bf.inp(x), bf.out('y', (B, L), d)
    R.call(lib, 'hk_triu_vec_fwd', bf, px, py, B, d)
    R.exact('fwd', bf.get('y'), x[:, iu[0], iu[1]])
    bf = Bufs(dev)
    pdy, pdx = bf.inp(dy, d), bf.out('dx', (B, d, d))
    R.call(lib, 'hk_triu_vec_bwd', bf, pdy, pdx, B, d)
    want = torch.zeros(B, d, d)
    want[:, iu[0], iu[1]] = dy
    R.exact('bwd', bf.get('dx'), want)
    R.done()


# Newton-Schulz: (d, iter_n, B, ns_tn, ns_streams, ns_sym, forward entry, backward entry).  d 128 / 256: the aligned fast path of
# hk_nsmm.h (d % 128 == 0) and the schedule of hk_ns_sqrtm_fwd_sym; 200, 70, 33: the guarded edge path (70 % 64 = 6 and 33 % 64 = 1: whole
# staged zero rows); 5: below a tile.  B = 9: the XCD-affine block map with a ragged last group.  B = 16 and 17: only from 16 samples up
# does ns_streams = 1 put the two halves of the batch on two queues (NsDispatch, mpn.hip:254: B >= 16, min(ns_streams, B / 8 - 1) helper
# queues; 17: ragged halves of 8 and 9) - each launch then carries a batch offset into ysave, zsave and the workspace; with fewer
# samples the knob changes nothing, and iter_n = 1 launches its one product unsplit (mpn.hip:354-359).  Not the full cross product: every
# value of every axis meets at least two values of every other axis (ns_axes_covered, asserted by the CPU tier).
NS_AXES = ('d', 'iter_n', 'B', 'ns_tn', 'ns_streams', 'ns_sym')
NS_CASES = [
    (128, 5, 3, 0, 1, 1, 'sym', 'bwd'),
    (128, 2, 1, 128, 0, 0, 'fwd', 'general'),
    (128, 3, 9, 64, 1, 0, 'triu_sym', 'bwd'),
    (128, 1, 3, 64, 0, 1, 'triu', 'general'),
    (256, 5, 1, 0, 0, 1, 'triu_sym', 'bwd'),
    (256, 1, 3, 64, 1, 0, 'sym', 'general'),
    (256, 2, 1, 128, 1, 1, 'fwd', 'bwd'),
    (256, 3, 9, 128, 0, 0, 'sym', 'bwd'),
    (200, 3, 1, 64, 0, 1, 'fwd', 'bwd'),
    (200, 1, 3, 0, 1, 0, 'triu', 'general'),
    (200, 2, 9, 128, 0, 0, 'sym', 'bwd'),
    (200, 5, 1, 128, 1, 1, 'triu_sym', 'general'),
    (70, 5, 9, 0, 0, 0, 'triu', 'bwd'),
    (70, 2, 3, 64, 1, 1, 'sym', 'general'),
    (70, 1, 1, 128, 1, 1, 'fwd', 'bwd'),
    (70, 3, 3, 0, 0, 0, 'triu_sym', 'general'),
    (33, 3, 9, 128, 1, 1, 'fwd', 'general'),
    (33, 5, 1, 64, 0, 0, 'sym', 'bwd'),
    (33, 1, 3, 0, 0, 1, 'triu_sym', 'bwd'),
    (33, 2, 9, 0, 1, 0, 'triu', 'general'),
    (5, 2, 9, 0, 1, 0, 'triu', 'bwd'),
    (5, 5, 3, 128, 0, 1, 'fwd', 'general'),
    (5, 3, 1, 64, 1, 0, 'sym', 'bwd'),
    (5, 1, 9, 64, 0, 1, 'triu_sym', 'general'),
    (128, 5, 16, 0, 1, 1, 'sym', 'bwd'),                  # two queues, 8 + 8, the fast path and the symmetric schedule
    (70, 2, 16, 64, 0, 0, 'triu', 'general'),             # the same batch on one queue
    (200, 2, 17, 128, 1, 0, 'fwd', 'bwd'),                # two queues, 8 + 9, the edge path
    (33, 5, 17, 0, 0, 1, 'triu_sym', 'general'),
    (70, 3, 17, 64, 1, 1, 'triu', 'general'),             # two queues: the packed triangle and the 38-product backward
    (256, 2, 16, 0, 1, 0, 'fwd', 'bwd'),
]
NS_IDS = ['d{}-it{}-b{}-tn{}-q{}-sym{}-{}-{}'.format(*c) for c in NS_CASES]


def ns_axes_covered(cases=NS_CASES):
    """[] if every value of every axis appears with at least two values of every other axis, else what is missing."""
    missing = []
    for i, a in enumerate(NS_AXES):
        for v in sorted({c[i] for c in cases}):
            for j, b in enumerate(NS_AXES):
                if i != j and len({c[j] for c in cases if c[i] == v}) < 2:
                    missing.append((a, v, b))
    return missing


def _ns_chain(a, iter_n):
    """MPNCOV.py:137-164 in the arithmetic of `a` -> out, trace, the saved iterates Y_i, Z_i [B, iter_n - 1, d, d]."""
    B, d, _ = a.shape
    eye3 = 3.0 * torch.eye(d, dtype=a.dtype).expand(B, d, d)
    tr = a.diagonal(dim1=1, dim2=2).sum(1)
    A = a / tr[:, None, None]
    zy = 0.5 * (eye3 - A)
    if iter_n < 2:
        return (A @ zy) * tr.sqrt()[:, None, None], tr, None, None
    ys, zs = [A @ zy], [zy]
    for _ in range(1, iter_n - 1):
        zy = 0.5 * (eye3 - zs[-1] @ ys[-1])
        ys.append(ys[-1] @ zy)
        zs.append(zy @ zs[-1])
    out = 0.5 * (ys[-1] @ (eye3 - zs[-1] @ ys[-1])) * tr.sqrt()[:, None, None]
    return out, tr, torch.stack(ys, 1), torch.stack(zs, 1)


@functools.lru_cache(maxsize=None)
def ns_case(d, iter_n, B):
    """a = the covariance of relu(randn) + 0.02 on a 4 x 5 map, as tests/test_emu_fuzz.py::test_fuzz_ns_variants feeds the chain (exactly
    symmetric: the _sym schedule's precondition); the upstream gradient is not symmetric."""
    g = _gen(7, d, iter_n, B)
    x = (torch.relu(torch.randn(B, d, 20, generator=g)) + 0.02).double()
    xc = x - x.mean(2, keepdim=True)
    a = xc @ xc.transpose(1, 2) / 20
    a = (0.5 * (a + a.transpose(1, 2))).float()
    a = torch.triu(a) + torch.triu(a, 1).transpose(1, 2)
    dout = torch.randn(B, d, d, generator=g)
    import hawkeye_oracle as O
    out, tr, ys, zs = _ns_chain(a.double(), iter_n)
    # the backward the kernels replace is the reference's hand-derived one (MPNCOV.py:166-202, transcribed in oracle/hawkeye_oracle.py::_Sqrtm),
    # which is autograd's gradient only for a symmetric upstream gradient: float64 through that transcription
    a64 = a.double().requires_grad_(True)
    out2 = O.sqrtm(a64, iter_n)
    assert rel(out2, out) < 1e-12
    (out2 * dout.double()).sum().backward()
    _finite(out, a64.grad)
    return Case(a=a, dout=dout, out=out, tr=tr, ys=ys, zs=zs, da=a64.grad)


def ns_forward(lib, dev, R, a, iter_n, entry, short_ws=False):
    """entry 'fwd' | 'sym' | 'triu' | 'triu_sym' -> dict(out, norm_a, ysave, zsave[, tv]) on the CPU."""
    B, d, _ = a.shape
    slots = max(iter_n - 1, 1)
    bf = Bufs(dev)
    pa, pout, pn = bf.inp(a), bf.out('out', (B, d, d)), bf.out('norm_a', (B,))
    pys, pzs = bf.out('ysave', (B, slots, d, d)), bf.out('zsave', (B, slots, d, d))
    ptv = bf.out('tv', (B, d * (d + 1) // 2), d) if entry.startswith('triu') else None
    pws, nws = bf.work(lib.hk_ns_sqrtm_ws_bytes(B, d, iter_n, 0))
    given, expect = (nws - 1, HK_ERR_WORKSPACE) if short_ws else (nws, 0)
    if entry.startswith('triu'):
        R.call(lib, 'hk_ns_sqrtm_triu_fwd', bf, pa, pout, ptv, pn, pys, pzs, B, d, iter_n, 1 if entry == 'triu_sym' else 0, pws, given, expect=expect)
    else:
        R.call(lib, 'hk_ns_sqrtm_fwd_sym' if entry == 'sym' else 'hk_ns_sqrtm_fwd', bf, pa, pout, pn, pys, pzs, B, d, iter_n, pws, given, expect=expect)
    o = {k: bf.get(k) for k in bf.outs}
    o['untouched'] = bf.untouched()
    return o


def ns_backward(lib, dev, R, a, saved, dout, iter_n, entry, short_ws=False):
    B, d, _ = a.shape
    bf = Bufs(dev)
    pa, pout, pn = bf.inp(a), bf.inp(saved['out']), bf.inp(saved['norm_a'])
    pys, pzs, pg, pda = bf.inp(saved['ysave']), bf.inp(saved['zsave']), bf.inp(dout), bf.out('da', (B, d, d))
    pws, nws = bf.work(lib.hk_ns_sqrtm_ws_bytes(B, d, iter_n, 1))
    given, expect = (nws - 1, HK_ERR_WORKSPACE) if short_ws else (nws, 0)
    R.call(lib, 'hk_ns_sqrtm_bwd_general' if entry == 'general' else 'hk_ns_sqrtm_bwd', bf, pa, pout, pn, pys, pzs, pg, pda, B, d, iter_n, pws,
           given, expect=expect)
    return bf.get('da'), bf.untouched()


def run_ns(lib, dev, case, knobs=None):
    """The knobs ns_tn, ns_streams and ns_sym are part of the case: the caller sets them (the `tune` fixture) before this runs."""
    d, iter_n, B, tn, q, sym, fwd, bwd = case
    c = ns_case(d, iter_n, B)
    R = Report(f'ns {case}')
    FWD, BWD = 'tests/test_gpu_parity.py:253', 'tests/test_gpu_parity.py:255'
    o = ns_forward(lib, dev, R, c.a, iter_n, fwd)
    R.norm('out', o['out'], c.out, 1e-5, FWD)
    R.norm('norm_a', o['norm_a'], c.tr, 1e-5, FWD)
    if iter_n >= 2:                                   # ysave / zsave: iter_n - 1 slots, all written (hawkeye_hip.h:181)
        R.norm('ysave', o['ysave'], c.ys, 1e-5, FWD)
        R.norm('zsave', o['zsave'], c.zs, 1e-5, FWD)
    if 'tv' in o:
        iu = torch.triu_indices(d, d)
        R.exact('tv = the packed upper triangle of out', o['tv'], o['out'][:, iu[0], iu[1]])
    if iter_n < 2:                                    # unused when iter_n < 2: the backward may not read them
        o['ysave'] = torch.full_like(o['ysave'], NAN)
        o['zsave'] = torch.full_like(o['zsave'], NAN)
    da, _ = ns_backward(lib, dev, R, c.a, o, c.dout, iter_n, bwd)
    R.norm('da', da, c.da, 1e-4, BWD)
    R.done()


# =============================================================================================================================== CBP
# (C, D, HW, B) and the values of cbp_bin each runs with (csrc/cbp.hip:893-911: -1 automatic, 0 row-sketch, 1 CSR gather, 2 row-scatter,
# 3 fused; a forced form that refuses the shape falls through to the next):
#   row-sketch (0): C <= 512, C % 4 == 0, nq8 <= 4, D >= 1024 nq8 (nq8 = ceil(ceil(D / 256) / 8)), emax <= 4            cbp.hip:895
#   row-scatter (2, and the automatic choice): C <= 512, C % 4 == 0, emax <= 4, its LDS <= 150 KB                        cbp.hip:897
#   fused (3, and the automatic choice): the plan has tile lists (C % 64 == 0, D + 1 <= 6144, cbp.hip:82) and HW is a panel size
#                                        (hk_cbp_fused.h:504-509)
#   else the CSR gather, cbp_bin_kernel                                                                                   cbp.hip:937
CBP_SHAPES = [
    (128, 1024, 49, 3),     # row-sketch at nq8 = 1 (D = 1024), row-scatter; HW = 49: no fused form, generic Gram
    (128, 1024, 64, 3),     # the same on a panel size: fused form, panel Gram, panel / bwd3c backward
    (64, 50, 15, 3),        # D < 1024: no row-sketch; tiny D: 82 entries per bin, emax > 4: CSR gather only
    (96, 333, 1, 2),        # one pixel, D a multiple of nothing
    (6, 7, 5, 2),           # C below a tile
    (3, 7, 4, 1),           # C % 4 != 0: only the CSR gather
    (64, 8192, 15, 2),      # D == CBP_FK * CBP_FT (cbp.hip:949, :982): the one-kernel finish and dc
    (64, 8193, 15, 2),      # D > CBP_FK * CBP_FT: partsum + norm, dot + dc
    (6, 50, 5, 2),          # D > C * C: at least 14 empty bins, exactly 0 in c_raw and y
]
# the other template instances of the binning kernels (cbp.hip:925-933), with cbp_bin -1, 0, 2 and 3
CBP_WIDE = [
    (320, 3000, 64, 2),     # C > 256: rowscatter_launch<2>, rowsketch_launch<2, 2> (nq8 = 2: D in 2049 .. 4096); five 64-blocks for the fused form
    (64, 3000, 15, 2),      # rowsketch_launch<1, 2>
    (64, 5000, 15, 2),      # rowsketch_launch<1, 3> (nq8 = 3: D in 4097 .. 6144)
]
# the other knobs at the panel shape: the generic Gram and backward; the panel backward forced; cbp_bwd3_kernel with 128-row blocks
# (cbp_bwd3_shape, bcnn_fast.hip:527-534, sees a batch of 200)
# (cbp_bwd3_shape, bcnn_fast.hip:527-534, sees a batch of 200; C = 128: 96 .. 191 give 64-row blocks, 32 .. 95 the 64-row blocks with the
# column tiles divided between two workgroups).  At C = 320 (five 64-blocks) the fused forward's work items (cbf_schedule,
# hk_cbp_fused.h:269-307) are single tiles for the real batch, runs of two tiles for a batch of 20, balanced row pairs for 200
CBP_VARIANTS = {'generic': dict(bcnn_generic=1), 'bwd_v': dict(bwd_v=1), 'sched': dict(sched_b=200), 'rows64': dict(sched_b=96),
                'colsplit': dict(sched_b=32), 'sched20': dict(sched_b=20)}
CBP_CASES = [(s, b) for s in CBP_SHAPES for b in (-1, 0, 1, 2, 3)] + [(s, b) for s in CBP_WIDE for b in (-1, 0, 2, 3)] + \
    [((128, 1024, 64, 3), -1, v) for v in ('generic', 'bwd_v', 'sched', 'rows64', 'colsplit')] + \
    [((320, 3000, 64, 2), -1, v) for v in ('sched20', 'sched')]
CBP_IDS = ['x'.join(map(str, c[0])) + f'-bin{c[1]}' + (f'-{c[2]}' if len(c) > 2 else '') for c in CBP_CASES]


def _hashes(c1, c2, d):
    import hawkeye_amd.functional as F
    return F.sketch_hashes(c1, c2, d)            # the reference's fixed count-sketch hashes (CBCNN.py:76-91), on the host


def _bins(h1, s1, h2, s2, d):
    idx = torch.from_numpy((h1[:, None].astype(np.int64) + h2[None, :]) % d).reshape(-1)
    sign = torch.from_numpy(s1[:, None].astype(np.float64) * s2[None, :]).reshape(-1)
    return idx, sign, torch.bincount(idx, minlength=d)


def _bin(m, idx, sign, d):
    """[B, C1 * C2] -> [B, D]: c_k = sum over the entries of bin k of sign * m."""
    return torch.zeros(m.shape[0], d, dtype=torch.float64).index_add_(1, idx, m * sign)


@functools.lru_cache(maxsize=None)
def cbp_case(shape):
    C, D, HW, B = shape
    g = _gen(8, *shape)
    x = torch.rand(B, C, HW, generator=g) + 0.1         # positive: bins that nearly cancel make a float32 evaluation unbounded (tests/test_gpu_parity.py:359)
    dy = torch.randn(B, D, generator=g)
    h = _hashes(C, C, D)
    idx, sign, count = _bins(*h, D)
    x64 = x.double()
    gram = (x64 @ x64.transpose(1, 2)).flatten(1)        # no 1 / HW: the sum over the locations (hawkeye_hip.h:226)
    c = _bin(gram, idx, sign, D)
    S = _bin(gram.abs(), idx, torch.ones_like(sign), D)
    mag = (c.abs() + 1e-10).sqrt()
    u = torch.where(c != 0, torch.sign(c) * mag, torch.zeros_like(c))
    nrm = u.norm(dim=1).clamp_min(1e-12)
    y, inv = u / nrm[:, None], 1.0 / nrm
    t = (y * dy.double()).sum(1)
    dc = torch.where(c != 0, inv[:, None] * (dy.double() - y * t[:, None]) / (2.0 * mag), torch.zeros_like(c))
    dg = (dc[:, idx] * sign).view(B, C, C)
    dx = (dg + dg.transpose(1, 2)) @ x64
    _scaled(c, S), _finite(y, inv, dx)
    return Case(x=x, dy=dy, h=h, count=count, c=c, S=S, y=y, inv=inv, dx=dx)


class Plan:
    """A plan blob between guard bytes; one width: hk_cbp_plan_build, else hk_cbp_rect_plan_build.  close() makes the library forget the
    address (hawkeye_hip.h:239) before the memory goes back to the allocator."""

    def __init__(self, lib, dev, h, d, square):
        h1, s1, h2, s2 = (np.ascontiguousarray(v) for v in h)
        self.lib, self.square = lib, square
        n = lib.hk_cbp_plan_bytes(len(h1), d) if square else lib.hk_cbp_rect_plan_bytes(len(h1), len(h2), d)
        self.g = Guarded(n, torch.uint8, dev, 4096)
        self.g.inner.fill_(0xFF)
        hp = lambda v: ctypes.c_void_p(v.ctypes.data)
        if square:
            self.rc = lib.hk_cbp_plan_build(hp(h1), hp(s1), hp(h2), hp(s2), len(h1), d, _p(self.g.inner), _st(dev))
        else:
            self.rc = lib.hk_cbp_rect_plan_build(hp(h1), hp(s1), len(h1), hp(h2), hp(s2), len(h2), d, _p(self.g.inner), _st(dev))
        self.ptr = _p(self.g.inner)

    def close(self):
        if self.square:
            self.lib.hk_cbp_plan_destroy(self.ptr)


def cbp_forward(lib, dev, shape, R, short_ws=False):
    C, D, HW, B = shape
    c = cbp_case(shape)
    plan = Plan(lib, dev, c.h, D, True)
    R.check('plan build', plan.rc == 0 and plan.g.intact(), plan.rc)
    bf = Bufs(dev)
    px, py, pc, pinv = bf.inp(c.x), bf.out('y', (B, D)), bf.out('c_raw', (B, D)), bf.out('inv', (B,))
    pws, nws = bf.work(lib.hk_cbp_ws_bytes(B, C, HW, D))
    given, expect = (nws - 1, HK_ERR_WORKSPACE) if short_ws else (nws, 0)
    R.call(lib, 'hk_cbp_fwd', bf, px, plan.ptr, py, pc, pinv, B, C, HW, D, pws, given, expect=expect)
    o = dict(y=bf.get('y'), c_raw=bf.get('c_raw'), inv=bf.get('inv'), untouched=bf.untouched())
    R.check('plan intact', plan.g.intact())
    plan.close()
    return o


def cbp_backward(lib, dev, shape, R):
    """hk_cbp_bwd on the float64 forward rounded to float32 -> dx."""
    C, D, HW, B = shape
    c = cbp_case(shape)
    plan = Plan(lib, dev, c.h, D, True)
    bf = Bufs(dev)
    px, py, pc, pinv = bf.inp(c.x), bf.inp(c.y.float()), bf.inp(c.c.float()), bf.inp(c.inv.float())
    pdy, pdx = bf.inp(c.dy), bf.out('dx', (B, C, HW))
    pws, nws = bf.work(lib.hk_cbp_ws_bytes(B, C, HW, D))
    R.call(lib, 'hk_cbp_bwd', bf, px, plan.ptr, py, pc, pinv, pdy, pdx, B, C, HW, D, pws, nws)
    R.check('plan intact', plan.g.intact())
    plan.close()
    return bf.get('dx')


def run_cbp(lib, dev, case, knobs=None):
    """cbp_bin (case[1]) and the variant's knob are set by the caller."""
    shape = case[0]
    C, D, HW, B = shape
    c = cbp_case(shape)
    R = Report(f'cbp {case}')
    o = cbp_forward(lib, dev, shape, R)
    # K per bin: HW terms per Gram entry times the entries of the bin, as one flat sum - the forms split it differently (row chunks,
    # tiles, work items) and add the partial vectors in a fixed order; the flat count bounds every split
    R.elem('c_raw', o['c_raw'], c.c, c.S, (c.count * HW).expand(B, D))
    R.norm('y', o['y'], c.y, 1e-5, 'tests/test_gpu_parity.py:365')
    R.norm('inv_norm', o['inv'], c.inv, 1e-5, 'tests/test_gpu_parity.py:365')
    empty = (c.count == 0).expand(B, D)
    R.check('empty bins exactly 0', bool((o['c_raw'][empty] == 0).all()) and bool((o['y'][empty] == 0).all()))
    R.norm('dx', cbp_backward(lib, dev, shape, R), c.dx, 1e-4, 'tests/test_gpu_parity.py:367')
    R.done()


# two inputs, (C1, C2, D, HW, B): cbp_bin_kernel, cbp_unbin_kernel, cbp_loc_fwd_kernel, cbp_loc_bwd_kernel (cbp.hip:764-805), one form each
RECT_CASES = [(24, 16, 64, 15, 2), (5, 3, 7, 1, 1), (70, 33, 129, 6, 2),
              (16, 16, 300, 4, 2)]        # D > C1 C2: empty bins
RECT_LDS_FLOATS = 144 * 1024 // 4         # hk_cbp_rect_loc_bwd holds D + 2 (C1 + C2) floats of a location in LDS (cbp.hip:147, :797-798)


@functools.lru_cache(maxsize=None)
def rect_case(shape):
    C1, C2, D, HW, B = shape
    g = _gen(9, *shape)
    x1, x2 = torch.randn(B, C1, HW, generator=g), torch.randn(B, C2, HW, generator=g)
    G, dcs = torch.randn(B, C1, C2, generator=g), torch.randn(B, D, generator=g)
    dcl = torch.randn(B, HW, D, generator=g)
    h = _hashes(C1, C2, D)
    idx, sign, count = _bins(*h, D)
    ones = torch.ones_like(sign)
    c_bin, S_bin = _bin(G.double().flatten(1), idx, sign, D), _bin(G.double().abs().flatten(1), idx, ones, D)
    dG = (dcs.double()[:, idx] * sign).view(B, C1, C2)
    outer = (x1.double().transpose(1, 2)[:, :, :, None] * x2.double().transpose(1, 2)[:, :, None, :]).reshape(B * HW, C1 * C2)
    c_loc, S_loc = _bin(outer, idx, sign, D).view(B, HW, D), _bin(outer.abs(), idx, ones, D).view(B, HW, D)
    dgl = (dcl.double().reshape(B * HW, D)[:, idx] * sign).view(B, HW, C1, C2)          # d c / d (x1_i x2_j) per location
    agl = dcl.double().abs().reshape(B * HW, D)[:, idx].view(B, HW, C1, C2)
    x1t, x2t = x1.double().transpose(1, 2), x2.double().transpose(1, 2)                  # [B, HW, C]
    dx1 = torch.einsum('bpij,bpj->bip', dgl, x2t)
    dx2 = torch.einsum('bpij,bpi->bjp', dgl, x1t)
    S1 = torch.einsum('bpij,bpj->bip', agl, x2t.abs())
    S2 = torch.einsum('bpij,bpi->bjp', agl, x1t.abs())
    for r, s in ((c_bin, S_bin), (c_loc, S_loc), (dx1, S1), (dx2, S2)):
        _scaled(r, s)
    return Case(x1=x1, x2=x2, G=G, dcs=dcs, dcl=dcl, h=h, count=count, c_bin=c_bin, S_bin=S_bin, dG=dG, c_loc=c_loc, S_loc=S_loc, dx1=dx1,
                dx2=dx2, S1=S1, S2=S2)


def run_rect(lib, dev, shape, knobs=None):
    C1, C2, D, HW, B = shape
    c = rect_case(shape)
    R = Report(f'cbp rect {shape}')
    plan = Plan(lib, dev, c.h, D, False)
    R.check('plan build', plan.rc == 0 and plan.g.intact(), plan.rc)
    bf = Bufs(dev)
    pG, pc = bf.inp(c.G), bf.out('c', (B, D))
    R.call(lib, 'hk_cbp_rect_bin_matrix', bf, pG, plan.ptr, pc, B, C1, C2, D)
    got = bf.get('c')
    R.elem('bin_matrix', got, c.c_bin, c.S_bin, c.count.expand(B, D))
    R.check('bin_matrix: empty bins exactly 0', bool((got[(c.count == 0).expand(B, D)] == 0).all()))
    bf = Bufs(dev)
    pdc, pdG = bf.inp(c.dcs), bf.out('dG', (B, C1, C2))
    R.call(lib, 'hk_cbp_rect_unbin_matrix', bf, pdc, plan.ptr, pdG, B, C1, C2, D)
    R.elem('unbin_matrix', bf.get('dG'), c.dG, c.dG.abs(), 1)
    bf = Bufs(dev)
    p1, p2, pcl = bf.inp(c.x1), bf.inp(c.x2), bf.out('c', (B, HW, D))
    R.call(lib, 'hk_cbp_rect_loc_fwd', bf, p1, p2, plan.ptr, pcl, B, C1, C2, HW, D)
    R.elem('loc_fwd', bf.get('c'), c.c_loc, c.S_loc, c.count.expand(B, HW, D))
    bf = Bufs(dev)
    p1, p2, pdc = bf.inp(c.x1), bf.inp(c.x2), bf.inp(c.dcl)
    pd1, pd2 = bf.out('dx1', (B, C1, HW)), bf.out('dx2', (B, C2, HW))
    for a1, a2 in ((pd1, pd2), (pd1, None), (None, pd2)):          # either gradient nullable (hawkeye_hip.h:265)
        bf.poison()
        R.call(lib, 'hk_cbp_rect_loc_bwd', bf, p1, p2, pdc, plan.ptr, a1, a2, B, C1, C2, HW, D)
        tag = 'loc_bwd' + ('' if a1 and a2 else ' (dx1 only)' if a1 else ' (dx2 only)')
        if a1:
            R.elem(tag + ' dx1', bf.get('dx1'), c.dx1, c.S1, C2)
        else:
            R.check(tag + ': dx1 not written', bool(torch.isnan(bf.get('dx1')).all()))
        if a2:
            R.elem(tag + ' dx2', bf.get('dx2'), c.dx2, c.S2, C1)
        else:
            R.check(tag + ': dx2 not written', bool(torch.isnan(bf.get('dx2')).all()))
    R.check('plan intact', plan.g.intact())
    R.done()


def run_rect_lds_limit(lib, dev, knobs=None):
    """hk_cbp_rect_loc_bwd at the largest D its LDS holds, and at D + 1: refused with HK_ERR_UNSUPPORTED, nothing written."""
    C1, C2, HW, B = 5, 3, 1, 1
    dmax = RECT_LDS_FLOATS - 2 * (C1 + C2)
    R = Report('cbp rect loc_bwd at the LDS limit')
    for D, want in ((dmax, 0), (dmax + 1, HK_ERR_UNSUPPORTED)):
        g = _gen(10, D)
        x1, x2, dc = torch.randn(B, C1, HW, generator=g), torch.randn(B, C2, HW, generator=g), torch.randn(B, HW, D, generator=g)
        h = _hashes(C1, C2, D)
        idx, sign, _ = _bins(*h, D)
        dgl = (dc.double().reshape(B * HW, D)[:, idx] * sign).view(B, HW, C1, C2)
        agl = dgl.abs()
        plan = Plan(lib, dev, h, D, False)
        bf = Bufs(dev)
        p1, p2, pdc = bf.inp(x1), bf.inp(x2), bf.inp(dc)
        pd1, pd2 = bf.out('dx1', (B, C1, HW)), bf.out('dx2', (B, C2, HW))
        R.call(lib, 'hk_cbp_rect_loc_bwd', bf, p1, p2, pdc, plan.ptr, pd1, pd2, B, C1, C2, HW, D, expect=want)
        if want == 0:
            x1t, x2t = x1.double().transpose(1, 2), x2.double().transpose(1, 2)
            R.elem(f'D = {D} dx1', bf.get('dx1'), torch.einsum('bpij,bpj->bip', dgl, x2t), torch.einsum('bpij,bpj->bip', agl, x2t.abs()), C2)
            R.elem(f'D = {D} dx2', bf.get('dx2'), torch.einsum('bpij,bpi->bjp', dgl, x1t), torch.einsum('bpij,bpi->bjp', agl, x1t.abs()), C1)
        else:
            R.check(f'D = {D}: nothing written', bf.untouched())
    R.done()


# ======================================================================================================================== classifier
# (B, J, K, linear_slabs, bias) (csrc/linear.hip):
LINEAR_CASES = [
    (3, 1000, 7, 0, True),        # J / 32 = 31 chunks < 128: the generic split-K tiles (linear.hip:173, :241-248)
    (3, 1000, 7, 0, False),
    (5, 333, 130, 0, True),       # J % 4 != 0: generic tiles with scalar loads (linear.hip:158, :242)
    (5, 333, 130, 0, False),
    (3, 112, 13, 2, True),        # J % 32 = 16: a forced slab count takes linear_skinny_kernel (linear.hip:173, :178) and the tail of
                                  #   linear_reduce_kernel (:235-237); backward: J < 4096, the generic tiles with J % 64 = 48 (:353)
    (3, 4144, 13, 0, True),       # J % 32 = 16 and J % 64 = 48 at J >= 4096, where the two tail kernels run by themselves: 129 chunks, the
                                  #   skinny forward with its tail, linear_bwd64_kernel + linear_bwd_tail_kernel (linear.hip:284, :306)
    (10, 640, 96, 1, True),       # forced slab counts: one slab,
    (10, 640, 96, 4, True),       #   four slabs of five chunks,
    (10, 640, 96, 5, False),      #   five slabs of four
    (2, 16384, 256, 0, True),     # the direct backward, linear_bwd16_kernel: B <= 16, 256 <= K <= 1024, J % 64 == 0, J >= 16384 (linear.hip:318)
    (33, 16448, 208, 0, True),    # linear_bwd64_kernel with 52 class steps, 257 chunks on 129 workgroups; the single products (linear.hip:298)
    (33, 16448, 208, -1, False),  # linear_slabs = -1: the generic tiles at that shape (linear.hip:157, :286)
    (3, 4160, 200, 0, True),      # K = 197 .. 200: linear_bwd64_kernel with 50 class steps (linear.hip:290), the 200-class classifiers
    (33, 4096, 250, 0, True),     # B >= 33 and K > 208: linear_skinny_kernel<15, 4>, two class groups (linear.hip:163-166)
]
LINEAR_IDS = ['x'.join(map(str, c[:3])) + f'-slabs{c[3]}' + ('' if c[4] else '-nobias') for c in LINEAR_CASES]


@functools.lru_cache(maxsize=2)
def linear_case(B, J, K):
    g = _gen(11, B, J, K)
    y = torch.randn(B, J, generator=g)
    w = torch.randn(K, J, generator=g) / J ** 0.5
    bias, gr = torch.randn(K, generator=g), torch.randn(B, K, generator=g)
    scale = torch.rand(B, generator=g) + 0.5
    y64, w64, g64 = y.double(), w.double(), gr.double()
    prod, S = y64 @ w64.t(), y64.abs() @ w64.abs().t()
    dy, S_dy = g64 @ w64, g64.abs() @ w64.abs()
    dw, S_dw = g64.t() @ y64, g64.abs().t() @ y64.abs()
    gs = g64 * scale.double()[:, None]
    dws, S_dws = gs.t() @ y64, gs.abs().t() @ y64.abs()
    db, S_db = g64.sum(0), g64.abs().sum(0)
    for r, s in ((prod, S), (dy, S_dy), (dw, S_dw), (dws, S_dws), (db, S_db)):
        _scaled(r, s)
    return Case(y=y, w=w, bias=bias, g=gr, scale=scale, prod=prod, S=S, dy=dy, S_dy=S_dy, dw=dw, S_dw=S_dw, dws=dws, S_dws=S_dws, db=db, S_db=S_db)


def linear_bwd_scaled_expected(B, J, K, slabs):
    """hk_linear_bwd_scaled is served by linear_bwd64_kernel only (linear.hip:284-286, :316)."""
    return 0 if B <= 64 and K <= 208 and J % 4 == 0 and J >= 4096 and slabs >= 0 else HK_ERR_UNSUPPORTED


def linear_forward(lib, dev, R, case, entry, short_ws=False):
    """entry 'fwd' | 'scaled' | 'ssq' -> dict(out[, inv])."""
    B, J, K, slabs, has_bias = case
    c = linear_case(B, J, K)
    bf = Bufs(dev)
    py, pw, pb = bf.inp(c.y), bf.inp(c.w), bf.inp(c.bias) if has_bias else None
    pout = bf.out('out', (B, K))
    pws, nws = bf.work(lib.hk_linear_ws_bytes(B, J, K))
    given, expect = (nws - 1, HK_ERR_WORKSPACE) if short_ws else (nws, 0)
    if entry == 'fwd':
        R.call(lib, 'hk_linear_fwd', bf, py, pw, pb, pout, B, J, K, pws, given, expect=expect)
    elif entry == 'scaled':
        R.call(lib, 'hk_linear_fwd_scaled', bf, py, pw, pb, bf.inp(c.scale), pout, B, J, K, pws, given, expect=expect)
    else:
        ss = torch.zeros(B, 64)
        ss[:, :3] = (c.y.double() ** 2).sum(1, keepdim=True).float() * torch.tensor([0.5, 0.3, 0.2])
        ss[:, 3:] = 1e30                                          # past nparts: never read
        pinv = bf.out('inv', (B,))
        R.call(lib, 'hk_linear_fwd_ssq', bf, py, pw, pb, bf.inp(ss), 3, pinv, pout, B, J, K, pws, given, expect=expect)
    o = {k: bf.get(k) for k in bf.outs}
    o['untouched'] = bf.untouched()
    return o


def linear_backward(lib, dev, R, case, want, scaled=False, expect=0):
    """want: a subset of 'ywb' -> dict(dy, dw, db), None where not asked for (a NULL pointer: skipped, hawkeye_hip.h:439)."""
    B, J, K, slabs, has_bias = case
    c = linear_case(B, J, K)
    bf = Bufs(dev)
    py, pw, pg = bf.inp(c.y), bf.inp(c.w), bf.inp(c.g)
    pdy = bf.out('dy', (B, J)) if 'y' in want else None
    pdw = bf.out('dw', (K, J)) if 'w' in want else None
    pdb = bf.out('db', (K,)) if 'b' in want else None
    if scaled:
        R.call(lib, 'hk_linear_bwd_scaled', bf, py, pw, pg, bf.inp(c.scale), pdy, pdw, pdb, B, J, K, expect=expect)
    else:
        R.call(lib, 'hk_linear_bwd', bf, py, pw, pg, pdy, pdw, pdb, B, J, K, expect=expect)
    o = {k: bf.get(k) for k in bf.outs}
    o['untouched'] = bf.untouched()
    return o


def run_linear(lib, dev, case, knobs=None):
    """linear_slabs (case[3]) is set by the caller."""
    B, J, K, slabs, has_bias = case
    c = linear_case(B, J, K)
    R = Report(f'linear {case}')
    b64 = c.bias.double() if has_bias else torch.zeros(K, dtype=torch.float64)
    o = linear_forward(lib, dev, R, case, 'fwd')
    R.elem('fwd', o['out'], c.prod + b64, c.S + b64.abs(), J)
    o = linear_forward(lib, dev, R, case, 'scaled')
    sc = c.scale.double()[:, None]
    R.elem('fwd_scaled', o['out'], sc * c.prod + b64, sc * c.S + b64.abs(), J)
    o = linear_forward(lib, dev, R, case, 'ssq')
    inv = 1.0 / (c.y.double() ** 2).sum(1).sqrt()
    R.norm('fwd_ssq inv_norm', o['inv'], inv, 1e-5, 'tests/test_gpu_kernels.py:1005')
    R.norm('fwd_ssq out', o['out'], inv[:, None] * c.prod + b64, 1e-5, 'tests/test_gpu_kernels.py:1005')
    for want in ('ywb', 'wb', 'yb', 'yw'):                       # all three, then each of dy, dw, db NULL in turn
        o = linear_backward(lib, dev, R, case, want)
        tag = f'bwd[{want}] '
        if 'y' in want:
            R.elem(tag + 'dy', o['dy'], c.dy, c.S_dy, K)
        if 'w' in want:
            R.elem(tag + 'dw', o['dw'], c.dw, c.S_dw, B)
        if 'b' in want:
            R.elem(tag + 'db', o['db'], c.db, c.S_db, B)
    want_rc = linear_bwd_scaled_expected(B, J, K, slabs)
    o = linear_backward(lib, dev, R, case, 'ywb', scaled=True, expect=want_rc)
    if want_rc == 0:
        R.elem('bwd_scaled dy', o['dy'], c.dy, c.S_dy, K)
        R.elem('bwd_scaled dw', o['dw'], c.dws, c.S_dws, B)
        R.elem('bwd_scaled db', o['db'], c.db, c.S_db, B)
    else:
        R.check('bwd_scaled refused: nothing written', o['untouched'])
    R.done()


# =============================================================================================================================== CIN
# (B, C, HW) (csrc/cin.hip:1049-1178): the one-kernel forms at HW in {49, 64, 36} and C % 64 == 0 (cin.hip:680-686, :528-539, :666-672);
# the stored-score forms at HW in {196, 144, 100} and C % 128 == 0 (cin_ax_covers, cin.hip:1006); the generic chains elsewhere, and
# everywhere with bcnn_generic = 1 for the forward (cin.hip:1052) and the stored backward (:1093)
CIN_SHAPES = [(2, 64, 49), (2, 128, 64), (2, 64, 36), (2, 128, 196), (2, 128, 144), (2, 256, 100), (2, 70, 5), (4, 24, 12),
              (2, 512, 100)]       # cin_row_stats_kernel<2> (cin.hip:1032); <4> and <8> need C = 1024 and 2048: not run here
CIN_CASES = [(s, g) for s in CIN_SHAPES for g in ((0, 1) if s[1] % 64 == 0 else (0,))]
CIN_IDS = ['x'.join(map(str, s)) + ('-generic' if g else '') for s, g in CIN_CASES]


@functools.lru_cache(maxsize=None)
def cin_case(shape):
    B, C, HW = shape
    g = _gen(12, *shape)
    x = torch.relu(torch.randn(B, C, HW, generator=g))
    wt = torch.randn(B, generator=g) * 0.7
    g1, g2, ge = torch.randn(B, C, HW, generator=g), torch.randn(B, C, HW, generator=g), torch.randn(B, C, C, generator=g) * 0.1
    sci = lambda t: torch.softmax(-(t @ t.transpose(1, 2)) / HW, dim=2)
    # SCI alone, and with an extra gradient reaching W
    xr = x.double().requires_grad_(True)
    w = sci(xr)
    y = w @ xr
    dx_plain, = torch.autograd.grad((y * g1.double()).sum(), xr, retain_graph=True)
    dx_extra, = torch.autograd.grad((y * g1.double()).sum() + (w * ge.double()).sum(), xr)
    # CCI on the float32 W the kernel is given (an input of its own there)
    w32 = w.detach().float()
    xc, wc, wtc = x.double().requires_grad_(True), w32.double().requires_grad_(True), wt.double().requires_grad_(True)
    yc = torch.abs(wc - wtc.view(-1, 1, 1) * torch.cat((wc[B // 2:], wc[:B // 2]), 0)) @ xc
    dxc, dwc, dwtc = torch.autograd.grad((yc * g2.double()).sum(), (xc, wc, wtc))
    _finite(w, y, dx_plain, dx_extra, yc, dxc, dwc, dwtc)
    return Case(x=x, wt=wt, g1=g1, g2=g2, ge=ge, w=w.detach(), y=y.detach(), dx_plain=dx_plain, dx_extra=dx_extra, w32=w32, yc=yc.detach(),
                dxc=dxc, dwc=dwc, dwtc=dwtc)


def cin_cci_backward(lib, dev, R, shape, short_ws=False):
    B, C, HW = shape
    c = cin_case(shape)
    bf = Bufs(dev)
    px, pw, pwt, pdy = bf.inp(c.x), bf.inp(c.w32), bf.inp(c.wt), bf.inp(c.g2)
    pdx, pdw, pdwt = bf.out('dx', (B, C, HW)), bf.out('dw', (B, C, C)), bf.out('dwt', (B,))
    pws, nws = bf.work(lib.hk_cin_cci_ws_bytes(B, C))
    given, expect = (nws - 1, HK_ERR_WORKSPACE) if short_ws else (nws, 0)
    R.call(lib, 'hk_cin_cci_bwd', bf, px, pw, pwt, pdy, pdx, pdw, pdwt, B, C, HW, pws, given, expect=expect)
    o = {k: bf.get(k) for k in bf.outs}
    o['untouched'] = bf.untouched()
    return o


def run_cin(lib, dev, case, knobs=None):
    """bcnn_generic (case[1]) is set by the caller."""
    shape = case[0]
    B, C, HW = shape
    c = cin_case(shape)
    R = Report(f'cin {case}')
    FWD, CCI, BWD = 'tests/test_gpu_kernels.py:764 (2e-6)', 'tests/test_gpu_kernels.py:764 (5e-6)', 'tests/test_gpu_kernels.py:765'
    bf = Bufs(dev)
    px, pw, py = bf.inp(c.x), bf.out('w', (B, C, C)), bf.out('y', (B, C, HW))
    R.call(lib, 'hk_cin_sci_fwd', bf, px, pw, py, B, C, HW)
    R.norm('sci w', bf.get('w'), c.w, 2e-6, FWD)
    R.norm('sci y', bf.get('y'), c.y, 2e-6, FWD)
    for extra in (0, 1):
        bf = Bufs(dev)
        px, pw, pdy, pdx = bf.inp(c.x), bf.inp(c.w32), bf.inp(c.g1), bf.out('dx', (B, C, HW))
        pbuf = bf.inout('dwbuf', c.ge) if extra else bf.out('dwbuf', (B, C, C))     # has_extra = 0: scratch, NaN on entry - may not be read
        R.call(lib, 'hk_cin_sci_bwd', bf, px, pw, pdy, pbuf, extra, pdx, B, C, HW)
        R.norm(f'sci bwd dx (has_extra {extra})', bf.get('dx'), c.dx_extra if extra else c.dx_plain, 2e-5, BWD)
    bf = Bufs(dev)
    px, pw, pwt, py = bf.inp(c.x), bf.inp(c.w32), bf.inp(c.wt), bf.out('y', (B, C, HW))
    R.call(lib, 'hk_cin_cci_fwd', bf, px, pw, pwt, py, B, C, HW)
    R.norm('cci y', bf.get('y'), c.yc, 5e-6, CCI)
    o = cin_cci_backward(lib, dev, R, shape)
    R.norm('cci bwd dx', o['dx'], c.dxc, 2e-5, BWD)
    R.norm('cci bwd dw', o['dw'], c.dwc, 2e-5, BWD)
    R.norm('cci bwd dwt', o['dwt'], c.dwtc, 2e-5, BWD)
    R.done()


# ================================================================================================================ runners by entry point
# every entry point of the families above and the runner that reaches it (tests/test_emu_core_guarded.py checks hawkeye_amd._lib.SIGNATURES
# against this table)
FAMILIES = ('hk_bcnn_', 'hk_cov_', 'hk_ns_', 'hk_triu_', 'hk_cbp_', 'hk_linear_', 'hk_cin_', 'hk_bgemm_')
RUNNERS = {
    'hk_bcnn_pool_fwd': run_bcnn, 'hk_bcnn_pool_bwd': run_bcnn, 'hk_bcnn_pool_bwd_tdot': run_bcnn, 'hk_bcnn_colsum_norm': run_bcnn,
    'hk_bcnn_gram_norm': run_bcnn, 'hk_bcnn_bwd_gemm': run_bcnn, 'hk_bcnn_bwd_rank1': run_bcnn,
    'hk_bcnn_ssqrt_pool_fwd': run_ssqrt, 'hk_bcnn_ssqrt_pool_fwd_unscaled': run_ssqrt, 'hk_bcnn_ssqrt_pool_fwd_parts': run_ssqrt,
    'hk_bcnn_ssqrt_pool_bwd': run_ssqrt, 'hk_bcnn_ssqrt_pool_bwd_unscaled': run_ssqrt, 'hk_bcnn_ssqrt_pool_bwd_tdot': run_ssqrt,
    'hk_cov_pool_fwd': run_cov, 'hk_cov_pool_bwd': run_cov,
    'hk_ns_sqrtm_fwd': run_ns, 'hk_ns_sqrtm_fwd_sym': run_ns, 'hk_ns_sqrtm_triu_fwd': run_ns, 'hk_ns_sqrtm_bwd': run_ns,
    'hk_ns_sqrtm_bwd_general': run_ns,
    'hk_triu_vec_fwd': run_triu, 'hk_triu_vec_bwd': run_triu,
    'hk_cbp_fwd': run_cbp, 'hk_cbp_bwd': run_cbp,
    'hk_cbp_rect_bin_matrix': run_rect, 'hk_cbp_rect_unbin_matrix': run_rect, 'hk_cbp_rect_loc_fwd': run_rect, 'hk_cbp_rect_loc_bwd': run_rect,
    'hk_linear_fwd': run_linear, 'hk_linear_fwd_scaled': run_linear, 'hk_linear_fwd_ssq': run_linear, 'hk_linear_bwd': run_linear,
    'hk_linear_bwd_scaled': run_linear,
    'hk_cin_sci_fwd': run_cin, 'hk_cin_sci_bwd': run_cin, 'hk_cin_cci_fwd': run_cin, 'hk_cin_cci_bwd': run_cin,
    'hk_bgemm_f32': run_bgemm,
}


def is_helper(name):
    """Size, plan-build and plan-destroy helpers: no kernel of their own to guard (the runners call them)."""
    return name.endswith('_bytes') or name.endswith('_plan_build') or name.endswith('_plan_destroy')


# =========================================================================================================================== refusals
def run_refusals(lib, dev, tune):
    """Every entry point that requires a workspace, given one byte less than hk_*_ws_bytes: HK_ERR_WORKSPACE, every guard intact, every
    output still NaN, the workspace still 0xFF.  hk_bcnn_pool_fwd and hk_bcnn_colsum_norm are not among them: their workspace is
    optional by contract (hawkeye_hip.h:156, tests/test_abi_errors_cpu.py:20-21, tests/test_gpu_kernels.py:961-964) - one too short
    for the column-sum partials, or none, selects the one-launch column sums; for them, with one byte less than the partials need and
    with a NULL workspace, in the stage entry point and in both forms of the forward: success, the right result, every guard intact,
    the workspace still 0xFF.  `tune(name, value)`: the conftest fixture."""
    R = Report('refusals')
    shape = (2, 128, 64)
    cb = bcnn_case(shape)
    for label, staged, fold, short in (('colsum_norm, short', True, 0, 'short'), ('colsum_norm, none', True, 0, 'null'),
                                       ('pool_fwd in two launches, short', False, -1, 'short'), ('pool_fwd in two launches, none', False, -1, 'null'),
                                       ('pool_fwd in one launch, short', False, 0, 'short'), ('pool_fwd in one launch, none', False, 0, 'null')):
        tune('fwd_fold', fold)
        y, inv, colsum, ws = bcnn_forward(lib, dev, shape, R, staged, short_ws=short)
        R.norm(f'{label}: y', y, cb.y, 1e-6, 'tests/test_gpu_parity.py:180')
        R.norm(f'{label}: inv_norm', inv, cb.inv, 1e-6, 'tests/test_gpu_parity.py:180')
        R.elem(f'{label}: colsum', colsum, cb.colsum, cb.x.double().abs().sum(1), shape[1])
    tune('fwd_fold', 0)
    # BCNN backward
    B, C, HW = shape
    bf, p = _bcnn_bwd_bufs(dev, cb, shape)
    pcs, pta, ptb, ptc = bf.inp(cb.colsum.float()), bf.inp(cb.ta), bf.inp(cb.tb), bf.inp(cb.tc)
    pws, nws = bf.work(lib.hk_bcnn_pool_ws_bytes(B, C, HW))
    R.call(lib, 'hk_bcnn_pool_bwd', bf, p.x, p.y, p.dy, p.inv, pcs, p.dx, B, C, HW, pws, nws - 1, expect=HK_ERR_WORKSPACE)
    R.check('hk_bcnn_pool_bwd: nothing written', bf.untouched())
    R.call(lib, 'hk_bcnn_pool_bwd_tdot', bf, p.x, p.y, p.dy, p.inv, pcs, pta, ptb, ptc, 3, p.dx, B, C, HW, pws, nws - 1, expect=HK_ERR_WORKSPACE)
    R.check('hk_bcnn_pool_bwd_tdot: nothing written', bf.untouched())
    # signed sqrt
    for entry in ('fwd', 'unscaled'):
        R.check(f'ssqrt {entry}: nothing written', ssqrt_forward(lib, dev, shape, R, entry, short_ws=True)['untouched'])
    cs = ssqrt_case(shape)
    bf = Bufs(dev)
    px, py, pdy, pinv, pdx = bf.inp(cs.x), bf.inp(cs.y.float(), C), bf.inp(cs.dy, C), bf.inp(cs.inv.float()), bf.out('dx', (B, C, HW))
    pta, ptb, ptc = bf.inp(cs.ta), bf.inp(cs.tb), bf.inp(cs.tc)
    pws, nws = bf.work(lib.hk_bcnn_ssqrt_ws_bytes(B, C, HW))
    for name, args in (('hk_bcnn_ssqrt_pool_bwd', (px, py, pdy, pinv, pdx)), ('hk_bcnn_ssqrt_pool_bwd_unscaled', (px, py, pdy, pinv, pdx)),
                       ('hk_bcnn_ssqrt_pool_bwd_tdot', (px, py, pdy, pinv, pta, ptb, ptc, 3, 0, pdx))):
        R.call(lib, name, bf, *args, B, C, HW, pws, nws - 1, expect=HK_ERR_WORKSPACE)
        R.check(f'{name}: nothing written', bf.untouched())
    # Newton-Schulz
    cn = ns_case(33, 3, 3)
    for entry in ('fwd', 'sym', 'triu'):
        R.check(f'ns {entry}: nothing written', ns_forward(lib, dev, R, cn.a, 3, entry, short_ws=True)['untouched'])
    saved = dict(out=cn.out.float(), norm_a=cn.tr.float(), ysave=cn.ys.float(), zsave=cn.zs.float())
    for entry in ('bwd', 'general'):
        R.check(f'ns {entry}: nothing written', ns_backward(lib, dev, R, cn.a, saved, cn.dout, 3, entry, short_ws=True)[1])
    # CBP
    cshape = (6, 7, 5, 2)
    R.check('cbp fwd: nothing written', cbp_forward(lib, dev, cshape, R, short_ws=True)['untouched'])
    cc = cbp_case(cshape)
    Cc, D, HWc, Bc = cshape
    plan = Plan(lib, dev, cc.h, D, True)
    bf = Bufs(dev)
    px, py, pc, pinv = bf.inp(cc.x), bf.inp(cc.y.float()), bf.inp(cc.c.float()), bf.inp(cc.inv.float())
    pdy, pdx = bf.inp(cc.dy), bf.out('dx', (Bc, Cc, HWc))
    pws, nws = bf.work(lib.hk_cbp_ws_bytes(Bc, Cc, HWc, D))
    R.call(lib, 'hk_cbp_bwd', bf, px, plan.ptr, py, pc, pinv, pdy, pdx, Bc, Cc, HWc, D, pws, nws - 1, expect=HK_ERR_WORKSPACE)
    R.check('hk_cbp_bwd: nothing written', bf.untouched())
    plan.close()
    # classifier, CIN
    for entry in ('fwd', 'scaled', 'ssq'):
        R.check(f'linear {entry}: nothing written', linear_forward(lib, dev, R, (3, 1000, 7, 0, True), entry, short_ws=True)['untouched'])
    R.check('cin cci bwd: nothing written', cin_cci_backward(lib, dev, R, (4, 24, 12), short_ws=True)['untouched'])
    R.done()


# ========================================================================================================= bit identity under poison
def run_bit_identity(lib, dev, tune):
    """The pairs of forms the existing A/B tests compare bit for bit, each run on freshly poisoned guarded buffers - the comparison an
    inherited buffer could have been faking.  `tune(name, value)`: the conftest fixture."""
    R = Report('bit identity')
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    # hk_bcnn_pool_fwd in one launch, in two (fwd_fold = -1) and as its stages: y, inv_norm, colsum (tests/test_gpu_kernels.py:960)
    for shape in ((2, 128, 196), (2, 64, 196), (2, 130, 12)):
        outs = []
        for fold, staged in ((0, False), (-1, False), (0, True)):
            tune('fwd_fold', fold)
            outs.append(bcnn_forward(lib, dev, shape, R, staged)[:3])
        tune('fwd_fold', 0)
        for i, o in enumerate(outs[1:]):
            R.check(f'bcnn forward {shape}: form {i + 1} against the one-launch form', all(same(a, b) for a, b in zip(o, outs[0])))
    # parts + hk_linear_fwd_ssq against unscaled + hk_linear_fwd_scaled: u, inv_norm, the logits (tests/test_gpu_kernels.py:996)
    shape = (2, 128, 64)
    B, C, HW = shape
    J, K = C * C, 5
    cs = ssqrt_case(shape)
    g = _gen(13, *shape)
    w, bias = torch.randn(K, J, generator=g) * 0.05, torch.randn(K, generator=g)
    un = ssqrt_forward(lib, dev, shape, R, 'unscaled')
    pa = ssqrt_forward(lib, dev, shape, R, 'parts')
    R.check('ssqrt parts against unscaled: u', pa['rc'] == 0 and same(pa['y'], un['y']))
    logits = []
    for which in ('scaled', 'ssq'):
        bf = Bufs(dev)
        pu, pw, pb, pout = bf.inp(un['y']), bf.inp(w), bf.inp(bias), bf.out('out', (B, K))
        pws, nws = bf.work(lib.hk_linear_ws_bytes(B, J, K))
        if which == 'scaled':
            R.call(lib, 'hk_linear_fwd_scaled', bf, pu, pw, pb, bf.inp(un['inv']), pout, B, J, K, pws, nws)
            logits.append((bf.get('out'), un['inv']))
        else:
            pinv = bf.out('inv', (B,))
            ss = pa['ss'].clone()
            ss[:, pa['nparts']:] = 1e30
            R.call(lib, 'hk_linear_fwd_ssq', bf, pu, pw, pb, bf.inp(ss), pa['nparts'], pinv, pout, B, J, K, pws, nws)
            logits.append((bf.get('out'), bf.get('inv')))
    R.check('ssqrt parts + fwd_ssq against unscaled + fwd_scaled: logits, inv_norm',
            same(logits[0][0], logits[1][0]) and same(logits[0][1], logits[1][1]))
    # CBP: row-scatter against row-sketch (tests/test_gpu_parity.py:478), and each form twice
    cshape = (128, 1024, 49, 3)
    ys = {}
    for b in (0, 2, 2, -1, -1):
        tune('cbp_bin', b)
        o = cbp_forward(lib, dev, cshape, R)
        if b in ys:
            R.check(f'cbp_bin {b} twice', same(ys[b]['y'], o['y']) and same(ys[b]['c_raw'], o['c_raw']))
        ys[b] = o
    tune('cbp_bin', -1)
    R.check('cbp row-scatter against row-sketch', same(ys[2]['y'], ys[0]['y']) and same(ys[2]['c_raw'], ys[0]['c_raw']))
    # cbp_bwd3_kernel: 128-row blocks, 64-row blocks, 64-row blocks with divided column tiles (tests/test_gpu_kernels.py:449-450)
    dxs = {}
    for sb in (200, 96, 32):
        tune('sched_b', sb)
        dxs[sb] = cbp_backward(lib, dev, (128, 1024, 64, 3), R)
        R.check(f'cbp backward, sched_b {sb}: twice', same(cbp_backward(lib, dev, (128, 1024, 64, 3), R), dxs[sb]))
    tune('sched_b', 0)
    R.check('cbp backward: 128-row against 64-row blocks', same(dxs[200], dxs[96]))
    R.check('cbp backward: divided column tiles against 64-row blocks', same(dxs[32], dxs[96]))
    # Newton-Schulz: the tile widths (tests/test_gpu_kernels.py:900), the queues (:1045), the symmetric entry where its schedule does not
    # apply (:932) and with ns_sym = 0 (:934), the fused upper triangle (:1023)
    for d, iter_n, Bn in ((70, 3, 17), (128, 2, 16)):              # B >= 16: ns_streams = 1 runs two queues (mpn.hip:254)
        cn = ns_case(d, iter_n, Bn)

        def both(entry='fwd'):
            o = ns_forward(lib, dev, R, cn.a, iter_n, entry)
            return o, ns_backward(lib, dev, R, cn.a, o, cn.dout, iter_n, 'bwd')[0]
        tune('ns_tn', 64)
        o64, da64 = both()
        tune('ns_tn', 128)
        o128, da128 = both()
        tune('ns_tn', 0)
        R.check(f'ns d = {d}: ns_tn 64 against 128', all(same(o64[k], o128[k]) for k in ('out', 'norm_a', 'ysave', 'zsave')) and same(da64, da128))
        tune('ns_streams', 0)
        o0, da0 = both()
        tune('ns_streams', 1)
        o1, da1 = both()
        R.check(f'ns d = {d}: one queue against two', all(same(o0[k], o1[k]) for k in ('out', 'norm_a', 'ysave', 'zsave')) and same(da0, da1))
        osym, _ = both('sym')
        if d % 128:
            R.check(f'ns d = {d}: the symmetric entry falls back to the full products', same(osym['out'], o1['out']))
        tune('ns_sym', 0)
        R.check(f'ns d = {d}: ns_sym = 0', same(ns_forward(lib, dev, R, cn.a, iter_n, 'sym')['out'], o1['out']))
        tune('ns_sym', 1)
        for entry, plain in (('triu', o1), ('triu_sym', osym)):
            ot = ns_forward(lib, dev, R, cn.a, iter_n, entry)
            R.check(f'ns d = {d}: {entry} out against the two calls', same(ot['out'], plain['out']))
    # classifier backward: each single product against the combined launch, and the two walks (tests/test_gpu_kernels.py:1140, :1147)
    case = (5, 16448, 208, 0, True)
    full = linear_backward(lib, dev, R, case, 'ywb')
    R.check('linear bwd: dy alone', same(linear_backward(lib, dev, R, case, 'yb')['dy'], full['dy']))
    wb = linear_backward(lib, dev, R, case, 'wb')
    R.check('linear bwd: dw and db alone', same(wb['dw'], full['dw']) and same(wb['db'], full['db']))
    for walk in (0, 1):
        tune('lin_walk', walk)
        o = linear_backward(lib, dev, R, case, 'ywb')
        R.check(f'linear bwd: lin_walk {walk}', all(same(o[k], full[k]) for k in ('dy', 'dw', 'db')))
    tune('lin_walk', -1)
    R.done()
