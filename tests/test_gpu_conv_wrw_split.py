"""The split form of hk_conv3x3_wrw (csrc/conv_wrw.hip, knob `wrw_split` at 1) on the GPU: every fp32 value as three bf16 pieces,
six bf16 MFMAs per tap with fp32 accumulation.

Bound, elementwise as for the fp32 form (tests/test_gpu_conv_wrw.py): |dW - dW64| <= 1e-6 S with S = the same sum over |x| and
|dy|, 1.5e-6 S for the case with 1260 pixels.  What the split itself may cost: the three pieces carry a value to 2^-27 relative,
the dropped products (mid lo, lo mid, lo lo) are below 2^-24 |x| |dy| - at most 3.9e-8 S; the rest of the bound is the fp32
accumulation, as before.  Inputs that stress the pieces rather than the sum: scaled gradients (the low pieces near the bottom of
bf16's range), half the values zero, values that are one piece, values whose residual pieces are negative, and a spread of
2^+-6 per element - the widest at which torch's own fp32 result on the CPU stays well under 4e-7 S (2.6e-7 S; 2^+-20 gives
7.6e-7 S and would test the accumulation, not the split)."""
import functools

import pytest
import torch

from test_gpu_conv_wrw import SMALL, _case, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPE = (2, 6, 40, 64)


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


def _ref64(x, dy):
    cout = dy.shape[1]
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, 64, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 64, 3, 3), dy.double().abs(), padding=1)
    return ref, scale


def _within(dw, ref, scale, bound, what):
    diff = (dw.double().cpu() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())
    print(f'{what}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), (what, worst)


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_small_shapes_against_float64(F, tune, shape):
    n, h, w, cout = shape
    x, dy, ref, scale = _case(*shape)
    tune('wrw_split', 1)
    dw = F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV))
    assert tuple(dw.shape) == (cout, 64, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    _within(dw, ref, scale, 1e-6 if n * h * w <= 1024 else 1.5e-6, shape)
    if shape == SHAPE:                                                 # the knob really switches kernels
        tune('wrw_split', 0)
        assert not torch.equal(F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV)), dw)


def test_one_workgroup_walks_every_job_and_adds_its_accumulators_to_the_partial_on_the_way(F, tune):
    """`wrw_wgs` at 1: the 12 jobs of this shape are 54 row steps of one workgroup - more than the 32 after which the split
    kernel adds its accumulators to its partial result and starts them from zero (the first time a store, then an addition)."""
    shape = (2, 9, 70, 64)
    x, dy, ref, scale = _case(*shape)
    tune('wrw_split', 1)
    tune('wrw_wgs', 1)
    dw = F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV))
    _within(dw, ref, scale, 1.5e-6, 'one workgroup')
    assert torch.equal(F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV)), dw)


@functools.lru_cache(maxsize=None)
def _stress(kind):
    n, h, w, cout = SHAPE
    x, dy, _, _ = _case(*SHAPE)
    nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(77)
    if kind == 'dy 1e-6':
        dy = dy * 1e-6
    elif kind == 'dy 1e-30':
        dy = dy * 1e-30
    elif kind == 'relu':
        x = torch.relu(x)
    elif kind == 'bf16 values':
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    elif kind == 'negative residuals':
        x = torch.full_like(x, 1.0 - 2.0 ** -24)
        dy = torch.where(dy < 0, -1.0, 1.0) * (2.0 - 2.0 ** -23)
    elif kind == 'spread 2^+-6':
        x = x * torch.exp2(torch.randint(-6, 7, x.shape, generator=g).float())
        dy = dy * torch.exp2(torch.randint(-6, 7, dy.shape, generator=g).float())
        x, dy = nhwc(x), nhwc(dy)
        ref, scale = _ref64(x, dy)
        f32 = torch.nn.grad.conv2d_weight(x, (cout, 64, 3, 3), dy, padding=1)
        assert float(((f32.double() - ref).abs() / scale).max()) < 4e-7         # the spread leaves the accumulation out of it
        return x, dy, ref, scale
    x, dy = nhwc(x), nhwc(dy)
    return (x, dy) + _ref64(x, dy)


@pytest.mark.parametrize('kind', ['dy 1e-6', 'dy 1e-30', 'relu', 'bf16 values', 'negative residuals', 'spread 2^+-6'])
def test_inputs_that_stress_the_split(F, tune, kind):
    x, dy, ref, scale = _stress(kind)
    tune('wrw_split', 1)
    _within(F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV)), ref, scale, 1e-6, kind)


def test_images_isolation_and_run_to_run_bits(F, tune):
    n, h, w, cout = SHAPE
    x, dy, _, _ = _case(*SHAPE)
    xg, dyg = x.to(DEV), dy.to(DEV)
    tune('wrw_split', 1)
    dw = F.conv3x3_wrw_raw(xg, dyg)
    parts = F.conv3x3_wrw_raw(xg[:1], dyg[:1]).double() + F.conv3x3_wrw_raw(xg[1:], dyg[1:]).double()
    assert rel(dw, parts) < 1e-6

    def guarded(t):                                                    # the same tensor inside an allocation that holds 1e30 elsewhere
        c = t.shape[1]
        pad = 3 * w * c
        big = torch.full((t.numel() + 2 * pad,), 1e30, device=DEV)
        inner = big[pad:pad + t.numel()].view(n, h, w, c)
        inner.copy_(t.permute(0, 2, 3, 1))
        v = inner.permute(0, 3, 1, 2)
        assert v.is_contiguous(memory_format=torch.channels_last) and v.data_ptr() % 16 == 0
        return v
    assert torch.equal(F.conv3x3_wrw_raw(guarded(xg), guarded(dyg)), dw)
    assert torch.equal(F.conv3x3_wrw_raw(xg, dyg), dw)


def test_non_finite_inputs_stay_where_the_fp32_kernel_has_them(F, tune):
    n, h, w, cout = SHAPE
    x, dy, _, _ = _case(*SHAPE)
    x = x.clone()
    x[0, 5, 2, 7] = float('inf')
    x[1, 40, 4, 33] = float('nan')
    ref, scale = _ref64(x, dy)
    tune('wrw_split', 0)
    plain = F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV)).cpu()
    tune('wrw_split', 1)
    dw = F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV)).cpu()
    bad = ~torch.isfinite(plain)
    assert 0 < int(bad.sum()) < bad.numel()
    assert torch.equal(~torch.isfinite(dw), bad)
    ok = ~bad
    finite_scale = torch.nn.grad.conv2d_weight(torch.nan_to_num(x, 0.0, 0.0, 0.0).double().abs(), (cout, 64, 3, 3), dy.double().abs(), padding=1)
    diff = (dw.double() - ref).abs()
    assert bool((diff[ok] <= 1e-6 * finite_scale[ok]).all())


def test_routing_and_refusals_for_both_knob_values(F, tune):
    from hawkeye_amd._lib import HawkeyeHipError
    from hawkeye_amd.model.backbone.vgg import conv_stack
    torch.manual_seed(5)
    stack = conv_stack((64, 64, 'M', 128)).to(DEV).to(memory_format=torch.channels_last)
    img = torch.randn(2, 3, 16, 24, device=DEV).contiguous(memory_format=torch.channels_last)

    def grads():
        stack.zero_grad(set_to_none=True)
        stack(img).square().sum().backward()
        return [p.grad.clone() for p in stack.parameters()]
    conv = lambda cin, cout: torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV).to(memory_format=torch.channels_last)
    nhwc = lambda *s, **k: torch.randn(*s, **k).contiguous(memory_format=torch.channels_last)
    x64, x32 = nhwc(1, 64, 4, 4, device=DEV), nhwc(1, 32, 4, 4, device=DEV)
    dy64, dy96 = nhwc(1, 64, 4, 4, device=DEV), nhwc(1, 96, 4, 4, device=DEV)
    flat = torch.randn(64 * 16 + 4, device=DEV)
    odd = flat[1:1 + 64 * 16].view(1, 4, 4, 64).permute(0, 3, 1, 2)
    got = {}
    for knob in (0, 1):
        tune('wrw_split', knob)
        got[knob] = grads()
        assert F.conv3x3_wrw_ok(x64, conv(64, 64)) and F.conv3x3_wrw_ok(x64, conv(64, 128))
        assert not F.conv3x3_wrw_ok(x32, conv(32, 64)) and not F.conv3x3_wrw_ok(x64, conv(64, 96)) and not F.conv3x3_wrw_ok(odd, conv(64, 64))
        for xs, dys in ((x32, dy64), (x64, dy96), (odd, dy64), (nhwc(1, 64, 4, 4), nhwc(1, 64, 4, 4)), (x64.double(), dy64.double())):
            with pytest.raises(HawkeyeHipError):
                F.conv3x3_wrw_raw(xs, dys)
    assert all(rel(a, b) < 1e-5 for a, b in zip(got[0], got[1]))
    assert any(not torch.equal(a, b) for a, b in zip(got[0], got[1]))
