"""hk_conv3x3_wrw with more than 64 input channels (csrc/conv_wrw.hip) on the GPU: the split form reads its 64-channel slice of `x`
out of Cin-wide pixels, a workgroup owns one (Cout slice, Cin slice) block of dW, the partial results are [workgroup][Cout][9][Cin].

Bound, elementwise as for 64 input channels (tests/test_gpu_conv_wrw.py, tests/test_gpu_conv_wrw_split.py): |dW - dW64| <= 1e-6 S
with S = the same sum over |x| and |dy|, 1.5e-6 S above 1024 pixels - an element of dW is the same sum over the same pixels whatever
Cin is.  The reference is torch.nn.grad.conv2d_weight in float64 on the CPU."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (N, H, W, Cin, Cout): two Cin slices, all border | both slice indices, a ragged second strip | W = 28: a single short strip, four
# Cin slices | an odd slice count, all border
SMALL = [(1, 2, 2, 128, 64), (1, 5, 33, 128, 128), (2, 6, 28, 256, 64), (3, 1, 1, 192, 64)]
ONE_WG = (2, 9, 70, 128, 64)          # 12 jobs, 54 row steps of one workgroup: the flush into the partial at a Cin offset of 64
SHAPE = (2, 6, 40, 128, 128)


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def _case(n, h, w, cin, cout):
    """Inputs (CPU, channels_last), the float64 weight gradient and its scale S - made once per shape."""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cin + cout)
    x = torch.randn(n, cin, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, cin, 3, 3), dy.double().abs(), padding=1)
    return x, dy, ref, scale


def _within(dw, ref, scale, bound, what):
    diff = (dw.double().cpu() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())             # (S = 0: a tap that only ever sees the border; dW is 0 there)
    print(f'{what}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), (what, worst)


def _check(F, tune, shape, what):
    n, h, w, cin, cout = shape
    x, dy, ref, scale = _case(*shape)
    xg, dyg = x.to(DEV), dy.to(DEV)
    dw = F.conv3x3_wrw_raw(xg, dyg)
    assert tuple(dw.shape) == (cout, cin, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    _within(dw, ref, scale, 1e-6 if n * h * w <= 1024 else 1.5e-6, what)
    # the first and the second Cin slice are what the split form gives for those 64 channels alone (same jobs, same workgroups),
    # bit for bit: a slice that read its neighbour's channels would differ
    tune('wrw_split', 1)
    for s in (0, 1):
        alone = F.conv3x3_wrw_raw(xg[:, 64 * s:64 * s + 64].contiguous(memory_format=torch.channels_last), dyg)
        assert torch.equal(dw[:, 64 * s:64 * s + 64], alone), (what, s)


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_small_shapes_against_float64(F, tune, shape):
    _check(F, tune, shape, shape)


def test_one_workgroup_adds_its_accumulators_to_the_partial_at_a_channel_offset(F, tune):
    """`wrw_wgs` at 1: one workgroup per slice walks the 12 jobs, 54 row steps - past the 32 after which the accumulators are added
    to the partial result, whose rows are 9 x 128 floats here and whose second Cin slice starts 64 floats into a tap."""
    tune('wrw_wgs', 1)
    _check(F, tune, ONE_WG, 'one workgroup')


def test_images_isolation_and_run_to_run_bits(F):
    n, h, w, cin, cout = SHAPE
    x, dy, _, _ = _case(*SHAPE)
    xg, dyg = x.to(DEV), dy.to(DEV)
    dw = F.conv3x3_wrw_raw(xg, dyg)
    parts = F.conv3x3_wrw_raw(xg[:1], dyg[:1]).double() + F.conv3x3_wrw_raw(xg[1:], dyg[1:]).double()
    assert rel(dw, parts) < 1e-6

    def guarded(t):                                                    # the same tensor inside an allocation that holds 1e30 elsewhere
        c = t.shape[1]
        pad = 3 * w * c                                                # three image rows on either side (16-byte multiple)
        big = torch.full((t.numel() + 2 * pad,), 1e30, device=DEV)
        inner = big[pad:pad + t.numel()].view(n, h, w, c)
        inner.copy_(t.permute(0, 2, 3, 1))
        v = inner.permute(0, 3, 1, 2)
        assert v.is_contiguous(memory_format=torch.channels_last) and v.data_ptr() % 16 == 0
        return v
    assert torch.equal(F.conv3x3_wrw_raw(guarded(xg), guarded(dyg)), dw)
    assert torch.equal(F.conv3x3_wrw_raw(xg, dyg), dw)


def test_512_channels_at_a_metric_like_shape(F):
    """16 x (512 -> 512) x 28 x 28, 64 slices of eight workgroups: (a) image 0 alone against float64 on the CPU, (b) the whole batch
    against the sum of its four quarters by the same kernel, (c) against the library's own float32 weight gradient (an atomic sum:
    loosely), (d) the same bits on a second call."""
    n, h, w, cin, cout = 16, 28, 28, 512, 512
    gen = torch.Generator(device=DEV).manual_seed(37)
    x = torch.empty(n, cin, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dy = torch.empty(n, cout, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dw = F.conv3x3_wrw_raw(x, dy)
    dw0 = F.conv3x3_wrw_raw(x[:1], dy[:1])
    ref0 = torch.nn.grad.conv2d_weight(x[:1].cpu().double(), (cout, cin, 3, 3), dy[:1].cpu().double(), padding=1)
    ra = rel(dw0, ref0)
    quarters = sum(F.conv3x3_wrw_raw(x[i:i + 4], dy[i:i + 4]).double() for i in range(0, n, 4))
    rb = rel(dw, quarters)
    wt = torch.empty(cout, cin, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    lib = torch.ops.aten.convolution_backward(dy, x, wt, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))[1]
    rc = rel(dw, lib)
    print(f'512 -> 512 at 28 x 28, batch 16: (a) {ra:.3e} (b) {rb:.3e} (c) {rc:.3e}')
    assert ra < 1e-5                                                  # (a)
    assert rb < 1e-5                                                  # (b)
    assert rc < 2e-3                                                  # (c)
    assert torch.equal(F.conv3x3_wrw_raw(x, dy), dw)                  # (d)


def test_routing_and_refusals(F, tune, monkeypatch):
    """ConvStack sends a 128-input-channel layer to the kernel where the rule routes it - here forced with `wrw_split` at 1, the map
    of this test is not one that was measured - and leaves it to the library by default and with `wrw_wide` or `wrw_split` at 0; the
    64-input-channel layers go to the kernel every time.  Either way the same gradients."""
    from hawkeye_amd._lib import HawkeyeHipError
    from hawkeye_amd.model.backbone.vgg import conv_stack
    calls = []
    real = F.conv3x3_wrw_raw
    monkeypatch.setattr(F, 'conv3x3_wrw_raw', lambda x, dy: (calls.append((x.shape[1],) + tuple(dy.shape)), real(x, dy))[1])
    torch.manual_seed(5)
    stack = conv_stack((64, 64, 'M', 128, 128)).to(DEV).to(memory_format=torch.channels_last)
    img = torch.randn(2, 3, 16, 24, device=DEV).contiguous(memory_format=torch.channels_last)

    def grads():
        del calls[:]
        stack.zero_grad(set_to_none=True)
        stack(img).square().sum().backward()
        return [p.grad.clone() for p in stack.parameters()]
    narrow = [(64, 2, 128, 8, 12), (64, 2, 64, 16, 24)]                # conv2_1, then conv1_2 (backward order)
    default = grads()
    assert calls == narrow                                            # 2 x 128 x 8 x 12 was never measured: the library's
    tune('wrw_split', 1)
    forced = grads()
    assert calls == [(128, 2, 128, 8, 12)] + narrow
    tune('wrw_wide', 0)
    off = grads()
    assert calls == narrow
    tune('wrw_wide', 1)
    tune('wrw_split', 0)
    fp32 = grads()
    assert calls == narrow
    for other in (default, off, fp32):
        assert all(rel(a, b) < 1e-5 for a, b in zip(forced, other))
    assert any(not torch.equal(a, b) for a, b in zip(forced, off))

    # the default rule (every knob back at its default): a measured layer at a measured batch goes to the kernel - argument order
    # (cout, n, h, w, cin) against the table's (cin, cout, h, w) -, another batch, map or an unmeasured pair of widths does not
    tune('wrw_split', -1)
    assert F.conv3x3_wrw_route(512, 16, 28, 28, 512) and F.conv3x3_wrw_route(512, 64, 56, 56, 256) and F.conv3x3_wrw_route(256, 64, 112, 112, 128)
    assert not F.conv3x3_wrw_route(512, 8, 28, 28, 512) and not F.conv3x3_wrw_route(512, 16, 27, 27, 512)
    assert not F.conv3x3_wrw_route(256, 64, 56, 56, 512) and not F.conv3x3_wrw_route(128, 64, 112, 112, 256)
    x512 = torch.empty(16, 512, 28, 28, device=DEV).contiguous(memory_format=torch.channels_last)
    conv5 = torch.nn.Conv2d(512, 512, 3, padding=1).to(DEV).to(memory_format=torch.channels_last)
    assert F.conv3x3_wrw_ok(x512, conv5) and not F.conv3x3_wrw_ok(x512[:8], conv5)
    tune('wrw_split', 0)

    conv = lambda cin, cout: torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV).to(memory_format=torch.channels_last)
    nhwc = lambda *s: torch.randn(*s, device=DEV).contiguous(memory_format=torch.channels_last)
    x128, x96, x32 = nhwc(1, 128, 4, 4), nhwc(1, 96, 4, 4), nhwc(1, 32, 4, 4)
    dy64 = nhwc(1, 64, 4, 4)
    monkeypatch.setattr(F, 'conv3x3_wrw_raw', real)
    assert not F.conv3x3_wrw_ok(x128, conv(128, 64))                  # wrw_split 0: the fp32 form serves 64 input channels only
    with pytest.raises(HawkeyeHipError):
        F.conv3x3_wrw_raw(x128, dy64)
    tune('wrw_split', -1)
    assert not F.conv3x3_wrw_ok(x128, conv(128, 64))                  # the default: not a measured layer
    F.conv3x3_wrw_raw(x128, dy64)                                     # ... which the entry point serves all the same
    tune('wrw_split', 1)
    assert F.conv3x3_wrw_ok(x128, conv(128, 64)) and F.conv3x3_wrw_ok(x128, conv(128, 128))
    assert not F.conv3x3_wrw_ok(x32, conv(32, 64)) and not F.conv3x3_wrw_ok(x96, conv(96, 64)) and not F.conv3x3_wrw_ok(x128, conv(128, 96))
    assert not F.conv3x3_wrw_ok(nhwc(1, 128, 4, 4).double(), conv(128, 64).double())
    assert not F.conv3x3_wrw_ok(x128, torch.nn.Conv2d(128, 64, 3, padding=1).to(DEV))        # an NCHW weight
    flat = torch.randn(128 * 16 + 4, device=DEV)
    odd = flat[1:1 + 128 * 16].view(1, 4, 4, 128).permute(0, 3, 1, 2)                         # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4 and not F.conv3x3_wrw_ok(odd, conv(128, 64))
    for xs, dys in ((x96, dy64), (x32, dy64), (odd, dy64), (x128, nhwc(1, 96, 4, 4))):
        with pytest.raises(HawkeyeHipError):
            F.conv3x3_wrw_raw(xs, dys)
    tune('wrw_wide', 0)
    assert not F.conv3x3_wrw_ok(x128, conv(128, 64))
    with pytest.raises(HawkeyeHipError):
        F.conv3x3_wrw_raw(x128, dy64)
