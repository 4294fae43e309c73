"""hk_conv3x3_wrw (csrc/conv_wrw.hip): the weight gradient of the trunk's 3 x 3 convolutions with 64 input channels, on the GPU.

Small shapes against float64 (every border case, a ragged strip, two Cout slices, a row-block boundary), isolation of the
images and of the two tensors from their surroundings, run-to-run bits, the two trunk layers at the metric's shapes, and the
routing of ConvStack.  Bound of the small cases, elementwise: |dW - dW64| <= 1e-6 S with S = the same sum over |x| and |dy|
(an fp32 MFMA chain is at 0.75 - 1.5e-7 sum |a b| for K <= 1024; that leaves about 7x for the fixed-order sum of the workgroups'
partial results), 1.5e-6 for the case with 1260 pixels."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (N, H, W, Cout): two images, a ragged second strip, fewer jobs than workgroups | odd width, a one-pixel last strip, two Cout
# slices | all border | all border | two row blocks (rows 0-4 and 5-8: a row block is at least four rows high)
SMALL = [(2, 6, 40, 64), (1, 5, 33, 128), (3, 1, 1, 64), (1, 2, 2, 64), (2, 9, 70, 64)]


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
def _case(n, h, w, cout):
    """Inputs (CPU, channels_last), the float64 weight gradient and its scale S - made once per shape."""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cout)
    x = torch.randn(n, 64, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, cout, h, w, generator=g).contiguous(memory_format=torch.channels_last)
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, 64, 3, 3), dy.double(), padding=1)
    scale = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 64, 3, 3), dy.double().abs(), padding=1)
    return x, dy, ref, scale


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_small_shapes_against_float64(F, shape):
    n, h, w, cout = shape
    x, dy, ref, scale = _case(*shape)
    dw = F.conv3x3_wrw_raw(x.to(DEV), dy.to(DEV))
    assert tuple(dw.shape) == (cout, 64, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
    bound = 1e-6 if n * h * w <= 1024 else 1.5e-6
    diff = (dw.double().cpu() - ref).abs()
    worst = float((diff / scale.clamp_min(1e-300)).max())             # (S = 0: a tap that only ever sees the border; dW is 0 there)
    print(f'{shape}: max |dW - dW64| / S = {worst:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * scale).all()), worst


def test_images_do_not_leak_into_each_other_and_nothing_outside_the_tensors_is_read(F):
    n, h, w, cout = 2, 6, 40, 64
    x, dy, _, _ = _case(n, h, w, cout)
    xg, dyg = x.to(DEV), dy.to(DEV)
    dw = F.conv3x3_wrw_raw(xg, dyg)
    parts = F.conv3x3_wrw_raw(xg[:1], dyg[:1]).double() + F.conv3x3_wrw_raw(xg[1:], dyg[1:]).double()
    assert rel(dw, parts) < 1e-6
    # the same tensors inside larger allocations whose other rows hold 1e30: one of them in a sum would show

    def guarded(t):
        c = t.shape[1]
        pad = 3 * w * c                                                # three image rows on either side (16-byte multiple)
        big = torch.full((t.numel() + 2 * pad,), 1e30, device=DEV)
        inner = big[pad:pad + t.numel()].view(n, h, w, c)
        inner.copy_(t.permute(0, 2, 3, 1))
        v = inner.permute(0, 3, 1, 2)
        assert v.is_contiguous(memory_format=torch.channels_last) and v.data_ptr() % 16 == 0
        return v
    assert torch.equal(F.conv3x3_wrw_raw(guarded(xg), guarded(dyg)), dw)


def test_same_input_same_bits(F):
    x, dy, _, _ = _case(1, 5, 33, 128)
    xg, dyg = x.to(DEV), dy.to(DEV)
    assert torch.equal(F.conv3x3_wrw_raw(xg, dyg), F.conv3x3_wrw_raw(xg, dyg))


def _library_wrw(x, dy, cout):
    w = torch.empty(cout, 64, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    return torch.ops.aten.convolution_backward(dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))[1]


def test_conv1_2_at_the_metric_shape(F):
    """64 x 64 x 448 x 448 (3.29 GB maps, byte offsets beyond 2^32), with the bounds of
    test_first_convolution_kernels_at_the_metric_shape: (a) image 0 alone against float64 on the CPU, (b) the whole batch
    against the sum of its four quarters by the same kernel - additivity ties the large-offset rows to the small-offset
    ones -, (c) against the library's own float32 weight gradient (an atomic sum over 12.8 M pixels: loosely), (d) the same
    bits on a second call."""
    n, h, w, cout = 64, 448, 448, 64
    gen = torch.Generator(device=DEV).manual_seed(29)
    x = torch.empty(n, 64, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dy = torch.empty(n, cout, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dw = F.conv3x3_wrw_raw(x, dy)
    dw0 = F.conv3x3_wrw_raw(x[:1], dy[:1])
    ref0 = torch.nn.grad.conv2d_weight(x[:1].cpu().double(), (cout, 64, 3, 3), dy[:1].cpu().double(), padding=1)
    ra = rel(dw0, ref0)
    quarters = sum(F.conv3x3_wrw_raw(x[i:i + 16], dy[i:i + 16]).double() for i in range(0, n, 16))
    rb = rel(dw, quarters)
    rc = rel(dw, _library_wrw(x, dy, cout))
    print(f'conv1_2 metric shape: (a) {ra:.3e} (b) {rb:.3e} (c) {rc:.3e}')
    assert ra < 1e-5                                                  # (a)
    assert rb < 1e-5                                                  # (b)
    assert rc < 2e-3                                                  # (c)
    assert torch.equal(F.conv3x3_wrw_raw(x, dy), dw)                  # (d)


def test_conv2_1_at_the_metric_shape(F):
    """64 x (64 -> 128) x 224 x 224: two Cout slices; (b) and (c) of the conv1_2 case."""
    n, h, w, cout = 64, 224, 224, 128
    gen = torch.Generator(device=DEV).manual_seed(31)
    x = torch.empty(n, 64, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dy = torch.empty(n, cout, h, w, device=DEV, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
    dw = F.conv3x3_wrw_raw(x, dy)
    quarters = sum(F.conv3x3_wrw_raw(x[i:i + 16], dy[i:i + 16]).double() for i in range(0, n, 16))
    rb = rel(dw, quarters)
    rc = rel(dw, _library_wrw(x, dy, cout))
    print(f'conv2_1 metric shape: (b) {rb:.3e} (c) {rc:.3e}')
    assert rb < 1e-5
    assert rc < 2e-3


def test_refusals(F):
    from hawkeye_amd._lib import HawkeyeHipError
    conv = lambda cin, cout: torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV).to(memory_format=torch.channels_last)
    nhwc = lambda *s, **k: torch.randn(*s, **k).contiguous(memory_format=torch.channels_last)
    x64, x32 = nhwc(1, 64, 4, 4, device=DEV), nhwc(1, 32, 4, 4, device=DEV)
    assert F.conv3x3_wrw_ok(x64, conv(64, 64)) and F.conv3x3_wrw_ok(x64, conv(64, 128))
    assert not F.conv3x3_wrw_ok(x32, conv(32, 64))                                       # Cin != 64
    assert not F.conv3x3_wrw_ok(x64, conv(64, 96))                                       # Cout % 64 != 0
    assert not F.conv3x3_wrw_ok(nhwc(1, 64, 4, 4), conv(64, 64))                         # a CPU tensor
    assert not F.conv3x3_wrw_ok(x64.double(), conv(64, 64).double())                     # not fp32
    assert not F.conv3x3_wrw_ok(x64, torch.nn.Conv2d(64, 64, 3, padding=1).to(DEV))      # an NCHW weight
    assert not F.conv3x3_wrw_ok(x64, torch.nn.Conv2d(64, 64, 3, padding=1, stride=2).to(DEV).to(memory_format=torch.channels_last))
    flat = torch.randn(64 * 16 + 4, device=DEV)
    odd = flat[1:1 + 64 * 16].view(1, 4, 4, 64).permute(0, 3, 1, 2)                       # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4 and not F.conv3x3_wrw_ok(odd, conv(64, 64))
    # ... and the entry point itself refuses them: nothing is launched, the caller hears about it
    dy64, dy96 = nhwc(1, 64, 4, 4, device=DEV), nhwc(1, 96, 4, 4, device=DEV)
    for xs, dys in ((x32, dy64), (x64, dy96), (odd, dy64), (nhwc(1, 64, 4, 4), nhwc(1, 64, 4, 4)), (x64.double(), dy64.double())):
        with pytest.raises(HawkeyeHipError):
            F.conv3x3_wrw_raw(xs, dys)


def test_conv_stack_routing(F, tune, monkeypatch):
    """ConvStack sends a 64-input-channel layer to the kernel on its channels_last path - and only there: an NCHW input, a
    hooked child or the `conv_wrw` knob at 0 leave every weight gradient to the library.  Either way the same gradients."""
    from hawkeye_amd.model.backbone.vgg import conv_stack
    calls = []
    real = F.conv3x3_wrw_raw
    monkeypatch.setattr(F, 'conv3x3_wrw_raw', lambda x, dy: (calls.append(tuple(dy.shape)), real(x, dy))[1])
    torch.manual_seed(5)
    stack = conv_stack((64, 64, 'M', 128)).to(DEV).to(memory_format=torch.channels_last)
    img = torch.randn(2, 3, 16, 24, device=DEV)

    def grads(inp):
        stack.zero_grad(set_to_none=True)
        stack(inp).square().sum().backward()
        return [p.grad.clone() for p in stack.parameters()]
    ours = grads(img.contiguous(memory_format=torch.channels_last))
    assert calls == [(2, 128, 8, 12), (2, 64, 16, 24)]                                   # conv2_1, then conv1_2 (backward order)
    del calls[:]
    plain = grads(img)                                                                   # NCHW: nn.Sequential's own forward
    assert calls == []
    h = stack[1].register_forward_hook(lambda m, i, o: None)
    hooked = grads(img.contiguous(memory_format=torch.channels_last))
    h.remove()
    assert calls == []
    tune('conv_wrw', 0)
    lib = grads(img.contiguous(memory_format=torch.channels_last))
    assert calls == []
    # knob at 0: the same forward bits, only the two weight gradients come from another fp32 kernel (K = 768 and 192 pixels:
    # rounding of 1e-7 per element); NCHW / hooked: every layer runs other fp32 kernels, forward included
    assert all(rel(a, b) < 1e-5 for a, b in zip(ours, lib))
    for other in (plain, hooked):
        assert all(rel(a, b) < 1e-4 for a, b in zip(ours, other))
