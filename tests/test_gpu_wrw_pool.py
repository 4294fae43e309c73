"""hk_conv3x3_wrw_pooled (csrc/conv_wrw.hip, "Pooled") on the GPU: the cases of tests/wrw_pool_cases.py.  What only the device shows: that
ds_read_b64_tr_b16 over the window image of wrp_aoff hands each lane the windows wrp_awin names, and that v_smfmac_f32_16x16x64_bf16
takes the operand, index and result layouts of csrc/hk_smfmac_bf16.h - on small integers any disagreement gives a wrong integer, and
the result has to equal the float64 gradient exactly.  Then the routing: a four-layer ConvStack with `wrw_pool` 1 against 0."""
import pytest
import torch

import wrw_pool_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
EACH = pytest.mark.parametrize('shape,wgs', C.CASES, ids=C.IDS)


@pytest.fixture(scope='module')
def lib():
    from hawkeye_amd import _lib
    lib_ = _lib.load()
    assert b'gfx950' in lib_.hk_version()
    return lib_


def _stream():
    from hawkeye_amd import _lib
    return _lib.stream()


def _run(lib, c, wgs=0, **kw):
    x, dp, p, am = c[:4]
    return C.run(lib, DEV, x, dp, p, am, wgs, _stream(), **kw)


@EACH
def test_small_integers_give_the_float64_gradient_exactly(lib, shape, wgs):
    c = C.case(shape, 'int')
    dw = _run(lib, c, wgs)
    assert torch.equal(dw.double(), c[5]), (shape, int((dw.double() != c[5]).sum()))


@EACH
def test_randn_within_the_bound_beside_the_dense_kernel(lib, shape, wgs):
    c = C.case(shape, 'randn')
    dw = _run(lib, c, wgs)
    ratio, diff = C.M.worst(dw, c[5], c[6])
    dense, _ = C.M.worst(C.run_dense(lib, DEV, c[0], c[4], wgs, _stream()), c[5], c[6])
    print(f'{shape}: max |dW - dW64| / S = {ratio:.3e} pooled, {dense:.3e} dense on g (bound {C.bound(shape):.1e})')
    assert bool((diff <= C.bound(shape) * c[6]).all()), (shape, ratio)
    assert torch.equal(_run(lib, c, wgs, guarded=False), dw), shape                 # a second launch: the same bits


@pytest.mark.parametrize('kind', ('codes 0', 'codes 3', 'one window column'))
def test_every_code_and_one_column_of_windows(lib, kind):
    c = C.case(C.SMALL, kind)
    ratio, diff = C.M.worst(_run(lib, c), c[5], c[6])
    print(f'{kind}: max |dW - dW64| / S = {ratio:.3e} (bound {C.bound(C.SMALL):.1e})')
    assert bool((diff <= C.bound(C.SMALL) * c[6]).all()), (kind, ratio)


def test_every_value_masked_gives_exact_zeros(lib):
    c = C.case(C.SMALL, 'all masked')
    assert float(c[4].abs().max()) == 0.0
    assert float(_run(lib, c).abs().max()) == 0.0


@pytest.mark.parametrize('kind', C.M.STRESS_KINDS)
def test_inputs_that_stress_the_split(lib, kind):
    c = C.stress(kind)
    ratio, diff = C.M.worst(_run(lib, c), c[5], c[6])
    bound = C.bound(C.M.STRESS_SHAPE)                                               # the stress inputs' own shape: dp is their dy
    print(f'{kind}: max |dW - dW64| / S = {ratio:.3e} (bound {bound:.1e})')
    assert bool((diff <= bound * c[6]).all()), (kind, ratio)


def test_the_images_add_up_and_a_wide_call_is_its_64_channel_slices(lib):
    x, dp, p, am, _, ref, scale = C.case(C.SMALL, 'randn')                          # (2, 6, 28, 256, 64)
    dw = C.run(lib, DEV, x, dp, p, am, 2, _stream())
    one = sum(C.run(lib, DEV, x[i:i + 1], dp[i:i + 1], p[i:i + 1], am[i:i + 1], 2, _stream()).double() for i in range(2))
    assert bool(((one - dw.double()).abs() <= 1e-6 * scale).all())
    cl = torch.channels_last
    for s in range(4):                                                              # the same workgroups per slice: the same jobs, the same bits
        xs = x[:, 64 * s:64 * s + 64].contiguous(memory_format=cl)
        assert torch.equal(C.run(lib, DEV, xs, dp, p, am, 2, _stream()), dw[:, 64 * s:64 * s + 64]), s


def test_knob_round_trip_and_who_is_served(lib):
    for v in (0, 1, -1):
        with C.M.Knobs(lib, wrw_pool=v):
            assert C.M.knob(lib, 'wrw_pool') == v
            assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 256, 64) == (1 if v == 1 else 0)         # below what the rule was measured on
            assert lib.hk_conv3x3_wrw_pooled_served(16, 28, 28, 512, 512) == (0 if v == 0 else 1)      # conv5_3 at batch 16: the rule's smallest map
            assert lib.hk_conv3x3_wrw_pooled_served(64, 448, 448, 64, 64) == (0 if v == 0 else 1)      # conv1_2 at batch 64
    with C.M.Knobs(lib, wrw_pool=1):
        assert lib.hk_conv3x3_wrw_pooled_served(2, 7, 28, 256, 64) == 0             # odd H
        assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 27, 256, 64) == 0             # odd W
        assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 96, 64) == 0              # Cin no multiple of 64
        with C.M.Knobs(lib, wrw_split=0):
            assert lib.hk_conv3x3_wrw_pooled_served(2, 6, 28, 256, 64) == 0
        # the kernel's lane offsets are 32-bit bytes into a row: a row of x, or a window row of dp, of 2^31 bytes or more is refused
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, (1 << 20) - 2, 512, 64) == 1
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, 1 << 20, 512, 64) == 0
        assert lib.hk_conv3x3_wrw_pooled_served(1, 2, 1 << 21, 64, 512) == 0
    x, dp, p, am = (t.to(DEV) for t in C.case((1, 2, 2, 64, 64), 'int')[:4])
    ws = torch.empty(lib.hk_conv3x3_wrw_ws_bytes(64, 64), dtype=torch.uint8, device=DEV)
    dw = torch.empty(64 * 9 * 64, device=DEV)
    q = C._p
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 3, 2, 64, 64, q(ws), ws.numel(), None) == -3       # odd H: unsupported
    ws2 = torch.empty(lib.hk_conv3x3_wrw_ws_bytes(512, 64), dtype=torch.uint8, device=DEV)
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 2, 1 << 20, 512, 64, q(ws2), ws2.numel(), None) == -3   # a 2^31-byte row: refused before any launch
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), q(am), q(x), q(dw), 1, 2, 2, 64, 64, q(ws), ws.numel() - 1, None) == -2   # workspace
    assert lib.hk_conv3x3_wrw_pooled(q(dp), q(p), None, q(x), q(dw), 1, 2, 2, 64, 64, q(ws), ws.numel(), None) == -1        # null


def _unpack(aux, cout):
    """bias_relu_pool_fwd's code bytes [N, Ho, Wo, C / 4] -> per-channel codes [N, C, Ho, Wo]."""
    n, ho, wo, _ = aux.shape
    q = aux.to(torch.int64).unsqueeze(-1) >> torch.tensor([0, 2, 4, 6])
    return (q & 3).reshape(n, ho, wo, cout).permute(0, 3, 1, 2)


def test_a_stack_with_two_pooled_layers_routes_them_and_stays_within_the_bound(lib, monkeypatch):
    import hawkeye_amd.functional as F
    from conv_epilogue_cases import make_stack
    knobs = dict(conv_fwd=1, conv_bwd_data=1, conv_wrw=1, wrw_split=1, wrw_wide=1, conv_epi=2)
    stack, x, dy = make_stack(DEV)
    convs = [m for m in stack if isinstance(m, torch.nn.Conv2d)]
    seen = []
    real = F.conv3x3_wrw_pooled_raw
    monkeypatch.setattr(F, 'conv3x3_wrw_pooled_raw', lambda *a: (seen.append([t.detach().clone() for t in a] + [real(*a)]), seen[-1][-1])[1])

    def grads(pool):
        with C.M.Knobs(lib, wrw_pool=pool, **knobs):
            stack.zero_grad(set_to_none=True)
            stack(x.clone().requires_grad_(True)).backward(dy)
        return [m.weight.grad.detach().clone().cpu() for m in convs]

    on = grads(1)
    assert len(seen) == 2                                                           # the two pooled layers, and only they
    off = grads(0)
    assert len(seen) == 2
    for xx, dp, p, aux, dw in seen:
        xx, dp, p, dw = xx.cpu(), dp.cpu(), p.cpu(), dw.cpu()
        shape = (xx.shape[0], xx.shape[2], xx.shape[3], xx.shape[1], dp.shape[1])
        g = C.full_gradient(dp, p, _unpack(aux.cpu(), dp.shape[1]))
        ref, scale = C.M._ref64(xx, g)
        ratio, diff = C.M.worst(dw, ref, scale)
        layer = 1 if shape[3] == 64 else 3
        dense = C.M.worst(off[layer], ref, scale)
        print(f'stack layer {layer} {shape}: max |dW - dW64| / S = {ratio:.3e} pooled, {dense[0]:.3e} dense on g (bound {C.bound(shape):.1e})')
        assert bool((diff <= C.bound(shape) * scale).all()), (shape, ratio)
        assert bool((dense[1] <= C.bound(shape) * scale).all()), (shape, dense[0])
        assert torch.equal(on[layer], dw)
    assert torch.equal(on[0], off[0]) and torch.equal(on[2], off[2])                # g is what it was: the other layers keep their bits
