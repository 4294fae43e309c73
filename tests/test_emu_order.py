"""CPU tier: order independence of every barrier-synchronised kernel that tests/test_emu_fuzz.py's order test (Gram pooling, CBP,
the MPN chain, attention pooling, ROI selection) does not reach: csrc/conv_fwd.hip, the three forms of csrc/conv_wrw.hip, the trunk
epilogues and the first-convolution kernels, the three CIN forms, the classifier kernels, the fused pool + classifier backward,
csrc/mamc.hip, the LDS form of the ROI backward, both forms of the peer loss and the DCL / NTS / CrossX / APINet heads and losses.

The emulator (tests/emu) switches work-items at barriers and wave collectives only, so one fixed resume order hides a race.  Each
case runs in the default order, then again with HK_EMU_ORDER = rev or rand:11: every output must keep its bits.  A kernel whose
lanes exchange data through LDS inside one wave, with no workgroup barrier, says so with HK_WAVE_SYNC() - the emulator switches
fibers there; any other difference is a missing barrier in the kernel.  Shapes: the smallest at which the kernel's pipeline takes
all its steps (two chunks, a strip boundary, the flush after 32 row steps, each CIN form).  What the check reaches, measured by
taking single barriers out, is written down in DESIGN.md."""
import numpy as np
import pytest
import torch

from conv_fwd_cases import case as conv_case
from emu.harness import emulated

ORDERS = ('rev', 'rand:11')
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated() as f:
        yield f


def _tensors(d):
    """The dicts of numpy results that the shared ops modules return -> tensors, in the order of their names."""
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(d[k]))) for k in sorted(d)]


def _same_bits(key, run, order, monkeypatch):
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    base = [t.detach().clone() for t in run()]
    monkeypatch.setenv('HK_EMU_ORDER', order)
    other = run()
    assert len(other) == len(base) and len(other) > 0
    for i, (p, q) in enumerate(zip(base, other)):
        assert p.shape == q.shape and torch.equal(p, q.detach()), (key, order, i)      # (torch.equal: a NaN would fail it, too)


# ------------------------------------------------------------------------------------------------------ convolutions
def run_conv3x3(F, tune):
    """(2, 7, 34, 128, 64): two K chunks (the x tile is replaced under the barrier pair at tap 8), a halo across a strip boundary,
    ragged row and column tiles; the input gradient is the same kernel behind the other weight pre-pass."""
    x, wt, dy = conv_case((2, 7, 34, 128, 64))[:3]
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    return [F.conv3x3_fwd_raw(x, wt), F.conv3x3_bwd_data_raw(dy, wt)]


WRW_FORMS = {'fp32': (64, 0), 'split': (64, 1), 'wide': (128, 1)}      # Cin, wrw_split


def run_conv3x3_wrw(F, tune, form):
    """One workgroup per slice walks 12 jobs, 54 row steps: the ring of x rows and the two dy buffers turn over under one barrier
    per step, and the split forms add their accumulators to the partial after 32 steps."""
    cin, split = WRW_FORMS[form]
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, 9, 70, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(2, 64, 9, 70, generator=g).contiguous(memory_format=torch.channels_last)
    tune('wrw_wgs', 1)
    tune('wrw_split', split)
    return [F.conv3x3_wrw_raw(x, dy)]


def run_trunk(F, tune, which):
    g = torch.Generator().manual_seed(21)
    if which == 'conv1_bias_relu':
        x = torch.randn(2, 3, 9, 13, generator=g).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(64, 3, 3, 3, generator=g) * 0.3).requires_grad_(True)
        b = (torch.randn(64, generator=g) * 0.2).requires_grad_(True)
        y = F.conv1_bias_relu(x, w, b)
        y.backward(torch.randn(2, 64, 9, 13, generator=g).contiguous(memory_format=torch.channels_last))
        return [y.detach(), w.grad, b.grad]
    x = (torch.randn(2, 64, 8, 8, generator=g) - 0.3).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b = (torch.randn(64, generator=g) * 0.3).requires_grad_(True)
    pool = which == 'bias_relu_pool'
    y = (F.bias_relu_pool if pool else F.bias_relu)(x * 1.0, b)
    y.backward(torch.randn(2, 64, 4 if pool else 8, 4 if pool else 8, generator=g).contiguous(memory_format=torch.channels_last))
    return [y.detach(), x.grad, b.grad]                    # b.grad: the partial sums of a workgroup go through static LDS


# ---------------------------------------------------------------------------------------------------------- heads
CIN_SHAPES = {'flash': (2, 128, 49), 'stored-score': (2, 128, 100), 'generic': (2, 70, 25)}


def run_cin(F, tune, form):
    b, c, hw = CIN_SHAPES[form]
    g = torch.Generator().manual_seed(c + hw)
    x = torch.relu(torch.randn(b, c, hw, generator=g)).requires_grad_(True)
    wt = torch.randn(b, generator=g).requires_grad_(True)
    y, w = F.cin_sci(x)
    yc = F.cin_cci(w, x, wt)
    ((y * torch.randn(b, c, hw, generator=g)).sum() + (yc * torch.randn(b, c, hw, generator=g)).sum()).backward()
    return [y.detach(), w.detach(), yc.detach(), x.grad, wt.grad]


def run_classifier(F, tune, which):
    g = torch.Generator().manual_seed(31)
    if which == 'linear':
        y = torch.randn(3, 1000, generator=g).requires_grad_(True)
        w = (torch.randn(7, 1000, generator=g) / 32).requires_grad_(True)
        b = torch.randn(7, generator=g).requires_grad_(True)
        out = F.linear(y, w, b)
        (out * torch.randn(3, 7, generator=g)).sum().backward()
        return [out.detach(), y.grad, w.grad, b.grad]
    x = torch.relu(torch.randn(2, 128, 14, 14, generator=g)).requires_grad_(True)
    if which == 'signed_sqrt_pool':
        y = F.bilinear_pool(x, signed_sqrt=True)
        (y * torch.randn(y.shape, generator=g)).sum().backward()
        return [y.detach(), x.grad]
    w = (torch.randn(7, 128 * 128, generator=g) * 0.05).requires_grad_(True)       # the fused pool + classifier: bwd3 with the rank-1 fold
    b = (torch.randn(7, generator=g) * 0.1).requires_grad_(True)
    out = F.bilinear_pool_linear(x, w, b)
    torch.nn.functional.cross_entropy(out, torch.tensor([3, 5])).backward()
    return [out.detach(), x.grad, w.grad, b.grad]


def run_npairs(F, tune):
    g = torch.Generator().manual_seed(41)
    x = torch.randn(8, 3, 200, generator=g).requires_grad_(True)
    loss = F.npairs_loss(x, torch.tensor([0, 1, 2, 0, 1, 2, 3, 3]))
    loss.backward()
    return [loss.detach(), x.grad]


def run_roi_lds(F, tune, mode):
    """The inputs of test_roi_crop_backward_lds_variant_bit_identical, the LDS variant alone (roi_bwd 0)."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 10, 56, 56, generator=g).requires_grad_(True)
    wt = torch.randn(4, 10, 56, 56, generator=g)
    box = torch.tensor([[3.2, 5.9, 40.1, 33.3], [0., 0., 56., 56.], [20.5, 21.5, 24.4, 25.9], [10., 2., 55.9, 17.2]])
    drop = torch.tensor([[10., 12., 20., 30.], [0., 0., -1., -1.], [0., 0., -1., -1.], [12., 3., 30., 9.]])
    tune('roi_bwd', 0)
    y = F.roi_crop_resize(x, box, drop, mode == 'train')
    (y * wt).sum().backward()
    return [y.detach(), x.grad]


def run_peer(F, tune, form):
    import peer_inputs
    l1, l2, y = peer_inputs.peer_inputs(7, 65, 37)         # CASES[3]'s shape: N no multiple of the rows per block; fits the resident form
    l1, l2 = torch.from_numpy(l1).requires_grad_(True), torch.from_numpy(l2).requires_grad_(True)
    tune('peer_form', form)
    loss_1, loss_2, stats = F.peer_learning_loss_with_stats(l1, l2, torch.from_numpy(y), 0.5)
    (loss_1 + loss_2).backward()
    return [loss_1.detach(), loss_2.detach(), l1.grad, l2.grad, stats.float()]


def _dcl_head():
    import dcl_inputs
    import dcl_ops
    return _tensors(dcl_ops.run_head(dcl_inputs.head_inputs((2, 70, 7, 7)), CPU))


def _dcl_loss():
    import dcl_ops
    return _tensors(dcl_ops.run_loss(dcl_ops.LOSS_CASES[0], CPU))


def _nts_nms():
    import nts_ops
    rs = np.random.RandomState(41)
    index, boxes = nts_ops.run_nms(rs.randint(0, 23, (2, 70)).astype(np.float32) / 8, nts_ops.small_table(70, 40), CPU)     # tied scores
    return [torch.from_numpy(index), torch.from_numpy(boxes)]


def _nts_loss():
    import nts_ops
    return _tensors(nts_ops.run_loss(nts_ops.LOSS_CASES[1], CPU))


def _crossx_me(case):
    import crossx_inputs
    import crossx_ops
    return _tensors(crossx_ops.run_me(crossx_inputs.me_inputs(case), case[4], CPU))


def _crossx_loss():
    import crossx_ops
    return _tensors(crossx_ops.run_loss(crossx_ops.LOSS_CASES[1], CPU))


def _apinet_interact():
    import apinet_ops
    return _tensors(apinet_ops.check_interact(CPU, 5, 70))


def _apinet_loss():
    import apinet_ops
    got = apinet_ops.check_loss(CPU, 8, 257, 'mixed')[0]
    return _tensors({k: np.asarray(v, dtype=np.float32) for k, v in got.items()})


PLUGIN_HEADS = {
    'dcl_head': _dcl_head, 'dcl_loss': _dcl_loss, 'nts_nms': _nts_nms, 'nts_loss': _nts_loss,
    'crossx_me_avg': lambda: _crossx_me((2, 2, 8, 196, 'avg')), 'crossx_me_max': lambda: _crossx_me((3, 1, 5, 49, 'max')),
    'crossx_loss': _crossx_loss, 'apinet_interact': _apinet_interact, 'apinet_loss': _apinet_loss,
}


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize('order', ORDERS)
def test_conv3x3_forward_and_input_gradient(F, order, monkeypatch, tune):
    _same_bits('conv3x3', lambda: run_conv3x3(F, tune), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('form', list(WRW_FORMS))
def test_conv3x3_weight_gradient(F, form, order, monkeypatch, tune):
    _same_bits('wrw ' + form, lambda: run_conv3x3_wrw(F, tune, form), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('which', ['bias_relu', 'bias_relu_pool', 'conv1_bias_relu'])
def test_trunk_epilogues_and_first_convolution(F, which, order, monkeypatch, tune):
    _same_bits('trunk ' + which, lambda: run_trunk(F, tune, which), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('form', list(CIN_SHAPES))
def test_cin_channel_interaction(F, form, order, monkeypatch, tune):
    _same_bits('cin ' + form, lambda: run_cin(F, tune, form), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('which', ['linear', 'signed_sqrt_pool', 'bilinear_pool_linear'])
def test_classifier_and_fused_pool_classifier(F, which, order, monkeypatch, tune):
    _same_bits('classifier ' + which, lambda: run_classifier(F, tune, which), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
def test_npairs_loss(F, order, monkeypatch, tune):
    _same_bits('npairs', lambda: run_npairs(F, tune), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_roi_crop_backward_lds_variant(F, mode, order, monkeypatch, tune):
    _same_bits('roi ' + mode, lambda: run_roi_lds(F, tune, mode), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('form', [1, 2], ids=['general', 'resident'])
def test_peer_loss(F, form, order, monkeypatch, tune):
    _same_bits(f'peer {form}', lambda: run_peer(F, tune, form), order, monkeypatch)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('which', list(PLUGIN_HEADS))
def test_plugin_heads_and_losses(F, which, order, monkeypatch, tune):
    _same_bits('plugin ' + which, PLUGIN_HEADS[which], order, monkeypatch)
