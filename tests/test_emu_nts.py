"""CPU tier: csrc/nts.hip compiled for the host (tests/emu) - every golden NMS, crop and loss case of the reference, the
NMS rules the goldens cannot hold (ties, a table that is no multiple of 64, the fill), the C ABI's error returns, an
unaligned output, an out-of-range label, bit-identical reruns, and a two-step NTSTrainer run with a stub trunk.  Test
infrastructure only."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from emu.harness import emulated

import nts_inputs as T
import nts_ops as O

HERE = os.path.dirname(os.path.abspath(__file__))
PLUGIN_MODULES = ('hawkeye_amd.model.methods.NTSNet', 'hawkeye_amd.examples.NTSNet')
CPU = torch.device('cpu')


@pytest.fixture(autouse=True, scope='module')
def _emulated_kernels():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated():
        yield


@pytest.mark.parametrize('case', O.NMS_CASES, ids=T.nms_case_id)
def test_golden_nms_cases(case):
    O.check_nms_case(case, CPU)


def test_nms_equal_scores_go_to_the_highest_index():
    O.check_nms_ties(CPU)


@pytest.mark.parametrize('a,b', [(70, 2), (5, 1), (256, 1), (257, 2), (2048, 1)])
def test_nms_on_tables_of_other_sizes_against_float64(a, b):
    O.check_nms_table(CPU, a, b, seed=40 + a)


def test_nms_fills_with_the_last_pick_when_fewer_than_topn_survive():
    O.check_nms_fill(CPU)


@pytest.mark.parametrize('case', O.CROP_CASES, ids=lambda c: f"out{c['out'][0]}x{c['out'][1]}")
def test_golden_crop_cases(case):
    O.check_crop_case(case, CPU)


@pytest.mark.parametrize('out', [(8, 12), (5, 7), (1, 4), (3, 1)])
def test_crop_boxes_across_every_edge_against_float64(out):
    O.check_crop_shapes(CPU, out)


def test_crop_into_an_unaligned_output():
    O.check_crop_unaligned_output(CPU)


@pytest.mark.parametrize('case', O.LOSS_CASES, ids=T.loss_case_id)
def test_golden_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, CPU):.3f}')


def test_loss_gradients_scale_exactly_and_take_their_own_routes():
    O.check_loss_scaling(O.LOSS_CASES[2], CPU)
    O.check_loss_gradient_routes(O.LOSS_CASES[1], CPU)


def test_label_out_of_range_reads_nothing_and_gives_nan():
    O.check_loss_bad_labels(CPU)


def test_strided_inputs_give_the_bits_of_dense_ones():
    O.check_noncontiguous(CPU)
    O.check_crop_shapes(CPU, (8, 12), strided=True)


def test_two_runs_agree_bit_for_bit():
    first, again = O.run_loss(O.LOSS_CASES[2], CPU), O.run_loss(O.LOSS_CASES[2], CPU)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    a, b = O.check_crop_shapes(CPU, (5, 7)), O.check_crop_shapes(CPU, (5, 7))
    assert torch.equal(a, b)
    assert np.array_equal(O.check_nms_table(CPU, 70, 2, seed=3), O.check_nms_table(CPU, 70, 2, seed=3))


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_abi_errors():
    from hawkeye_amd import _lib
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    bad, big = _lib.HK_ERR_BAD_ARG, _lib.HK_ERR_UNSUPPORTED
    b, a, topn = 2, 2049, 3
    scores, anchors = torch.randn(b, a), torch.from_numpy(O.small_table(a, 1))
    index, boxes = torch.zeros(b, topn, dtype=torch.int32), torch.zeros(b, topn, 4, dtype=torch.int32)
    assert lib.hk_nts_nms(p(scores), p(anchors), p(index), p(boxes), b, a, topn, 0.25, None) == big              # A above 2048
    assert lib.hk_nts_nms(z, p(anchors), p(index), p(boxes), b, 5, topn, 0.25, None) == bad
    assert lib.hk_nts_nms(p(scores), p(anchors), p(index), z, b, 5, topn, 0.25, None) == bad
    for bb, aa, tt in ((0, 5, topn), (b, 0, topn), (b, 5, 0)):
        assert lib.hk_nts_nms(p(scores), p(anchors), p(index), p(boxes), bb, aa, tt, 0.25, None) == bad
    assert lib.hk_nts_nms(p(scores), p(anchors), p(index), p(boxes), b, 5, topn, float('nan'), None) == bad
    assert not index.any() and not boxes.any()                                                                   # nothing launched
    assert lib.hk_nts_nms(p(scores), p(anchors), p(index), p(boxes), b, 2048, topn, 0.25, None) == _lib.HK_OK and boxes.any()

    images, bx, out = torch.randn(2, 3, 8, 8), torch.zeros(2, 3, 4, dtype=torch.int32), torch.zeros(6, 3, 4, 4)
    bx[..., 2:] = 8

    def crop(first=p(images), B=2, N=3, C=3, H=8, W=8, pad=2, oh=4, ow=4):
        return lib.hk_nts_crop_resize(first, p(bx), p(out), B, N, C, H, W, pad, oh, ow, None)
    assert crop(first=z) == bad
    for kw in (dict(B=0), dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(pad=-1), dict(oh=0), dict(ow=0)):
        assert crop(**kw) == bad
    assert crop(B=40000) == big                                                                                  # B N above the grid's 65535
    assert not out.any()
    assert crop() == _lib.HK_OK and out.any()

    B, N, C = 2, 3, 5
    raw, cat, part, prob = torch.randn(B, C), torch.randn(B, C), torch.randn(B, N, C), torch.randn(B, N)
    y = torch.zeros(B, dtype=torch.int32)
    loss, g = torch.zeros(5), [torch.zeros(B, C), torch.zeros(B, C), torch.zeros(B, N, C), torch.zeros(B, N)]
    need = lib.hk_nts_loss_ws_bytes(B, N, C)
    assert need > 0 and lib.hk_nts_loss_ws_bytes(1 << 21, 6, C) == 0
    ws = torch.zeros(need, dtype=torch.uint8)

    def call(smoothing=0.1, nbytes=need, first=p(raw), rows=B, last=p(g[3])):
        return lib.hk_nts_loss(first, p(cat), p(part), p(prob), p(y), smoothing, p(loss), p(g[0]), p(g[1]), p(g[2]), last, rows, N, C,
                               p(ws), nbytes, None)
    for smoothing in (-0.1, 1.5, float('nan')):
        assert call(smoothing=smoothing) == bad
    assert call(first=z) == bad and call(last=z) == bad and call(rows=0) == bad
    assert call(rows=1 << 21) == big
    assert call(nbytes=need - 1) == _lib.HK_ERR_WORKSPACE
    assert not loss.any() and not any(t.any() for t in g)
    assert call() == _lib.HK_OK and g[2].any() and torch.isfinite(loss).all()


class TinyTrunk(torch.nn.Module):
    """A stand-in for ResNet-50 with its attribute names: 224 x 224 -> a 7 x 7 map of 16 channels."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 16, 7, stride=8, padding=3)
        self.bn1, self.relu = torch.nn.Identity(), torch.nn.ReLU()
        self.maxpool = torch.nn.MaxPool2d(4, 4)
        self.layer1 = self.layer2 = self.layer3 = torch.nn.Identity()
        self.layer4 = torch.nn.Conv2d(16, 16, 1)
        self.avgpool, self.fc = torch.nn.Identity(), torch.nn.Identity()


def test_two_step_trainer_run_with_a_stub_trunk(tmp_path, monkeypatch):
    """NTSTrainer from configs/NTSNet_synthetic.yaml with a tiny stand-in trunk: two steps through nts_nms,
    nts_crop_resize and nts_loss on the emulated kernels - a finite loss, gradients on the navigator, the scrutinizer,
    the teacher's classifier and the trunk, and a validation pass."""
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.registry import MODEL
    from hawkeye_amd.train import Trainer
    assert 'NTSNet' not in MODEL
    ex = importlib.import_module(PLUGIN_MODULES[1])               # the trainer does the opt-in import of the plugin
    plugin = sys.modules[PLUGIN_MODULES[0]]
    try:
        assert 'NTSNet' in MODEL
        monkeypatch.setattr(Trainer, 'select_device', lambda self, cfg: torch.device('cpu'))
        monkeypatch.setattr(plugin, 'FEATURES', 16)
        monkeypatch.setattr(plugin, 'CLASSES', 5)
        monkeypatch.setattr(plugin, 'resnet50', lambda pretrained=True: TinyTrunk())
        cfg = CfgNode.load_cfg(open(os.path.join(os.path.dirname(HERE), 'configs', 'NTSNet_synthetic.yaml')))
        cfg.dataset.samples, cfg.dataset.batch_size, cfg.dataset.num_workers = 4, 2, 0
        cfg.model.proposal_num, cfg.model.cat_num, cfg.train.criterion.proposal_num, cfg.model.num_classes = 3, 2, 3, 5
        cfg.experiment.log_dir = str(tmp_path)
        cfg.train.optimizer.lr = 1e-2
        cfg.freeze()
        tr = ex.NTSTrainer(cfg)
        net = tr.model
        assert isinstance(tr.criterion, ex.NTSLoss) and net.topN == 3 and tuple(net.concat_net.weight.shape) == (5, 48)
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        seen, step = [], tr.optimizer.step

        def recording_step(*a, **k):
            seen.append({n: float(q.grad.abs().max()) for n, q in net.named_parameters() if q.grad is not None})
            return step(*a, **k)
        monkeypatch.setattr(tr.optimizer, 'step', recording_step)
        outputs = []
        forward = net.forward
        monkeypatch.setattr(net, 'forward', lambda x: outputs.append(forward(x)) or outputs[-1])
        tr.train()
        assert len(seen) == 2
        for grads in seen:
            for name in ('proposal_net.down1.weight', 'proposal_net.down1.bias', 'concat_net.weight', 'partcls_net.bias',
                         'pretrained_model.conv1.weight', 'pretrained_model.fc.weight'):
                assert np.isfinite(grads[name]) and grads[name] > 0, name
        raw, cat, part, index, prob = outputs[0]
        assert raw.shape == (2, 5) and cat.shape == (2, 5) and part.shape == (2, 3, 5) and prob.shape == (2, 3)
        assert index.dtype == torch.int64 and index.shape == (2, 3) and int(index.min()) >= 0 and int(index.max()) < 426
        loss = tr.performance_meters['train']['loss'].values
        assert len(loss) == 1 and np.isfinite(loss[0])
        assert len(tr.performance_meters['val']['acc'].values) == 1
        after = net.state_dict()
        for k in ('proposal_net.down1.weight', 'concat_net.weight', 'partcls_net.weight', 'pretrained_model.conv1.weight'):
            assert not torch.equal(before[k], after[k]), k
    finally:
        MODEL.pop('NTSNet', None)
        for name in PLUGIN_MODULES:
            sys.modules.pop(name, None)
