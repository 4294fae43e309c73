"""NTS-Net, host side: opt-in registration, the constructor's contract and the state_dict against the reference's key
list, the anchor table against the reference's, the functional wrappers' refusals, the loss module's contract, the
synthetic yaml and the golden tool's --check.  No GPU."""
import copy
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hawkeye_amd.model  # noqa: F401
from hawkeye_amd.config import CfgNode
from hawkeye_amd.model.registry import MODEL, install_into
from hawkeye_amd.utils.repository import Repository

import nts_inputs as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = json.load(open(os.path.join(HERE, 'golden', 'nts_state_dict.json')))
PLUGIN_MODULES = ('hawkeye_amd.model.methods.NTSNet', 'hawkeye_amd.examples.NTSNet')
CONFIG = dict(name='NTSNet', image_size=224, proposal_num=6, cat_num=4)


def forget_plugin():
    MODEL.pop('NTSNet', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


@pytest.fixture
def plugin():
    """The opt-in import, undone afterwards: the registry other tests see holds the default plugins only."""
    assert 'NTSNet' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    forget_plugin()


def test_absent_from_the_default_registry_and_registered_by_the_import():
    default = ['APCNN', 'BCNN', 'CBCNN', 'CIN', 'MPN', 'OSMENet', 'ResNet101', 'ResNet50']       # what tests/test_models_cpu.py pins
    assert sorted(MODEL) == default and sorted(install_into(Repository())) == default
    mod = importlib.import_module(PLUGIN_MODULES[0])
    try:
        assert sorted(MODEL) == sorted(default + ['NTSNet']) and MODEL.get('NTSNet') is mod.NTSNet
        ref = Repository()
        install_into(ref)
        assert ref['NTSNet'] is mod.NTSNet
    finally:
        forget_plugin()
    assert sorted(MODEL) == default


@pytest.fixture
def net(plugin):
    torch.manual_seed(0)
    return plugin.NTSNet(CfgNode(CONFIG))


def test_constructor_contract_state_dict_and_deepcopy(net):
    assert (net.topN, net.proposal_num, net.CAT_NUM, net.image_size, net.pad_side) == (6, 6, 4, 224, 224)
    assert isinstance(net.pretrained_model.avgpool, torch.nn.AdaptiveAvgPool2d) and net.pretrained_model.avgpool.output_size == 1
    assert tuple(net.pretrained_model.fc.weight.shape) == (200, 2048)
    assert tuple(net.concat_net.weight.shape) == (200, 2048 * 5) and tuple(net.partcls_net.weight.shape) == (200, 2048)
    assert [n for n, _ in net.proposal_net.named_children()] == ['down1', 'down2', 'down3', 'ReLU', 'tidy1', 'tidy2', 'tidy3']
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == KEYS['state_dict']
    assert [n for n, _ in net.named_children()] == KEYS['children'] == ['pretrained_model', 'proposal_net', 'concat_net', 'partcls_net']
    assert sum(p.numel() for p in net.parameters()) == KEYS['n_params']
    assert isinstance(net.edge_anchors, np.ndarray) and net.edge_anchors.shape == (426, 4) and net.edge_anchors.dtype.kind == 'i'
    twin = copy.deepcopy(net)
    for (ka, va), (kb, vb) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert ka == kb and torch.equal(va, vb) and va.data_ptr() != vb.data_ptr()
    assert torch.equal(twin._anchors, net._anchors) and net._anchors.dtype == torch.int32


def test_bad_configurations_raise(plugin, monkeypatch):
    monkeypatch.setattr(plugin, 'resnet50', lambda pretrained=True: torch.nn.Module())
    with pytest.raises(ValueError, match='cat_num'):
        plugin.NTSNet(CfgNode(dict(CONFIG, cat_num=7)))
    with pytest.raises(ValueError, match='cat_num'):
        plugin.NTSNet(CfgNode(dict(CONFIG, cat_num=0)))


@pytest.mark.parametrize('size', [224, 448])
def test_anchor_table_equals_the_reference_table(plugin, size):
    z = T.load()
    table = (plugin.default_edge_anchors(size) + np.float32(224)).astype(int)
    assert table.shape == ((426, 4) if size == 224 else (1614, 4))
    assert np.array_equal(table, z[f'anchors_{size}'])
    per_level = [(-(-size // s)) ** 2 * len(sc) * 3 for s, _, sc in plugin.LEVELS]          # the proposal net's channel counts: 6, 6, 9
    assert sum(per_level) == len(table) and [len(sc) * 3 for _, _, sc in plugin.LEVELS] == [6, 6, 9]


def test_model_attribute_holds_the_padded_table_and_the_buffer_the_image_one(net):
    z = T.load()
    assert np.array_equal(net.edge_anchors, z['anchors_224'])
    assert np.array_equal(net._anchors.numpy(), z['anchors_224'] - 224)
    assert '_anchors' not in net.state_dict()


def test_functional_wrappers_refuse_bad_arguments():
    import hawkeye_amd.functional as F
    from hawkeye_amd._lib import HawkeyeHipError
    from hawkeye_amd.model.loss import NTSLoss
    scores, anchors = torch.randn(2, 5), torch.zeros(5, 4, dtype=torch.int32)
    images, boxes = torch.randn(2, 3, 8, 8), torch.zeros(2, 3, 4, dtype=torch.int32)
    raw, cat, part, prob, y = torch.randn(2, 7), torch.randn(2, 7), torch.randn(2, 3, 7), torch.randn(2, 3), torch.zeros(2, dtype=torch.long)
    crit = NTSLoss(CfgNode(dict(name='NTSLoss', proposal_num=3)))
    assert crit.PROPOSAL_NUM == 3
    for call in (lambda: F.nts_nms(scores, anchors, 3), lambda: F.nts_crop_resize(images, boxes, 4, 6),
                 lambda: F.nts_loss(raw, cat, part, prob, y), lambda: F.nts_loss_with_parts(raw, cat, part, prob, y),
                 lambda: crit([raw, cat, part, None, prob], y)):
        with pytest.raises(HawkeyeHipError, match='CPU tensor'):                      # device: no CPU fallback
            call()
    bad = [
        (lambda: F.nts_nms(scores[0], anchors, 3), r'\[B, A\]'),
        (lambda: F.nts_nms(scores, anchors[:4], 3), 'anchors must have the shape'),
        (lambda: F.nts_nms(scores, anchors.float(), 3), 'integers'),
        (lambda: F.nts_nms(scores.double(), anchors, 3), 'fp32'),
        (lambda: F.nts_nms(scores, anchors, 0), 'topn'),
        (lambda: F.nts_crop_resize(images[0], boxes, 4, 6), r'\[B, C, H, W\]'),
        (lambda: F.nts_crop_resize(images, boxes[:1], 4, 6), 'boxes must have the shape'),
        (lambda: F.nts_crop_resize(images, boxes.float(), 4, 6), 'integers'),
        (lambda: F.nts_crop_resize(images, boxes, -1, 6), 'pad'),
        (lambda: F.nts_crop_resize(images, boxes, 4, (6, 0)), 'size'),
        (lambda: F.nts_loss(raw, cat[:, :5], part, prob, y), 'one shape'),
        (lambda: F.nts_loss(raw, cat, part[:, :, :5], prob, y), 'part_logits'),
        (lambda: F.nts_loss(raw, cat, part, prob[:, :2], y), 'top_n_prob'),
        (lambda: F.nts_loss(raw, cat, part, prob, y[:1]), 'labels of shape'),
        (lambda: F.nts_loss(raw, cat, part, prob, y.float()), 'integers'),
        (lambda: F.nts_loss(raw.double(), cat.double(), part, prob, y), 'fp32'),
    ]
    for call, message in bad:
        with pytest.raises(HawkeyeHipError, match=message):
            call()
    with pytest.raises(ValueError, match='proposal_num'):
        crit([raw, cat, part[:, :2], None, prob[:, :2]], y)


def test_host_side_queries_need_no_gpu():
    from hawkeye_amd import _lib
    lib = _lib.load()
    assert lib.hk_nts_loss_ws_bytes(4, 6, 200) >= (4 * 8 + 2 * 24) * 4
    assert lib.hk_nts_loss_ws_bytes(0, 6, 200) == 0 and lib.hk_nts_loss_ws_bytes(4, 0, 200) == 0 and lib.hk_nts_loss_ws_bytes(4, 6, 0) == 0
    assert len([n for n in _lib.SIGNATURES if n.startswith('hk_nts_')]) == 4


def test_synthetic_yaml_parses_and_names_the_plugin():
    cfg = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'NTSNet_synthetic.yaml')))
    ref = CfgNode.load_cfg(open(os.path.join(HERE, 'golden', 'reference_configs', 'NTSNet.yaml')))
    assert {k: cfg.model[k] for k in ref.model} == dict(ref.model) and cfg.model.num_classes == 200 and cfg.train.optimizer == ref.train.optimizer and cfg.train.scheduler == ref.train.scheduler
    assert cfg.train.criterion == ref.train.criterion and cfg.dataset.batch_size == ref.dataset.batch_size == 4
    assert cfg.dataset.name == 'synthetic' and cfg.model.name == 'NTSNet'


def test_trainer_builds_adam_and_the_warmup_cosine_schedule(plugin):
    ex = importlib.import_module(PLUGIN_MODULES[1])
    tr = ex.NTSTrainer.__new__(ex.NTSTrainer)
    tr.model = torch.nn.Linear(3, 2)
    tr.optimizer = tr.get_optimizer(CfgNode(dict(name='Adam', lr=0.0004, weight_decay=0.00002)))
    tr.scheduler = tr.get_scheduler(CfgNode(dict(name='', T_max=200, warmup_epochs=10, lr_warmup_decay=0.01)))
    assert isinstance(tr.optimizer, torch.optim.Adam) and tr.optimizer.defaults['weight_decay'] == 0.00002
    assert isinstance(tr.get_criterion(CfgNode(dict(name='NTSLoss', proposal_num=6))), ex.NTSLoss)
    lrs = []
    for _ in range(12):
        lrs.append(tr.optimizer.param_groups[0]['lr'])
        tr.optimizer.step()
        tr.scheduler.step()
    assert lrs[0] == pytest.approx(4e-6) and lrs[10] == pytest.approx(4e-4) and lrs[11] < lrs[10]
    assert all(a < b for a, b in zip(lrs[:10], lrs[1:11]))


def test_golden_inputs_are_a_pure_function_of_the_recipe_and_the_files_are_small():
    z = T.load()
    a, b = T.loss_inputs(3, 3, 6, 200), T.loss_inputs(3, 3, 6, 200)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[2].shape == (3, 6, 200) and a[2].dtype == np.float32
    largest = max(os.path.getsize(os.path.join(HERE, 'golden', f)) for f in os.listdir(os.path.join(HERE, 'golden'))
                  if f.endswith('.npz') and not f.startswith('nts_'))
    for f in T.FILES:
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= largest
    for case in T.load_nms_cases(z):
        s = case['scores']
        assert s.shape == (case['B'], len(case['anchors'])) and all(len(np.unique(row)) == len(row) for row in s)       # no ties
        assert np.array_equal(np.stack([T.nms_trace(row, case['anchors'])[0] for row in s]), case['index'])
        if case['kind'] == 'quarter':                       # the winner's IoU-exactly-0.25 partners hold the next scores and are gone
            for row, index in zip(s, case['index']):
                partners = T.quarter_partners(case['anchors'], index[0])
                assert len(partners) >= 2 and set(np.argsort(-row)[1:1 + len(partners)]) == set(partners)
                assert not np.isin(partners, index).any()
    for case in T.load_loss_cases(z):
        assert case['loss_f64'].dtype == np.float64 and case['loss_f32'].dtype == np.float32 and case['indicator'].dtype == bool
        assert case['indicator'].shape == (case['B'], case['N'], case['N'])
        if case['B'] * case['N'] >= 18:                     # active and inactive hinges behind a true indicator
            s = case['prob'].astype(np.float64)
            gated = (1 - s[:, :, None] + s[:, None, :])[case['indicator']]
            assert (gated > 0).any() and (gated < 0).any()


def reference_dir():
    d = os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference'))
    return d if os.path.isfile(os.path.join(d, 'model', 'methods', 'NTS_Net', 'NTSNet.py')) else None


@pytest.mark.skipif(reference_dir() is None, reason='the reference checkout is not present')
def test_golden_tool_check_reproduces_the_committed_bytes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_nts_golden.py'), '--check', '--reference', reference_dir()],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.count('identical') == len(T.FILES) + 1 and 'DIFFERENT' not in r.stdout
