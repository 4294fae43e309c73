"""CPU tier, no kernels: the MGE-CNN plugin's contracts - opt-in registration, the reference's state_dict keys and children,
`get_params` partitioning the parameters as the reference does, construction from the reference's yaml, the argument checks of
the functional layer, the agreement of include/hawkeye_mge.h, hawkeye_amd/_lib.py: MGE_SIGNATURES and the built library, the
criterion's contract, the trainer's parameter groups and the synthetic yaml."""
import importlib
import os
import re
import sys

import pytest
import torch

import mge_inputs as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLUGIN_MODULES = ('hawkeye_amd.model.methods.MGE_CNN', 'hawkeye_amd.examples.MGE_CNN')


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    import hawkeye_amd.model  # noqa: F401
    assert 'MGE_CNN' not in MODEL                          # importing hawkeye_amd.model alone does not register it
    yield importlib.import_module(PLUGIN_MODULES[0])
    MODEL.pop('MGE_CNN', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def short(plugin, monkeypatch, **over):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.backbone import ResNet, Bottleneck
    c = T.MODEL_CASE
    monkeypatch.setattr(plugin, 'resnet50', lambda pretrained=False, **kw: ResNet(Bottleneck, list(c['layers'])))
    cfg = dict(num_classes=c['classes'], box_thred=c['box_thred'], image_size=c['size'])
    cfg.update(over)
    return plugin.MGE_CNN(CfgNode(cfg))


def test_registration_is_opt_in(plugin):
    from hawkeye_amd.model.registry import MODEL
    assert 'MGE_CNN' in MODEL and MODEL.get('MGE_CNN') is plugin.MGE_CNN


def test_state_dict_keys_and_children_are_the_references(plugin, monkeypatch):
    want = T.state_dict_keys()
    net = short(plugin, monkeypatch)
    assert isinstance(net, plugin.LocalCamNet)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want['state_dict']
    assert [n for n, _ in net.named_children()] == want['children']
    assert sum(q.numel() for q in net.parameters()) == want['n_params']
    assert isinstance(net.classifier, plugin.Classifier) and isinstance(net.conv6, torch.nn.Conv2d) and net.conv6.padding == (1, 1)
    assert isinstance(net.pool_max, torch.nn.AdaptiveMaxPool2d) and (net.num_classes, net.box_thred, net.image_size) == (4, 0.6, 96)


def test_get_params_partitions_the_parameters_as_the_reference_does(plugin, monkeypatch):
    want = T.state_dict_keys()
    net = short(plugin, monkeypatch)
    names = {id(q): n for n, q in net.named_parameters()}
    extractor = [names[id(q)] for q in net.get_params('extractor')]
    classifier = [names[id(q)] for q in net.get_params(prefix='classifier')]
    assert extractor == want['extractor'] == [names[id(q)] for q in net.get_params('extract')] and classifier == want['classifier']
    assert not set(extractor) & set(classifier) and len(extractor) + len(classifier) == len(names)
    assert net.get_params('other') is None


def test_the_model_builds_from_the_references_yaml(plugin, monkeypatch):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.backbone import ResNet, Bottleneck
    from hawkeye_amd.model.registry import MODEL
    ref = CfgNode.load_cfg(open(os.path.join(HERE, 'golden', 'reference_configs', 'MGE_CNN.yaml')))
    monkeypatch.setattr(plugin, 'resnet50', lambda pretrained=False, **kw: ResNet(Bottleneck, [1, 1, 1, 1]))
    net = MODEL.get(ref.model.name)(ref.model)
    assert (net.num_classes, net.box_thred, net.image_size) == (200, 0.2, 224)
    assert net.conv6.weight.shape == (2000, 1024, 1, 1) and net.cls_cat_a.fc.weight.shape == (200, 3 * 4048)
    assert net.cls_gate[1].fc.weight.shape == (3, 512)
    ours = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'MGE_CNN_synthetic.yaml')))
    assert ours.dataset.name == 'synthetic' and ours.model == ref.model and ours.train.optimizer == ref.train.optimizer
    assert ours.train.scheduler == ref.train.scheduler and ours.dataset.batch_size == ref.dataset.batch_size == 4
    with pytest.raises(ValueError, match='224'):
        net(torch.zeros(1, 3, 64, 64))


def test_argument_checks_come_before_any_launch():
    import hawkeye_amd.functional as HF
    err = HF._lib.HawkeyeHipError
    x = torch.zeros(2, 32, 3, 3)
    for args, text in (((torch.zeros(2, 32, 3), torch.zeros(5, 32), torch.zeros(5)), r'\[B, Cin, H, W\]'),
                       ((torch.zeros(2, 48, 3, 3), torch.zeros(5, 48), torch.zeros(5)), 'multiple of 32'),
                       ((x, torch.zeros(5, 64), torch.zeros(5)), r'\[Cout, 32\]'), ((x, torch.zeros(5, 32, 1, 1), torch.zeros(4)), '5 values')):
        with pytest.raises(err, match=text):
            HF.mge_partpool(*args)
    c5, w = torch.zeros(2, 8, 3, 3), torch.zeros(4, 8)
    for args, text in (((c5[0], w, torch.zeros(2, dtype=torch.int64), 0.2, 96), r'\[B, C, h, w\]'), ((c5, torch.zeros(4, 9), torch.zeros(2, dtype=torch.int64), 0.2, 96), 'classes, 8'),
                       ((c5, w, torch.zeros(2), 0.2, 96), 'integers'), ((c5, w, torch.zeros(3, dtype=torch.int64), 0.2, 96), 'shape'),
                       ((c5, w, torch.zeros(2, dtype=torch.int64), 0.2, 4096), '2048')):
        with pytest.raises(err, match=text):
            HF.mge_cam_bbox(*args)
    y = torch.zeros(2, dtype=torch.int64)
    for args, text in ((([], y), '1 .. 16'), (([torch.zeros(2, 3)] * 17, y), '1 .. 16'), (([torch.zeros(2, 3), torch.zeros(2, 4)], y), 'one shape'),
                       (([torch.zeros(2, 3)], y.float()), 'integers'), (([torch.zeros(2, 3)], torch.zeros(3, dtype=torch.int64)), 'shape')):
        with pytest.raises(err, match=text):
            HF.mge_loss(*args)
    with pytest.raises(err, match='CPU tensor'):
        HF.mge_partpool(x, torch.zeros(5, 32), torch.zeros(5))
    got = HF.mge_cam_weights(torch.tensor([[1.0, -2.0], [-3.0, 4.0]]), torch.tensor([1, 0]), 4)
    assert got.tolist() == [[0.0, 1.0], [0.25, 0.0]]


def test_header_table_and_library_agree():
    from hawkeye_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hawkeye_mge.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(hk_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(_lib.MGE_SIGNATURES) and len(declared) == 6
    others = set(_lib.SIGNATURES) | set(_lib.TRUNK_SIGNATURES) | set(_lib.TRUNK_EPI_SIGNATURES) | set(_lib.TRUNK_TILE_SIGNATURES) | set(_lib.INTERP_SIGNATURES)
    assert not set(_lib.MGE_SIGNATURES) & others
    main = open(os.path.join(ROOT, 'include', 'hawkeye_hip.h')).read()
    assert '#include "hawkeye_mge.h"' in main and 'hk_mge_' not in main.replace('hawkeye_mge.h', '')
    for name, (_, args) in _lib.MGE_SIGNATURES.items():
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', src).group(1)
        assert len(params.split(',')) == len(args), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in _lib.MGE_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.hk_mge_partpool_fwd_ws_bytes(4, 1024, 2000, 14, 14) == 4 * 2000 * 4 * 8             # 196 pixels: four column tiles
    assert lib.hk_mge_partpool_fwd_ws_bytes(4, 48, 2000, 14, 14) == 0 and lib.hk_mge_loss_ws_bytes(10, 4) == 160
    assert lib.hk_mge_loss_ws_bytes(17, 4) == 0


def test_criterion_contract():
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import MGELoss
    assert MGELoss(CfgNode({})).label_smoothing == 0.1 and MGELoss(CfgNode(dict(label_smoothing=0.0))).label_smoothing == 0.0
    with pytest.raises(ValueError, match='logits'):
        MGELoss(CfgNode({}))({'logits': []}, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='logits'):
        MGELoss(CfgNode({}))(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_trainer_parameter_groups(plugin, monkeypatch):
    from hawkeye_amd.config import CfgNode
    ex = importlib.import_module(PLUGIN_MODULES[1])
    net = short(plugin, monkeypatch)

    class Fake:
        get_model_module = lambda self: net
    for extra, rate in (({}, 0.1), ({'lr_rate': 0.5}, 0.5)):
        opt = ex.MGE_CNNTrainer.get_optimizer(Fake(), CfgNode(dict(lr=0.0004, weight_decay=0.00002, **extra)))
        assert isinstance(opt, torch.optim.Adam) and [g['lr'] for g in opt.param_groups] == pytest.approx([0.0004, 0.0004 * rate])
        assert all(g['weight_decay'] == 0.00002 for g in opt.param_groups)
    names = {id(q): n for n, q in net.named_parameters()}
    first = {names[id(q)].split('.')[0] for q in opt.param_groups[0]['params']}
    second = {names[id(q)].split('.')[0] for q in opt.param_groups[1]['params']}
    assert second == {s + b for s in ('conv4', 'conv5') for b in ('', '_box', '_box_2', '_gate')} and not first & second
    assert sum(len(g['params']) for g in opt.param_groups) == len(names)
