"""CrossX, host side: opt-in registration, the constructor's contract and the state_dict for one, two and three parts
against the reference's key lists, the functional wrappers' refusals, the loss module's contract, the synthetic yaml,
the trainer's optimizer and scheduler, and the golden tool's --check.  No GPU."""
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

import crossx_inputs as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = json.load(open(os.path.join(HERE, 'golden', 'crossx_state_dict.json')))
PLUGIN_MODULES = ('hawkeye_amd.model.methods.CrossX', 'hawkeye_amd.examples.CrossX')


def forget_plugin():
    MODEL.pop('CrossX', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


@pytest.fixture
def plugin():
    """The opt-in import, undone afterwards: the registry other tests see holds the default plugins only."""
    assert 'CrossX' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    forget_plugin()


def test_absent_from_the_default_registry_and_registered_by_the_import():
    default = ['APCNN', 'BCNN', 'CBCNN', 'CIN', 'MPN', 'OSMENet', 'ResNet101', 'ResNet50']       # what tests/test_models_cpu.py pins
    assert sorted(MODEL) == default and sorted(install_into(Repository())) == default
    mod = importlib.import_module(PLUGIN_MODULES[0])
    try:
        assert sorted(MODEL) == sorted(default + ['CrossX']) and MODEL.get('CrossX') is mod.CrossX
        ref = Repository()
        install_into(ref)
        assert ref['CrossX'] is mod.CrossX
    finally:
        forget_plugin()
    assert sorted(MODEL) == default


@pytest.mark.parametrize('parts', [1, 2, 3])
def test_state_dict_children_and_attributes_are_the_reference_ones(plugin, parts):
    torch.manual_seed(0)
    net = plugin.CrossX(CfgNode(dict(name='CrossX', num_parts=parts, num_classes=200, pretrained=False)))
    want = KEYS[str(parts)]
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want['state_dict']
    assert [n for n, _ in net.named_children()] == want['children']
    assert sum(p.numel() for p in net.parameters()) == want['n_params']
    assert (net.nparts, net.nclass, net.meflag) == (parts, 200, parts > 1)
    assert isinstance(net.adpavgpool, torch.nn.AdaptiveAvgPool2d) and tuple(net.fc_ulti.weight.shape) == (200, 2048 * parts)
    names = [k for k, _ in want['state_dict']]
    if parts == 1:
        assert not hasattr(net, 'fc_plty') and not any('.me.' in k for k in names)
        return
    assert isinstance(net.adpmaxpool, torch.nn.AdaptiveMaxPool2d)
    assert tuple(net.fc_plty.weight.shape) == tuple(net.fc_cmbn.weight.shape) == (200, 1024 * parts)
    for i in range(1, parts + 1):
        assert tuple(getattr(net, f'conv2_{i}').weight.shape) == (1024, 2048, 1, 1) and tuple(getattr(net, f'conv3_{i}').weight.shape) == (1024, 1024, 3, 3)
        assert isinstance(getattr(net, f'bn3_{i}'), torch.nn.BatchNorm2d)
    assert not hasattr(net, f'conv2_{parts + 1}')
    for layer, block, width, hidden in ((net.layer3, 5, 1024, 4), (net.layer4, 2, 2048, 8)):
        me = layer[block].me
        assert len(layer) == block + 1 and me.nparts == parts and len(me.parts) == parts and isinstance(me.avg_pool, torch.nn.AdaptiveAvgPool2d)
        assert tuple(me.parts[parts - 1][0].weight.shape) == (hidden, width) and tuple(me.parts[0][2].weight.shape) == (width, hidden)
        assert isinstance(me.parts[0][1], torch.nn.ReLU) and isinstance(me.parts[0][3], torch.nn.Sigmoid)
        assert not any(hasattr(b, 'me') for b in list(layer)[:-1])
    assert f'layer3.5.me.parts.{parts - 1}.2.bias' in names and 'layer4.2.me.parts.0.0.weight' in names
    # the reference's initialisation: normal(0, sqrt(2 / (k k out))) convolutions, BatchNorm at 1 / 0
    w = net.conv3_1.weight.detach()
    assert abs(float(w.std()) - (2.0 / (9 * 1024)) ** 0.5) < 2e-4 and abs(float(w.mean())) < 1e-4
    assert float(net.bn3_2.weight.min()) == 1 and not net.bn3_2.bias.any()
    if parts == 2:
        twin = copy.deepcopy(net)
        for (ka, va), (kb, vb) in zip(net.state_dict().items(), twin.state_dict().items()):
            assert ka == kb and torch.equal(va, vb) and va.data_ptr() != vb.data_ptr()


def test_constructor_contracts(plugin, monkeypatch, tmp_path):
    for bad in (0, 4):
        with pytest.raises(ValueError, match='num_parts'):
            plugin.CrossX(CfgNode(dict(num_parts=bad, pretrained=False)))
    built = []
    real = plugin.CrossXNet
    monkeypatch.setattr(plugin, 'CrossXNet', lambda **kw: built.append(kw) or torch.nn.Linear(2, 2))
    looked = []
    monkeypatch.setattr(plugin._pre, 'load', lambda arch: looked.append(arch))                          # -> None: nothing to load
    plugin.CrossX(CfgNode(dict(num_parts=2)))
    assert built[-1] == dict(nparts=2, meflag=True, num_classes=200) and looked == ['resnet50']           # the defaults: 200 classes, pretrained
    plugin.CrossX(CfgNode(dict(num_parts=1, num_classes=7, pretrained=False)))
    assert built[-1] == dict(nparts=1, meflag=False, num_classes=7) and looked == ['resnet50']
    # pretrained weights load non-strictly: trunk entries are taken, the classifier of another shape and unknown keys are not
    monkeypatch.setattr(plugin, 'CrossXNet', real)
    small = torch.nn.Module()
    small.conv1, small.fc_ulti = torch.nn.Conv2d(3, 4, 3), torch.nn.Linear(4, 2)
    monkeypatch.setattr(plugin, 'CrossXNet', lambda **kw: small)
    sd = {'conv1.weight': torch.full((4, 3, 3, 3), 0.5), 'fc.weight': torch.zeros(1000, 2048), 'fc_ulti.weight': torch.zeros(9, 9)}
    monkeypatch.setattr(plugin._pre, 'load', lambda arch: sd)
    before = small.fc_ulti.weight.clone()
    assert plugin.CrossX(CfgNode(dict(num_parts=2))) is small
    assert (small.conv1.weight == 0.5).all() and torch.equal(small.fc_ulti.weight, before)


def test_functional_wrappers_refuse_bad_arguments():
    import hawkeye_amd.functional as F
    from hawkeye_amd._lib import HawkeyeHipError
    from hawkeye_amd.model.loss import CrossXLoss
    out, res, gates = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4), torch.rand(2, 2, 3)
    a, b = torch.randn(1, 2, 4, 4), torch.randn(1, 2, 2, 2)
    logits = [torch.randn(2, 7) for _ in range(3)]
    feats = [[torch.rand(2, c, 1, 1) for _ in range(2)] for c in (8, 4, 4)]
    y = torch.zeros(2, dtype=torch.long)
    crit = CrossXLoss(CfgNode(dict(name='CrossXLoss', num_parts=2, gamma=[0.5, 0.25, 0.5])))
    assert crit.num_parts == 2 and crit.gamma == [0.5, 0.25, 0.5]
    for call in (lambda: F.crossx_me(out, res, gates, 'max'), lambda: F.crossx_up_add(a, b), lambda: F.crossx_loss(*logits, *feats, y, T.GAMMA),
                 lambda: F.crossx_loss_with_terms(*logits, *[torch.stack([f.flatten(1) for f in l]) for l in feats], y, T.GAMMA),
                 lambda: crit((*logits, *feats), y)):
        with pytest.raises(HawkeyeHipError, match='CPU tensor'):                      # device: no CPU fallback
            call()
    bad = [
        (lambda: F.crossx_me(out, res, gates, 'sum'), "'max' or 'avg'"),
        (lambda: F.crossx_me(out[0], res, gates, 'max'), r'\[N, C, H, W\]'),
        (lambda: F.crossx_me(out, res[:, :2], gates, 'max'), 'res must have the shape'),
        (lambda: F.crossx_me(out, res, gates[:, :1], 'max'), 'gates must be'),
        (lambda: F.crossx_me(out, res, torch.rand(4, 2, 3), 'max'), 'gates must be'),
        (lambda: F.crossx_me(out.double(), res, gates, 'avg'), 'fp32'),
        (lambda: F.crossx_up_add(a, torch.randn(1, 2, 3, 2)), 'multiple'),
        (lambda: F.crossx_up_add(a, b[:, :1]), 'one N and C'),
        (lambda: F.crossx_loss(logits[0], logits[1][:, :5], logits[2], *feats, y, T.GAMMA), 'one shape'),
        (lambda: F.crossx_loss(*[l[:1] for l in logits], *[[f[:1] for f in l] for l in feats], y[:1], T.GAMMA), 'at least 2'),
        (lambda: F.crossx_loss(*logits, feats[0], feats[1][:1], feats[2], y, T.GAMMA), 'parts'),
        (lambda: F.crossx_loss(*logits, [f[:1] for f in feats[0]], feats[1], feats[2], y, T.GAMMA), 'ulti_ftrs'),
        (lambda: F.crossx_loss(*logits, *feats, y[:1], T.GAMMA), 'labels of shape'),
        (lambda: F.crossx_loss(*logits, *feats, y.float(), T.GAMMA), 'integers'),
        (lambda: F.crossx_loss(*logits, *feats, y, (0.5, 0.5)), 'gamma'),
    ]
    for call, message in bad:
        with pytest.raises(HawkeyeHipError, match=message):
            call()
    with pytest.raises(ValueError, match='num_parts'):
        crit((*logits, feats[0][:1], feats[1], feats[2]), y)
    with pytest.raises(ValueError, match='gamma'):
        CrossXLoss(CfgNode(dict(num_parts=2, gamma=[0.5])))
    one = CrossXLoss(CfgNode(dict(num_parts=1, gamma=[0.5, 0.25, 0.5])))             # one part: a plain cross entropy
    assert torch.equal(one(logits[0], y), torch.nn.functional.cross_entropy(logits[0], y, label_smoothing=0.1))


def test_host_side_queries_need_no_gpu():
    from hawkeye_amd import _lib
    lib = _lib.load()
    assert lib.hk_crossx_loss_ws_bytes(8, 200, 2, 2048, 1024, 1024) >= (8 * 200 + 2 * 4096) * 4
    assert lib.hk_crossx_loss_ws_bytes(1, 200, 2, 2048, 1024, 1024) == 0 and lib.hk_crossx_loss_ws_bytes(8, 200, 4, 8, 8, 8) == 0
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('hk_crossx_')) == [
        'hk_crossx_loss', 'hk_crossx_loss_ws_bytes', 'hk_crossx_me_bwd', 'hk_crossx_me_fwd', 'hk_crossx_up_add_bwd', 'hk_crossx_up_add_fwd']
    assert len(_lib.SIGNATURES) == 104


def test_synthetic_yaml_parses_and_names_the_plugin():
    cfg = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'CrossX_synthetic.yaml')))
    ref = CfgNode.load_cfg(open(os.path.join(HERE, 'golden', 'reference_configs', 'CrossX.yaml')))
    assert dict(cfg.model) == dict(ref.model) and cfg.train.optimizer == ref.train.optimizer and cfg.train.scheduler == ref.train.scheduler
    assert cfg.train.criterion == ref.train.criterion and cfg.dataset.batch_size == ref.dataset.batch_size == 8
    assert cfg.dataset.transformer == ref.dataset.transformer
    assert cfg.dataset.name == 'synthetic' and cfg.model.name == 'CrossX' and tuple(cfg.train.criterion.gamma) == T.GAMMA


def test_trainer_builds_sgd_multistep_and_the_reference_transforms(plugin):
    from PIL import Image
    ex = importlib.import_module(PLUGIN_MODULES[1])
    tr = ex.CrossXTrainer.__new__(ex.CrossXTrainer)
    tr.model = torch.nn.Linear(3, 2)
    tr.optimizer = tr.get_optimizer(CfgNode(dict(name='SGD', lr=0.0025, weight_decay=0.00002, momentum=0.9)))
    tr.scheduler = tr.get_scheduler(CfgNode(dict(name='MultiStepLR', milestones=[15, 25], gamma=0.1)))
    assert isinstance(tr.optimizer, torch.optim.SGD) and tr.optimizer.defaults['momentum'] == 0.9 and tr.optimizer.defaults['weight_decay'] == 0.00002
    assert isinstance(tr.scheduler, torch.optim.lr_scheduler.MultiStepLR)
    assert isinstance(tr.get_criterion(CfgNode(dict(name='CrossXLoss', num_parts=2, gamma=[0.5, 0.25, 0.5]))), ex.CrossXLoss)
    lrs = []
    for _ in range(27):
        lrs.append(tr.optimizer.param_groups[0]['lr'])
        tr.optimizer.step()
        tr.scheduler.step()
    assert lrs[14] == pytest.approx(2.5e-3) and lrs[15] == pytest.approx(2.5e-4) and lrs[25] == pytest.approx(2.5e-5)
    tf = tr.get_transformers(CfgNode(dict(image_size=448, resize_size=600)))
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, (50, 80, 3), dtype=np.uint8))
    for split in ('train', 'val'):
        t = tf[split](img)
        assert t.shape == (3, 448, 448) and t.dtype == torch.float32
    assert torch.equal(tf['val'](img), tf['val'](img))
    tr.config = CfgNode(dict(model=dict(num_parts=2)))
    a, b, c = torch.randn(2, 5), torch.randn(2, 5), torch.randn(2, 5)
    assert torch.equal(tr.summed_logits((a, b, c, None, None, None)), a + b + c)


def test_golden_inputs_are_a_pure_function_of_the_recipe_and_the_files_are_small():
    a, b = T.loss_inputs(3, 3, 200, 3, (70, 33, 33)), T.loss_inputs(3, 3, 200, 3, (70, 33, 33))
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[4].shape == (3, 3, 70) and a[4].dtype == np.float32 and a[3].dtype == np.int64
    largest = max(os.path.getsize(os.path.join(HERE, 'golden', f)) for f in os.listdir(os.path.join(HERE, 'golden'))
                  if f.endswith('.npz') and not f.startswith('crossx_'))
    for f in T.FILES:
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= largest
    for case in T.load_loss_cases():
        assert case['loss_f64'].dtype == np.float64 and case['loss_f32'].dtype == np.float32 and case['loss_f64'].shape == (6,)
        assert case['df_plty_f64'].shape == (case['P'], case['B'], case['widths'][1])
        for l, name in enumerate(('f_ulti', 'f_plty', 'f_cmbn')):             # the reference's float64 run is a true float64 one
            assert abs(case['loss_f64'][3 + l] - T.regulariser_closed_form(case[name], T.GAMMA[l])) <= 1e-12
        assert abs(case['loss_f64'][0] - case['loss_f64'][1:].sum()) < 1e-12
    for case in T.ME_CASES:                                                    # the accepted seed meets both conditions
        x = T.me_inputs(case)
        assert T.me_seed_ok(x['out'], x['res'], x['gates']) and x['gates'].min() > 0 and x['gates'].max() < 1
    model = T.load_model_case()
    assert model['ulti_ftrs_f64'].shape == (2, 2, 2048) and model['plty_ftrs_f32'].shape == (2, 2, 1024) and model['cmbn_logits_f64'].shape == (2, 200)


def reference_dir():
    d = os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference'))
    return d if os.path.isfile(os.path.join(d, 'model', 'methods', 'CrossX.py')) else None


@pytest.mark.skipif(reference_dir() is None, reason='the reference checkout is not present')
def test_golden_tool_check_reproduces_the_committed_bytes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_crossx_golden.py'), '--check', '--reference', reference_dir()],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.count('identical') == len(T.FILES) + 1 and 'DIFFERENT' not in r.stdout
