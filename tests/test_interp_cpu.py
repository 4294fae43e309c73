"""CPU tier, no kernels: the InterpParts plugin's contracts - opt-in registration, the reference's state_dict keys, attribute
names, initialisation and `__repr__`; the Gaussian window and the Beta prior against the reference's own; the argument checks
of the functional layer; the agreement of include/hawkeye_interp.h, hawkeye_amd/_lib.py: INTERP_SIGNATURES and the built
library; the criterion's defaults; the trainer's parameter groups; the yaml."""
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import interp_inputs as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLUGIN_MODULES = ('hawkeye_amd.model.methods.InterpParts', 'hawkeye_amd.examples.InterpParts')
GOLDEN = T.load()


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    import hawkeye_amd.model  # noqa: F401
    assert 'IP_ResNet50' not in MODEL and 'IP_ResNet101' not in MODEL          # importing hawkeye_amd.model alone registers neither
    yield importlib.import_module(PLUGIN_MODULES[0])
    for name in ('IP_ResNet50', 'IP_ResNet101'):
        MODEL.pop(name, None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def test_registration_is_opt_in(plugin):
    from hawkeye_amd.model.registry import MODEL
    assert 'IP_ResNet50' in MODEL and 'IP_ResNet101' in MODEL


def test_state_dict_keys_children_and_repr_are_the_references(plugin):
    want = json.load(open(os.path.join(HERE, 'golden', 'interp_state_dict.json')))
    c = T.MODEL_CASE
    net = plugin.ResNet(plugin.Bottleneck, list(c['layers']), c['classes'], c['parts'])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want['state_dict']
    assert [n for n, _ in net.named_children()] == want['children']
    assert sum(q.numel() for q in net.parameters()) == want['n_params']
    assert repr(net.grouping) == want['repr_grouping'] == 'GroupingUnit (1024 -> 5)'
    assert (net.n_parts, net.num_classes, net.inplanes) == (c['parts'], c['classes'], 1024)


def test_initialisation_is_the_references(plugin):
    torch.manual_seed(3)
    net = plugin.ResNet(plugin.Bottleneck, [1, 1, 1], 7, 5)
    blocks = [m for m in net.modules() if isinstance(m, (plugin.Bottleneck, plugin.Bottleneck1x1))]
    assert len(blocks) == 3 + 4 + 2 and all(not m.bn3.weight.any() for m in blocks)
    assert all((m.bn1.weight == 1).all() and not m.bn1.bias.any() for m in blocks)
    assert float(net.grouping.weight.min()) == pytest.approx(1e-5) and not net.grouping.smooth_factor.any()
    assert net.grouping.weight.shape == (5, 1024, 1, 1) and net.grouping.weight.dtype == torch.float32
    w = net.post_block[0].conv1.weight                                          # kaiming, fan-out: std = sqrt(2 / (out k k))
    assert float(w.std()) == pytest.approx(np.sqrt(2.0 / 512), rel=0.05)
    centres, factors = torch.rand(5, 1024), torch.randn(5)
    net.grouping.reset_parameters(centres, factors)
    assert torch.equal(net.grouping.weight[:, :, 0, 0], centres) and torch.equal(net.grouping.smooth_factor, factors)


def test_missing_pretrained_file_warns_once_and_keeps_the_initialisation(plugin, monkeypatch, tmp_path):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.backbone import pretrained
    monkeypatch.setenv('HAWKEYE_PRETRAINED_DIR', str(tmp_path))
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path))
    monkeypatch.setattr(pretrained, '_warned', set())
    monkeypatch.setattr(plugin, 'ResNet', lambda block, layers, classes, parts: torch.nn.Linear(parts, classes))
    with pytest.warns(UserWarning, match='resnet50'):
        net = plugin.IP_ResNet50(CfgNode(dict(num_classes=3, num_parts=2)))
    assert isinstance(net, torch.nn.Linear)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        plugin.IP_ResNet50(CfgNode(dict(num_classes=3, num_parts=2)))          # the second time: no warning
        plugin.IP_ResNet101(CfgNode(dict(num_classes=3, num_parts=2, pretrained=False)))      # no lookup at all


def test_gaussian_window_is_bit_equal_to_the_references():
    import hawkeye_amd.functional as HF
    for radius, std in T.WINDOWS:
        w = HF.ip_gaussian_window(radius, std)
        assert w.dtype == torch.float32 and w.numpy().tobytes() == GOLDEN[f'window_r{radius}'].tobytes(), radius
    assert HF.ip_gaussian_window(0, 0.4).tolist() == [[1.0]]


def _closed_form(alpha, beta):
    return alpha == 1.0 or beta == 1.0


def _check_prior(n, alpha, beta):
    import hawkeye_amd.functional as HF
    p = HF.ip_beta_prior(n, alpha, beta)
    assert p.dtype == torch.float32 and p.numpy().tobytes() == GOLDEN[f'prior_n{n}_b{beta}'].tobytes(), (n, alpha, beta)
    assert HF.ip_beta_prior(n, alpha, beta) is p                                  # made once


def test_beta_prior_is_bit_equal_to_the_references(monkeypatch):
    import hawkeye_amd.functional as HF
    closed = [q for q in T.PRIORS if _closed_form(*q[1:])]
    assert closed
    for n, alpha, beta in closed:
        _check_prior(n, alpha, beta)
    assert (HF.ip_beta_prior(16, 1, 0.001) == 1).all()                            # the yaml's prior: every grid point rounds to 1.0f
    assert np.allclose(HF.ip_beta_prior(8, 1.0, 2.0).numpy(), T.prior64(8, 1.0, 2.0), rtol=1e-7)
    monkeypatch.setitem(sys.modules, 'scipy', None)                               # no closed form and no scipy: a clear error
    with pytest.raises(HF._lib.HawkeyeHipError, match='scipy'):
        HF.ip_beta_prior(5, 2.5, 3.5)


def test_beta_prior_without_a_closed_form_goes_through_scipy():
    pytest.importorskip('scipy')
    for n, alpha, beta in T.PRIORS:
        if not _closed_form(alpha, beta):
            _check_prior(n, alpha, beta)


def test_argument_checks_come_before_any_launch():
    import hawkeye_amd.functional as HF
    err = HF._lib.HawkeyeHipError
    x, s = torch.zeros(2, 64, 3, 3), torch.zeros(5)
    for bad_x, w, sm, text in ((torch.zeros(2, 64, 3), torch.zeros(5, 64, 1, 1), s, r'\[N, C, H, W\]'),
                               (x, torch.zeros(5, 32, 1, 1), s, r'\[K, 64'), (x, torch.zeros(5, 64, 1, 1), torch.zeros(4), '5 values'),
                               (x, torch.zeros(33, 64, 1, 1), torch.zeros(33), 'parts'),
                               (torch.zeros(2, 96, 3, 3), torch.zeros(5, 96, 1, 1), s, 'multiple of 64'),
                               (torch.zeros(2, 2048, 3, 3), torch.zeros(5, 2048, 1, 1), s, 'up to 1024')):
        with pytest.raises(err, match=text):
            HF.ip_group(bad_x, w, sm)
    logits, assign, y = torch.zeros(2, 3), torch.zeros(2, 5, 6, 6), torch.zeros(2, dtype=torch.int64)
    for args, text in (((torch.zeros(3, 3), assign, y), 'one N'), ((logits, assign[:, :, :4], y), 'smaller than the 5 x 5 window'),
                       ((logits, assign, y.float()), 'integers'), ((logits, assign, torch.zeros(3, dtype=torch.int64)), 'shape')):
        with pytest.raises(err, match=text):
            HF.ip_loss(*args)


def test_header_table_and_library_agree():
    from hawkeye_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hawkeye_interp.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(hk_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(_lib.INTERP_SIGNATURES) and len(declared) == 6
    assert not set(_lib.INTERP_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.TRUNK_SIGNATURES) | set(_lib.TRUNK_EPI_SIGNATURES))
    assert '#include "hawkeye_interp.h"' in open(os.path.join(ROOT, 'include', 'hawkeye_hip.h')).read()
    for name, (_, args) in _lib.INTERP_SIGNATURES.items():
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', src).group(1)
        assert len(params.split(',')) == len(args), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in _lib.INTERP_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.hk_ip_group_fwd_ws_bytes(16, 1024, 5, 28, 28) >= 16 * 25 * 5 * 1024 * 4          # a share of q per 32-pixel tile
    assert lib.hk_ip_group_fwd_ws_bytes(1, 96, 5, 4, 4) == 0 and lib.hk_ip_group_bwd_ws_bytes(1, 64, 33, 4, 4) == 0
    assert lib.hk_ip_group_bwd_ws_bytes(1, 64, 32, 1, 1) > 0 and lib.hk_ip_loss_ws_bytes(16, 5) > 0


def test_criterion_defaults_and_contract():
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import InterpPartsLoss
    crit = InterpPartsLoss(CfgNode({}))
    assert (crit.radius, crit.std, crit.num_parts, crit.alpha, crit.beta, crit.coeff) == (2, 0.4, 5, 1, 0.001, 0.5)
    crit = InterpPartsLoss(CfgNode(dict(radius=1, std=1.0, num_parts=3, alpha=2, beta=2.0, coeff=0.25)))
    assert (crit.radius, crit.std, crit.num_parts, crit.alpha, crit.beta, crit.coeff) == (1, 1.0, 3, 2, 2.0, 0.25)
    with pytest.raises(ValueError, match='logits, att, assign'):
        crit((torch.zeros(2, 3), torch.zeros(2, 3, 4, 4)), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='5 parts'):
        crit((torch.zeros(2, 3), None, torch.zeros(2, 5, 4, 4)), torch.zeros(2, dtype=torch.int64))


def test_trainer_parameter_groups_and_yaml(plugin):
    from hawkeye_amd.config import CfgNode
    ex = importlib.import_module(PLUGIN_MODULES[1])
    net = plugin.ResNet(plugin.Bottleneck, [1, 1, 1], 7, 5)

    class Fake:
        get_model_module = lambda self: net
    opt = ex.InterpPartsTrainer.get_optimizer(Fake(), CfgNode(dict(lr=0.001, weight_decay=0.0005)))
    assert isinstance(opt, torch.optim.SGD) and [g['lr'] for g in opt.param_groups] == pytest.approx([0.001, 0.02])
    assert all(g['momentum'] == 0.9 and g['weight_decay'] == 0.0005 for g in opt.param_groups)
    names = {id(q): n for n, q in net.named_parameters()}
    first = {names[id(q)].split('.')[0] for q in opt.param_groups[0]['params']}
    assert first == {'conv1', 'bn1', 'layer1', 'layer2', 'layer3'}
    assert sum(len(g['params']) for g in opt.param_groups) == len(names)
    cfg = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'InterpParts_synthetic.yaml')))
    ref = CfgNode.load_cfg(open(os.path.join(HERE, 'golden', 'reference_configs', 'InterpPartsNet.yaml')))
    assert cfg.dataset.name == 'synthetic' and cfg.model == ref.model and cfg.train.criterion == ref.train.criterion
    assert cfg.train.optimizer == ref.train.optimizer and cfg.dataset.batch_size == ref.dataset.batch_size == 16
    tf = ex.TrainTransform(40, 32, 1.0)
    from PIL import Image
    out = tf(Image.fromarray(np.random.RandomState(0).randint(0, 256, (50, 70, 3)).astype(np.uint8)))
    assert out['u8'].shape == (32, 32, 3) and out['u8'].dtype == torch.uint8 and out['erase'].dtype == torch.int32 and out['erase'][2] > 0
