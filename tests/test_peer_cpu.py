"""Peer learning, host side: the golden file against a restatement of the loss's formula, the PeerLearningNet plugin's
surface (opt-in registration, state_dict, children, the two nets' weights), the trainer's drop-rate schedule and the
functional's refusals.  No GPU."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import hawkeye_amd.model  # noqa: F401
from hawkeye_amd.config import CfgNode
from hawkeye_amd.model.registry import MODEL, install_into
from hawkeye_amd.utils.repository import Repository

import peer_inputs as P

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = json.load(open(os.path.join(HERE, 'golden', 'state_dict_keys.json')))
CASES = P.load_cases()
PLUGIN_MODULES = ('hawkeye_amd.model.methods.PeerLearningNet', 'hawkeye_amd.examples.PeerLearning')


@pytest.fixture
def peer_plugin():
    """The opt-in import, undone afterwards: the registry other tests see holds the default plugins only."""
    assert 'PeerLearningNet' not in MODEL
    mod = importlib.import_module(PLUGIN_MODULES[0])
    yield mod
    MODEL.pop('PeerLearningNet', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def restated(l1, l2, y, drop_rate):
    """The formula of the loss (rows, selection, crossed keep sets, means) in torch, differentiable in the logits."""
    lse = [torch.logsumexp(l, 1) for l in (l1, l2)]
    ce = [s - l.gather(1, y[:, None])[:, 0] for s, l in zip(lse, (l1, l2))]
    pred = [l.argmax(1) for l in (l1, l2)]
    agree = pred[0] == pred[1]
    n = int(agree.sum())
    m = int((1 - drop_rate) * n)
    idx = torch.arange(l1.shape[0])
    rank = []
    for c in ce:
        c = c.detach()
        before = (c[None, :] < c[:, None]) | ((c[None, :] == c[:, None]) & (idx[None, :] < idx[:, None]))
        rank.append((before & agree[None, :]).sum(1))
    keep = [~agree | (rank[1] < m), ~agree | (rank[0] < m)]            # crossed
    loss = [(c * k).sum() / k.sum() for c, k in zip(ce, keep)]
    return loss, keep, n, m


@pytest.mark.parametrize('case', CASES, ids=P.case_id)
def test_golden_file_equals_the_restated_formula(case):
    """The stored float64 results of the reference equal the formula run in float64 (to float64 rounding), the stored
    float32 results lie within float32 rounding of them, and n, m and the masks are the formula's."""
    l1 = torch.from_numpy(case['l1']).double().requires_grad_(True)
    l2 = torch.from_numpy(case['l2']).double().requires_grad_(True)
    loss, keep, n, m = restated(l1, l2, torch.from_numpy(case['y']), case['drop_rate'])
    assert (n, m) == (case['n'], case['m'])
    assert np.array_equal(keep[0].numpy(), case['keep1']) and np.array_equal(keep[1].numpy(), case['keep2'])
    if case['mode'] == 'mixed':
        assert 0.25 * case['N'] <= n <= 0.85 * case['N']
    if m == 0 and n == case['N']:
        assert np.isnan(case['loss_f64']).all() and np.isnan(case['loss_f32']).all()
        assert torch.isnan(loss[0]) and torch.isnan(loss[1])
        for name in ('dl1_f32', 'dl2_f32', 'dl1_f64', 'dl2_f64'):
            assert not case[name].any()
        return
    (loss[0] + loss[1]).backward()
    got = dict(loss=np.array([loss[0].item(), loss[1].item()]), dl1=l1.grad.numpy(), dl2=l2.grad.numpy())
    for name, value in got.items():
        ref64, ref32 = case[f'{name}_f64'], case[f'{name}_f32']
        assert ref64.dtype == np.float64 and ref32.dtype == np.float32
        den = np.linalg.norm(ref64)
        assert np.linalg.norm(value - ref64) / den < 1e-13, name                      # float64: a few ulps of summation order
        assert np.linalg.norm(ref32.astype(np.float64) - ref64) / den < 1e-6, name    # float32 rounding of the reference itself


def test_peer_inputs_are_a_pure_function_of_the_recipe():
    a, b = P.peer_inputs(3, 7, 13), P.peer_inputs(3, 7, 13)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].dtype == np.float32 and a[2].dtype == np.int64 and a[0].shape == (7, 13)
    assert not np.array_equal(a[0], P.peer_inputs(4, 7, 13)[0])


def test_registration_is_opt_in(peer_plugin):
    assert 'PeerLearningNet' in MODEL and MODEL.get('PeerLearningNet') is peer_plugin.PeerLearningNet
    ref = Repository()
    install_into(ref)
    assert ref['PeerLearningNet'] is peer_plugin.PeerLearningNet


def test_absent_from_the_default_registry():
    assert 'PeerLearningNet' not in MODEL
    assert 'PeerLearningNet' not in install_into(Repository())


@pytest.fixture
def peer_net(peer_plugin):
    torch.manual_seed(0)
    cfg = CfgNode(dict(name='PeerLearningNet', base_model=dict(name='BCNN', stage=2, num_classes=200), drop_rate=0.35, T_k=10))
    return MODEL.get('PeerLearningNet')(cfg)


def test_state_dict_children_and_the_two_nets_weights(peer_net):
    want = [[prefix + k, shape] for prefix in ('base_model.', 'base_model2.') for k, shape in KEYS['BCNN']['state_dict']]
    assert [[k, list(v.shape)] for k, v in peer_net.state_dict().items()] == want
    assert [n for n, _ in peer_net.named_children()] == ['base_model', 'base_model2']
    a, b = peer_net.base_model, peer_net.base_model2
    assert not torch.equal(a.classifier.weight, b.classifier.weight)                 # re-initialised
    assert b.classifier.weight.abs().max() > 0
    for (ka, pa), (kb, pb) in zip(a.backbone.state_dict().items(), b.backbone.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb) and pa.data_ptr() != pb.data_ptr()   # equal values, own storage


@pytest.mark.parametrize('epochs,t_k,drop_rate', [(200, 10, 0.35), (5, 10, 0.35)])
def test_drop_rate_schedule(peer_plugin, epochs, t_k, drop_rate):
    pl = importlib.import_module(PLUGIN_MODULES[1])
    want = np.ones(epochs) * drop_rate
    ramp = np.linspace(0, drop_rate, t_k)
    want[:t_k] = ramp[:epochs]                         # fewer epochs than T_k: the ramp's first `epochs` values
    got = pl.drop_rate_schedule(epochs, t_k, drop_rate)
    assert got.shape == (epochs,) and np.array_equal(got, want)

    class Shell(pl.PLTrainer):                         # the constructor's own use of it, without a device
        def __init__(self):
            self.config = CfgNode(dict(model=dict(T_k=t_k, drop_rate=drop_rate), train=dict(epoch=epochs)))
            model = self.config.model
            self.rate_scheduler = pl.drop_rate_schedule(self.config.train.epoch, model.T_k, model.drop_rate)
    assert np.array_equal(Shell().rate_scheduler, want)


def test_stage_one_optimises_both_classifiers(peer_net, peer_plugin):
    pl = importlib.import_module(PLUGIN_MODULES[1])

    class Shell:
        pass
    sh = Shell()
    sh.config = CfgNode(dict(model=dict(name='PeerLearningNet', base_model=dict(name='BCNN', stage=1, num_classes=200))))
    sh.get_model_module = lambda model=None: peer_net
    opt = pl.PLTrainer.get_optimizer(sh, CfgNode(dict(lr=1e-5, weight_decay=1e-5)))
    assert isinstance(opt, torch.optim.Adam)
    ids = {id(p) for g in opt.param_groups for p in g['params']}
    assert ids == {id(p) for m in (peer_net.base_model, peer_net.base_model2) for p in m.classifier.parameters()}


def test_ws_bytes_needs_no_gpu():
    from hawkeye_amd import _lib
    lib = _lib.load()
    assert lib.hk_peer_loss_ws_bytes(64, 200) > 0 and lib.hk_peer_loss_ws_bytes(1, 1) > 0
    assert lib.hk_peer_loss_ws_bytes(130, 200) >= lib.hk_peer_loss_ws_bytes(64, 200)
    assert lib.hk_peer_loss_ws_bytes(0, 200) == 0


def test_cpu_tensors_and_mismatches_are_refused():
    import hawkeye_amd.functional as F
    from hawkeye_amd._lib import HawkeyeHipError
    from hawkeye_amd.model.loss import PeerLearningLoss
    l1, l2, y = torch.randn(4, 5), torch.randn(4, 5), torch.randint(0, 5, (4,))
    for fn in (F.peer_learning_loss, PeerLearningLoss, F.peer_learning_stats):
        with pytest.raises(HawkeyeHipError):
            fn(l1, l2, y, 0.35)
    with pytest.raises(HawkeyeHipError):
        F.peer_learning_loss(l1, torch.randn(4, 6), y, 0.35)                  # shapes
    with pytest.raises(HawkeyeHipError):
        F.peer_learning_loss(l1, l2, torch.randint(0, 5, (3,)), 0.35)         # label count
    with pytest.raises(HawkeyeHipError):
        F.peer_learning_loss(l1.double(), l2.double(), y, 0.35)               # dtype
    with pytest.raises(HawkeyeHipError):
        F.peer_learning_loss(l1, l2, y.float(), 0.35)                         # float labels
