"""CPU tier: csrc/peer.hip compiled for the host (tests/emu) against the reference's golden results - every case in
the general form, every case that fits in the resident form, the two forms bit-identical - the C ABI's error returns,
and a two-step PLTrainer run on the emulated heads.  Test infrastructure only."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from emu.harness import emulated

import peer_inputs as P

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = P.load_cases()
PLUGIN_MODULES = ('hawkeye_amd.model.methods.PeerLearningNet', 'hawkeye_amd.examples.PeerLearning')
LDS_LIMIT = 160 * 1024


def fits_resident(n, c):
    return (2 * n * c + 10 * n + 32) * 4 <= LDS_LIMIT          # csrc/peer.hip: peer_resident_lds


@pytest.fixture(autouse=True, scope='module')
def _emulated_heads():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated():
        yield


def run(case, form, tune):
    import hawkeye_amd.functional as F
    tune('peer_form', form)
    l1 = torch.from_numpy(case['l1']).requires_grad_(True)
    l2 = torch.from_numpy(case['l2']).requires_grad_(True)
    loss_1, loss_2, stats = F.peer_learning_loss_with_stats(l1, l2, torch.from_numpy(case['y']), case['drop_rate'])
    (loss_1 + loss_2).backward()
    return (np.array([loss_1.item(), loss_2.item()], dtype=np.float32), l1.grad.numpy().copy(), l2.grad.numpy().copy(),
            stats.numpy().copy())


@pytest.mark.parametrize('case', CASES, ids=P.case_id)
def test_golden_cases_both_forms(case, tune):
    general = run(case, 1, tune)
    P.judge(case, *general, label='emulated general')
    if not fits_resident(case['N'], case['C']):
        assert case['N'] == 130
        return
    resident = run(case, 2, tune)
    P.judge(case, *resident, label='emulated resident')
    for name, a, b in zip(('loss', 'dl1', 'dl2', 'stats'), general, resident):
        assert a.tobytes() == b.tobytes(), f'{name}: the two forms differ'
    automatic = run(case, 0, tune)
    for a, b in zip(general, automatic):
        assert a.tobytes() == b.tobytes()


def test_stats_function_returns_a_tensor(tune):
    import hawkeye_amd.functional as F
    case = CASES[0]
    stats = F.peer_learning_stats(torch.from_numpy(case['l1']), torch.from_numpy(case['l2']), torch.from_numpy(case['y']),
                                  case['drop_rate'])
    assert isinstance(stats, torch.Tensor) and stats.dtype == torch.int32 and not stats.requires_grad
    assert stats.tolist() == [case['n'], case['m'], int(case['keep1'].sum()), int(case['keep2'].sum())]


def test_label_out_of_range_reads_nothing_and_gives_nan(tune):
    import hawkeye_amd.functional as F
    case = CASES[2]
    y = torch.from_numpy(case['y']).clone()
    y[1] = case['C'] + 1000000
    y[3] = -5
    for form in (1, 2):
        tune('peer_form', form)
        loss_1, loss_2 = F.peer_learning_loss(torch.from_numpy(case['l1']), torch.from_numpy(case['l2']), y, 0.0)
        assert torch.isnan(loss_1) and torch.isnan(loss_2)           # drop_rate 0 keeps every row, the two bad ones too


def abi_call(lib, case, drop_rate, ws_bytes=None, form=None):
    l1, l2 = torch.from_numpy(case['l1']), torch.from_numpy(case['l2'])
    y = torch.from_numpy(case['y']).to(torch.int32)
    n, c = l1.shape
    loss, stats = torch.zeros(2), torch.zeros(4, dtype=torch.int32)
    dl1, dl2 = torch.zeros_like(l1), torch.zeros_like(l2)
    need = lib.hk_peer_loss_ws_bytes(n, c)
    ws = torch.zeros(need, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    return lib.hk_peer_loss(p(l1), p(l2), p(y), drop_rate, p(loss), p(dl1), p(dl2), p(stats), n, c, p(ws),
                            need if ws_bytes is None else ws_bytes, None), dl1, dl2


def test_abi_errors(tune):
    from hawkeye_amd import _lib
    lib = _lib.load()
    case = CASES[0]
    for bad in (-0.01, 1.01, float('nan'), float('inf')):
        assert abi_call(lib, case, bad)[0] == _lib.HK_ERR_BAD_ARG
    assert abi_call(lib, case, 0.0)[0] == _lib.HK_OK and abi_call(lib, case, 1.0)[0] == _lib.HK_OK
    need = lib.hk_peer_loss_ws_bytes(case['N'], case['C'])
    rc, dl1, dl2 = abi_call(lib, case, 0.35, ws_bytes=need - 1)
    assert rc == _lib.HK_ERR_WORKSPACE and not dl1.any() and not dl2.any()         # nothing launched
    big = CASES[4]
    assert (big['N'], big['C']) == (130, 200)
    tune('peer_form', 2)
    rc, dl1, dl2 = abi_call(lib, big, 0.1)
    assert rc == _lib.HK_ERR_UNSUPPORTED and not dl1.any() and not dl2.any()
    tune('peer_form', 0)
    assert abi_call(lib, big, 0.1)[0] == _lib.HK_OK                                 # automatic: the general form
    # null pointer / sizes
    z = ctypes.c_void_p(0)
    ok = ctypes.c_void_p(torch.zeros(16).data_ptr())
    assert lib.hk_peer_loss(z, ok, ok, 0.35, ok, ok, ok, ok, 1, 1, ok, 1 << 20, None) == _lib.HK_ERR_BAD_ARG
    assert lib.hk_peer_loss(ok, ok, ok, 0.35, ok, ok, ok, ok, 0, 1, ok, 1 << 20, None) == _lib.HK_ERR_BAD_ARG
    # above what the selection kernel's LDS holds (include/hawkeye_hip.h: N <= 2048); refused before anything is read
    assert lib.hk_peer_loss(ok, ok, ok, 0.35, ok, ok, ok, ok, 2049, 1, ok, 1 << 20, None) == _lib.HK_ERR_UNSUPPORTED


def test_two_step_trainer_run_on_emulated_heads(tmp_path, monkeypatch):
    """PLTrainer from configs/PeerLearning_BCNN_synthetic.yaml, shrunk: two steps, finite loss1 / loss2, both classifiers
    move, and the second net's trunk gets a gradient of its own."""
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.registry import MODEL
    from hawkeye_amd.train import Trainer
    assert 'PeerLearningNet' not in MODEL
    pl = importlib.import_module(PLUGIN_MODULES[1])               # the trainer does the opt-in import of the plugin
    try:
        assert 'PeerLearningNet' in MODEL
        monkeypatch.setattr(Trainer, 'select_device', lambda self, cfg: torch.device('cpu'))
        cfg = CfgNode.load_cfg(open(os.path.join(os.path.dirname(HERE), 'configs', 'PeerLearning_BCNN_synthetic.yaml')))
        cfg.dataset.samples, cfg.dataset.batch_size, cfg.dataset.transformer.image_size = 8, 4, 64
        cfg.model.base_model.num_classes = 3
        cfg.model.T_k = 0                                # no ramp: drop_rate 0.35 in the only epoch, the selection is exercised
        cfg.experiment.log_dir = str(tmp_path)
        cfg.dataset.num_workers = 0
        cfg.train.optimizer.lr = 1e-3
        cfg.freeze()
        tr = pl.PLTrainer(cfg)
        assert list(tr.rate_scheduler) == [0.35]
        net = tr.model
        before = [m.classifier.weight.detach().clone() for m in (net.base_model, net.base_model2)]
        grads = []
        step = tr.optimizer.step

        def recording_step(*a, **k):                      # the gradients as the optimiser sees them
            grads.append((net.base_model.backbone[0].weight.grad.clone(), net.base_model2.backbone[0].weight.grad.clone()))
            return step(*a, **k)
        monkeypatch.setattr(tr.optimizer, 'step', recording_step)
        tr.train()
        assert len(grads) == 2                            # 8 samples / batches of 4
        for name in ('loss1', 'loss2'):
            values = tr.performance_meters['train'][name].values
            assert len(values) == 1 and np.isfinite(values[0])
        for name in ('acc', 'acc1', 'acc2'):
            assert len(tr.performance_meters['val'][name].values) == 1
        after = [m.classifier.weight.detach() for m in (net.base_model, net.base_model2)]
        assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
        for g1, g2 in grads:
            assert g1.abs().max() > 0 and g2.abs().max() > 0 and not torch.equal(g1, g2)
    finally:
        MODEL.pop('PeerLearningNet', None)
        for name in PLUGIN_MODULES:
            sys.modules.pop(name, None)
