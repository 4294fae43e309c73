"""GPU tier: the peer-learning loss of the gfx950 build against the reference's golden results (both forms, bit-identical
to each other), autograd scaling, the NaN case, non-contiguous inputs, and hipGraph capture in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import peer_inputs as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = P.load_cases()
DEV = 'cuda'
LDS_LIMIT = 160 * 1024


def fits_resident(n, c):
    return (2 * n * c + 10 * n + 32) * 4 <= LDS_LIMIT          # csrc/peer.hip: peer_resident_lds


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(case, form, tune, l1=None, l2=None, a=1.0, b=1.0):
    import hawkeye_amd.functional as F
    tune('peer_form', form)
    l1 = (dev(case['l1']) if l1 is None else l1).requires_grad_(True)
    l2 = (dev(case['l2']) if l2 is None else l2).requires_grad_(True)
    loss_1, loss_2, stats = F.peer_learning_loss_with_stats(l1, l2, dev(case['y']), case['drop_rate'])
    (loss_1 * a + loss_2 * b).backward()
    return (torch.stack([loss_1.detach(), loss_2.detach()]).cpu().numpy(), l1.grad.cpu().numpy(), l2.grad.cpu().numpy(),
            stats.cpu().numpy())


@pytest.mark.parametrize('case', CASES, ids=P.case_id)
def test_golden_cases_both_forms(case, tune):
    general = run(case, 1, tune)
    P.judge(case, *general, label='gfx950 general')
    if not fits_resident(case['N'], case['C']):
        assert case['N'] == 130
        return
    resident = run(case, 2, tune)
    P.judge(case, *resident, label='gfx950 resident')
    for name, a, b in zip(('loss', 'dl1', 'dl2', 'stats'), general, resident):
        assert a.tobytes() == b.tobytes(), f'{name}: the two forms differ'
    automatic = run(case, 0, tune)
    for a, b in zip(general, automatic):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('form', [1, 2])
def test_autograd_scales_the_two_gradients_independently(form, tune):
    case = CASES[1]
    assert (case['N'], case['C']) == (64, 200)
    base = run(case, form, tune)
    scaled = run(case, form, tune, a=2.0, b=3.0)
    assert np.array_equal(scaled[0], base[0])
    assert np.array_equal(scaled[1], base[1] * np.float32(2.0))       # a power of two: exact
    assert np.array_equal(scaled[2], base[2] * np.float32(3.0))       # one rounding in either: the same product


@pytest.mark.parametrize('form', [1, 2])
def test_nan_case(form, tune):
    case = CASES[8]
    assert (case['n'], case['m']) == (4, 0)
    loss, dl1, dl2, stats = run(case, form, tune)
    assert np.isnan(loss).all() and not dl1.any() and not dl2.any()
    assert stats.tolist() == [4, 0, 0, 0]


@pytest.mark.parametrize('form', [1, 2])
def test_non_contiguous_views_equal_the_dense_case(form, tune):
    case = CASES[1]
    n, c = case['N'], case['C']
    wide_1 = torch.full((n, c + 9), 7.0, device=DEV)
    wide_2 = torch.full((n, c + 9), -3.0, device=DEV)
    wide_1[:, 5:5 + c] = dev(case['l1'])
    wide_2[:, 5:5 + c] = dev(case['l2'])
    v1, v2 = wide_1[:, 5:5 + c], wide_2[:, 5:5 + c]
    assert not v1.is_contiguous()
    dense = run(case, form, tune)
    views = run(case, form, tune, l1=v1.detach(), l2=v2.detach())
    for a, b in zip(dense, views):
        assert a.tobytes() == b.tobytes()


def test_label_out_of_range_gives_nan_and_no_fault(tune):
    import hawkeye_amd.functional as F
    case = CASES[2]
    y = dev(case['y']).clone()
    y[1] = case['C'] + 1000000
    y[3] = -5
    for form in (1, 2):
        tune('peer_form', form)
        loss_1, loss_2 = F.peer_learning_loss(dev(case['l1']), dev(case['l2']), y, 0.0)
        torch.cuda.synchronize()
        assert torch.isnan(loss_1).item() and torch.isnan(loss_2).item()


def test_graph_capture_in_a_child_process():
    """Forward + backward captured with torch.cuda.graph, three replays bit-identical to eager (tools/peer_graph_check.py).
    A host synchronisation inside the call would abort the capture.  One attempt; the child has its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'peer_graph_check.py')], cwd=ROOT, capture_output=True,
                       text=True, timeout=170)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert 'peer_graph_check ok' in r.stdout
