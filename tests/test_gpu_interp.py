"""GPU tier: csrc/interp.hip of the gfx950 build - the op cases of the emulated tier (the grouping unit against the reference's
op sequence in float64, the reference's loss goldens and the loss's exact properties), the whole short model against the
reference in eval and train mode, one training step, and hipGraph capture of the head and criterion in a child process."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import interp_inputs as T
import interp_ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device('cuda')
PLUGIN_MODULES = ('hawkeye_amd.model.methods.InterpParts', 'hawkeye_amd.examples.InterpParts')


@pytest.mark.parametrize('case', T.GROUP_CASES, ids=T.group_case_id)
def test_group_forward_and_backward_against_float64(case):
    print(f'worst ratio {O.check_group_case(case, DEV):.3f}')


@pytest.mark.parametrize('missing', O.GRADS)
def test_group_null_gradient_raw_and_through_autograd(missing):
    O.check_group_null_gradient(missing, DEV)


def test_group_need_flags():
    O.check_group_need_flags(DEV)
    O.check_group_need_flags(DEV, (2, 1024, 5, 28, 28))


def test_group_unaligned_and_strided_views_give_the_bits_of_dense_ones():
    O.check_group_views(DEV)
    O.check_group_views(DEV, (2, 1024, 5, 28, 28))


def test_group_clamp_case():
    print(f'worst ratio {O.check_group_clamp(DEV):.3f}')


def test_group_active_clamp_of_the_assignment_sum():
    print(f'worst ratio {O.check_group_s_clamp(DEV):.3f}')


def test_group_refuses_33_parts_and_96_channels():
    O.check_group_refused(DEV)


def test_group_workspace_query_is_what_the_call_needs():
    O.check_group_workspace(DEV)


@pytest.mark.parametrize('case', O.LOSS_CASES, ids=T.loss_case_id)
def test_golden_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, DEV):.3f}')


def test_loss_coeff_zero_and_powers_of_two_are_exact():
    O.check_loss_coeff(O.LOSS_CASES[4], DEV)


def test_loss_all_equal_maps_follow_the_tie_rules():
    O.check_loss_all_equal(DEV)


def test_loss_refuses_a_map_smaller_than_the_window():
    O.check_loss_refused(DEV)


def test_label_out_of_range_gives_nan_and_no_fault():
    O.check_loss_bad_labels(O.LOSS_CASES[0], DEV)
    torch.cuda.synchronize()


def test_two_runs_agree_bit_for_bit():
    O.check_loss_reruns(O.LOSS_CASES[3], DEV)
    O.check_group_reruns(DEV, (2, 1024, 5, 28, 28))


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    assert 'IP_ResNet101' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    for name in ('IP_ResNet50', 'IP_ResNet101'):
        MODEL.pop(name, None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


@pytest.mark.parametrize('mode', T.MODEL_MODES)
def test_whole_short_model_matches_the_reference(plugin, mode):
    print(f'worst ratio {O.check_model(plugin, mode, DEV):.3f}')


def test_one_training_step_gives_finite_gradients_everywhere(plugin):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import InterpPartsLoss
    case = T.load_model_case()
    net = O.short_model(plugin, case, DEV).train()
    out = net(torch.from_numpy(case['images']).to(DEV))
    loss = InterpPartsLoss(CfgNode(dict(radius=1, num_parts=case['parts'], beta=2.0)))(out, torch.tensor([3, 5], device=DEV))
    loss.backward()
    assert torch.isfinite(loss).item()
    for name, q in net.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), name
    # (not attconv.2.bias: it shifts every part's attention logit alike, and the softmax over the parts takes that away)
    for name in ('grouping.weight', 'grouping.smooth_factor', 'mylinear.weight', 'conv1.weight', 'attconv.2.weight'):
        assert dict(net.named_parameters())[name].grad.abs().max() > 0, name


def test_graph_capture_of_the_head_and_criterion_in_a_child_process():
    """Grouping unit -> classifier -> loss, forward + backward, captured with torch.cuda.graph; three replays bit-identical
    to eager (tools/interp_graph_check.py).  A host synchronisation anywhere would abort the capture.  One attempt; the
    child has its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'interp_graph_check.py')], cwd=ROOT, capture_output=True,
                       text=True, timeout=170)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert 'interp_graph_check ok' in r.stdout
