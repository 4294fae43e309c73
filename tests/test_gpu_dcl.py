"""GPU tier: csrc/dcl.hip of the gfx950 build - the op cases of the emulated tier (the head, the reference's loss goldens
and the loss's exact properties, the swap law against the reference's indices), the whole model at 448 x 448 against the
reference in eval(), one training step, and hipGraph capture of the head in a child process."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import dcl_inputs as T
import dcl_ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device('cuda')
PLUGIN_MODULES = ('hawkeye_amd.model.methods.DCL', 'hawkeye_amd.examples.DCL')
MODEL_BOUND = 1e-4                                          # the README's whole-model bound, norm-wise


@pytest.mark.parametrize('case', T.HEAD_CASES, ids=T.head_case_id)
def test_head_forward_and_backward_against_float64(case):
    print(f'worst ratio {O.check_head_case(case, DEV):.3f}')


@pytest.mark.parametrize('missing', O.GRADS)
def test_head_null_gradient_raw_and_through_autograd(missing):
    O.check_head_null_gradient(missing, DEV)


def test_head_zero_d_mask_gives_exact_zeros():
    O.check_head_zero_d_mask(DEV)


def test_head_unaligned_and_strided_views_give_the_bits_of_dense_ones():
    O.check_head_views(DEV)
    O.check_head_views(DEV, (2, 2048, 14, 14))


def test_head_refuses_a_map_of_one_row():
    O.check_head_refused(DEV)


@pytest.mark.parametrize('case', O.LOSS_CASES, ids=T.loss_case_id)
def test_golden_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, DEV):.3f}')


def test_loss_gradients_scale_exactly_under_a_power_of_two_weight():
    O.check_loss_scaling(O.LOSS_CASES[1], DEV)


def test_loss_zero_coefficients_give_exact_zeros():
    O.check_loss_zero_coefficients(O.LOSS_CASES[0], DEV)


def test_label_out_of_range_gives_nan_and_no_fault():
    O.check_loss_bad_labels(O.LOSS_CASES[1], DEV)
    torch.cuda.synchronize()


def test_two_runs_agree_bit_for_bit():
    O.check_loss_reruns(O.LOSS_CASES[0], DEV)
    O.check_head_reruns(DEV)


@pytest.mark.parametrize('name', list(T.LAW_CASES))
def test_swap_law_against_the_reference(name):
    O.check_law_case(name, DEV)


def test_swap_law_of_a_batch_is_per_image():
    O.check_law_batch(DEV)


def test_swap_law_refuses_an_image_smaller_than_the_grid():
    O.check_law_refused(DEV)


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    assert 'DCL' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    MODEL.pop('DCL', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def seeded_model(plugin, case):
    from inputs import seeded_init
    from hawkeye_amd.config import CfgNode
    net = plugin.DCL(CfgNode(dict(num_classes=T.CLASSES, cls_2=case['cls_2'], cls_2xmul=case['cls_2xmul'], pretrained=False)))
    seeded_init(net, case['init_seed'])
    return net.to(DEV)


def test_whole_model_matches_the_reference_in_eval(plugin):
    """ResNet-50, the head and both classifiers at 448 x 448, B = 2, seeded weights (tests/golden/inputs.py:seeded_init
    on both sides), eval(): the class logits, the swap logits and the mask within 1e-4 (norm-wise) of the reference's
    float64 run, and the class of outputs[0]."""
    case = T.load_model_case()
    net = seeded_model(plugin, case).eval()
    with torch.no_grad():
        out = net(torch.from_numpy(case['images']).to(DEV))
    assert isinstance(out, list) and [tuple(t.shape) for t in out] == [(case['B'], T.CLASSES), (case['B'], 2), (case['B'], 49)]
    for name, t in zip(T.MODEL_OUTPUTS, out):
        d, d32 = T.distance(t.cpu().numpy(), case[f'{name}_f64']), T.distance(case[f'{name}_f32'], case[f'{name}_f64'])
        print(f'dcl whole model {name}: distance {d:.3e}, reference fp32 {d32:.3e}, bound {MODEL_BOUND:.0e}')
        assert d <= MODEL_BOUND, (name, d)
    assert out[0].argmax(1).cpu().numpy().tolist() == case['logits_f64'].argmax(1).tolist()


def test_one_training_step_gives_finite_gradients_everywhere(plugin):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.data import dcl_law_ramp
    from hawkeye_amd.model.loss import DCLLoss
    case = T.load_model_case()
    net = seeded_model(plugin, case).train()
    out = net(torch.from_numpy(case['images']).to(DEV))
    law = dcl_law_ramp(49).to(DEV).expand(case['B'], 49)
    loss = DCLLoss(CfgNode(dict(alpha=1, beta=1, gamma=1)))(out, torch.tensor([3, 150], device=DEV), torch.tensor([1, 0], device=DEV), law)
    loss.backward()
    assert torch.isfinite(loss).item()
    for name, q in net.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), name
    for name in ('Convmask.bias', 'Convmask.weight', 'classifier.weight', 'classifier_swap.weight', 'backbone.0.weight'):
        assert dict(net.named_parameters())[name].grad.abs().max() > 0, name


def test_graph_capture_of_the_head_in_a_child_process():
    """Swap law -> head -> classifiers -> loss, forward + backward, captured with torch.cuda.graph; three replays
    bit-identical to eager (tools/dcl_graph_check.py).  A host synchronisation anywhere would abort the capture.  One
    attempt; the child has its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'dcl_graph_check.py')], cwd=ROOT, capture_output=True,
                       text=True, timeout=170)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert 'dcl_graph_check ok' in r.stdout
