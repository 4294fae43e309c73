"""GPU tier: csrc/crossx.hip of the gfx950 build - the op cases of the emulated tier (the multi-excitation block, the
upsample + add, the reference's loss goldens and the loss's exact properties), the whole model at 448 x 448 against the
reference in eval(), one training step, and hipGraph capture of the head in a child process."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import crossx_inputs as T
import crossx_ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device('cuda')
PLUGIN_MODULES = ('hawkeye_amd.model.methods.CrossX', 'hawkeye_amd.examples.CrossX')


@pytest.mark.parametrize('case', T.ME_CASES, ids=T.me_case_id)
def test_me_forward_and_backward_against_float64(case):
    print(f'worst ratio {O.check_me_case(case, DEV):.3f}')


def test_me_all_negative_row_and_duplicated_maximum():
    O.check_me_special_rows(DEV)


@pytest.mark.parametrize('missing', ['d_main', 'd_parts', 'dz'])
def test_me_null_gradient(missing):
    O.check_me_null_gradient(missing, DEV)


def test_me_autograd_node_passes_unused_outputs_as_null():
    O.check_me_autograd(DEV)


def test_me_unaligned_and_strided_views_give_the_bits_of_dense_ones():
    O.check_me_views(DEV)


@pytest.mark.parametrize('case', T.UP_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_up_add_against_interpolate_and_add(case):
    O.check_up_add_case(case, DEV)


def test_up_add_refuses_a_size_that_is_no_multiple():
    O.check_up_add_refused(DEV)


@pytest.mark.parametrize('case', O.LOSS_CASES, ids=T.loss_case_id)
def test_golden_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, DEV):.3f}')


def test_loss_gradients_scale_exactly_under_a_power_of_two_weight():
    O.check_loss_scaling(O.LOSS_CASES[1], DEV)


def test_loss_gamma_zero_gives_exact_zeros():
    O.check_loss_zero_gamma(O.LOSS_CASES[1], DEV)


def test_label_out_of_range_gives_nan_and_no_fault():
    O.check_loss_bad_labels(O.LOSS_CASES[1], DEV)
    torch.cuda.synchronize()


def test_one_sample_is_refused():
    O.check_loss_refuses_one_sample(DEV)


def test_zero_feature_row_gives_nan():
    O.check_loss_zero_feature_row(DEV)


def test_two_runs_agree_bit_for_bit():
    O.check_loss_reruns(O.LOSS_CASES[2], DEV)
    x = O.me_case(T.ME_CASES[1])[0]
    a, b = O.run_me(x, 'max', DEV), O.run_me(x, 'max', DEV)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    assert 'CrossX' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    MODEL.pop('CrossX', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def seeded_model(plugin, case):
    from inputs import seeded_init
    from hawkeye_amd.config import CfgNode
    net = plugin.CrossX(CfgNode(dict(num_parts=case['P'], num_classes=T.CLASSES, pretrained=False)))
    seeded_init(net, case['init_seed'])
    return net.to(DEV)


def test_whole_model_matches_the_reference_in_eval(plugin):
    """ResNet-50 with both ME blocks, the combined branch and the three classifiers at 448 x 448, P = 2, B = 2, seeded
    weights (tests/golden/inputs.py:seeded_init on both sides), eval(): the three logit tensors and the 3 x P pooled
    features by the project's rule against the reference's float64 run, and the class of the summed logits."""
    case = T.load_model_case()
    net = seeded_model(plugin, case).eval()
    with torch.no_grad():
        out = net(torch.from_numpy(case['images']).to(DEV))
    xf, xp, xc, ulti, plty, cmbn = out
    assert all(len(l) == case['P'] for l in (ulti, plty, cmbn)) and tuple(ulti[0].shape) == (case['B'], 2048, 1, 1)
    assert tuple(plty[1].shape) == tuple(cmbn[1].shape) == (case['B'], 1024, 1, 1)
    got = dict(ulti_logits=xf, plty_logits=xp, cmbn_logits=xc, ulti_ftrs=torch.stack([t.flatten(1) for t in ulti]),
               plty_ftrs=torch.stack([t.flatten(1) for t in plty]), cmbn_ftrs=torch.stack([t.flatten(1) for t in cmbn]))
    for name in T.MODEL_OUTPUTS:
        T.judge_value('whole model', name, got[name].cpu().numpy(), case[f'{name}_f32'], case[f'{name}_f64'])
    want = (case['ulti_logits_f64'] + case['plty_logits_f64'] + case['cmbn_logits_f64']).argmax(1)
    assert (xf + xp + xc).argmax(1).cpu().numpy().tolist() == want.tolist()


def test_one_training_step_gives_finite_gradients_everywhere(plugin):
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import CrossXLoss
    case = T.load_model_case()
    net = seeded_model(plugin, case).train()
    out = net(torch.from_numpy(case['images']).to(DEV))
    loss = CrossXLoss(CfgNode(dict(num_parts=case['P'], gamma=list(T.GAMMA))))(out, torch.tensor([3, 150], device=DEV))
    loss.backward()
    assert torch.isfinite(loss).item()
    params = dict(net.named_parameters())
    for name in ('layer3.5.me.parts.0.0.weight', 'layer4.2.me.parts.1.2.bias', 'conv2_1.weight', 'conv3_2.weight', 'bn3_1.weight',
                 'fc_ulti.weight', 'fc_plty.weight', 'fc_cmbn.weight', 'conv1.weight'):
        g = params[name].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, name


def test_graph_capture_of_the_head_in_a_child_process():
    """Both ME blocks -> upsample + add -> loss, forward + backward, captured with torch.cuda.graph; three replays
    bit-identical to eager (tools/crossx_graph_check.py).  A host synchronisation anywhere would abort the capture.  One
    attempt; the child has its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'crossx_graph_check.py')], cwd=ROOT, capture_output=True,
                       text=True, timeout=170)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert 'crossx_graph_check ok' in r.stdout
