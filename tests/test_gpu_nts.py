"""GPU tier: csrc/nts.hip of the gfx950 build - the reference's NMS, crop and loss cases and the op cases of the emulated
tier, non-contiguous inputs, exact scaling under a power-of-two loss weight, the whole model at 224 x 224 against the
reference in eval(), one training step, and hipGraph capture of the head in a child process."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nts_inputs as T
import nts_ops as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = torch.device('cuda')
PLUGIN_MODULES = ('hawkeye_amd.model.methods.NTSNet', 'hawkeye_amd.examples.NTSNet')


@pytest.mark.parametrize('case', O.NMS_CASES, ids=T.nms_case_id)
def test_golden_nms_cases(case):
    O.check_nms_case(case, DEV)


def test_nms_equal_scores_go_to_the_highest_index():
    O.check_nms_ties(DEV)


@pytest.mark.parametrize('a,b', [(70, 2), (5, 1), (256, 1), (257, 2), (2048, 1)])
def test_nms_on_tables_of_other_sizes_against_float64(a, b):
    O.check_nms_table(DEV, a, b, seed=40 + a)


def test_nms_fills_with_the_last_pick_when_fewer_than_topn_survive():
    O.check_nms_fill(DEV)


def test_nms_above_the_anchor_limit_is_refused():
    import hawkeye_amd.functional as F
    from hawkeye_amd._lib import HawkeyeHipError
    with pytest.raises(HawkeyeHipError, match='-3'):
        F.nts_nms(torch.zeros(1, 2049, device=DEV), torch.zeros(2049, 4, dtype=torch.int32, device=DEV), 3)


@pytest.mark.parametrize('case', O.CROP_CASES, ids=lambda c: f"out{c['out'][0]}x{c['out'][1]}")
def test_golden_crop_cases(case):
    O.check_crop_case(case, DEV)


@pytest.mark.parametrize('out', [(8, 12), (5, 7), (1, 4), (3, 1)])
def test_crop_boxes_across_every_edge_against_float64(out):
    O.check_crop_shapes(DEV, out)


def test_crop_into_an_unaligned_output():
    O.check_crop_unaligned_output(DEV)
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', O.LOSS_CASES, ids=T.loss_case_id)
def test_golden_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, DEV):.3f}')


def test_gradients_scale_exactly_under_a_power_of_two_loss_weight():
    O.check_loss_scaling(O.LOSS_CASES[2], DEV)
    O.check_loss_gradient_routes(O.LOSS_CASES[1], DEV)


def test_label_out_of_range_gives_nan_and_no_fault():
    O.check_loss_bad_labels(DEV)
    torch.cuda.synchronize()


def test_non_contiguous_inputs_equal_the_dense_case():
    O.check_noncontiguous(DEV)
    O.check_crop_shapes(DEV, (8, 12), strided=True)


def test_two_runs_agree_bit_for_bit():
    first, again = O.run_loss(O.LOSS_CASES[2], DEV), O.run_loss(O.LOSS_CASES[2], DEV)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    a, b = O.check_crop_shapes(DEV, (5, 7)), O.check_crop_shapes(DEV, (5, 7))
    assert torch.equal(a, b)
    case = O.NMS_CASES[3]
    a, b = O.run_nms(case['scores'], case['anchors'], DEV), O.run_nms(case['scores'], case['anchors'], DEV)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    assert 'NTSNet' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    MODEL.pop('NTSNet', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def test_whole_model_matches_the_reference_in_eval(plugin):
    """ResNet-50 + navigator + crops + second trunk pass at 224 x 224, B = 2, seeded weights (tests/golden/inputs.py:
    seeded_init on both sides), eval(): the chosen proposals exactly, the three logit tensors and top_n_prob by the
    project's rule against the reference's float64 run."""
    from inputs import seeded_init
    from hawkeye_amd.config import CfgNode
    case = T.load_model_case(O.GOLDEN)
    net = plugin.NTSNet(CfgNode(dict(image_size=case['size'], proposal_num=case['proposal_num'], cat_num=case['cat_num'])))
    seeded_init(net, case['init_seed'])
    net = net.to(DEV).eval()
    with torch.no_grad():
        out = net(torch.from_numpy(case['images']).to(DEV))
    raw, cat, part, index, prob = out
    assert index.dtype == torch.int64 and index.cpu().numpy().tolist() == case['top_n_index'].tolist()
    assert part.shape == (case['B'], case['proposal_num'], 200)
    for name, got in (('raw_logits', raw), ('concat_logits', cat), ('part_logits', part), ('top_n_prob', prob)):
        T.judge_value('whole model', name, got.cpu().numpy(), case[f'{name}_f32'], case[f'{name}_f64'])
        ref = case[f'{name}_f32']
        if name != 'top_n_prob':
            assert got.argmax(-1).cpu().numpy().tolist() == ref.argmax(-1).tolist()


def test_one_training_step_gives_finite_gradients_everywhere(plugin):
    from inputs import seeded_init
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import NTSLoss
    case = T.load_model_case(O.GOLDEN)
    net = plugin.NTSNet(CfgNode(dict(image_size=224, proposal_num=6, cat_num=4)))
    seeded_init(net, case['init_seed'])
    net = net.to(DEV).train()
    torch.manual_seed(5)
    out = net(torch.from_numpy(case['images']).to(DEV))
    loss = NTSLoss(CfgNode(dict(proposal_num=6)))(out, torch.tensor([3, 150], device=DEV))
    loss.backward()
    assert torch.isfinite(loss).item()
    for name in ('proposal_net.down1.weight', 'proposal_net.down1.bias', 'concat_net.weight', 'partcls_net.weight',
                 'pretrained_model.conv1.weight', 'pretrained_model.layer4.2.conv3.weight', 'pretrained_model.fc.weight'):
        g = dict(net.named_parameters())[name].grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, name


def test_graph_capture_of_the_head_in_a_child_process():
    """nms -> gather -> crops and the loss, forward + backward, captured with torch.cuda.graph; three replays
    bit-identical to eager (tools/nts_graph_check.py).  A host synchronisation anywhere would abort the capture.  One
    attempt; the child has its own time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'nts_graph_check.py')], cwd=ROOT, capture_output=True,
                       text=True, timeout=170)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert 'nts_graph_check ok' in r.stdout
