"""CPU tier: csrc/mge.hip compiled for the host (tests/emu) - the part pool forward and backward against float64 and against
autograd of the reference's op sequence, its directed cases, NULL outputs, views, refusals and the workspace size; the Grad-CAM
box against the reference's arithmetic in float64 with its directed cases, the crop behind it and the closed form against the
reference's own GradCam output; the criterion against its float64 restatement and the reference trainer's golden; the whole
short model against the reference in eval mode and in one train-mode step, and a two-step MGE_CNNTrainer run.  Test
infrastructure only."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from emu.harness import emulated

import mge_inputs as T
import mge_ops as O

HERE = os.path.dirname(os.path.abspath(__file__))
PLUGIN_MODULES = ('hawkeye_amd.model.methods.MGE_CNN', 'hawkeye_amd.examples.MGE_CNN')
CPU = torch.device('cpu')


@pytest.fixture(autouse=True, scope='module')
def _emulated_kernels():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated():
        yield


@pytest.mark.parametrize('case', T.POOL_CASES, ids=T.pool_case_id)
def test_partpool_forward_and_backward_against_float64(case):
    print(f'worst ratio {O.check_pool_case(case, CPU):.3f}')


@pytest.mark.parametrize('kind', ('border_wins', 'all_negative', 'zero_image'))
def test_partpool_directed_cases(kind):
    O.directed_pool(CPU, kind)


def test_partpool_null_dw_and_null_db_raw_and_through_autograd():
    O.check_pool_null_outputs(CPU)


def test_partpool_strided_and_offset_views_give_the_bits_of_dense_ones():
    O.check_pool_views(CPU)


def test_partpool_refuses_48_channels_and_the_workspace_query_is_what_the_call_needs():
    O.check_pool_refused_and_workspace(CPU)


@pytest.mark.parametrize('rate', T.CAM_RATES)
@pytest.mark.parametrize('case', T.CAM_CASES, ids=T.cam_case_id)
def test_cam_boxes_are_the_references(case, rate):
    O.check_cam_case(case, rate, CPU)


@pytest.mark.parametrize('kind', ('constant', 'single_maximum', 'hot_corner', 'hot_first_corner', 'index_out_of_range'))
def test_cam_directed_cases(kind):
    O.directed_cam(CPU, kind)


def test_cam_box_through_the_crop_kernel_matches_interpolate():
    print(f'worst ratio {O.check_cam_crop(CPU):.3f}')


def test_cam_refusals():
    O.check_cam_refused(CPU)


def test_cam_closed_form_matches_the_references_gradcam():
    O.check_cam_closed_form()


@pytest.mark.parametrize('case', T.LOSS_CASES, ids=T.loss_case_id)
def test_loss_cases(case):
    print(f'worst ratio {O.check_loss_case(case, CPU):.3f}')


def test_loss_refuses_17_tensors():
    O.check_loss_refused(CPU)


@pytest.fixture
def plugin():
    from hawkeye_amd.model.registry import MODEL
    assert 'MGE_CNN' not in MODEL
    yield importlib.import_module(PLUGIN_MODULES[0])
    MODEL.pop('MGE_CNN', None)
    for name in PLUGIN_MODULES:
        sys.modules.pop(name, None)


def test_whole_short_model_matches_the_reference_in_eval(plugin, monkeypatch):
    print(f'worst error {O.check_model_eval(plugin, CPU, monkeypatch):.2e}')


def test_train_mode_step_without_labels_matches_the_reference(plugin, monkeypatch):
    print(f'worst ratio {O.check_model_train_step(plugin, CPU, monkeypatch):.3f}')


def test_two_step_trainer_run_with_a_short_trunk(tmp_path, monkeypatch):
    O.check_trainer(CPU, tmp_path, monkeypatch)
