"""The routing of the trunk's 3 x 3 kernels between the two bf16 MFMA shapes (functional.conv3x3_mfma_route, knob `conv_mfma`) without a
GPU: VGG-16 at 448 x 448, batch 64 and 16, takes the 16 x 16 x 32 shape exactly where the committed measurements say - every layer of
a (Cin, Cout, H, W) shape cleared the stand-alone bar (profiles/conv_mfma_timing.json) and was faster in the training step
(profiles/conv_mfma_step_layers.json); 0 and 1 force their shape; what was not measured keeps 32 x 32 x 16."""
import contextlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (Cin, Cout, side) of VGG-16's twelve 3 x 3 layers with multiples of 64 channels at a 448 x 448 input
LAYERS = {'conv1_2': (64, 64, 448), 'conv2_1': (64, 128, 224), 'conv2_2': (128, 128, 224), 'conv3_1': (128, 256, 112),
          'conv3_2': (256, 256, 112), 'conv3_3': (256, 256, 112), 'conv4_1': (256, 512, 56), 'conv4_2': (512, 512, 56),
          'conv4_3': (512, 512, 56), 'conv5_1': (512, 512, 28), 'conv5_2': (512, 512, 28), 'conv5_3': (512, 512, 28)}


@pytest.fixture
def route(monkeypatch):
    import hawkeye_amd.functional as F
    knobs = {b'conv_mfma': -1}
    monkeypatch.setattr(F, '_knob', lambda name: knobs[name])
    return F, knobs


def test_the_layers_are_the_stacks_own():
    from hawkeye_amd.model.backbone.vgg import VGG16_LAYOUT
    side, cin, found = 448, 3, []
    for v in VGG16_LAYOUT:
        if v == 'M':
            side //= 2
        else:
            if cin % 64 == 0:
                found.append((cin, v, side))
            cin = v
    assert found == list(LAYERS.values())


@pytest.mark.parametrize('batch', [64, 16])
def test_vgg16_takes_the_new_shape_where_the_committed_measurements_say(route, batch):
    F, knobs = route
    timing = json.load(open(os.path.join(ROOT, 'profiles', 'conv_mfma_timing.json')))['routing']
    step = json.load(open(os.path.join(ROOT, 'profiles', 'conv_mfma_step_layers.json')))[f'b{batch}']
    routed = 0
    for direction, section in (('fwd', 'forward'), ('bwd_data', 'input_gradient')):
        for name, (cin, cout, side) in LAYERS.items():
            same_shape = [m for m, s in LAYERS.items() if s == (cin, cout, side)]
            want = all(timing[f'{m}_{direction}_b{batch}']['clears_the_bar'] and step[section][m]['faster_in_the_step'] for m in same_shape)
            assert F.conv3x3_mfma_route(direction, cin, cout, batch, side, side) == want, (name, direction, batch)
            routed += want
    assert routed > 0


def test_the_knob_forces_either_shape_and_the_unmeasured_keeps_the_parents(route):
    F, knobs = route
    measured = next(iter(F.CONV_MFMA16_BWD_DATA.items()))
    (cin, cout, h, w), batches = measured
    assert F.conv3x3_mfma_route('bwd_data', cin, cout, batches[0], h, w)
    assert not F.conv3x3_mfma_route('bwd_data', cin, cout, 8, h, w)                 # a batch nobody measured
    assert not F.conv3x3_mfma_route('bwd_data', cin, cout, batches[0], h, w + 2)    # a map size nobody measured
    assert not F.conv3x3_mfma_route('fwd', 64, 64, 2, 8, 36)
    knobs[b'conv_mfma'] = 0
    assert not F.conv3x3_mfma_route('bwd_data', cin, cout, batches[0], h, w)
    assert isinstance(F._conv3x3_mfma('bwd_data', cin, cout, batches[0], h, w), contextlib.nullcontext)
    knobs[b'conv_mfma'] = 1
    assert F.conv3x3_mfma_route('fwd', 64, 64, 2, 8, 36) and F.conv3x3_mfma_route('bwd_data', cin, cout, 8, h, w)
    assert isinstance(F._conv3x3_mfma('fwd', 64, 64, 2, 8, 36), contextlib.nullcontext)      # a forced knob is the library's to read


def test_the_default_reaches_the_library_for_the_length_of_the_call(route):
    from hawkeye_amd import _lib
    F, knobs = route
    (cin, cout, h, w), batches = next(iter(F.CONV_MFMA16_FWD.items()))
    scope = F._conv3x3_mfma('fwd', cin, cout, batches[0], h, w)
    assert isinstance(scope, _lib.tuning) and scope.knobs == {'conv_mfma': 1}
    assert isinstance(F._conv3x3_mfma('fwd', cin, cout, 8, h, w), contextlib.nullcontext)
