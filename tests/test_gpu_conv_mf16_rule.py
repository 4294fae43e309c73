"""The MFMA shape of conv3x3_split_kernel chosen in the library (csrc/conv_fwd.hip, conv3x3_mfma16_wins) on the GPU: at the default of
knob `conv_mfma` every entry point - forward, input gradient, the four epilogues - runs on 16 x 16 x 32 at every shape of
tests/conv_mf16_cases.py (each tile geometry, a mixed launch, a restart of the chains), seen by its bits; and that result is held to
float64, to the passes the epilogues replace, to a second launch and to its guard rows (the checks and their bounds:
tests/conv_mf16_cases.py)."""
import pytest
import torch

import conv_mf16_cases as C

pytestmark = pytest.mark.gpu
EACH = pytest.mark.parametrize('shape', C.SHAPES, ids=C.IDS)


@pytest.fixture(scope='module')
def runs():
    from hawkeye_amd import _lib
    lib = _lib.load()
    assert b'gfx950' in lib.hk_version()
    return C.Runs(lib, torch.device('cuda'), _lib.stream())


def test_the_knob_defaults_to_the_rule(runs):
    import ctypes
    v = ctypes.c_int(0)
    assert runs.lib.hk_tuning_get(b'conv_mfma', ctypes.byref(v)) == 0 and v.value == -1


@EACH
def test_the_default_knob_runs_the_16x16x32_kernels(runs, shape):
    C.check_rule(runs, shape)


@EACH
def test_the_default_knob_against_float64_the_passes_and_a_second_launch(runs, shape):
    C.check_default(runs, shape)
