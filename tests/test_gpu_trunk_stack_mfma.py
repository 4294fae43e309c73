"""The assembled trunk on the GPU with every 3 x 3 kernel on the 16 x 16 x 32 bf16 MFMA (knob `conv_mfma` 1) against float64, single shot,
at the activation pattern the device chose: tests/trunk_stack_cases.py's judge, its factor of 5 over the CPU yardstick, its 0.02 % cap
on undecided outputs and its counted calls, on the short stack (2 x 64 x 8 x 36) and the two-stage 1 x 64 x 2 x 2 stack."""
import pytest
import torch

import trunk_stack_cases as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


@pytest.fixture(scope='module')
def F():
    import hawkeye_amd.functional as F_
    from hawkeye_amd import _lib
    assert b'gfx950' in _lib.load().hk_version()
    return F_


@pytest.fixture
def lib(F, tune):
    from hawkeye_amd import _lib
    tune('conv_mfma', 1)
    return _lib.load()


def test_short_stack_against_float64_at_the_device_pattern(F, lib, tune, monkeypatch):
    T.check_judged(F, lib, DEV, tune, monkeypatch, T.short_case(DEV))


def test_batch_of_one_on_a_two_by_two_map_against_float64(F, lib, tune, monkeypatch):
    T.check_judged(F, lib, DEV, tune, monkeypatch, T.tiny_case(DEV))
