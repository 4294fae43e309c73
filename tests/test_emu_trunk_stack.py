"""The assembled trunk through the CPU emulation, with no GPU: the judge of tests/trunk_stack_cases.py (float64 at the pattern the
kernels chose) on the short stack at 1 x 64 x 4 x 36, and the link protocol's configurations, the units driven by
conv_epilogue_cases.forward_by_hand as tests/test_emu_conv_epilogue.py drives them."""
import pytest
import torch

import trunk_stack_cases as T
from emu.harness import emulated

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated() as f:
        yield f


@pytest.fixture
def lib(F):
    from hawkeye_amd import _lib
    return _lib.load()


def test_emulated_short_stack_against_float64_at_the_kernels_pattern(F, lib, tune, monkeypatch):
    T.check_judged(F, lib, CPU, tune, monkeypatch, T.short_case(CPU, by_hand=True), by_hand=True)


@pytest.mark.parametrize('name', T.LINK_CASES)
@pytest.mark.parametrize('epi', [2, 1])
def test_emulated_link_protocol(F, lib, tune, monkeypatch, epi, name):
    T.link_case(F, lib, CPU, tune, monkeypatch, epi, name, by_hand=True)
