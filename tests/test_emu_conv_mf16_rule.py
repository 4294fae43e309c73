"""The MFMA shape of conv3x3_split_kernel chosen in the library (csrc/conv_fwd.hip, conv3x3_mfma16_wins) through the CPU emulation, with
no GPU: the checks of tests/conv_mf16_cases.py - the default of knob `conv_mfma` gives every entry point the bits of `conv_mfma` 1 and
not those of 0, and that result holds against float64, the passes the epilogues replace and a second launch - and, with the
work-items of a workgroup resumed in reverse and in a shuffled order, the default knob's bits once more.

The rule is host code: the emulated build runs the same function.  What the emulation cannot see is a fragment read moved across a
barrier (tests/test_emu_conv_wdma.py's docstring); the recorded device digests of tests/test_gpu_conv_wdma.py are the check for that."""
import pytest
import torch

import conv_mf16_cases as C


@pytest.fixture(scope='module')
def runs():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    from emu.harness import emulated
    from hawkeye_amd import _lib
    with emulated():
        yield C.Runs(_lib.load(), torch.device('cpu'))


@pytest.mark.parametrize('shape', C.SHAPES, ids=C.IDS)
def test_emulated_default_knob_runs_the_16x16x32_kernels_and_holds(runs, shape):
    C.check_rule(runs, shape)
    C.check_default(runs, shape)


@pytest.mark.parametrize('order', ('rev', 'rand:11'))
@pytest.mark.parametrize('shape', C.SHAPES, ids=C.IDS)
def test_emulated_default_knob_in_another_work_item_order(runs, monkeypatch, shape, order):
    want = runs(shape, -1)                                               # the emulator's own order (made once per module)
    monkeypatch.setenv('HK_EMU_ORDER', order)
    got = runs.fresh(shape, -1)
    differ = [k for k in want if not C.same(want[k], got[k])]
    assert sorted(got) == C.names(shape) and not differ, (shape, order, differ)
