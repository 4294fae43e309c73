"""The library's original ops through the C ABI on the GPU: the cases of tests/core_guarded_cases.py - guarded and poisoned buffers, a
workspace of exactly hk_*_ws_bytes, every element judged against float64.  What only the device shows: the matrix instructions' operand
and result layouts in every dispatch form, the LDS-DMA and buffer addressing at ragged edges (a store past the end lands in a guard
row, not in the allocator's slack), the LDS limits, and the forms that run on more than one queue.  Every case prints its worst
error / bound per output."""
import pytest
import torch

import core_guarded_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')


@pytest.fixture(scope='module')
def lib():
    from hawkeye_amd import _lib
    lib_ = _lib.load()
    assert b'gfx950' in lib_.hk_version()
    return lib_


@pytest.mark.parametrize('case', C.BGEMM_CASES, ids=C.BGEMM_IDS)
def test_bgemm(lib, case):
    C.run_bgemm(lib, DEV, case)


@pytest.mark.parametrize('case', C.BCNN_CASES, ids=C.BCNN_IDS)
def test_bcnn(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_bcnn(lib, DEV, shape, dict(knobs))


@pytest.mark.parametrize('case', C.SSQRT_CASES, ids=C.SSQRT_IDS)
def test_signed_sqrt(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_ssqrt(lib, DEV, shape, dict(knobs))


@pytest.mark.parametrize('case', C.COV_CASES, ids=C.COV_IDS)
def test_covariance(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_cov(lib, DEV, shape, dict(knobs))


@pytest.mark.parametrize('case', C.NS_CASES, ids=C.NS_IDS)
def test_newton_schulz(lib, tune, case):
    tune('ns_tn', case[3])
    tune('ns_streams', case[4])
    tune('ns_sym', case[5])
    C.run_ns(lib, DEV, case)


@pytest.mark.parametrize('case', C.TRIU_CASES, ids=[f'b{b}-d{d}' for b, d in C.TRIU_CASES])
def test_triu_vec(lib, case):
    C.run_triu(lib, DEV, case)


@pytest.mark.parametrize('case', C.CBP_CASES, ids=C.CBP_IDS)
def test_cbp(lib, tune, case):
    tune('cbp_bin', case[1])
    for k, v in (C.CBP_VARIANTS[case[2]] if len(case) > 2 else {}).items():
        tune(k, v)
    C.run_cbp(lib, DEV, case)


@pytest.mark.parametrize('shape', C.RECT_CASES, ids=['x'.join(map(str, s)) for s in C.RECT_CASES])
def test_cbp_two_inputs(lib, shape):
    C.run_rect(lib, DEV, shape)


def test_cbp_per_location_backward_at_the_lds_limit(lib):
    C.run_rect_lds_limit(lib, DEV)


@pytest.mark.parametrize('case', C.LINEAR_CASES, ids=C.LINEAR_IDS)
def test_classifier(lib, tune, case):
    tune('linear_slabs', case[3])
    C.run_linear(lib, DEV, case)


@pytest.mark.parametrize('case', C.CIN_CASES, ids=C.CIN_IDS)
def test_cin(lib, tune, case):
    tune('bcnn_generic', case[1])
    C.run_cin(lib, DEV, case)


def test_short_workspaces_are_refused_and_nothing_is_written(lib, tune):
    C.run_refusals(lib, DEV, tune)


def test_forms_that_agree_bit_for_bit_still_do_on_poisoned_buffers(lib, tune):
    C.run_bit_identity(lib, DEV, tune)
