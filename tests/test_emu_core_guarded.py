"""The library's original ops through the C ABI on the CPU emulation, with no GPU: the cases of tests/core_guarded_cases.py - guarded and
poisoned buffers, a workspace of exactly hk_*_ws_bytes, every element judged against float64.  What the emulation shows: the index
arithmetic of every dispatch form (an out-of-bounds store lands in a guard row, an element nobody writes stays NaN), the workspace
layouts, the summation lengths.  That the device's own instructions agree is tests/test_gpu_core_guarded.py's.

Also here, needing neither: every entry point of these families has a runner (test_every_core_entry_point_has_a_guarded_runner)."""
import pytest
import torch

import core_guarded_cases as C

CPU = torch.device('cpu')

# Cases left out of THIS tier only (the GPU tier runs them all): {family: {case: the reason}}; at most a quarter of a family, and never the
# only case of a dispatch form (test_the_emulation_tier_leaves_out_little).  Empty: the largest case, nine 256 x 256 Newton-Schulz chains,
# takes half a minute here.
EMU_SLOW = {}


@pytest.fixture
def lib(monkeypatch):
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    monkeypatch.delenv('HK_EMU_ORDER', raising=False)
    from emu.harness import emulated
    from hawkeye_amd import _lib
    with emulated():
        yield _lib.load()


def _kept(family, cases, ids):
    slow = EMU_SLOW.get(family, {})
    return pytest.mark.parametrize('case', [c for c in cases if c not in slow], ids=[i for c, i in zip(cases, ids) if c not in slow])


@_kept('bgemm', C.BGEMM_CASES, C.BGEMM_IDS)
def test_bgemm(lib, case):
    C.run_bgemm(lib, CPU, case)


@_kept('bcnn', C.BCNN_CASES, C.BCNN_IDS)
def test_bcnn(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_bcnn(lib, CPU, shape, dict(knobs))


@_kept('ssqrt', C.SSQRT_CASES, C.SSQRT_IDS)
def test_signed_sqrt(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_ssqrt(lib, CPU, shape, dict(knobs))


@_kept('cov', C.COV_CASES, C.COV_IDS)
def test_covariance(lib, tune, case):
    shape, knobs = case
    for k, v in knobs:
        tune(k, v)
    C.run_cov(lib, CPU, shape, dict(knobs))


@_kept('ns', C.NS_CASES, C.NS_IDS)
def test_newton_schulz(lib, tune, case):
    tune('ns_tn', case[3])
    tune('ns_streams', case[4])
    tune('ns_sym', case[5])
    C.run_ns(lib, CPU, case)


@pytest.mark.parametrize('case', C.TRIU_CASES, ids=[f'b{b}-d{d}' for b, d in C.TRIU_CASES])
def test_triu_vec(lib, case):
    C.run_triu(lib, CPU, case)


@_kept('cbp', C.CBP_CASES, C.CBP_IDS)
def test_cbp(lib, tune, case):
    tune('cbp_bin', case[1])
    for k, v in (C.CBP_VARIANTS[case[2]] if len(case) > 2 else {}).items():
        tune(k, v)
    C.run_cbp(lib, CPU, case)


@pytest.mark.parametrize('shape', C.RECT_CASES, ids=['x'.join(map(str, s)) for s in C.RECT_CASES])
def test_cbp_two_inputs(lib, shape):
    C.run_rect(lib, CPU, shape)


def test_cbp_per_location_backward_at_the_lds_limit(lib):
    C.run_rect_lds_limit(lib, CPU)


@_kept('linear', C.LINEAR_CASES, C.LINEAR_IDS)
def test_classifier(lib, tune, case):
    tune('linear_slabs', case[3])
    C.run_linear(lib, CPU, case)


@_kept('cin', C.CIN_CASES, C.CIN_IDS)
def test_cin(lib, tune, case):
    tune('bcnn_generic', case[1])
    C.run_cin(lib, CPU, case)


def test_short_workspaces_are_refused_and_nothing_is_written(lib, tune):
    C.run_refusals(lib, CPU, tune)


def test_forms_that_agree_bit_for_bit_still_do_on_poisoned_buffers(lib, tune):
    C.run_bit_identity(lib, CPU, tune)


# ------------------------------------------------------------------------------------------------------------------ no library needed
def test_every_core_entry_point_has_a_guarded_runner():
    """An entry point added to one of these families without a guarded case fails here."""
    from hawkeye_amd._lib import SIGNATURES
    core = [n for n in SIGNATURES if n.startswith(C.FAMILIES)]
    assert len(core) >= 38
    missing = [n for n in core if n not in C.RUNNERS and not C.is_helper(n)]
    assert missing == []
    assert [n for n in C.RUNNERS if n not in SIGNATURES] == []                      # and the table names nothing that is gone
    helpers = sorted(n for n in core if C.is_helper(n))
    assert helpers == ['hk_bcnn_pool_ws_bytes', 'hk_bcnn_ssqrt_ws_bytes', 'hk_cbp_plan_build', 'hk_cbp_plan_bytes', 'hk_cbp_plan_destroy',
                       'hk_cbp_rect_plan_build', 'hk_cbp_rect_plan_bytes', 'hk_cbp_ws_bytes', 'hk_cin_cci_ws_bytes', 'hk_linear_ws_bytes',
                       'hk_ns_sqrtm_ws_bytes']


def test_newton_schulz_cases_cover_every_pair_of_axes():
    assert C.ns_axes_covered() == []
    for axis, values in (('d', {128, 256, 200, 70, 33, 5}), ('iter_n', {1, 2, 3, 5}), ('B', {1, 3, 9, 16, 17}), ('ns_tn', {0, 64, 128}),
                         ('ns_streams', {0, 1}), ('ns_sym', {0, 1})):
        assert {c[C.NS_AXES.index(axis)] for c in C.NS_CASES} == values, axis
    assert {c[6] for c in C.NS_CASES} == {'fwd', 'sym', 'triu', 'triu_sym'} and {c[7] for c in C.NS_CASES} == {'bwd', 'general'}
    # the two-queue dispatch exists only from 16 samples up and from two iterations up (NsDispatch, csrc/mpn.hip:254, :354): it has to be
    # reached with even and ragged halves, on the fast and the edge path, by every forward entry and both backwards
    two = [c for c in C.NS_CASES if c[2] >= 16 and c[4] == 1 and c[1] >= 2]
    assert {c[2] for c in two} == {16, 17} and {c[0] % 128 == 0 for c in two} == {True, False}
    assert {c[6] for c in two} >= {'fwd', 'sym', 'triu'} and {c[7] for c in two} == {'bwd', 'general'}
    assert any(c[2] >= 16 and c[4] == 0 for c in C.NS_CASES)


def test_the_emulation_tier_leaves_out_little():
    families = dict(bgemm=C.BGEMM_CASES, bcnn=C.BCNN_CASES, ssqrt=C.SSQRT_CASES, cov=C.COV_CASES, ns=C.NS_CASES, cbp=C.CBP_CASES,
                    linear=C.LINEAR_CASES, cin=C.CIN_CASES)
    for family, slow in EMU_SLOW.items():
        assert all(c in families[family] for c in slow), family
        assert 4 * len(slow) <= len(families[family]), family
        assert all(len(reason) > 10 for reason in slow.values())
