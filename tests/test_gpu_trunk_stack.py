"""The assembled VGG trunk on the GPU against float64, single shot: ConvStack.forward's routing, functional._ConvUnit and the ConvLink
protocol, judged at the activation pattern the device chose (tests/trunk_stack_cases.py: the judge, its bounds and the stacks), the
link protocol in the configurations of a real training step and of fine-tuning, and one print-only diagnostic of the library's
routes under the same judge.  No comparison here is repeated."""
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
def lib(F):
    from hawkeye_amd import _lib
    return _lib.load()


def test_vgg16_stack_against_float64_at_the_device_pattern(F, lib, tune, monkeypatch):
    """The whole VGG-16 stack on 2 x 3 x 32 x 80 (T.vgg_case): forward elementwise, the free-pattern cap, every dW and db within 5 x
    the largest yardstick, `conv_epi` 2, 1 and 0 against each other.  The calls are counted: the first layer on hk_conv1_bias_relu,
    all twelve 3 x 3 layers as fused units (four pooled inside the kernel; the last stage's 2 x 5 map is odd, so its pool is the
    MaxPool2d child), the masked input gradient for all seven linked pairs - a silent fall-back to the library fails here."""
    case = T.vgg_case(DEV)
    judge, runs = T.check_judged(F, lib, DEV, tune, monkeypatch, case)
    e = T.expected_calls(case[0], judge.maps, False)
    assert (e['hk_conv1_bias_relu_fwd'], e['hk_conv3x3_bias_relu_fwd'], e['hk_conv3x3_bias_relu_pool_fwd'], e['hk_conv3x3_masked_bwd_data'],
            e['hk_conv3x3_bwd_data'], e['hk_conv3x3_wrw'], e['hk_bias_relu_bwd'], e['hk_bias_relu_pool_bwd']) == (1, 8, 4, 7, 5, 12, 1, 4)
    assert tuple(runs[2]['y'].shape) == (2, 512, 1, 2) and 'dx' not in runs[2] and len(runs[2]) == 1 + 26


def test_short_stack_against_float64_at_the_device_pattern(F, lib, tune, monkeypatch):
    """64 -> 64, 64 -> 64 + pool, 64 -> 128, 128 -> 128 + pool on 2 x 64 x 8 x 36, the input requiring a gradient: the all-trainable
    run that the link cases below take as their reference."""
    T.check_judged(F, lib, DEV, tune, monkeypatch, T.short_case(DEV))


def test_batch_of_one_on_a_two_by_two_map_against_float64(F, lib, tune, monkeypatch):
    """1 x 64 x 2 x 2 through two stages, the second (a linked pair) at 1 x 1."""
    T.check_judged(F, lib, DEV, tune, monkeypatch, T.tiny_case(DEV))


@pytest.mark.parametrize('name', T.LINK_CASES)
@pytest.mark.parametrize('epi', [2, 1])
def test_link_protocol(F, lib, tune, monkeypatch, epi, name):
    """The ConvLink protocol on the short stack in one configuration nobody had run (T.link_case: frozen producers and consumers, no
    input gradient, accumulation, a partial backward, overlapping graphs, no_grad, checkpointing), `conv_epi` 2 and 1: the gradients
    it computes equal the all-trainable run's bit for bit - that run is the one the test above judges against float64."""
    T.link_case(F, lib, DEV, tune, monkeypatch, epi, name)


def test_library_routes_under_the_same_judge_print_only(F, lib, tune):
    """Diagnostic, asserts nothing beyond "finite": the VGG-16 stack with the five route knobs at 0 (the library's convolutions around
    the first layer's kernel and the hk_bias_relu_* passes) through the same judge, twice.  Printed: whether the two runs' prefix
    patterns are identical, and each gradient's distance to float64 at its own run's pattern (DESIGN 3.10 records the lines)."""
    for knob in T.KNOBS:
        tune(knob, 0)
    stack, x, dy, x_grad = T.vgg_case(DEV)
    fwd = T.forward_of(F, False)
    judges = []
    for attempt in range(2):
        maps = T.prefix_maps(fwd, stack, x)
        if judges and T.same_patterns(judges[0].patterns, T.patterns_of(maps, asserting=False)):
            judge = judges[0]                                          # the same pattern: the same reference
        else:
            judge = T.Judge(stack, x, dy, maps, asserting=False)
        judges.append(judge)
        got = T.train_run(fwd, stack, x, dy, x_grad)
        same_y = T.same_bits(got['y'], maps[-1][1])
        print(f'[library routes, run {attempt}] the full run\'s output equals the last prefix bit for bit: {same_y}')
        judge.gradients(f'library routes, run {attempt}', got, asserting=False)
        assert all(bool(torch.isfinite(v).all()) for v in got.values())
    print(f'[library routes] prefix patterns of the two runs identical: {judges[0] is judges[1]}')
