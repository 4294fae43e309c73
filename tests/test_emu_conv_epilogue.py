"""The epilogues inside conv3x3_split_kernel (csrc/conv_fwd.hip, EPI) through the CPU emulation, with no GPU: the checks of
tests/conv_epilogue_cases.py at their smallest shapes - the sign bytes' exchange between the two lanes of a pixel, the parked tile
and the pooled windows, the mask bytes and the butterfly of the column sums, ragged tiles in both directions - and the order
independence of the two epilogues that add barrier intervals (the pooled forward and the partial sums), run the way
tests/test_emu_order.py runs its kernels."""
import pytest
import torch

import conv_epilogue_cases as C
from emu.harness import emulated

ORDERS = ('rev', 'rand:11')
CPU = torch.device('cpu')
SMALL_A, SMALL_B = C.SHAPES_A[:4], C.SHAPES_B[:3]


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    with emulated() as f:
        yield f


@pytest.fixture
def lib(F, tune):
    from hawkeye_amd import _lib
    tune('conv_fwd', 1)
    tune('conv_bwd_data', 1)
    tune('conv_epi', 2)
    return _lib.load()


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', SMALL_A, ids=C.ids(SMALL_A))
def test_emulated_bias_relu_forward_equals_the_two_kernels(F, lib, shape, variant):
    C.check_bias_relu(F, lib, CPU, shape, variant)


@pytest.mark.parametrize('variant', ['signed', 'zero'])
@pytest.mark.parametrize('shape', SMALL_B, ids=C.ids(SMALL_B))
def test_emulated_bias_relu_pool_forward_equals_the_two_kernels(F, lib, shape, variant):
    C.check_bias_relu_pool(F, lib, CPU, shape, variant)


@pytest.mark.parametrize('variant', ['random', 'set'])
@pytest.mark.parametrize('shape', SMALL_A, ids=C.ids(SMALL_A))
def test_emulated_masked_input_gradient_equals_the_two_kernels(F, lib, shape, variant):
    C.check_masked_bwd_data(F, lib, CPU, shape, variant)


def test_emulated_stack_with_the_epilogues_inside_against_the_passes(F, lib, tune, monkeypatch):
    C.check_stack(F, lib, CPU, tune, monkeypatch, by_hand=True)


ORDER_CASES = [('pool', shape) for shape in SMALL_B] + [('masked', shape) for shape in SMALL_A]


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('which,shape', ORDER_CASES, ids=[w + '-' + i for (w, _), i in zip(ORDER_CASES, C.ids(SMALL_B) + C.ids(SMALL_A))])
def test_emulated_epilogues_do_not_depend_on_the_work_item_order(F, lib, which, shape, order, monkeypatch):
    """The same cases pass with the work-items of a workgroup resumed in another order: the outputs still equal the two-kernel path's bit
    for bit (whose own order independence is tests/test_emu_order.py's).  A difference would be a missing barrier around the parked
    tile or the waves' partial sums."""
    monkeypatch.setenv('HK_EMU_ORDER', order)
    if which == 'pool':
        C.check_bias_relu_pool(F, lib, CPU, shape, 'signed')
    else:
        C.check_masked_bwd_data(F, lib, CPU, shape, 'random')


def test_emulated_entry_points_refuse_below_their_level(F, lib, tune):
    from hawkeye_amd._lib import HK_ERR_UNSUPPORTED
    shape = (1, 2, 2, 64, 64)
    n, h, w, cin, cout = shape
    x, wt, bias = C.forward_inputs(shape, 'zero', CPU)
    dy, _, mask = C.backward_inputs(shape, 'set', CPU)
    ws = torch.empty(lib.hk_conv3x3_masked_ws_bytes(n, h, w, cin, cout), dtype=torch.uint8)
    y, mk, db = torch.empty(n, h, w, cout), torch.empty(n, h, w, cout // 4, dtype=torch.uint8), torch.empty(cin)
    fwd = lambda: lib.hk_conv3x3_bias_relu_fwd(C._p(x), C._p(wt), C._p(bias), C._p(y), C._p(mk), n, h, w, cin, cout, C._p(ws), ws.numel(), None)
    pool = lambda hh: lib.hk_conv3x3_bias_relu_pool_fwd(C._p(x), C._p(wt), C._p(bias), C._p(y), C._p(mk), n, hh, w, cin, cout, C._p(ws), ws.numel(), None)
    bwd = lambda: lib.hk_conv3x3_masked_bwd_data(C._p(dy), C._p(wt), C._p(mask), C._p(y), C._p(db), n, h, w, cin, cout, C._p(ws), ws.numel(), None)
    assert (fwd(), pool(h), bwd()) == (0, 0, 0)
    assert pool(1) == HK_ERR_UNSUPPORTED                                   # an odd height
    tune('conv_epi', 1)
    assert (fwd(), pool(h), bwd()) == (0, 0, HK_ERR_UNSUPPORTED)
    tune('conv_epi', 0)
    assert (fwd(), pool(h), bwd()) == (HK_ERR_UNSUPPORTED,) * 3
