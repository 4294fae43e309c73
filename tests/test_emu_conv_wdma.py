"""The weight tiles of conv3x3_split_kernel by LDS-DMA (csrc/conv_fwd.hip, load_w: glds16 instead of registers + ds_write_b128) through
the CPU emulation, with no GPU: forward, input gradient and the four epilogues on both MFMA shapes, every output bit-equal to what the
register-staged kernel of the commit before gave (tests/golden/conv_wdma_emu.json, SHA-256 digests recorded with
tools/gen_conv_wdma_golden.py emu on that commit) - in the emulator's own work-item order and with the work-items of a workgroup
resumed in reverse and in a shuffled order.

What the emulation sees of the pipeline (tried on scratch copies of the kernel): the DMA of a tile issued one barrier
early - into the buffer the tap reads - changes every digest of every shape on both MFMA shapes when the request stands in front of
the tap's fragment reads (the emulated copy lands at once), and NONE when it stands behind the tap's MFMAs, in front of the barrier:
every work-item runs to its first MFMA, a wave collective, before any goes on, so all fragment reads of a tap are done before any
request behind them is made.  The end-of-tap wait loosened by one is INVISIBLE as well: s_waitcnt has no meaning in a model whose
memory operations complete when they are issued.  Only the device tells (tests/test_gpu_conv_wdma.py), and there only by chance."""
import pytest
import torch

import conv_wdma_cases as W

ORDERS = (None, 'rev', 'rand:11')
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def F():
    from emu import build_emu
    if build_emu._compiler() is None:
        pytest.skip('no clang++ to build the emulated kernels')
    from emu.harness import emulated
    with emulated() as f:
        yield f


@pytest.fixture(scope='module')
def recorded():
    return W.golden('emu')


@pytest.mark.parametrize('order', ORDERS, ids=lambda o: o or 'default')
@pytest.mark.parametrize('mf', (0, 1), ids=('mfma32', 'mfma16'))
@pytest.mark.parametrize('shape', W.SHAPES, ids=W.IDS)
def test_every_output_keeps_the_bits_of_the_register_staged_kernel(F, recorded, monkeypatch, shape, mf, order):
    from hawkeye_amd import _lib
    if order is not None:
        monkeypatch.setenv('HK_EMU_ORDER', order)
    want = recorded['x'.join(map(str, shape))][f'mf{mf}']
    got = W.digests(_lib.load(), CPU, shape, mf)
    assert sorted(got) == sorted(want)
    assert len(got) == (8 if shape[1] % 2 == 0 and shape[2] % 2 == 0 else 6)              # (the pooled forward wants even H and W)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (shape, mf, order, differ)
