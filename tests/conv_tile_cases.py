"""Shapes, expected plans and the comparison shared by tests/test_emu_conv_tile.py (CPU emulation), tests/test_gpu_conv_tile.py (MI355X)
and tests/test_conv_tile_plan_cpu.py: the tile geometries of conv3x3_split_kernel (csrc/conv_fwd.hip, G; knob `conv_tile`).  Not a test module.

Which 128 pixels a workgroup takes changes no operand and no order of additions of any output element - only the lane that holds it - so
every output of every entry point at `conv_tile` = -1 (the plan) keeps the bits it has at `conv_tile` = 0 (4 x 32 everywhere).  One
exception in kind, none expected in bits: the bias gradient of the masked input gradient is a float64 sum over other partial rows, rounded
once; where it ever differs it has to stay inside db_bound of tests/conv_epilogue_cases.py.

The inputs and the guard rows are those of tests/conv_wdma_cases.py: outputs() runs all entry points between 1e30 guard rows."""
import ctypes

import torch

from conv_epilogue_cases import bits, db_bound
from conv_wdma_cases import _Knobs, outputs

# (N, H, W, Cin, Cout): the smallest that reach each geometry and each way a tile can be ragged; all even-sized: the pooled epilogue runs
SHAPES = [
    (1, 8, 16, 64, 64),                         # one 8 x 16 tile
    (2, 18, 48, 128, 128),                      # 8 x 16: ragged rows, three strips, two images, two Cout tiles, a chain restart
    (1, 16, 24, 64, 64),                        # 8 x 16 and 16 x 8 regions in one launch
    (1, 20, 40, 192, 64),                       # both regions ragged in rows, an odd chunk count
    (1, 16, 8, 64, 64),                         # 16 x 8 alone
]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
MIXED = SHAPES[2]

# hk_conv3x3_tile_plan at `conv_tile` = -1: (tiles per image, [(tile rows, tile columns, row blocks, strips, first column) per region])
PLAN = {
    1: {                                        # 16 x 16 x 32 MFMA: all three geometries
        SHAPES[0]: (1, [(8, 16, 1, 1, 0)]),
        SHAPES[1]: (9, [(8, 16, 3, 3, 0)]),
        SHAPES[2]: (3, [(8, 16, 2, 1, 0), (16, 8, 1, 1, 16)]),
        SHAPES[3]: (8, [(8, 16, 3, 2, 0), (16, 8, 2, 1, 32)]),
        SHAPES[4]: (1, [(16, 8, 1, 1, 0)]),
    },
    0: {                                        # 32 x 32 x 16 MFMA: no 16 x 8
        SHAPES[0]: (1, [(8, 16, 1, 1, 0)]),
        SHAPES[1]: (9, [(8, 16, 3, 3, 0)]),
        SHAPES[2]: (4, [(4, 32, 4, 1, 0)]),     # 8 x 16 gives four tiles as well: a tie keeps 4 x 32
        SHAPES[3]: (9, [(8, 16, 3, 3, 0)]),
        SHAPES[4]: (2, [(8, 16, 2, 1, 0)]),
    },
}


def plan(lib, n, h, w, mf):
    """hk_conv3x3_tile_plan under the knobs as they stand -> (tiles per image, [region tuples])."""
    out = (ctypes.c_int * 12)(*([-7] * 12))
    assert lib.hk_conv3x3_tile_plan(n, h, w, mf, ctypes.cast(out, ctypes.c_void_p)) == 0
    v = list(out)
    assert v[1] in (1, 2) and (v[1] == 2 or v[7:] == [0] * 5)
    return v[0], [tuple(v[2 + 5 * i:7 + 5 * i]) for i in range(v[1])]


def tiles_4x32(h, w):
    return ((h + 3) // 4) * ((w + 31) // 32)


def check_against_4x32(lib, dev, shape, mf, stream=None, twice=False):
    """Every output of every entry point at `shape` with the planned tiling against 4 x 32 everywhere, bit for bit; the plan asserted
    through hk_conv3x3_tile_plan.  `twice`: the planned tiling a second time, bit-equal to the first."""
    n, h, w, cin, cout = shape
    with _Knobs(lib, conv_tile=0):
        assert plan(lib, n, h, w, mf) == (tiles_4x32(h, w), [(4, 32, (h + 3) // 4, (w + 31) // 32, 0)])
        ref = outputs(lib, dev, shape, mf, stream)
    with _Knobs(lib, conv_tile=-1):
        assert plan(lib, n, h, w, mf) == PLAN[mf][shape], (shape, mf)
        got = outputs(lib, dev, shape, mf, stream)
        again = outputs(lib, dev, shape, mf, stream) if twice else got
    assert sorted(got) == sorted(ref) and len(got) == 8
    for k in ref:
        assert ref[k].shape == got[k].shape and torch.equal(bits(again[k]), bits(got[k])), (shape, mf, k, 'two launches')
        if k == 'masked_bwd_data_db':
            continue
        assert torch.equal(bits(got[k]), bits(ref[k])), (shape, mf, k)
    db, db0 = got['masked_bwd_data_db'], ref['masked_bwd_data_db']
    if not torch.equal(bits(db), bits(db0)):
        # another grouping of the float64 partial sums met a rounding boundary: still the float next to the exact sum
        db64, allowed = db_bound(ref['masked_bwd_data'].view(n, h, w, cin).permute(0, 3, 1, 2))
        err = (db.double() - db64).abs()
        print(f'bias gradient {shape} mf{mf}: differs from 4 x 32 in {int((bits(db) != bits(db0)).sum())} channels, '
              f'max |db - db64| = {float(err.max()):.3e} (allowed there {float(allowed[err.argmax()]):.3e})')
        assert bool((err <= allowed).all()), (shape, mf)
