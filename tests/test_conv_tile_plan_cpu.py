"""The tiling plan of conv3x3_split_kernel (csrc/conv_fwd.hip: conv3x3_plan, knob `conv_tile`) through hk_conv3x3_tile_plan - a host-side
query, no GPU: the tile counts of VGG-16's maps at 448 x 448 input, ties, the upper bound the masked input gradient's workspace relies
on, and the knob's plumbing."""
import ctypes
import os

import pytest

from conv_tile_cases import PLAN, SHAPES, plan, tiles_4x32
from conv_wdma_cases import _Knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from hawkeye_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# map side -> tiles per image with the plan; 4 x 32 everywhere gives tiles_4x32
VGG = {448: 1568, 224: 392, 112: 98, 56: 25, 28: 7}
VGG_4x32 = {448: 1568, 224: 392, 112: 112, 56: 28, 28: 7}


def test_the_knob_defaults_to_the_plan_and_reads_the_environment_name(lib):
    v = ctypes.c_int(7)
    assert lib.hk_tuning_get(b'conv_tile', ctypes.byref(v)) == 0
    assert v.value == int(os.environ.get('HK_CONV_TILE', -1))
    src = open(os.path.join(ROOT, 'hawkeye_amd', 'csrc', 'api.hip')).read()
    assert '{"conv_tile", "HK_CONV_TILE", &Tuning::conv_tile}' in src


@pytest.mark.parametrize('side', sorted(VGG))
def test_tiles_of_the_vgg_maps(lib, side):
    with _Knobs(lib, conv_tile=-1):
        tiles, regions = plan(lib, 64, side, side, 1)
        assert tiles == VGG[side]
        if side == 112:
            assert regions == [(8, 16, 14, 7, 0)]
        elif side == 56:
            assert regions == [(8, 16, 7, 3, 0), (16, 8, 4, 1, 48)]
        else:
            assert regions == [(4, 32, (side + 3) // 4, (side + 31) // 32, 0)]          # (448 and 224: 8 x 16 ties; a tie keeps 4 x 32)
    with _Knobs(lib, conv_tile=0):
        for mf in (0, 1):
            assert plan(lib, 64, side, side, mf) == (VGG_4x32[side], [(4, 32, (side + 3) // 4, (side + 31) // 32, 0)])
            assert tiles_4x32(side, side) == VGG_4x32[side]


def test_the_32x32x16_shape_has_no_16x8(lib):
    with _Knobs(lib, conv_tile=-1):
        assert plan(lib, 64, 56, 56, 0) == (28, [(4, 32, 14, 2, 0)])                    # 8 x 16 alone: 7 x 4 = 28, a tie
        assert plan(lib, 64, 112, 112, 0) == (98, [(8, 16, 14, 7, 0)])
        for side in (448, 224, 28):
            assert plan(lib, 64, side, side, 0)[0] == VGG[side]
        for h in range(1, 40):
            for w in range(1, 70):
                assert all(r[:2] != (16, 8) for r in plan(lib, 1, h, w, 0)[1]), (h, w)


@pytest.mark.parametrize('mf', (0, 1))
def test_never_more_tiles_than_4x32_and_ties_keep_it(lib, mf):
    with _Knobs(lib, conv_tile=-1):
        for h in list(range(1, 40)) + [56, 112]:
            for w in list(range(1, 70)) + [112, 224]:
                tiles, regions = plan(lib, 1, h, w, mf)
                old = tiles_4x32(h, w)
                assert tiles <= old, (h, w)
                assert tiles == sum(r[2] * r[3] for r in regions)
                if tiles == old:
                    assert regions == [(4, 32, (h + 3) // 4, (w + 31) // 32, 0)], (h, w)
                # the regions cover the map's columns exactly once, the last strip possibly ragged; every tile is 128 pixels
                col = 0
                for th, tw, nrb, nstrips, c0 in regions:
                    assert th * tw == 128 and c0 == col and nrb == (h + th - 1) // th and nstrips > 0
                    col += tw * nstrips
                assert w <= col < w + regions[-1][1]
                if len(regions) == 2:
                    assert regions[0][:2] == (8, 16) and regions[1][:2] == (16, 8) and regions[1][4] == 16 * (w // 16)


def test_the_kernel_tests_shapes_reach_what_they_say(lib):
    with _Knobs(lib, conv_tile=-1):
        for mf in (0, 1):
            for s in SHAPES:
                assert plan(lib, s[0], s[1], s[2], mf) == PLAN[mf][s], (s, mf)
        assert plan(lib, 2, 7, 34, 1) == (3, [(8, 16, 1, 3, 0)]) and tiles_4x32(7, 34) == 4     # the shape of the recorded digests


def test_header_table_and_library_agree(lib):
    import re
    from hawkeye_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hawkeye_conv_tile.h')).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(hk_[a-z0-9_]+)\s*\(', src))) == sorted(_lib.TRUNK_TILE_SIGNATURES) == ['hk_conv3x3_tile_plan']
    assert '#include "hawkeye_conv_tile.h"' in open(os.path.join(ROOT, 'include', 'hawkeye_hip.h')).read()
    params = re.search(r'\bhk_conv3x3_tile_plan\s*\(([^)]*)\)', src).group(1)
    assert len(params.split(',')) == len(_lib.TRUNK_TILE_SIGNATURES['hk_conv3x3_tile_plan'][1])
    assert hasattr(lib, 'hk_conv3x3_tile_plan')


def test_bad_arguments(lib):
    out = (ctypes.c_int * 12)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert lib.hk_conv3x3_tile_plan(1, 8, 8, 1, None) == -1
    assert lib.hk_conv3x3_tile_plan(0, 8, 8, 1, p) == -1 and lib.hk_conv3x3_tile_plan(1, 8, 0, 1, p) == -1
    assert lib.hk_conv3x3_tile_plan(1, 8, 8, 2, p) == -1
