"""The routing of the trunk's forward and input gradient (functional.CONV_FWD_WINS / CONV_BWD_DATA_WINS, knobs `conv_fwd` /
`conv_bwd_data`) and the agreement of include/hawkeye_conv.h, hawkeye_amd/_lib.py: TRUNK_SIGNATURES and the built library - no GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the twelve layers of VGG-16 at a 448 x 448 input: the only shapes that were measured (tools/conv_rows.py)
VGG_448 = {(64, 64, 448, 448), (64, 128, 224, 224), (128, 128, 224, 224), (128, 256, 112, 112), (256, 256, 112, 112),
           (256, 512, 56, 56), (512, 512, 56, 56), (512, 512, 28, 28)}


@pytest.fixture
def F():
    import hawkeye_amd.functional as F_
    return F_


@pytest.mark.parametrize('direction', ['fwd', 'bwd_data'])
def test_routing_tables_and_knob_semantics(F, monkeypatch, direction):
    knob_name = b'conv_' + direction.encode()
    table = F.CONV_FWD_WINS if direction == 'fwd' else F.CONV_BWD_DATA_WINS
    route = F.conv3x3_fwd_route if direction == 'fwd' else F.conv3x3_bwd_data_route
    knobs = {b'conv_fwd': -1, b'conv_bwd_data': -1}
    monkeypatch.setattr(F, '_knob', lambda name: knobs[name])
    # nothing that was not measured is in a table
    assert set(table) <= VGG_448 and all(set(b) <= {64, 16} and len(b) > 0 for b in table.values())
    shapes = sorted(VGG_448 | {(64, 64, 6, 8), (128, 64, 7, 34)})
    for (cin, cout, h, w) in shapes:
        for n in (1, 16, 32, 64):
            knobs[knob_name] = -1
            assert route(cin, cout, n, h, w) == (n in table.get((cin, cout, h, w), ()))      # default: the measured pairs only
            knobs[knob_name] = 0
            assert not route(cin, cout, n, h, w)
            knobs[knob_name] = 1
            assert route(cin, cout, n, h, w)
    # the two knobs are independent
    other = b'conv_bwd_data' if direction == 'fwd' else b'conv_fwd'
    knobs[knob_name], knobs[other] = 0, 1
    assert not route(64, 64, 64, 448, 448)


def _declared():
    src = open(os.path.join(ROOT, 'include', 'hawkeye_conv.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(hk_[a-z0-9_]+)\s*\(', src)))


def test_header_table_and_library_agree():
    from hawkeye_amd import _lib
    assert _declared() == sorted(_lib.TRUNK_SIGNATURES) == ['hk_conv3x3_bwd_data', 'hk_conv3x3_fwd', 'hk_conv3x3_ws_bytes']
    assert not set(_lib.TRUNK_SIGNATURES) & set(_lib.SIGNATURES)
    main = open(os.path.join(ROOT, 'include', 'hawkeye_hip.h')).read()
    assert '#include "hawkeye_conv.h"' in main and not any(name in main for name in _lib.TRUNK_SIGNATURES)
    # argument counts of the header against the table
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hawkeye_conv.h')).read(), flags=re.S)
    for name, (_, args) in _lib.TRUNK_SIGNATURES.items():
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', src).group(1)
        assert len(params.split(',')) == len(args), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()                                        # attach() walks both tables: a missing symbol raises here
    for name in _lib.TRUNK_SIGNATURES:
        assert hasattr(lib, name), name
    assert lib.hk_conv3x3_ws_bytes(512, 512) == 8 * 16 * 9 * 15360 and lib.hk_conv3x3_ws_bytes(0, 64) == 0
