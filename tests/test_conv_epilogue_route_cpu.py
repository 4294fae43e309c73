"""The routing of the trunk's fused units (model/backbone/vgg.py: ConvStack.forward, functional.ConvEpilogue / ConvLink, knob
`conv_epi`) without a GPU: ConvStack's own loop runs over stand-in tensors (meta tensors that say they are HIP tensors) with the
functional layer's calls recorded instead of launched; and the agreement of include/hawkeye_conv_epi.h, hawkeye_amd/_lib.py:
TRUNK_EPI_SIGNATURES and the built library."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Hip(torch.Tensor):
    """A meta tensor that passes for a 16-byte aligned HIP tensor."""
    is_cuda = property(lambda self: True)

    def data_ptr(self):
        return 0


def _map(n, c, h, w):
    return torch.empty(n, c, h, w, device='meta').contiguous(memory_format=torch.channels_last).as_subclass(_Hip)


@pytest.fixture
def route(monkeypatch):
    import hawkeye_amd.functional as F
    knobs = {b'conv_fwd': -1, b'conv_bwd_data': -1, b'conv_wrw': 1, b'wrw_split': -1, b'wrw_wide': 1, b'conv_epi': 2}
    calls = []
    monkeypatch.setattr(F, '_knob', lambda name: knobs[name])
    monkeypatch.setattr(F, '_conv3x3_served', lambda x, conv: conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0)
    monkeypatch.setattr(F, 'conv1_ok', lambda x, conv: conv.in_channels == 3)
    monkeypatch.setattr(F, 'trunk_epilogue_ok', lambda y, pool=False: not pool or (y.shape[2] % 2 == 0 and y.shape[3] % 2 == 0))
    monkeypatch.setattr(F, 'conv1_bias_relu', lambda x, w, b: (calls.append(('conv1',)), _map(x.shape[0], 64, *x.shape[2:]))[1])

    def conv3x3(x, w, fwd=False, bwd=False, wrw=True):
        e = F.ConvEpilogue.take()
        n, _, h, wd = x.shape
        if e is None:
            calls.append(('conv3x3', fwd, bwd, wrw))
            return _map(n, w.shape[0], h, wd)
        assert fwd
        if not e.pool:
            e.link.mask = 'the sign mask'
        calls.append(('unit', e.pool, e.masked, bwd, wrw))
        return _map(n, w.shape[0], h // 2, wd // 2) if e.pool else _map(n, w.shape[0], h, wd)
    monkeypatch.setattr(F, 'conv3x3', conv3x3)
    monkeypatch.setattr(F, 'bias_relu', lambda y, b: (calls.append(('bias_relu',)), y)[1])
    monkeypatch.setattr(F, 'bias_relu_pool', lambda y, b: (calls.append(('bias_relu_pool',)), _map(y.shape[0], y.shape[1], y.shape[2] // 2, y.shape[3] // 2))[1])
    return knobs, calls


@pytest.fixture(scope='module')
def vgg():
    from hawkeye_amd.model.backbone.vgg import VGG16_LAYOUT, conv_stack
    return conv_stack(VGG16_LAYOUT).to('meta')


PARENT = ([('conv1',)] + [('conv3x3', True, True, True), ('bias_relu_pool',)]                                       # conv1_1, conv1_2 + pool
          + [('conv3x3', True, True, True), ('bias_relu',), ('conv3x3', True, True, True), ('bias_relu_pool',)]     # stage 2
          + 3 * ([('conv3x3', True, True, True), ('bias_relu',)] * 2 + [('conv3x3', True, True, True), ('bias_relu_pool',)]))


@pytest.mark.parametrize('batch', [64, 16])
def test_vgg16_at_the_metric_shape_is_twelve_units_and_seven_links(route, vgg, batch):
    knobs, calls = route
    out = vgg(_map(batch, 3, 448, 448))
    assert tuple(out.shape) == (batch, 512, 14, 14)
    units = [c for c in calls if c[0] == 'unit']
    assert calls[0] == ('conv1',) and len(calls) == 13 and len(units) == 12
    assert [c[1] for c in units] == [True, False, True, False, False, True, False, False, True, False, False, True]      # 7 + 5 forwards
    # a unit takes its producer's mask along exactly where the producer was an unpooled unit: 7 links
    assert [c[2] for c in units] == [False, False, True, False, True, True, False, True, True, False, True, True]
    assert sum(c[2] for c in units) == 7 and all(c[3] and c[4] for c in units)
    del calls[:]
    knobs[b'conv_epi'] = 1                                          # the forward fusions only
    vgg(_map(batch, 3, 448, 448))
    units = [c for c in calls if c[0] == 'unit']
    assert len(units) == 12 and not any(c[2] for c in units)
    for knob, value in ((b'conv_epi', 0), (b'conv_fwd', 0)):        # the parent's calls
        del calls[:]
        knobs[b'conv_epi'], knobs[b'conv_fwd'] = 2, -1
        knobs[knob] = value
        vgg(_map(batch, 3, 448, 448))
        fwd = knob != b'conv_fwd'
        assert calls == [c if c[0] != 'conv3x3' else ('conv3x3', fwd, True, True) for c in PARENT]


def test_an_unmeasured_batch_keeps_the_parents_calls(route, vgg):
    knobs, calls = route
    vgg(_map(8, 3, 448, 448))                                       # batch 8 is in no table: the library's forward, no unit
    assert not any(c[0] == 'unit' for c in calls) and ('conv3x3', False, False, True) in calls


def test_odd_sizes_keep_the_pooled_form_off(route):
    from hawkeye_amd.model.backbone.vgg import conv_stack
    knobs, calls = route
    knobs[b'conv_fwd'] = knobs[b'conv_bwd_data'] = 1
    stack = conv_stack((64, 64, 'M', 128)).to('meta')
    for h, w, pooled in ((8, 12, True), (7, 12, False), (8, 11, False)):
        del calls[:]
        out = stack(_map(2, 3, h, w))
        assert tuple(out.shape) == (2, 128, h // 2, w // 2)
        units = [c for c in calls if c[0] == 'unit']
        # conv1_2 in front of the pool: pooled only with even H and W, otherwise the unpooled unit and nn.MaxPool2d behind it - whose output
        # carries no mask to the next unit
        assert [c[1] for c in units] == [pooled, False] and not any(c[2] for c in units), (h, w)


def test_header_table_and_library_agree():
    from hawkeye_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hawkeye_conv_epi.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(hk_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(_lib.TRUNK_EPI_SIGNATURES) and len(declared) == 4
    assert not set(_lib.TRUNK_EPI_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.TRUNK_SIGNATURES))
    assert '#include "hawkeye_conv_epi.h"' in open(os.path.join(ROOT, 'include', 'hawkeye_hip.h')).read()
    for name, (_, args) in _lib.TRUNK_EPI_SIGNATURES.items():
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', src).group(1)
        assert len(params.split(',')) == len(args), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in _lib.TRUNK_EPI_SIGNATURES:
        assert hasattr(lib, name), name
    # the split weights, then one fp64 partial row per 4 x 32 tile (and per group of 128 of them past 128)
    assert lib.hk_conv3x3_masked_ws_bytes(1, 4, 32, 64, 64) == lib.hk_conv3x3_ws_bytes(64, 64) + 64 * 8
    assert lib.hk_conv3x3_masked_ws_bytes(64, 224, 224, 128, 128) == lib.hk_conv3x3_ws_bytes(128, 128) + (25088 + 196) * 128 * 8
    assert lib.hk_conv3x3_masked_ws_bytes(0, 4, 4, 64, 64) == 0
