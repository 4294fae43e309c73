"""Stand-alone times of the pooled layers' weight gradient: hk_conv3x3_wrw on the full-resolution gradient g (the split form on the
16 x 16 x 32 MFMA) against hk_conv3x3_wrw_pooled on (dp, p, codes) (the 2:4 sparse MFMA), the five pooled layers of VGG-16 at 448 x 448
at batch 64 and 16.  HIP events around single calls, the two arms interleaved, after a warm-up; g is made by hk_bias_relu_pool_bwd.
    python tools/wrw_pool_rows.py [--reps 7] [--batches 64,16] [--out profiles/wrw_pool_rows.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hawkeye_amd import _lib  # noqa: E402

LAYERS = [('conv1_2', 448, 64, 64), ('conv2_2', 224, 128, 128), ('conv3_3', 112, 256, 256), ('conv4_3', 56, 512, 512), ('conv5_3', 28, 512, 512)]


def p_(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batches', default='64,16')
    ap.add_argument('--layers', default=','.join(l[0] for l in LAYERS))
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device('cuda')
    st = _lib.stream()
    rows = []
    for n in [int(b) for b in a.batches.split(',')]:
        for name, hw, cin, cout in LAYERS:
            if name not in a.layers.split(','):
                continue
            g_ = torch.Generator(device='cpu').manual_seed(hw + n)
            ho = hw // 2
            x = torch.randn(n * hw * hw * cin, device=dev)
            dp = torch.randn(n * ho * ho * cout, device=dev)
            p = torch.randn(n * ho * ho * cout, device=dev).clamp_min_(0.0)
            am = torch.randint(0, 256, (n * ho * ho * cout // 4,), generator=g_, dtype=torch.uint8).to(dev)
            g = torch.empty(n * hw * hw * cout, device=dev)
            db = torch.empty(cout, device=dev)
            tws = torch.empty(lib.hk_trunk_ws_bytes(cout), dtype=torch.uint8, device=dev)
            _lib.check(lib.hk_bias_relu_pool_bwd(p_(dp), p_(p), p_(am), p_(g), p_(db), n, hw, hw, cout, p_(tws), tws.numel(), st), 'pool_bwd')
            nws = lib.hk_conv3x3_wrw_ws_bytes(cin, cout)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            dw = [torch.empty(cout * 9 * cin, device=dev) for _ in range(2)]

            def dense():
                _lib.check(lib.hk_conv3x3_wrw(p_(g), p_(x), p_(dw[0]), n, hw, hw, cin, cout, p_(ws), nws, st), 'hk_conv3x3_wrw')

            def pooled():
                _lib.check(lib.hk_conv3x3_wrw_pooled(p_(dp), p_(p), p_(am), p_(x), p_(dw[1]), n, hw, hw, cin, cout, p_(ws), nws, st), 'hk_conv3x3_wrw_pooled')

            for f in (dense, pooled, dense, pooled):
                f()
            torch.cuda.synchronize()
            t = {'dense': [], 'pooled': []}
            for _ in range(a.reps):
                for key, f in (('dense', dense), ('pooled', pooled)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    t[key].append(e0.elapsed_time(e1))
            diff = float((dw[0] - dw[1]).abs().max()) / max(float(dw[0].abs().max()), 1e-30)
            row = {'layer': name, 'batch': n, 'dense_ms': sorted(t['dense']), 'pooled_ms': sorted(t['pooled']),
                   'ratio_of_medians': sorted(t['pooled'])[a.reps // 2] / sorted(t['dense'])[a.reps // 2], 'max_abs_diff_over_max_abs': diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, dp, p, am, g, ws, dw
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'what': 'hk_conv3x3_wrw on g against hk_conv3x3_wrw_pooled, stand-alone, HIP events, ms', 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
