"""hk_conv3x3_fwd and hk_conv3x3_bwd_data stand-alone at the trunk's twelve 3 x 3 layers with multiples of 64 channels (VGG-16 at a
448 x 448 input), batch 64 and 16, against the library: F.conv2d for the forward, torch.ops.aten.convolution_backward with the mask
(True, False, False) for the input gradient - its zero-fill of the output included, as our side includes the weight pre-pass.

Per row: two warm-up calls, then six timed calls, HIP events around the call; the six times, their min and max, and TF/s of the
useful 2 * pixels * Cout * 9 Cin FLOP at the min.  The routing rule of DESIGN 3.10: a layer-direction goes to the kernel if the
kernel's slowest repeat is faster than the library's fastest by more than three times the library's own min-max spread.  The file
is rewritten after every row.

    python tools/conv_rows.py [--out profiles/conv_split_timing.json] [--batches 64,16]

--mfma: a third arm, the kernel on the 16 x 16 x 32 bf16 MFMA (knob `conv_mfma` 1) beside the kernel on 32 x 32 x 16 (`conv_mfma` 0) and
the library, the three arms interleaved call by call (two warm-up rounds, six timed ones) on random data.  A layer-direction clears the
bar when the 32 x 32 x 16 arm's min minus the 16 x 16 x 32 arm's max exceeds three times the 32 x 32 x 16 arm's own spread.

    python tools/conv_rows.py --mfma [--out profiles/conv_mfma_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from wrw_rows import CALLS, WARMUP, row, timed, write  # noqa: E402

# side, Cin, Cout at a 448 x 448 input
LAYERS = {'conv1_2': (448, 64, 64), 'conv2_1': (224, 64, 128), 'conv2_2': (224, 128, 128), 'conv3_1': (112, 128, 256),
          'conv3_2': (112, 256, 256), 'conv3_3': (112, 256, 256), 'conv4_1': (56, 256, 512), 'conv4_2': (56, 512, 512),
          'conv4_3': (56, 512, 512), 'conv5_1': (28, 512, 512), 'conv5_2': (28, 512, 512), 'conv5_3': (28, 512, 512)}


def rows(HF, _lib, dev, result, out, batches):
    from hawkeye_amd.miopen_cache import use_in_tree_cache
    use_in_tree_cache()                                        # the library's kernels of the training step, not a fresh search
    result['unit'] = ('milliseconds per call (HIP events): `library` = F.conv2d / aten.convolution_backward (input gradient only), '
                      'zero-fills included; `split` = hk_conv3x3_fwd / hk_conv3x3_bwd_data, the weight pre-pass included')
    gen = torch.Generator(device=dev).manual_seed(37)
    for batch in batches:
        for name, (side, cin, cout) in LAYERS.items():
            x = torch.empty(batch, cin, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen).relu_()
            dy = torch.empty(batch, cout, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            wt = torch.empty(cout, cin, 3, 3, device=dev).normal_(0.0, 0.05, generator=gen).contiguous(memory_format=torch.channels_last)
            flop = 2.0 * batch * side * side * cout * 9 * cin
            sides = {
                'fwd': (x, lambda a, w: torch.nn.functional.conv2d(a, w, None, 1, 1), HF.conv3x3_fwd_raw),
                'bwd_data': (dy, lambda a, w: torch.ops.aten.convolution_backward(a, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                                                   (True, False, False))[0], HF.conv3x3_bwd_data_raw),
            }
            with _lib.tuning(conv_fwd=1, conv_bwd_data=1):
                for direction, (src, library, ours) in sides.items():
                    r = {'library': row(timed(HF, src, wt, library), flop), 'split': row(timed(HF, src, wt, ours), flop)}
                    a, b = library(src, wt).double(), ours(src, wt).double()
                    r['rel_difference_split_vs_library'] = float((a - b).norm() / a.norm())
                    key = f'{name}_{direction}_b{batch}'
                    result['rows'][key] = r
                    lib, spl = r['library'], r['split']
                    spread = lib['max'] - lib['min']
                    result['routing'][key] = {'library_min': lib['min'], 'library_spread': round(spread, 4), 'split_max': spl['max'],
                                              'gain_ms': round(lib['min'] - spl['max'], 4),
                                              'to_kernel': bool(lib['min'] - spl['max'] > 3 * spread)}
                    print(key, result['routing'][key], 'TF/s', lib['tflops_at_min'], spl['tflops_at_min'], flush=True)
                    write(result, out)                         # (after every row: a run cut short leaves what it measured)
                    del a, b
            del x, dy, wt, sides
            torch.cuda.empty_cache()


def interleaved(arms, src, wt):
    """arms: name -> call; one call of every arm per round, WARMUP rounds untimed, then CALLS timed ones -> name -> milliseconds."""
    ms = {name: [] for name in arms}
    for r in range(WARMUP + CALLS):
        for name, call in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call(src, wt)
            t1.record()
            t1.synchronize()
            if r >= WARMUP:
                ms[name].append(t0.elapsed_time(t1))
    return ms


def mfma_rows(HF, _lib, dev, result, out, batches):
    from hawkeye_amd.miopen_cache import use_in_tree_cache
    use_in_tree_cache()
    result['unit'] = ('milliseconds per call (HIP events), the arms interleaved call by call: `library` as in conv_split_timing.json; `mfma32` / '
                      '`mfma16` = hk_conv3x3_fwd / hk_conv3x3_bwd_data with `conv_mfma` 0 / 1, the weight pre-pass included')
    gen = torch.Generator(device=dev).manual_seed(37)

    def knob(v, fn):
        def call(a, w):
            with _lib.tuning(conv_mfma=v):
                return fn(a, w)
        return call
    for batch in batches:
        for name, (side, cin, cout) in LAYERS.items():
            x = torch.empty(batch, cin, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen).relu_()
            dy = torch.empty(batch, cout, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            wt = torch.empty(cout, cin, 3, 3, device=dev).normal_(0.0, 0.05, generator=gen).contiguous(memory_format=torch.channels_last)
            flop = 2.0 * batch * side * side * cout * 9 * cin
            sides = {
                'fwd': (x, lambda a, w: torch.nn.functional.conv2d(a, w, None, 1, 1), HF.conv3x3_fwd_raw),
                'bwd_data': (dy, lambda a, w: torch.ops.aten.convolution_backward(a, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                                                   (True, False, False))[0], HF.conv3x3_bwd_data_raw),
            }
            with _lib.tuning(conv_fwd=1, conv_bwd_data=1):
                for direction, (src, library, ours) in sides.items():
                    ms = interleaved({'library': library, 'mfma32': knob(0, ours), 'mfma16': knob(1, ours)}, src, wt)
                    r = {arm: row(v, flop) for arm, v in ms.items()}
                    a, b = knob(0, ours)(src, wt).double(), knob(1, ours)(src, wt).double()
                    r['rel_difference_mfma16_vs_mfma32'] = float((a - b).norm() / a.norm())
                    key = f'{name}_{direction}_b{batch}'
                    result['rows'][key] = r
                    old, new = r['mfma32'], r['mfma16']
                    spread = old['max'] - old['min']
                    result['routing'][key] = {'mfma32_min': old['min'], 'mfma32_spread': round(spread, 4), 'mfma16_max': new['max'],
                                              'gain_ms': round(old['min'] - new['max'], 4),
                                              'clears_the_bar': bool(old['min'] - new['max'] > 3 * spread)}
                    print(key, result['routing'][key], 'TF/s', old['tflops_at_min'], new['tflops_at_min'], flush=True)
                    write(result, out)
                    del a, b
            del x, dy, wt, sides
            torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--mfma', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--batches', default='64,16')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('conv_rows needs an MI355X: nothing is measured without one')
        sys.exit(2)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    import hawkeye_amd.functional as HF
    from hawkeye_amd import _lib
    result = {'device': torch.cuda.get_device_name(0), 'warmup_calls': 2, 'timed_calls': 6, 'rows': {}, 'routing': {}}
    (mfma_rows if args.mfma else rows)(HF, _lib, dev, result, args.out, [int(b) for b in args.batches.split(',')])
    write(result, args.out)
