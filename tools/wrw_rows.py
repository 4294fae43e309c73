"""hk_conv3x3_wrw stand-alone at the trunk's two 64-input-channel layers (conv1_2: 64 -> 64 at 448 x 448, conv2_1: 64 -> 128 at
224 x 224), batch 64 and 16, the fp32-MFMA kernel (knob wrw_split 0) against the three-way split bf16-MFMA kernel (1), each at
two workgroups per CU (knob wrw_wgs 0: 512 workgroups over all Cout slices) and at one (256 over all slices).

Per row: two warm-up calls, then six timed calls, HIP events around the entry point (the main kernel + partial_sum_kernel); the
six times, their min and max, and TF/s of the useful 2 * pixels * Cout * 576 FLOP at the min.  The routing rule of DESIGN 3.10 is
applied to the default (two per CU) rows: a layer goes to the split kernel if its slowest repeat is faster than the fp32 kernel's
fastest by more than three times the fp32 kernel's own min-max spread.  Writes the rows as json.

    python tools/wrw_rows.py [--out profiles/wrw_split_timing.json]

--set wide: the trunk's ten layers with more than 64 input channels at batch 64 and 16, hk_conv3x3_wrw (the split form on 64-channel
slices of x) against the library's weight gradient (torch.ops.aten.convolution_backward, mask (False, True, False)), same calls
and the same bar: a layer is routed if the kernel's slowest repeat is faster than the library's fastest by more than three times
the library's own min-max spread.  The file is rewritten after every row.

    python tools/wrw_rows.py --set wide [--out profiles/wrw_wide_timing.json]

--set mfma: all twelve layers at batch 64 and 16, the split form on v_mfma_f32_32x32x16_bf16 (knob wrw_mfma 0) against the same kernel
on v_mfma_f32_16x16x32_bf16 (1), same calls.  For the record only: the rule behind the knob's default (conv_wrw.hip:
wrw_mfma16_wins) was decided by the layers' times inside the training step (profiles/wrw_mfma_step_layers.json).

    python tools/wrw_rows.py --set mfma [--out profiles/wrw_mfma_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

LAYERS = {'conv1_2': (448, 64), 'conv2_1': (224, 128)}       # side, Cout
# side, Cin, Cout at a 448 x 448 input
WIDE_LAYERS = {'conv2_2': (224, 128, 128), 'conv3_1': (112, 128, 256), 'conv3_2': (112, 256, 256), 'conv3_3': (112, 256, 256),
               'conv4_1': (56, 256, 512), 'conv4_2': (56, 512, 512), 'conv4_3': (56, 512, 512), 'conv5_1': (28, 512, 512),
               'conv5_2': (28, 512, 512), 'conv5_3': (28, 512, 512)}
WARMUP, CALLS = 2, 6


def timed(HF, x, dy, call=None):
    call = call or HF.conv3x3_wrw_raw
    for _ in range(WARMUP):
        call(x, dy)
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call(x, dy)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def row(ms, flop):
    return {'ms': [round(m, 4) for m in ms], 'min': round(min(ms), 4), 'max': round(max(ms), 4),
            'tflops_at_min': round(flop / (min(ms) * 1e-3) / 1e12, 1)}


def write(result, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')


def split_rows(HF, _lib, dev, result):
    """The two 64-input-channel layers: fp32 form against split form, two and one workgroup per CU."""
    result['unit'] = 'milliseconds per call of hk_conv3x3_wrw (HIP events around the entry point)'
    gen = torch.Generator(device=dev).manual_seed(29)
    for name, (side, cout) in LAYERS.items():
        for batch in (64, 16):
            x = torch.empty(batch, 64, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            dy = torch.empty(batch, cout, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            HF.conv3x3_wrw_raw(x[:1], dy[:1])                  # (the workspace is allocated outside the timed calls)
            flop = 2.0 * batch * side * side * cout * 576
            rows = {}
            for split in (0, 1):
                for per_cu, wgs in ((2, 0), (1, 256 // (cout // 64))):
                    with _lib.tuning(wrw_split=split, wrw_wgs=wgs):
                        rows[f'split{split}_wg_per_cu{per_cu}'] = row(timed(HF, x, dy), flop)
            with _lib.tuning(wrw_split=0):
                a = HF.conv3x3_wrw_raw(x, dy).double()
            with _lib.tuning(wrw_split=1):
                b = HF.conv3x3_wrw_raw(x, dy).double()
            rows['rel_difference_split_vs_fp32'] = float((a - b).norm() / a.norm())
            key = f'{name}_b{batch}'
            result['rows'][key] = rows
            f32, spl = rows['split0_wg_per_cu2'], rows['split1_wg_per_cu2']
            spread = f32['max'] - f32['min']
            result['routing'][key] = {'fp32_min': f32['min'], 'fp32_spread': round(spread, 4), 'split_max': spl['max'],
                                      'gain_ms': round(f32['min'] - spl['max'], 4), 'to_split': bool(f32['min'] - spl['max'] > 3 * spread)}
            del x, dy
            torch.cuda.empty_cache()


def wide_rows(HF, dev, result, out):
    """The ten layers with more than 64 input channels: the library's weight gradient against hk_conv3x3_wrw."""
    from hawkeye_amd.miopen_cache import use_in_tree_cache
    use_in_tree_cache()                                        # the library's kernels of the training step, not a fresh search
    result['unit'] = ('milliseconds per call (HIP events): `library` = torch.ops.aten.convolution_backward, weight gradient only '
                      '(its zero-fill included), `split` = hk_conv3x3_wrw (the main kernel + partial_sum_kernel)')
    gen = torch.Generator(device=dev).manual_seed(31)
    for batch in (64, 16):
        for name, (side, cin, cout) in WIDE_LAYERS.items():
            x = torch.empty(batch, cin, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            dy = torch.empty(batch, cout, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            wt = torch.empty(cout, cin, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
            library = lambda a, b: torch.ops.aten.convolution_backward(b, a, wt, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                                        (False, True, False))[1]
            HF.conv3x3_wrw_raw(x[:1], dy[:1])                  # (the workspace is allocated outside the timed calls)
            flop = 2.0 * batch * side * side * cout * 9 * cin
            rows = {'library': row(timed(HF, x, dy, library), flop), 'split': row(timed(HF, x, dy), flop)}
            a, b = library(x, dy).double(), HF.conv3x3_wrw_raw(x, dy).double()
            rows['rel_difference_split_vs_library'] = float((a - b).norm() / a.norm())
            key = f'{name}_b{batch}'
            result['rows'][key] = rows
            lib, spl = rows['library'], rows['split']
            spread = lib['max'] - lib['min']
            result['routing'][key] = {'library_min': lib['min'], 'library_spread': round(spread, 4), 'split_max': spl['max'],
                                      'gain_ms': round(lib['min'] - spl['max'], 4), 'to_kernel': bool(lib['min'] - spl['max'] > 3 * spread)}
            print(key, result['routing'][key], flush=True)
            write(result, out)                                 # (after every row: a run cut short leaves what it measured)
            del x, dy, wt, a, b
            torch.cuda.empty_cache()


def mfma_rows(HF, _lib, dev, result, out):
    """All twelve layers: the split form on either bf16 MFMA."""
    result['unit'] = ('milliseconds per call of hk_conv3x3_wrw (HIP events around the entry point), knob wrw_split 1: `mfma32` = wrw_mfma 0, '
                      '`mfma16` = wrw_mfma 1')
    gen = torch.Generator(device=dev).manual_seed(37)
    layers = {**{k: (s, 64, c) for k, (s, c) in LAYERS.items()}, **WIDE_LAYERS}
    for batch in (64, 16):
        for name, (side, cin, cout) in layers.items():
            x = torch.empty(batch, cin, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            dy = torch.empty(batch, cout, side, side, device=dev, memory_format=torch.channels_last).normal_(0.0, 1.0, generator=gen)
            flop = 2.0 * batch * side * side * cout * 9 * cin
            rows, dw = {}, {}
            for key, v in (('mfma32', 0), ('mfma16', 1)):
                with _lib.tuning(wrw_split=1, wrw_mfma=v):
                    HF.conv3x3_wrw_raw(x[:1], dy[:1])          # (the workspace is allocated outside the timed calls)
                    rows[key] = row(timed(HF, x, dy), flop)
                    dw[key] = HF.conv3x3_wrw_raw(x, dy).double()
            rows['rel_difference_mfma16_vs_mfma32'] = float((dw['mfma16'] - dw['mfma32']).norm() / dw['mfma32'].norm())
            key = f'{name}_b{batch}'
            result['rows'][key] = rows
            m32, m16 = rows['mfma32'], rows['mfma16']
            result['routing'][key] = {'mfma32_min': m32['min'], 'mfma32_spread': round(m32['max'] - m32['min'], 4), 'mfma16_max': m16['max'],
                                      'gain_ms': round(m32['min'] - m16['max'], 4), 'min_ratio': round(m16['min'] / m32['min'], 4)}
            print(key, result['routing'][key], flush=True)
            write(result, out)
            del x, dy, dw
            torch.cuda.empty_cache()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--set', default='split', choices=['split', 'wide', 'mfma'])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('wrw_rows needs an MI355X: nothing is measured without one')
        sys.exit(2)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    import hawkeye_amd.functional as HF
    from hawkeye_amd import _lib
    result = {'device': torch.cuda.get_device_name(0), 'warmup_calls': WARMUP, 'timed_calls': CALLS, 'rows': {}, 'routing': {}}
    if args.set == 'wide':
        wide_rows(HF, dev, result, args.out)
    elif args.set == 'mfma':
        mfma_rows(HF, _lib, dev, result, args.out)
    else:
        split_rows(HF, _lib, dev, result)
    print(json.dumps(result, indent=1))
    write(result, args.out)
