"""Per layer and direction, the main kernel of csrc/conv_fwd.hip in the training step on either bf16 MFMA, from two kernel traces of
bench.py (the sibling of tools/conv_epi_step_layers.py):

    HK_CONV_MFMA=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o before -- python bench.py --gpus 1 --steps 8 --warmup 3
    HK_CONV_MFMA=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after  -- python bench.py --gpus 1 --steps 8 --warmup 3
    python tools/conv_mfma_step_layers.py --steps 8 b64 DIR/before_kernel_trace.csv DIR/after_kernel_trace.csv [b16 ...] --out profiles/conv_mfma_step_layers.json

A step launches the twelve 3 x 3 forwards conv1_2 ... conv5_3 and then their twelve input gradients in backward order: 24 launches of
conv3x3_split_kernel, slot by slot the same layer-direction in both traces.  Per slot the mean time over the last `--steps` steps of
each trace, in ms; and, because the weight gradient shares the chip's clock with its neighbours, the per-step sums of the
conv3x3_wrw kernels and of everything else in the same window (from the first of those launches to the end of the trace)."""
import argparse
import json

from conv_epi_step_layers import FWD, _last, _mean_by_slot, _ms, _rows


def table(before, after, steps):
    split = lambda k: 'conv3x3_split_kernel' in k
    out = {'forward': {}, 'input_gradient': {}}
    arms = {}
    for arm, path in (('mfma32', before), ('mfma16', after)):
        rows = _rows(path)
        mine = _last(rows, split, 24, steps)
        first = int(mine[0]['Start_Timestamp'])
        window = [r for r in rows if int(r['Start_Timestamp']) >= first]
        wrw = sum(_ms(r) for r in window if 'conv3x3_wrw' in r['Kernel_Name']) / steps
        rest = sum(_ms(r) for r in window if 'conv3x3_wrw' not in r['Kernel_Name'] and not split(r['Kernel_Name'])) / steps
        arms[arm] = (_mean_by_slot(mine, 24), [mine[i]['Kernel_Name'].split('conv3x3_split_kernel')[1].split('(')[0] for i in range(24)], wrw, rest)
    for slot in range(24):
        name = FWD[slot] if slot < 12 else FWD[23 - slot]
        a, b = arms['mfma32'][0][slot], arms['mfma16'][0][slot]
        out['forward' if slot < 12 else 'input_gradient'][name] = {
            'mfma32_kernel': 'conv3x3_split_kernel' + arms['mfma32'][1][slot], 'mfma32_ms': round(a, 4),
            'mfma16_kernel': 'conv3x3_split_kernel' + arms['mfma16'][1][slot], 'mfma16_ms': round(b, 4),
            'saved_ms': round(a - b, 4), 'faster_in_the_step': bool(b < a)}
    out['sums_ms_per_step'] = {
        'split_kernels_mfma32': round(sum(arms['mfma32'][0]), 3), 'split_kernels_mfma16': round(sum(arms['mfma16'][0]), 3),
        'wrw_kernels_beside_mfma32': round(arms['mfma32'][2], 3), 'wrw_kernels_beside_mfma16': round(arms['mfma16'][2], 3),
        'everything_else_beside_mfma32': round(arms['mfma32'][3], 3), 'everything_else_beside_mfma16': round(arms['mfma16'][3], 3)}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('traces', nargs='+', help='LABEL BEFORE AFTER, repeated')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert len(args.traces) % 3 == 0
    result = {'unit': 'milliseconds per launch, mean over the timed steps of each trace; before = HK_CONV_MFMA=0, after = HK_CONV_MFMA=1', 'steps': args.steps}
    for i in range(0, len(args.traces), 3):
        result[args.traces[i]] = table(args.traces[i + 1], args.traces[i + 2], args.steps)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
