"""Per-layer forward and input-gradient times of the VGG-16 trunk inside the training step, from a kernel trace of bench.py (the
sibling of tools/wrw_step_layers.py):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 8 --warmup 3
    python tools/conv_step_layers.py --steps 8 NAME=DIR/NAME_kernel_trace.csv [NAME2=...] --out profiles/conv_split_step_layers.json

A step launches twelve 3 x 3 forwards besides the first layer's (conv1_2 ... conv5_3) and then their twelve input gradients in
backward order: the library's `igemm_fwd_*` / `igemm_bwd_*` kernel or hk::conv3x3_split_kernel, which serves both directions (the
main kernel alone: not the library's zero-fill in front of its kernel, not conv3x3_wsplit_kernel in front of ours).  Only the last
`--steps` steps of the trace count.  Per layer and direction: which kernel ran, mean / min / max in ms."""
import argparse
import csv
import json

FWD = ['conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3']
SLOTS = [(n, 'fwd') for n in FWD] + [(n, 'bwd_data') for n in reversed(FWD)]


def layers(path, steps):
    rows = [r for r in csv.DictReader(open(path))
            if 'igemm_fwd' in r['Kernel_Name'] or 'igemm_bwd' in r['Kernel_Name'] or 'conv3x3_split_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    rows = rows[-steps * len(SLOTS):]
    assert len(rows) == steps * len(SLOTS), (path, len(rows))
    out = {}
    for i, (name, direction) in enumerate(SLOTS):
        mine = rows[i::len(SLOTS)]
        kinds = {'hk_conv3x3' if 'conv3x3_split_kernel' in r['Kernel_Name'] else 'library' for r in mine}
        assert len(kinds) == 1, (path, name, direction, kinds)            # the same kernel at the same place in every step
        if 'library' in kinds:
            assert all(('igemm_fwd' in r['Kernel_Name']) == (direction == 'fwd') for r in mine), (path, name, direction)
        ms = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6 for r in mine]
        out[f'{name}_{direction}'] = {'kernel': kinds.pop(), 'launches': len(ms), 'mean_ms': round(sum(ms) / len(ms), 4),
                                      'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}
    sums = {}
    for direction in ('fwd', 'bwd_data'):
        for k in ('library', 'hk_conv3x3'):
            sums[f'{direction}_{k}'] = round(sum(v['mean_ms'] for n, v in out.items() if n.endswith('_' + direction) and v['kernel'] == k), 3)
    out['sum_of_means_ms'] = sums
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('traces', nargs='+', help='NAME=path of a *_kernel_trace.csv')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'unit': 'milliseconds per launch, the timed steps of the trace only', 'steps': args.steps, 'traces': {}}
    for t in args.traces:
        name, path = t.split('=', 1)
        result['traces'][name] = layers(path, args.steps)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
