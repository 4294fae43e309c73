"""Per-layer weight-gradient times of the VGG-16 trunk inside the training step, from a kernel trace of bench.py:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --gpus 1 --steps 8 --warmup 3
    python tools/wrw_step_layers.py --steps 8 NAME=DIR/NAME_kernel_trace.csv [NAME2=...] --out profiles/wrw_wide_step_layers.json

A step launches twelve 3 x 3 weight gradients besides the first layer's, in backward order (conv5_3 ... conv1_2): the library's
`igemm_wrw_*` kernel or hk::conv3x3_wrw_*kernel (the main kernel alone: not the library's zero-fill in front of it, not
partial_sum_kernel behind ours).  Only the last `--steps` steps of the trace count - the timed ones; warm-up steps and whatever a
kernel search of the library launched before them are left out.  Per layer: which kernel ran, its grid, mean / min / max in ms."""
import argparse
import csv
import json

LAYERS = ['conv5_3', 'conv5_2', 'conv5_1', 'conv4_3', 'conv4_2', 'conv4_1', 'conv3_3', 'conv3_2', 'conv3_1', 'conv2_2', 'conv2_1', 'conv1_2']


def layers(path, steps):
    rows = [r for r in csv.DictReader(open(path)) if 'igemm_wrw' in r['Kernel_Name'] or 'conv3x3_wrw' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    rows = rows[-steps * len(LAYERS):]
    assert len(rows) == steps * len(LAYERS), (path, len(rows))
    out = {}
    for i, name in enumerate(LAYERS):
        mine = rows[i::len(LAYERS)]
        kinds = {'library' if 'igemm_wrw' in r['Kernel_Name'] else 'hk_conv3x3_wrw' for r in mine}
        grids = {(r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z']) for r in mine}
        assert len(kinds) == 1 and len(grids) == 1, (path, name, kinds, grids)      # the same kernel at the same place in every step
        ms = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6 for r in mine]
        out[name] = {'kernel': kinds.pop(), 'grid_threads': [int(g) for g in grids.pop()], 'launches': len(ms),
                     'mean_ms': round(sum(ms) / len(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}
    out['sum_of_means_ms'] = {k: round(sum(v['mean_ms'] for v in out.values() if v['kernel'] == k), 3) for k in ('library', 'hk_conv3x3_wrw')}
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
