"""Per layer, the weight-gradient kernel of csrc/conv_wrw.hip inside the training step with the pooled form off (HK_WRW_POOL=0: every
layer on conv3x3_wrw_split_kernel / conv3x3_wrw_kernel) and by the library's rule (the default), from two kernel traces of bench.py on
the same build per batch size - what wrw_pool_wins rests on:

    HK_WRW_POOL=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o before -- python bench.py --gpus 1 --steps 8 --warmup 3 [--batch 16]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after -- python bench.py --gpus 1 --steps 8 --warmup 3 [--batch 16]
    python tools/wrw_pool_step_layers.py b64 DIR/before_kernel_trace.csv DIR/after_kernel_trace.csv b16 ... --out profiles/wrw_pool_step_layers.json

The backward pass launches the twelve routed layers' weight gradients from conv5_3 down to conv1_2; launch k of a step is layer
LAYERS[k].  The warm-up steps are dropped."""
import argparse
import csv
import json

LAYERS = ['conv5_3', 'conv5_2', 'conv5_1', 'conv4_3', 'conv4_2', 'conv4_1', 'conv3_3', 'conv3_2', 'conv3_1', 'conv2_2', 'conv2_1', 'conv1_2']
POOLED = ('conv5_3', 'conv4_3', 'conv3_3', 'conv2_2', 'conv1_2')


def per_layer(path, steps):
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if 'conv3x3_wrw' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    assert len(rows) % 12 == 0 and len(rows) // 12 >= steps, (path, len(rows))
    rows = rows[-12 * steps:]
    out = {}
    for k, name in enumerate(LAYERS):
        mine = rows[k::12]
        ms = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6 for r in mine]
        kernels = sorted(set(r['Kernel_Name'].split('(')[0].replace('void ', '') for r in mine))
        assert len(kernels) == 1, (name, kernels)
        out[name] = {'ms': round(sum(ms) / len(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'kernel': kernels[0]}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('traces', nargs='+', help='LABEL BEFORE AFTER, repeated')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert len(a.traces) % 3 == 0
    result = {'unit': 'milliseconds per launch, mean (min, max) over the timed steps of each trace; dense = HK_WRW_POOL=0, rule = the default',
              'steps': a.steps}
    for i in range(0, len(a.traces), 3):
        before, after = per_layer(a.traces[i + 1], a.steps), per_layer(a.traces[i + 2], a.steps)
        t = {'layers': {}}
        for name in LAYERS:
            b, r = before[name], after[name]
            row = {'dense_ms': b['ms'], 'dense_range': [b['min_ms'], b['max_ms']], 'rule_ms': r['ms'], 'rule_range': [r['min_ms'], r['max_ms']],
                   'rule_kernel': r['kernel'], 'pooled_layer': name in POOLED}
            if 'pooled' in r['kernel']:
                row['faster_in_the_step'] = r['max_ms'] < b['min_ms']
            t['layers'][name] = row
        t['twelve_layers_dense_ms'] = round(sum(before[n]['ms'] for n in LAYERS), 3)
        t['twelve_layers_rule_ms'] = round(sum(after[n]['ms'] for n in LAYERS), 3)
        t['pooled_layers_dense_ms'] = round(sum(before[n]['ms'] for n in POOLED), 3)
        t['pooled_layers_rule_ms'] = round(sum(after[n]['ms'] for n in POOLED), 3)
        t['sent_to_the_pooled_form_and_not_faster'] = [n for n, r in t['layers'].items() if r.get('faster_in_the_step') is False]
        result[a.traces[i]] = t
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')
