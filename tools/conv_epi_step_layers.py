"""Per layer, what the epilogues inside conv3x3_split_kernel (csrc/conv_fwd.hip, EPI) cost in the training step beside what they
removed, from two kernel traces of bench.py (the sibling of tools/conv_step_layers.py):

    HK_CONV_EPI=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o before -- python bench.py --gpus 1 --steps 8 --warmup 3
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after  -- python bench.py --gpus 1 --steps 8 --warmup 3
    python tools/conv_epi_step_layers.py --steps 8 DIR/before_kernel_trace.csv DIR/after_kernel_trace.csv --out profiles/conv_epi_step_layers.json

A step launches the twelve 3 x 3 forwards conv1_2 ... conv5_3 and then their twelve input gradients in backward order.  Before, each
forward is followed by bias_relu_fwd_kernel<true> (the seven layers not in front of a pool) or bias_relu_pool_fwd_kernel (the five
others), and the input gradient of layer L + 1 by bias_relu_bwd_kernel<true> + trunk_db_final_kernel of layer L.  After, the forward
is conv3x3_split_kernel<1> or <2>, and the input gradient of a layer whose producer was an unpooled unit is conv3x3_split_kernel<3>
followed by one or two conv3x3_colsum_kernel launches.  Per layer and direction: the mean time of the pair before and of the fused
form after, in ms, over the last `--steps` steps of each trace.  (trunk_db_final_kernel also ends the pooled layers' backward pass,
which does not change: it is left out on both sides.)"""
import argparse
import csv
import json

FWD = ['conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3']
POOLED = {'conv1_2', 'conv2_2', 'conv3_3', 'conv4_3', 'conv5_3'}
UNPOOLED = [n for n in FWD if n not in POOLED]
# the input gradient of layer L + 1 that carries the mask of (unpooled) layer L
CONSUMER = {FWD[i]: FWD[i + 1] for i in range(len(FWD) - 1) if FWD[i] not in POOLED}


def _rows(path):
    rows = [r for r in csv.DictReader(open(path))]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return rows


def _ms(r):
    return (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6


def _last(rows, match, per_step, steps):
    mine = [r for r in rows if match(r['Kernel_Name'])]
    assert len(mine) >= per_step * steps, (len(mine), per_step, steps)
    return mine[-per_step * steps:] if per_step else []


def _mean_by_slot(rows, per_step):
    return [sum(_ms(r) for r in rows[i::per_step]) / max(len(rows[i::per_step]), 1) for i in range(per_step)]


def table(before, after, steps):
    b, a = _rows(before), _rows(after)
    split = lambda k: 'conv3x3_split_kernel' in k
    # before: 24 main-kernel launches a step, 7 + 5 forward epilogues, 7 ReLU backward passes
    b_main = _mean_by_slot(_last(b, split, 24, steps), 24)
    b_relu = _mean_by_slot(_last(b, lambda k: 'bias_relu_fwd_kernel' in k, 7, steps), 7)
    b_pool = _mean_by_slot(_last(b, lambda k: 'bias_relu_pool_fwd_kernel' in k, 5, steps), 5)
    b_bwd = _mean_by_slot(_last(b, lambda k: 'bias_relu_bwd_kernel' in k, 7, steps), 7)
    a_rows = _last(a, split, 24, steps)
    a_main = _mean_by_slot(a_rows, 24)
    a_kind = [a_rows[i]['Kernel_Name'].split('conv3x3_split_kernel')[1][:3] for i in range(24)]
    # after: the reduction launches belong to the masked input gradient they follow
    first = int(a_rows[0]['Start_Timestamp'])
    red, slot = [0.0] * 24, -1
    for r in a:
        if int(r['Start_Timestamp']) < first:
            continue
        if split(r['Kernel_Name']):
            slot = (slot + 1) % 24
        elif 'conv3x3_colsum_kernel' in r['Kernel_Name']:
            red[slot] += _ms(r) / steps
    a_left = {k: len([r for r in a if k in r['Kernel_Name']]) for k in ('bias_relu_fwd_kernel', 'bias_relu_pool_fwd_kernel', 'bias_relu_bwd_kernel')}
    out = {'forward': {}, 'input_gradient': {}, 'rows_left_after': a_left}
    relu_i = pool_i = 0
    for i, name in enumerate(FWD):
        if name in POOLED:
            epi, pool_i = b_pool[pool_i], pool_i + 1
        else:
            epi, relu_i = b_relu[relu_i], relu_i + 1
        out['forward'][name] = {'before_conv_ms': round(b_main[i], 4), 'before_epilogue_ms': round(epi, 4), 'before_ms': round(b_main[i] + epi, 4),
                                'after_kernel': 'conv3x3_split_kernel' + a_kind[i], 'after_ms': round(a_main[i], 4),
                                'saved_ms': round(b_main[i] + epi - a_main[i], 4)}
    # backward order: slot 12 + j is the input gradient of FWD[11 - j]; the ReLU backward passes run for the unpooled layers in reverse
    rev_unpooled = list(reversed(UNPOOLED))
    for j in range(12):
        name = FWD[11 - j]
        producer = next((p for p, c in CONSUMER.items() if c == name), None)
        row = {'before_conv_ms': round(b_main[12 + j], 4), 'after_kernel': 'conv3x3_split_kernel' + a_kind[12 + j], 'after_conv_ms': round(a_main[12 + j], 4)}
        if producer is not None:
            row['mask_of'] = producer
            row['before_relu_bwd_ms'] = round(b_bwd[rev_unpooled.index(producer)], 4)
            row['before_ms'] = round(row['before_conv_ms'] + row['before_relu_bwd_ms'], 4)
            masked = a_kind[12 + j] == '<3>'
            row['after_reduction_ms'] = round(red[12 + j], 4)
            row['after_ms'] = round(row['after_conv_ms'] + red[12 + j] + (0.0 if masked else row['before_relu_bwd_ms']), 4)
            row['saved_ms'] = round(row['before_ms'] - row['after_ms'], 4)
        out['input_gradient'][name] = row
    f, g = out['forward'].values(), [r for r in out['input_gradient'].values() if 'saved_ms' in r]
    out['sums_ms'] = {'forward_before': round(sum(r['before_ms'] for r in f), 3), 'forward_after': round(sum(r['after_ms'] for r in f), 3),
                      'input_gradient_with_mask_before': round(sum(r['before_ms'] for r in g), 3),
                      'input_gradient_with_mask_after': round(sum(r['after_ms'] for r in g), 3)}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('before')
    ap.add_argument('after')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'unit': 'milliseconds per launch, mean over the timed steps of each trace', 'steps': args.steps}
    result.update(table(args.before, args.after, args.steps))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
