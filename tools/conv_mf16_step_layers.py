"""Per layer and direction, the main kernel of csrc/conv_fwd.hip in the training step on 32 x 32 x 16 everywhere (HK_CONV_MFMA=0) and by
the library's rule (the default: conv3x3_mfma16_wins), from two kernel traces of bench.py on the same build per batch size
(tools/conv_mfma_step_layers.py's table; this is what the rule rests on):

    HK_CONV_MFMA=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mf0 -- python bench.py --gpus 1 --steps 8 --warmup 3 [--batch 16]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after -- python bench.py --gpus 1 --steps 8 --warmup 3 [--batch 16]
    python tools/conv_mf16_step_layers.py --steps 8 b64 DIR/mf0_kernel_trace.csv DIR/after_kernel_trace.csv b16 ... --out profiles/conv_mf16_step_layers.json

Per row `mfma32_*` is the HK_CONV_MFMA=0 trace and `mfma16_*` the default one; `launches_on_mfma32_by_default` counts the default trace's
launches that are not conv3x3_split_kernel<*, 1, *>."""
import argparse
import json

from conv_mfma_step_layers import table

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('traces', nargs='+', help='LABEL MFMA0 DEFAULT, repeated')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert len(args.traces) % 3 == 0
    result = {'unit': 'milliseconds per launch, mean over the timed steps of each trace; mfma32 = HK_CONV_MFMA=0, mfma16 = the default (the rule)',
              'steps': args.steps}
    for i in range(0, len(args.traces), 3):
        t = table(args.traces[i + 1], args.traces[i + 2], args.steps)
        rows = list(t['forward'].values()) + list(t['input_gradient'].values())
        t['launches_on_mfma32_by_default'] = sum(1 for r in rows if ', 1, ' not in r['mfma16_kernel'])
        t['slower_in_the_step'] = [d + ' ' + n for d in ('forward', 'input_gradient') for n, r in t[d].items() if not r['faster_in_the_step']]
        result[args.traces[i]] = t
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
