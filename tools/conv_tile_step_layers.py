"""Per layer and direction, the main kernel of csrc/conv_fwd.hip in the training step with 4 x 32 tiles everywhere (HK_CONV_TILE=0) and
with the planned tile geometries (the default), from two kernel traces of bench.py on the same build with the same routing
(tools/conv_mfma_step_layers.py's table under other names):

    HK_CONV_TILE=0 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o before -- python bench.py --gpus 1 --steps 8 --warmup 3
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after -- python bench.py --gpus 1 --steps 8 --warmup 3
    python tools/conv_tile_step_layers.py --steps 8 DIR/before_kernel_trace.csv DIR/after_kernel_trace.csv --out profiles/conv_tile_step_layers.json"""
import argparse
import json

from conv_mfma_step_layers import table

NAMES = (('mfma32', 'tile_4x32'), ('mfma16', 'planned'))


def renamed(o):
    if isinstance(o, dict):
        out = {}
        for k, v in o.items():
            for old, new in NAMES:
                k = k.replace(old, new)
            out[k] = renamed(v)
        return out
    return o


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('before')
    ap.add_argument('after')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    result = {'unit': 'milliseconds per launch, mean over the timed steps of each trace; tile_4x32 = HK_CONV_TILE=0, planned = the default',
              'steps': args.steps}
    result.update(renamed(table(args.before, args.after, args.steps)))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
