"""Per layer and direction, the main kernel of csrc/conv_fwd.hip in the training step with its weight tiles staged through registers
(the parent commit's build) and by LDS-DMA, from two kernel traces of bench.py with the same routing (tools/conv_mfma_step_layers.py's
table under other names):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o before -- python bench.py --gpus 1 --steps 8 --warmup 3      # parent build
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o after  -- python bench.py --gpus 1 --steps 8 --warmup 3      # this build
    python tools/conv_wdma_step_layers.py --steps 8 DIR/before_kernel_trace.csv DIR/after_kernel_trace.csv --out profiles/conv_wdma_step_layers.json"""
import argparse
import json

from conv_mfma_step_layers import table

NAMES = (('mfma32', 'registers'), ('mfma16', 'lds_dma'))


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
    result = {'unit': 'milliseconds per launch, mean over the timed steps of each trace; registers = the parent build, lds_dma = this one',
              'steps': args.steps}
    result.update(renamed(table(args.before, args.after, args.steps)))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
