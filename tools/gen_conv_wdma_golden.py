"""Writes tests/golden/conv_wdma_emu.json or tests/golden/conv_wdma_gpu.json: SHA-256 digests of every output of csrc/conv_fwd.hip's
entry points (forward, input gradient, the four epilogues of conv3x3_split_kernel) at the shapes of tests/conv_wdma_cases.py on both
MFMA shapes.

    python tools/gen_conv_wdma_golden.py emu [--out FILE] [--check]      # the CPU emulation of the kernel sources (tests/emu)
    python tools/gen_conv_wdma_golden.py gpu [--out FILE] [--check]      # the gfx950 build on the MI355X

Run on the commit whose bits are the yardstick: the committed files were recorded on the parent of the commit that moved the weight
tiles into LDS by DMA, and the tests hold that commit and every later one to them.  --check compares with the file instead of
writing it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import conv_wdma_cases as W  # noqa: E402


def record(lib, dev, stream):
    out = {}
    for shape, name in zip(W.SHAPES, W.IDS):
        out[name] = {f'mf{mf}': W.digests(lib, dev, shape, mf, stream) for mf in (0, 1)}
        print(name, {k: len(v) for k, v in out[name].items()}, flush=True)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('which', choices=['emu', 'gpu'])
    ap.add_argument('--out', default=None)
    ap.add_argument('--check', action='store_true', help='compare with the file instead of writing it')
    args = ap.parse_args()
    path = args.out or os.path.join(W.GOLDEN, f'conv_wdma_{args.which}.json')
    if args.which == 'emu':
        from emu.harness import load_emu
        got = record(load_emu(), torch.device('cpu'), None)
    else:
        from hawkeye_amd import _lib
        lib = _lib.load()
        assert b'gfx950' in lib.hk_version()
        got = record(lib, torch.device('cuda'), _lib.stream())
        torch.cuda.synchronize()
    if args.check:
        with open(path) as f:
            same = json.load(f) == got
        print('identical' if same else 'DIFFERENT', path)
        sys.exit(0 if same else 1)
    with open(path, 'w') as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {path}')
