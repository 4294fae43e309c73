"""Writes tests/golden/wrw_mfma_emu.json or tests/golden/wrw_mfma_gpu.json: SHA-256 digests of hk_conv3x3_wrw's split form on the
32 x 32 x 16 bf16 MFMA (knob `wrw_mfma` 0) at the cases and 'randn' inputs of tests/wrw_mfma_cases.py.

    python tools/gen_wrw_mfma_golden.py emu [--out FILE] [--check]      # the CPU emulation of the kernel sources (tests/emu)
    python tools/gen_wrw_mfma_golden.py gpu [--out FILE] [--check]      # the gfx950 build on the MI355X

Run on the commit whose bits are the yardstick: the committed files were recorded on the parent of the commit that gave the kernel
its second MFMA shape - a build without the knob, whose only split kernel is what `wrw_mfma` 0 selects since - and the tests hold that
commit and every later one to them.  --check compares with the file instead of writing it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import wrw_mfma_cases as C  # noqa: E402


def record(lib, dev, stream):
    out = {}
    for (shape, wgs), name in zip(C.CASES, C.IDS):
        x, dy, _, _ = C.case(shape, 'randn')
        out[name] = C.digest(C.run(lib, dev, x, dy, 0, wgs, stream, optional=('wrw_mfma',)))
        print(name, out[name][:16], flush=True)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('which', choices=['emu', 'gpu'])
    ap.add_argument('--out', default=None)
    ap.add_argument('--check', action='store_true', help='compare with the file instead of writing it')
    args = ap.parse_args()
    path = args.out or os.path.join(C.GOLDEN, f'wrw_mfma_{args.which}.json')
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
