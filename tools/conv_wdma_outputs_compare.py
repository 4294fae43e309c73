"""The comparison of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/conv_wdma_outputs_compare.txt (the sibling of
tools/conv_mfma_outputs_compare.py):

    python tools/conv_wdma_outputs_compare.py PARENT_A PARENT_B NEW > profiles/conv_wdma_outputs_compare.txt

PARENT_* ran on the parent commit's build (weight tiles staged through registers), NEW on this one (LDS-DMA), same arguments, same
routing.  How a weight tile reaches LDS changes no operand and no order of additions, so the verdicts are
  parent - parent   bit-identical
  new - parent      bit-identical, every array
Exit status 1 if a verdict fails."""
import os
import sys

import numpy as np


def main(pa, pb, new):
    names = sorted(f[:-4] for f in os.listdir(pa) if f.endswith('.npy'))
    load = lambda d, n: np.load(os.path.join(d, n + '.npy'))
    same = lambda u, v: u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
    ok = {'parent-parent': True, 'new-parent': True}
    for n in names:
        a, b, u = (load(d, n) for d in (pa, pb, new))
        pp, np_ = same(a, b), same(a, u)
        ok['parent-parent'] &= pp
        ok['new-parent'] &= np_
        print(f'{n} {a.dtype} {tuple(a.shape)} parent-parent {"identical" if pp else "DIFFERENT"} new-parent {"identical" if np_ else "DIFFERENT"} '
              f'norm {float(np.linalg.norm(a.astype(np.float64))):.6e}')
    print(f'{len(names)} arrays; ' + '; '.join(f'{k}: {"bit-identical" if v else "FAILS"}' for k, v in ok.items()))
    return 0 if names and all(ok.values()) else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:4]))
