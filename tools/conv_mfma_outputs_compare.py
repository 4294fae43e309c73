"""The comparisons of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/conv_mfma_outputs_compare.txt (the sibling of
tools/conv_epi_outputs_compare.py):

    python tools/conv_mfma_outputs_compare.py PARENT_A PARENT_B NEW_A NEW_B PARENT_WRW_SPLIT_0 > profiles/conv_mfma_outputs_compare.txt

PARENT_* ran with HK_CONV_MFMA=0 (the parent's routing: 32 x 32 x 16 everywhere), NEW_* with the default routing (the measured table of
functional.py), the last one with HK_CONV_MFMA=0 HK_WRW_SPLIT=0 - the project's yardstick for a difference that is rounding alone.
Per array the l2 distances, and the verdicts:
  parent - parent   bit-identical
  new - new         bit-identical
  loss              identical to the seven digits printed here
  new - parent      another order of the same additions: no array farther than 2 x the yardstick's distance
Exit status 1 if a verdict fails."""
import os
import sys

import numpy as np


def main(pa, pb, na, nb, ws0):
    names = sorted(f[:-4] for f in os.listdir(pa) if f.endswith('.npy'))
    load = lambda d, n: np.load(os.path.join(d, n + '.npy')).astype(np.float64)
    same = lambda u, v: u.shape == v.shape and np.array_equal(u.view(np.int64), v.view(np.int64))
    rows, ok = [], {'parent-parent': True, 'new-new': True, 'loss': True, 'new-parent': True}
    for n in names:
        a, b, u, v, y = (load(d, n) for d in (pa, pb, na, nb, ws0))
        d_pp, d_nn, d_n, d_y = float(np.linalg.norm(b - a)), float(np.linalg.norm(v - u)), float(np.linalg.norm(u - a)), float(np.linalg.norm(y - a))
        ok['parent-parent'] &= same(a, b)
        ok['new-new'] &= same(u, v)
        ok['new-parent'] &= d_n <= 2.0 * d_y
        if n == 'loss':
            ok['loss'] &= f'{float(a[0]):.7g}' == f'{float(u[0]):.7g}'
            print(f'loss parent {float(a[0]):.7g} new {float(u[0]):.7g} parent(wrw_split 0) {float(y[0]):.7g}')
        ratio = d_n / d_y if d_y > 0 else (0.0 if d_n == 0 else float('inf'))
        rows.append((ratio, f'{n} parent-parent {d_pp:.3e} new-new {d_nn:.3e} new-parent {d_n:.3e} parent(wrw_split 0)-parent {d_y:.3e} '
                            f'new / yardstick {ratio:.2f} norm {float(np.linalg.norm(a)):.3e}'))
    for _, line in sorted(rows, reverse=True):
        print(line)
    print(f'{len(names)} arrays; ' + '; '.join(f'{k}: {"holds" if v else "FAILS"}' for k, v in ok.items()))
    return 0 if all(ok.values()) else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:6]))
