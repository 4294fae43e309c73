"""The comparisons of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/wrw_pool_outputs_compare.txt:

    python tools/wrw_pool_outputs_compare.py PARENT_A PARENT_B PARENT_WRW_SPLIT_0 NEW > profiles/wrw_pool_outputs_compare.txt

PARENT_* ran on the parent commit's build, PARENT_WRW_SPLIT_0 on the same build with HK_WRW_SPLIT=0 - the project's yardstick for a
difference that is rounding alone -, NEW on this build (the five pooled layers' weight gradient on the 2:4 sparse MFMA, by the library's
rule).  Per array the l2 distances, the loss of every run, and the verdicts:
  parent - parent    bit-identical
  new - parent       five launches add other products in another order: no array farther than 2 x the yardstick's distance
An array that misses is listed as MISSES.  Exit status 1 if a verdict fails."""
import os
import sys

import numpy as np


def main(pa, pb, ws0, new):
    names = sorted(f[:-4] for f in os.listdir(pa) if f.endswith('.npy'))
    raw = lambda d, n: np.load(os.path.join(d, n + '.npy'))
    same = lambda u, v: u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
    dist = lambda u, v: float(np.linalg.norm(u.astype(np.float64) - v.astype(np.float64)))
    dirs = [('parent', pa), ('parent again', pb), ('parent(wrw_split 0)', ws0), ('new', new)]
    print('loss ' + ' '.join(f'{k} {float(raw(d, "loss").reshape(-1)[0]):.7g}' for k, d in dirs))
    rows, ok = [], {'parent-parent': True, 'new-parent': True}
    for n in names:
        a, b, y, u = (raw(d, n) for d in (pa, pb, ws0, new))
        d_n, d_y = dist(u, a), dist(y, a)
        ok['parent-parent'] &= same(a, b)
        holds = d_n <= 2.0 * d_y
        ok['new-parent'] &= holds
        ratio = d_n / d_y if d_y > 0 else (0.0 if d_n == 0 else float('inf'))
        rows.append((ratio, f'{n} parent-parent {"identical" if same(a, b) else "DIFFERENT"} new-parent {d_n:.3e} parent(wrw_split 0)-parent {d_y:.3e} '
                            f'new / yardstick {ratio:.2f} {"holds" if holds else "MISSES"} norm {float(np.linalg.norm(a.astype(np.float64))):.3e}'))
    for _, line in sorted(rows, reverse=True):
        print(line)
    print(f'{len(names)} arrays; ' + '; '.join(f'{k}: {"holds" if v else "FAILS"}' for k, v in ok.items()))
    return 0 if names and all(ok.values()) else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:5]))
