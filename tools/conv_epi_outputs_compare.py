"""The three comparisons of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/conv_epi_outputs_compare.txt:

    python tools/conv_epi_outputs_compare.py PARENT_A PARENT_B EPI1 EPI2 PARENT_WRW_SPLIT_0 > profiles/conv_epi_outputs_compare.txt

PARENT_* ran with HK_CONV_EPI=0, EPI1 / EPI2 with HK_CONV_EPI=1 / 2, the last one with HK_CONV_EPI=0 HK_WRW_SPLIT=0 - the project's
yardstick for a difference that is rounding alone.  Per array the l2 distances, and three verdicts:
  parent - parent   bit-identical
  epi 1 - parent    bit-identical (the forward epilogues compute the same bits)
  epi 2 - parent    only the order of the bias sums differs: no array farther than 2 x the yardstick's distance
Exit status 1 if a verdict fails."""
import os
import sys

import numpy as np


def main(pa, pb, e1, e2, ws0):
    names = sorted(f[:-4] for f in os.listdir(pa) if f.endswith('.npy'))
    load = lambda d, n: np.load(os.path.join(d, n + '.npy')).astype(np.float64)
    same = lambda u, v: u.shape == v.shape and np.array_equal(u.view(np.int64), v.view(np.int64))
    rows, ok = [], {'parent-parent': True, 'epi1-parent': True, 'epi2-parent': True}
    for n in names:
        a, b, u, v, y = (load(d, n) for d in (pa, pb, e1, e2, ws0))
        d_pp, d_1, d_2, d_y = (float(np.linalg.norm(t - a)) for t in (b, u, v, y))
        ok['parent-parent'] &= same(a, b)
        ok['epi1-parent'] &= same(a, u)
        ok['epi2-parent'] &= d_2 <= 2.0 * d_y
        ratio = d_2 / d_y if d_y > 0 else (0.0 if d_2 == 0 else float('inf'))
        rows.append((ratio, f'{n} parent-parent {d_pp:.3e} epi1-parent {d_1:.3e} epi2-parent {d_2:.3e} parent(wrw_split 0)-parent {d_y:.3e} '
                            f'epi2 / yardstick {ratio:.2f} norm {float(np.linalg.norm(a)):.3e}'))
    for _, line in sorted(rows, reverse=True):
        print(line)
    print(f'{len(names)} arrays; ' + '; '.join(f'{k}: {"holds" if v else "FAILS"}' for k, v in ok.items()))
    return 0 if all(ok.values()) else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:6]))
