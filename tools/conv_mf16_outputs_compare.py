"""The comparisons of `bench.py --steps 5 --warmup 2 --dump-outputs DIR` behind profiles/conv_mf16_outputs_compare.txt (the sibling of
tools/conv_mfma_outputs_compare.py):

    python tools/conv_mf16_outputs_compare.py PARENT PARENT_WRW_SPLIT_0 NEW_A NEW_B [READ_AHEAD] > profiles/conv_mf16_outputs_compare.txt

PARENT ran on the parent commit's build (the MFMA shape per layer by functional.py's tables), PARENT_WRW_SPLIT_0 on the same build with
HK_WRW_SPLIT=0 - the project's yardstick for a difference that is rounding alone -, NEW_* on this build (16 x 16 x 32 in every launch,
by the library's rule), READ_AHEAD on the build that also read the pixel fragments one tap ahead (not kept).  Per array the
l2 distances, the loss of every run, and the verdicts:
  new - new          bit-identical
  new - parent       twelve launches add in another order: no array farther than 2 x the yardstick's distance
  read-ahead - new   bit-identical (no operand and no order changes)
Exit status 1 if a verdict fails."""
import os
import sys

import numpy as np


def main(pa, ws0, na, nb, ra=None):
    names = sorted(f[:-4] for f in os.listdir(pa) if f.endswith('.npy'))
    raw = lambda d, n: np.load(os.path.join(d, n + '.npy'))
    same = lambda u, v: u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes()
    dist = lambda u, v: float(np.linalg.norm(u.astype(np.float64) - v.astype(np.float64)))
    dirs = [('parent', pa), ('parent(wrw_split 0)', ws0), ('new', na), ('new again', nb)] + ([('read-ahead', ra)] if ra else [])
    print('loss ' + ' '.join(f'{k} {float(raw(d, "loss").reshape(-1)[0]):.7g}' for k, d in dirs))
    rows, ok = [], {'new-new': True, 'new-parent': True}
    if ra:
        ok['read-ahead-new'] = True
    for n in names:
        a, y, u, v = (raw(d, n) for d in (pa, ws0, na, nb))
        d_n, d_y = dist(u, a), dist(y, a)
        ok['new-new'] &= same(u, v)
        ok['new-parent'] &= d_n <= 2.0 * d_y
        extra = ''
        if ra:
            s = same(raw(ra, n), u)
            ok['read-ahead-new'] &= s
            extra = f' read-ahead-new {"identical" if s else "DIFFERENT"}'
        ratio = d_n / d_y if d_y > 0 else (0.0 if d_n == 0 else float('inf'))
        rows.append((ratio, f'{n} new-new {"identical" if same(u, v) else "DIFFERENT"}{extra} new-parent {d_n:.3e} parent(wrw_split 0)-parent {d_y:.3e} '
                            f'new / yardstick {ratio:.2f} norm {float(np.linalg.norm(a.astype(np.float64))):.3e}'))
    for _, line in sorted(rows, reverse=True):
        print(line)
    print(f'{len(names)} arrays; ' + '; '.join(f'{k}: {"holds" if v else "FAILS"}' for k, v in ok.items()))
    return 0 if names and all(ok.values()) else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:6]))
