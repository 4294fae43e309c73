"""conv3x3_split_kernel's counters with 4 x 32 tiles (HK_CONV_TILE=0) and with the planned geometry side by side, from the rocprofv3
counter passes of tools/run_conv_fwd.py (HK_CONV_MFMA=1; each pass a run of its own, never with tracing; the sibling of
tools/conv_mfma_pmc.py, whose aggregation this uses):

    python tools/conv_tile_pmc.py DIR_4x32 DIR_PLANNED > profiles/conv_tile_conv4_2_pmc.csv

Rows: Tiles,Counter,Dispatches,MeanValue, and per counter the ratio planned / 4 x 32."""
import csv
import sys

from conv_mfma_pmc import rows_of

if __name__ == '__main__':
    w = csv.writer(sys.stdout)
    w.writerow(['Tiles', 'Counter', 'Dispatches', 'MeanValue'])
    arms = [rows_of(d) for d in sys.argv[1:3]]
    for tiles, rows in zip(('4x32', 'planned'), arms):
        for c, (n, v) in rows.items():
            w.writerow([tiles, c, n, round(v, 4)])
    for c in arms[0]:
        if c in arms[1] and arms[0][c][1]:
            w.writerow(['planned/4x32', c, '', round(arms[1][c][1] / arms[0][c][1], 4)])
