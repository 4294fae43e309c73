"""conv3x3_wrw_split_kernel's counters side by side, from the rocprofv3 counter passes of tools/run_conv_wrw.py (each pass a run of its
own, never with tracing):

    python tools/wrw_mfma_pmc.py NAME=DIR [NAME2=DIR2 ...] > profiles/wrw_mfma_pmc.csv

Rows: Run,Counter,Dispatches,MeanValue - per dispatch a counter's values are summed over its instances, then averaged over the
dispatches (tools/conv_mfma_pmc.py's rule); `wall_ms` is the dispatch's own End - Start in the pass that read GRBM_GUI_ACTIVE,
`clock_GHz` = GRBM_GUI_ACTIVE / 8 / wall (the counter is the sum over the 8 XCDs), `mfma_busy_share` = SQ_VALU_MFMA_BUSY_CYCLES /
SQ_BUSY_CU_CYCLES where both were read."""
import csv
import glob
import os
import sys
from collections import defaultdict


def rows_of(d, kernel='conv3x3_wrw_split_kernel'):
    acc, wall = defaultdict(lambda: defaultdict(float)), {}
    for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            if kernel not in r['Kernel_Name']:
                continue
            acc[r['Counter_Name']][(f, r['Dispatch_Id'])] += float(r['Counter_Value'])
            if r['Counter_Name'] == 'GRBM_GUI_ACTIVE':
                wall[(f, r['Dispatch_Id'])] = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
    out = {c: (len(v), sum(v.values()) / len(v)) for c, v in sorted(acc.items())}
    if wall:
        out['wall_ms'] = (len(wall), sum(wall.values()) / len(wall))
        out['clock_GHz'] = (len(wall), out['GRBM_GUI_ACTIVE'][1] / 8 / (out['wall_ms'][1] * 1e-3) / 1e9)
    if 'SQ_VALU_MFMA_BUSY_CYCLES' in out and 'SQ_BUSY_CU_CYCLES' in out:
        out['mfma_busy_share'] = (out['SQ_VALU_MFMA_BUSY_CYCLES'][0], out['SQ_VALU_MFMA_BUSY_CYCLES'][1] / out['SQ_BUSY_CU_CYCLES'][1])
    return out


if __name__ == '__main__':
    w = csv.writer(sys.stdout)
    w.writerow(['Run', 'Counter', 'Dispatches', 'MeanValue'])
    for arg in sys.argv[1:]:
        name, d = arg.split('=', 1)
        for c, (n, v) in rows_of(d).items():
            w.writerow([name, c, n, round(v, 4)])
