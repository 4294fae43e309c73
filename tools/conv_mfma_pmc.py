"""conv3x3_split_kernel's counters on either bf16 MFMA side by side, from the rocprofv3 counter passes of tools/run_conv_fwd.py (each
pass a run of its own, never with tracing; HK_CONV_MFMA=0 and =1):

    python tools/conv_mfma_pmc.py DIR_MFMA32 DIR_MFMA16 > profiles/conv_mfma_conv1_2_pmc.csv

Rows: Shape,Counter,Dispatches,MeanValue - per dispatch a counter's values are summed over its instances, then averaged over the
dispatches (tools/pmc_summary.py's rule); `wall_ms` is the dispatch's own End - Start in the pass that read GRBM_GUI_ACTIVE, and
`clock_GHz` = GRBM_GUI_ACTIVE / 8 / wall (the counter is the sum over the 8 XCDs)."""
import csv
import glob
import os
import sys
from collections import defaultdict


def rows_of(d):
    acc, wall = defaultdict(lambda: defaultdict(float)), {}
    for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            if 'conv3x3_split_kernel' not in r['Kernel_Name']:
                continue
            acc[r['Counter_Name']][(f, r['Dispatch_Id'])] += float(r['Counter_Value'])
            if r['Counter_Name'] == 'GRBM_GUI_ACTIVE':
                wall[(f, r['Dispatch_Id'])] = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
    out = {c: (len(v), sum(v.values()) / len(v)) for c, v in sorted(acc.items())}
    out['wall_ms'] = (len(wall), sum(wall.values()) / len(wall))
    out['clock_GHz'] = (len(wall), out['GRBM_GUI_ACTIVE'][1] / 8 / (out['wall_ms'][1] * 1e-3) / 1e9)
    return out


if __name__ == '__main__':
    w = csv.writer(sys.stdout)
    w.writerow(['Shape', 'Counter', 'Dispatches', 'MeanValue'])
    for shape, d in zip(('32x32x16', '16x16x32'), sys.argv[1:3]):
        for c, (n, v) in rows_of(d).items():
            w.writerow([shape, c, n, round(v, 4)])
