"""conv3x3_split_kernel's counters with the weight tiles staged through registers (the parent commit's build) and by LDS-DMA side by
side, from the rocprofv3 counter passes of tools/run_conv_fwd.py (each pass a run of its own, never with tracing; the sibling of
tools/conv_mfma_pmc.py, whose aggregation this uses):

    python tools/conv_wdma_pmc.py DIR_PARENT DIR_NEW > profiles/conv_wdma_conv1_2_pmc.csv

Rows: Staging,Counter,Dispatches,MeanValue."""
import csv
import sys

from conv_mfma_pmc import rows_of

if __name__ == '__main__':
    w = csv.writer(sys.stdout)
    w.writerow(['Staging', 'Counter', 'Dispatches', 'MeanValue'])
    for staging, d in zip(('registers', 'lds_dma'), sys.argv[1:3]):
        for c, (n, v) in rows_of(d).items():
            w.writerow([staging, c, n, round(v, 4)])
