"""profiles/wrw_pool_pmc.csv from rocprofv3's counter files: the dense weight gradient on g against the pooled entry point, per layer.

Every pass is a run of its own, no tracing:
    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d DIR/conv1_2_mfma -o pmc -- \\
        python tools/wrw_pool_rows.py --reps 1 --layers conv1_2 --batches 64
    ... --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR/conv1_2_lds ...; ... --pmc GRBM_GUI_ACTIVE -d DIR/conv1_2_grbm ...; the same for conv4_3
    python tools/wrw_pool_pmc.py --out profiles/wrw_pool_pmc.csv conv1_2 DIR/conv1_2_* conv4_3 DIR/conv4_3_*

Per (layer, kernel, counter) the mean over the kernel's launches (tools/wrw_pool_rows.py launches each three times with --reps 1); `wall_ms`
is the mean of End - Start of the same launches, taken under the counters; `pooled_over_dense` stands on the pooled rows only."""
import argparse
import collections
import csv
import glob
import os

LAYERS = ('conv1_2', 'conv2_2', 'conv3_3', 'conv4_3', 'conv5_3')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('args', nargs='+', help='LAYER DIR [DIR ...], repeated')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    groups, layer = collections.OrderedDict(), None
    for t in a.args:
        if t in LAYERS:
            layer = t
            groups[layer] = []
        else:
            groups[layer].append(t)
    lines = ['layer,batch,kernel,counter,launches,mean_per_launch,wall_ms,pooled_over_dense']
    for layer, dirs in groups.items():
        val, wall = collections.defaultdict(list), collections.defaultdict(list)
        for d in dirs:
            for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
                with open(f) as fh:
                    for r in csv.DictReader(fh):
                        if 'conv3x3_wrw' not in r['Kernel_Name']:
                            continue
                        arm = 'pooled' if 'pooled' in r['Kernel_Name'] else 'dense'
                        val[arm, r['Counter_Name']].append(float(r['Counter_Value']))
                        wall[arm, r['Counter_Name']].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6)
        mean = {k: sum(v) / len(v) for k, v in val.items()}
        for arm, name in (('dense', 'hk_conv3x3_wrw on g (conv3x3_wrw_split_kernel 16x16x32)'), ('pooled', 'hk_conv3x3_wrw_pooled (conv3x3_wrw_pooled_kernel)')):
            for (k, c) in sorted(mean):
                if k != arm:
                    continue
                ratio = ''
                if arm == 'pooled' and mean.get(('dense', c)):
                    ratio = f"{mean[arm, c] / mean['dense', c]:.4f}"
                w = wall[arm, c]
                lines.append(f'{layer},{a.batch},{name},{c},{len(val[arm, c])},{mean[arm, c]:.0f},{sum(w) / len(w):.4f},{ratio}')
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
