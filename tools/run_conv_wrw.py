"""Launch hk_conv3x3_wrw three times at one trunk layer - the target of a counter pass (`rocprofv3 --pmc ...`, a run of its own, never
combined with tracing; aggregate with tools/wrw_mfma_pmc.py).  The MFMA shape comes from the environment (HK_WRW_MFMA=0 / 1):

    python tools/run_conv_wrw.py conv1_2 [--batch 64]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from wrw_rows import LAYERS, WIDE_LAYERS  # noqa: E402

ALL = {**{k: (s, 64, c) for k, (s, c) in LAYERS.items()}, **WIDE_LAYERS}      # side, Cin, Cout

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('layer', choices=sorted(ALL))
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('run_conv_wrw needs an MI355X')
        sys.exit(2)
    import hawkeye_amd.functional as HF
    from hawkeye_amd import _lib
    side, cin, cout = ALL[args.layer]
    x = torch.randn(args.batch, side, side, cin, device='cuda').relu_().permute(0, 3, 1, 2)
    dy = torch.randn(args.batch, side, side, cout, device='cuda').permute(0, 3, 1, 2)
    with _lib.tuning(wrw_split=1):
        for _ in range(3):
            HF.conv3x3_wrw_raw(x, dy)
    torch.cuda.synchronize()
