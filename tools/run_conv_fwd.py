"""Launch hk_conv3x3_fwd three times at one trunk layer - the target of a counter pass (`rocprofv3 --pmc ...`, never combined with
tracing; aggregate with tools/pmc_summary.py --only conv3x3_split):

    python tools/run_conv_fwd.py conv1_2 [--batch 64]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from conv_rows import LAYERS  # noqa: E402

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('layer', choices=sorted(LAYERS))
    ap.add_argument('--batch', type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('run_conv_fwd needs an MI355X')
        sys.exit(2)
    import hawkeye_amd.functional as HF
    from hawkeye_amd import _lib
    side, cin, cout = LAYERS[args.layer]
    x = torch.randn(args.batch, side, side, cin, device='cuda').relu_().permute(0, 3, 1, 2)
    wt = (0.05 * torch.randn(cout, cin, 3, 3, device='cuda')).contiguous(memory_format=torch.channels_last)
    with _lib.tuning(conv_fwd=1):
        for _ in range(3):
            HF.conv3x3_fwd_raw(x, wt)
    torch.cuda.synchronize()
