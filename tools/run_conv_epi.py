"""Launch the forward of one trunk layer three times as the two-kernel pair (hk_conv3x3_fwd + hk_bias_relu_pool_fwd, or
hk_bias_relu_fwd) and three times with the epilogue inside the kernel - the target of a counter pass in a run of its own
(`rocprofv3 --pmc WRITE_SIZE FETCH_SIZE`, never combined with tracing):

    python tools/run_conv_epi.py conv1_2 [--batch 64] [--no-pool]"""
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
    ap.add_argument('--no-pool', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('run_conv_epi needs an MI355X')
        sys.exit(2)
    import hawkeye_amd.functional as HF
    from hawkeye_amd import _lib
    side, cin, cout = LAYERS[args.layer]
    x = torch.randn(args.batch, side, side, cin, device='cuda').relu_().permute(0, 3, 1, 2)
    wt = (0.05 * torch.randn(cout, cin, 3, 3, device='cuda')).contiguous(memory_format=torch.channels_last)
    bias = 0.1 * torch.randn(cout, device='cuda')
    with _lib.tuning(conv_fwd=1, conv_epi=2), torch.no_grad():
        for _ in range(3):
            y = HF.conv3x3_fwd_raw(x, wt)
            (HF.bias_relu if args.no_pool else HF.bias_relu_pool)(y, bias)
            del y
        for _ in range(3):
            with HF.ConvEpilogue(bias, not args.no_pool, False, None):
                HF.conv3x3(x, wt, True, True, True)
    torch.cuda.synchronize()
