"""DCL's head, loss and swap law at the yaml's shapes (B = 8 images and their swapped copies: a [16,2048,14,14] map, 200
classes, a 7 x 7 grid on 448 x 448 images), forward + backward where there is one, two ways each:

  head   (i) dcl_head; (ii) the reference's sequence in torch (DCL.py:33-39): Conv2d 1 x 1, AvgPool2d(2), tanh, view,
         AdaptiveAvgPool2d(1), and autograd's backward through them;
  loss   (i) dcl_loss; (ii) the reference's criterion restated in torch (DCL_loss.py:17-20): two label-smoothed cross
         entropies, an L1 loss, the weighted sum;
  law    (i) dcl_swap_law on uint8 batches on the device; (ii) the reference's procedure (dataset_DCL.py:48-62) on the
         host, as it runs there: per image 98 crops, 98 ImageStat means and a 49 x 49 search in Python (host clock only).

Times are the host clock around eager calls ending in a synchronise and, where both variants capture, device events around
hipGraph replays (tools/crossx_rows.py's two clocks).  Writes the rows as json.

    python tools/dcl_rows.py [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from crossx_rows import PEAK_HBM, graph_timed, merge, timed  # noqa: E402

B, K, C, SIDE, IMAGE, GRID = 8, 200, 2048, 14, 448, (7, 7)
COEF = (1.0, 1.0, 1.0)


def torch_head(x, w, bias):
    mask = torch.tanh(F.avg_pool2d(F.conv2d(x, w, bias), 2, stride=2))
    return F.adaptive_avg_pool2d(x, 1).view(x.size(0), -1), mask.view(mask.size(0), -1)


def head_piece(HF, dev, samples, calls):
    rs = np.random.RandomState(1)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(dev)
    x, w, bias = t(2 * B, C, SIDE, SIDE).requires_grad_(True), (t(1, C, 1, 1) / C ** 0.5).requires_grad_(True), t(1).requires_grad_(True)
    d_pooled, d_mask = t(2 * B, C), t(2 * B, 49)
    fused = lambda: torch.autograd.grad(HF.dcl_head(x, w, bias), [x, w, bias], [d_pooled, d_mask])
    yardstick = lambda: torch.autograd.grad(torch_head(x, w, bias), [x, w, bias], [d_pooled, d_mask])
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(fused(), yardstick()))
    rows = merge(timed({'fused': fused, 'torch_sequence': yardstick}, samples, calls), graph_timed({'fused': fused, 'torch_sequence': yardstick}))
    moved = 2 * B * C * SIDE * SIDE * 4 * 3                 # x read forward, x read and dx written backward
    rows['fused']['bytes_moved'] = moved
    rows['fused']['achieved_TBps'] = round(moved / (rows['fused']['graph_median_us'] * 1e-6) / 1e12, 3)
    rows['fused']['share_of_hbm_peak'] = round(moved / (rows['fused']['graph_median_us'] * 1e-6) / PEAK_HBM, 3)
    rows['max_relative_gradient_difference'] = worst
    return rows


def loss_piece(HF, dev, samples, calls):
    rs = np.random.RandomState(2)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(dev)
    leaves = [t(2 * B, K).requires_grad_(True), t(2 * B, 2).requires_grad_(True), torch.tanh(t(2 * B, 49)).requires_grad_(True)]
    y, ys = torch.from_numpy(rs.randint(0, K, 2 * B)).to(dev), torch.from_numpy(rs.randint(0, 2, 2 * B)).to(dev)
    law = torch.from_numpy(((rs.randint(0, 49, (2 * B, 49)) - 24) / 49).astype(np.float32)).to(dev)

    def torch_loss():
        return COEF[0] * F.cross_entropy(leaves[0], y, label_smoothing=0.1) + COEF[1] * F.cross_entropy(leaves[1], ys, label_smoothing=0.1) + \
            COEF[2] * F.l1_loss(leaves[2], law)
    fused = lambda: torch.autograd.grad(HF.dcl_loss(*leaves, y, ys, law, *COEF), leaves)
    yardstick = lambda: torch.autograd.grad(torch_loss(), leaves)
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(fused(), yardstick()))
    rows = merge(timed({'fused': fused, 'torch_sequence': yardstick}, samples, calls), graph_timed({'fused': fused, 'torch_sequence': yardstick}))
    rows['max_relative_gradient_difference'] = worst
    return rows


def host_law(unswap, swapped, grid):
    """The reference's procedure on PIL images, restated: crops, ImageStat means, the nearest-mean search."""
    from PIL import Image, ImageStat
    from hawkeye_amd.transforms import patch_bounds

    def stats(arr):
        img = Image.fromarray(arr)
        w, h = img.size
        xs, ys = patch_bounds(w, grid[0]), patch_bounds(h, grid[1])
        return [sum(ImageStat.Stat(img.crop((xs[i], ys[j], min(xs[i + 1], w), min(ys[j + 1], h)))).mean) for j in range(grid[1]) for i in range(grid[0])]
    parts = grid[0] * grid[1]
    law = []
    for a, s in zip(unswap, swapped):
        un = stats(a)
        row = []
        for v in stats(s):
            distance = [abs(v - u) for u in un]
            row.append((distance.index(min(distance)) - parts // 2) / parts)
        law.append(row)
    return law


def law_piece(HF, dev, samples, calls):
    import dcl_inputs as T
    rs = np.random.RandomState(3)
    un = np.stack([T.smooth_image(rs, IMAGE, IMAGE, cells=14) for _ in range(B)])
    sw = np.stack([T.permute_patches(u, rs.permutation(49), GRID) for u in un])
    dun, dsw = torch.from_numpy(un).to(dev), torch.from_numpy(sw).to(dev)
    fused = lambda: HF.dcl_swap_law(dun, dsw, GRID)
    same = np.array_equal(fused()[0].cpu().numpy(), np.array(host_law(un, sw, GRID), dtype=np.float64).astype(np.float32))
    rows = merge(timed({'fused': fused}, samples, calls), graph_timed({'fused': fused}))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_law(un, sw, GRID)
        ts.append((time.perf_counter() - t0) * 1e6)
    rows['host_python'] = {'median_us': round(sorted(ts)[1], 1), 'min_us': round(min(ts), 1), 'note': 'one process, no data workers; the images are already decoded'}
    rows['fused']['bytes_read'] = 2 * B * IMAGE * IMAGE * 3
    rows['law_equal_to_the_host_procedure'] = bool(same)
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('dcl_rows needs an MI355X: nothing is measured without one')
        sys.exit(2)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    import hawkeye_amd.functional as HF
    result = {'shape': {'B': B, 'rows': 2 * B, 'K': K, 'map': [2 * B, C, SIDE, SIDE], 'image': IMAGE, 'grid': list(GRID)}, 'samples': args.samples,
              'calls_per_sample': args.calls, 'device': torch.cuda.get_device_name(0),
              'unit': 'microseconds per call (forward + backward for head and loss): host clock around eager calls, and device events around hipGraph replays (graph_*)'}
    result['head'] = head_piece(HF, dev, args.samples, args.calls)
    result['loss'] = loss_piece(HF, dev, args.samples, args.calls)
    result['law'] = law_piece(HF, dev, args.samples, args.calls)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
