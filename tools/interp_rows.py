"""InterpParts' grouping unit and criterion at the yaml's shapes (a [16,1024,28,28] layer-3 map, 5 parts, 200 classes) and
with the reference class's default of 32 parts, two ways each:

  group  (i) ip_group; (ii) the reference's sequence in torch (Interp_Parts.py:56-122): bmm, pow(2).sum(1), the expanded
         temporaries, clamp, softmax, the permuted bmm, the residual coding, normalize - forward alone, and forward +
         backward through autograd;
  loss   (i) ip_loss; (ii) the reference's criterion restated in torch (InterpParts_loss.py:24-138): cross entropy, the
         depthwise conv2d, adaptive_max_pool2d, sort, the log difference - with the window and the prior already on the device,
         which spares the reference its per-call .cpu().numpy() and scipy solve (a yardstick kinder than the reference is).

Times are the host clock around eager calls ending in a synchronise and device events around hipGraph replays
(tools/crossx_rows.py's two clocks: warm-up, repeated samples, alternating order).  The grouping rows also give the bytes
that must move (the map read once forward; read once and its gradient written once backward) against the 8 TB/s peak.
Writes the rows as json.

    python tools/interp_rows.py [--out FILE.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'tests'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from crossx_rows import PEAK_HBM, graph_timed, merge, timed  # noqa: E402

N, C, H, W, CLASSES = 16, 1024, 28, 28, 200
CRITERION = dict(radius=2, std=0.4, alpha=1.0, beta=0.001, coeff=0.5)


def torch_group(inputs, weight, smooth):
    n, c, h, w = inputs.shape
    k = weight.shape[0]
    centers = weight.contiguous().view(1, k, c).expand(n, k, c)
    cx = torch.bmm(centers, inputs.contiguous().view(n, c, h * w)).contiguous().view(n, k, h, w)
    x_sq = inputs.pow(2).sum(1, keepdim=True).expand(-1, k, -1, -1)
    c_sq = centers.pow(2).sum(2).unsqueeze(2).unsqueeze(3).expand(-1, -1, h, w)
    beta = torch.sigmoid(smooth)
    assign = F.softmax((2 * cx - x_sq - c_sq).clamp(max=0.0) / beta.unsqueeze(0).unsqueeze(2).unsqueeze(3).expand(n, -1, h, w), dim=1)
    x = inputs.contiguous().view(n, c, -1).permute(0, 2, 1)
    assign = assign.contiguous().view(n, k, -1)
    qx = torch.bmm(assign, x)
    sum_ass = torch.sum(assign, dim=2, keepdim=True).expand(-1, -1, c).clamp(min=1e-5)
    out = ((qx / sum_ass) - centers) / (beta / 2).sqrt().unsqueeze(0).unsqueeze(2)
    return F.normalize(out, dim=2).permute(0, 2, 1), assign.contiguous().view(n, k, h, w)


def group_piece(HF, dev, k, samples, calls):
    import interp_inputs as T
    a = T.group_arrays(5, (N, C, k, H, W))
    x, weight, smooth = (torch.from_numpy(a[name]).to(dev).requires_grad_(True) for name in ('x', 'weight', 'smooth'))
    d_out, d_assign = torch.from_numpy(a['d_outputs_t']).to(dev), torch.from_numpy(a['d_assign']).to(dev)
    leaves = [x, weight, smooth]

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(x, weight, smooth)
        return run
    both = lambda fn: (lambda: torch.autograd.grad(fn(x, weight, smooth), leaves, [d_out, d_assign]))
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(both(HF.ip_group)(), both(torch_group)()))
    rows = {'max_relative_gradient_difference': worst}
    map_bytes = N * C * H * W * 4
    for label, wrap, moved in (('forward', forward, map_bytes), ('forward_backward', both, 3 * map_bytes)):
        fns = {'fused': wrap(HF.ip_group), 'torch_sequence': wrap(torch_group)}
        r = merge(timed(fns, samples, calls), graph_timed(fns))
        r['fused']['bytes_that_must_move'] = moved
        r['fused']['achieved_TBps'] = round(moved / (r['fused']['graph_median_us'] * 1e-6) / 1e12, 3)
        r['fused']['share_of_hbm_peak'] = round(moved / (r['fused']['graph_median_us'] * 1e-6) / PEAK_HBM, 3)
        rows[label] = r
    return rows


def loss_piece(HF, dev, k, samples, calls):
    import interp_inputs as T
    logits_np, assign_np, y_np = T.loss_arrays(7, (N, k, H, W, CLASSES), CRITERION['radius'])
    logits, assign = (torch.from_numpy(v).to(dev).requires_grad_(True) for v in (logits_np, assign_np))
    y = torch.from_numpy(y_np).to(dev)
    r = CRITERION['radius']
    window = HF.ip_gaussian_window(r, CRITERION['std']).view(1, 1, 2 * r + 1, 2 * r + 1).expand(k, 1, -1, -1).contiguous().to(dev)
    log_prior = (HF.ip_beta_prior(N, CRITERION['alpha'], CRITERION['beta'], dev).unsqueeze(1) + 1e-5).log()

    def torch_loss():
        occ = F.adaptive_max_pool2d(F.conv2d(assign, window, groups=k), (1, 1)).squeeze(2).squeeze(2)
        emp, _ = occ.sort(dim=0, descending=False)
        return F.cross_entropy(logits, y) + CRITERION['coeff'] * ((emp + 1e-5).log() - log_prior).abs().mean()
    fns = {'fused': lambda: torch.autograd.grad(HF.ip_loss(logits, assign, y, **CRITERION), [logits, assign]),
           'torch_sequence': lambda: torch.autograd.grad(torch_loss(), [logits, assign])}
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(fns['fused'](), fns['torch_sequence']()))
    rows = merge(timed(fns, samples, calls), graph_timed(fns))
    rows['max_relative_gradient_difference'] = worst
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('interp_rows needs an MI355X: nothing is measured without one')
        sys.exit(2)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    import hawkeye_amd.functional as HF
    result = {'shape': {'map': [N, C, H, W], 'classes': CLASSES, 'parts': [5, 32], 'criterion': CRITERION}, 'samples': args.samples,
              'calls_per_sample': args.calls, 'device': torch.cuda.get_device_name(0),
              'unit': 'microseconds per call: host clock around eager calls, and device events around hipGraph replays (graph_*)'}
    for k in (5, 32):
        result[f'group_K{k}'] = group_piece(HF, dev, k, args.samples, args.calls)
        result[f'loss_K{k}'] = loss_piece(HF, dev, k, args.samples, args.calls)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
