"""NTS-Net's head at the yaml's shapes (B = 4, 426 anchors, 6 proposals, 24 crops of 3 x 224 x 224, 24 x 200 part
logits), piece by piece, on one device in one process:

  nms    (i) nts_nms + the gather of the chosen scores; (ii) the reference's sequence restated in torch / numpy
         (NTSNet.py:35-41): all scores copied to the host, a table per image, a sort, a greedy loop with vectorised IoU,
         the indices uploaded, the gather;
  crop   (i) nts_crop_resize; (ii) F.pad of the batch, a zeros() buffer and B x topN F.interpolate calls on slices whose
         corners are host integers (NTSNet.py:31,42-47);
  loss   forward + backward: (i) nts_loss; (ii) log_softmax + one .item() per part row + stack, three smoothed cross
         entropies and the per-proposal ranking loop (NTS_loss.py:15-47);
  head   all three in sequence, and (i) replayed from one hipGraph (tools/nts_graph_check.py's capture).

(ii) is a yardstick only; nothing in the package calls it.  Times are host-clock medians over `--samples` samples of
`--calls` calls, each sample ending in a device synchronise, the variants of a piece taken in turn after a warm-up.  The
crop kernel is also timed with device events around `--calls` back-to-back launches, and its achieved bandwidth is the
bytes it must write (the source window stays in L2) over that time.  `--step` adds the step time of
configs/NTSNet_synthetic.yaml's model (ResNet-50, 4 + 24 images of 224 x 224, forward + backward + Adam).

    python tools/nts_rows.py [--out FILE.json] [--step]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nts_graph_check as G  # noqa: E402

PEAK_HBM = 8.0e12           # bytes / s, MI355X


def host_nms(rows, topn, thresh):
    """One image: rows [A, 6] = score, y0, x0, y1, x1, index (float64) -> the chosen rows, greedy from the sorted end."""
    rows = rows[np.argsort(rows[:, 0])]
    chosen = []
    while len(rows) and len(chosen) < topn:
        top, rows = rows[-1], rows[:-1]
        chosen.append(top)
        side = np.minimum(rows[:, 3:5], top[3:5]) - np.maximum(rows[:, 1:3], top[1:3])
        inter = side[:, 0] * side[:, 1]
        inter[(side < 0).any(1)] = 0
        union = (rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2]) + (top[3] - top[1]) * (top[4] - top[2]) - inter
        rows = rows[inter / union < thresh]
    return np.array(chosen)


def torch_nms(scores, padded_anchors, topn):
    host = scores.detach().cpu().numpy()
    ids = np.arange(host.shape[1]).reshape(-1, 1)
    tables = [np.concatenate((row.reshape(-1, 1), padded_anchors, ids), axis=1) for row in host]
    top = np.array([host_nms(t, topn, 0.25) for t in tables])
    index = torch.from_numpy(top[:, :, -1].astype(np.int64)).to(scores.device)
    return top, index, torch.gather(scores, 1, index)


def torch_crops(images, top, pad, size):
    b, n = top.shape[:2]
    x_pad = F.pad(images, (pad, pad, pad, pad), mode='constant', value=0)
    parts = torch.zeros([b, n, images.shape[1], size, size], device=images.device)
    for i in range(b):
        for j in range(n):
            y0, x0, y1, x1 = top[i][j, 1:5].astype(int)
            parts[i:i + 1, j] = F.interpolate(x_pad[i:i + 1, :, y0:y1, x0:x1], size=(size, size), mode='bilinear', align_corners=True)
    return parts.view(b * n, images.shape[1], size, size)


def torch_loss(raw, cat, part, prob, y):
    b, n, c = part.shape
    flat, yy = part.view(b * n, c), y.unsqueeze(1).repeat(1, n).view(-1)
    logp = F.log_softmax(flat, -1)
    part_loss = torch.stack([-logp[i][yy[i].item()] for i in range(b * n)]).view(b, n)
    rank = torch.zeros(1, device=raw.device)
    for i in range(n):
        gate = (part_loss > part_loss[:, i].unsqueeze(1)).float()
        rank = rank + torch.sum(F.relu((1 - prob[:, i].unsqueeze(1) + prob) * gate))
    ce = lambda l, t: F.cross_entropy(l, t, label_smoothing=0.1)
    return ce(raw, y) + rank / b + ce(cat, y) + ce(flat, yy)


def timed(variants, samples, calls):
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(samples):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / calls * 1e6)
    rows = {}
    for name, ts in times.items():
        ts.sort()
        rows[name] = {'median_us': round(ts[len(ts) // 2], 1), 'min_us': round(ts[0], 1), 'p90_us': round(ts[int(0.9 * len(ts))], 1)}
    return rows


def event_time_us(fn, calls, repeats=15):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    out.sort()
    return {'median_us': round(out[len(out) // 2], 2), 'min_us': round(out[0], 2), 'max_us': round(out[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('nts_rows needs an MI355X')
        return 2
    import hawkeye_amd.functional as HF
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    padded = G.T.load()['anchors_224']
    anchors = torch.from_numpy(padded - 224).to(dev)
    case = G.device_case(1, padded, dev)
    images, scores, y = case['images'], case['scores'], case['y']
    leaves = [case[k].clone().requires_grad_(True) for k in ('raw', 'cat', 'part')]
    B, N, SIZE = G.B, G.N, G.SIZE

    # the two formulations agree on the same inputs (the yardstick computes what the kernels compute)
    index, boxes = HF.nts_nms(scores, anchors, N)
    top, ref_index, ref_prob = torch_nms(scores, padded.astype(np.float64), N)
    prob = torch.gather(scores, 1, index).requires_grad_(True)
    crops, ref_crops = HF.nts_crop_resize(images, boxes, 224, SIZE), torch_crops(images, top, 224, SIZE)
    ours_loss, ref_loss = HF.nts_loss(*leaves, prob, y), torch_loss(*leaves, prob, y)
    g_ours = torch.autograd.grad(ours_loss, leaves + [prob])
    g_ref = torch.autograd.grad(ref_loss, leaves + [prob])
    agree = dict(index_equal=bool(torch.equal(index, ref_index)), crops_rel=float((crops - ref_crops).norm() / ref_crops.norm()),
                 loss_rel=abs(ours_loss.item() - ref_loss.item()) / abs(ref_loss.item()),
                 grads_rel=[float((a - b).norm() / b.norm()) for a, b in zip(g_ours, g_ref)])

    def ours_nms():
        i, bx = HF.nts_nms(scores, anchors, N)
        return bx, torch.gather(scores, 1, i)

    def ours_loss_step(p=prob):
        for t in leaves + [prob]:
            t.grad = None
        HF.nts_loss(*leaves, p, y).backward()

    def ref_loss_step(p=prob):
        for t in leaves + [prob]:
            t.grad = None
        torch_loss(*leaves, p, y).backward()

    def ours_head():
        bx, _ = ours_nms()
        HF.nts_crop_resize(images, bx, 224, SIZE)
        ours_loss_step()

    def ref_head():
        t, _, _ = torch_nms(scores, padded.astype(np.float64), N)
        torch_crops(images, t, 224, SIZE)
        ref_loss_step()

    cap = G.Step(padded, dev)
    cap.load(case)
    cap.capture()
    result = {'shape': {'B': B, 'A': int(len(padded)), 'topN': N, 'crops': [B * N, 3, SIZE, SIZE], 'C': G.C}, 'samples': args.samples,
              'calls': args.calls, 'agreement': agree}
    result['nms'] = timed({'new_ops': ours_nms, 'torch_reference_sequence': lambda: torch_nms(scores, padded.astype(np.float64), N)},
                          args.samples, args.calls)
    result['crop'] = timed({'new_ops': lambda: HF.nts_crop_resize(images, boxes, 224, SIZE),
                            'torch_reference_sequence': lambda: torch_crops(images, top, 224, SIZE)}, args.samples, args.calls)
    result['loss_fwd_bwd'] = timed({'new_ops': ours_loss_step, 'torch_reference_sequence': ref_loss_step}, args.samples, args.calls)
    result['head'] = timed({'new_ops': ours_head, 'torch_reference_sequence': ref_head, 'new_ops_graph_replay': cap.replay},
                           args.samples, args.calls)
    kernel = event_time_us(lambda: HF.nts_crop_resize(images, boxes, 224, SIZE), args.calls)
    written = B * N * 3 * SIZE * SIZE * 4
    kernel['bytes_written'] = written
    kernel['achieved_TBps_at_median'] = round(written / (kernel['median_us'] * 1e-6) / 1e12, 3)
    kernel['fraction_of_peak_hbm'] = round(written / (kernel['median_us'] * 1e-6) / PEAK_HBM, 3)
    result['crop_kernel_device_events'] = kernel
    result['nms_kernel_device_events'] = event_time_us(lambda: HF.nts_nms(scores, anchors, N), args.calls)
    result['loss_fwd_bwd_device_events'] = event_time_us(ours_loss_step, args.calls)
    if args.step:
        result['model_step'] = model_step(dev)
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    return 0


def model_step(dev, steps=8):
    import hawkeye_amd.model.methods.NTSNet as plugin
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import NTSLoss
    cfg = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'NTSNet_synthetic.yaml')))
    net = plugin.NTSNet(cfg.model).to(dev).train()
    crit = NTSLoss(cfg.train.criterion)
    opt = torch.optim.Adam(net.parameters(), lr=cfg.train.optimizer.lr, weight_decay=cfg.train.optimizer.weight_decay)
    b, size = cfg.dataset.batch_size, cfg.dataset.transformer.image_size
    x = torch.randn(b, 3, size, size, device=dev)
    y = torch.arange(b, device=dev) * 7
    ts = []
    for i in range(3 + steps):
        t0 = time.perf_counter()
        opt.zero_grad()
        crit(net(x), y).backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {'images': b, 'part_images': b * cfg.model.proposal_num, 'size': size, 'median_ms': round(ts[len(ts) // 2], 2),
            'min_ms': round(ts[0], 2), 'steps': steps}


if __name__ == '__main__':
    sys.exit(main())
