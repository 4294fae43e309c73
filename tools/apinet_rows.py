"""APINet's head and loss at the yaml's shape (B = 40 = 10 classes x 4 images, D = 2048, hidden 512, C = 200), forward +
backward, on one device in one process:

  (i)   the package's path: api_pairs, api_pair_features, hk_linear for map1 / map2 / fc, api_interact, apinet_loss;
  (ii)  the same arithmetic as torch ops in the reference's sequence (model/methods/APINet.py:34-68,76-113 and
        model/loss/APINet_loss.py:29-39), INCLUDING its device-to-host copy of the distance matrix, the numpy pair search
        and the four index uploads - a yardstick only; nothing in the package calls it;
  (iii) the replay of (i) captured into one hipGraph (tools/apinet_graph_check.py's capture).

Both run in training mode (dropout active).  Times are host-clock medians over `--samples` samples of `--calls` calls,
each sample ending in a device synchronise, the variants taken in turn after a warm-up; kernel launches per call are
counted with torch.profiler in a pass of their own, by kernel name (`launches_by_kernel`).  `--step` adds the step time of configs/APINet_synthetic.yaml's
model (ResNet-101, 40 images of 224 x 224, forward + backward + Adam), for information.

    python tools/apinet_rows.py [--out FILE.json] [--step]"""
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

import apinet_graph_check as G  # noqa: E402


def torch_pairs(pool, targets):
    """The reference's pair search: distance matrix on the device, everything else on the host."""
    sq = pool.pow(2).sum(1)
    dist = (-2 * pool.mm(pool.t()) + sq.view(1, -1) + sq.view(-1, 1)).detach().cpu().numpy()
    lab = targets.detach().cpu().numpy().reshape(-1, 1)
    n = lab.shape[0]
    same = lab == lab.T
    same[np.diag_indices(n)] = False
    d_same = dist.copy()
    d_same[~same] = np.inf
    intra = np.argmin(d_same, 1)
    same[np.diag_indices(n)] = True
    d_diff = dist.copy()
    d_diff[same] = np.inf
    inter = np.argmin(d_diff, 1)
    pairs = {k: np.zeros([n, 2]) for k in ('intra_p', 'inter_p', 'intra_l', 'inter_l')}
    for i in range(n):                                  # the reference fills its four tables row by row
        pairs['intra_p'][i], pairs['inter_p'][i] = (i, intra[i]), (i, inter[i])
        pairs['intra_l'][i], pairs['inter_l'][i] = (lab[i, 0], lab[intra[i], 0]), (lab[i, 0], lab[inter[i], 0])
    return {k: torch.from_numpy(v).long().to(pool.device) for k, v in pairs.items()}


def torch_head_and_loss(net, pool, targets):
    fn = torch.nn.functional
    p = torch_pairs(pool, targets)
    f1 = torch.cat([pool[p['intra_p'][:, 0]], pool[p['inter_p'][:, 0]]])
    f2 = torch.cat([pool[p['intra_p'][:, 1]], pool[p['inter_p'][:, 1]]])
    labels1 = torch.cat([p['intra_l'][:, 0], p['inter_l'][:, 0]])
    labels2 = torch.cat([p['intra_l'][:, 1], p['inter_l'][:, 1]])
    m = net.map2(net.drop(net.map1(torch.cat([f1, f2], 1))))
    g1, g2 = torch.sigmoid(m * f1), torch.sigmoid(m * f2)
    parts = [net.fc(net.drop(v)) for v in (g1 * f1 + f1, g2 * f1 + f1, g2 * f2 + f2, g1 * f2 + f2)]    # 1-self, 1-other, 2-self, 2-other
    rows = 2 * f1.shape[0]
    self_logits = torch.zeros(rows, parts[0].shape[1], device=pool.device)
    other_logits = torch.zeros(rows, parts[0].shape[1], device=pool.device)
    self_logits[:rows // 2], self_logits[rows // 2:] = parts[0], parts[2]
    other_logits[:rows // 2], other_logits[rows // 2:] = parts[1], parts[3]
    y = torch.cat([labels1, labels2])
    ce = fn.cross_entropy(torch.cat([self_logits, other_logits]), torch.cat([y, y]), label_smoothing=0.1)
    idx = torch.arange(rows, device=pool.device)
    s, o = torch.softmax(self_logits, 1)[idx, y], torch.softmax(other_logits, 1)[idx, y]
    return ce + fn.margin_ranking_loss(s, o, torch.ones(rows, device=pool.device), margin=0.05)


def kernel_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower():
                names[e.name] = names.get(e.name, 0) + 1
        return names
    except Exception as exc:                            # the count is information; the timing does not depend on it
        print(f'kernel count not available: {exc!r}')
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--samples', type=int, default=40)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('apinet_rows needs an MI355X')
        return 2
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    ours, ref, cap = (G.Step(G.head_only(dev).train(), dev) for _ in range(3))
    case = G.device_case(1, dev)
    for s in (ours, ref, cap):
        s.load(*case)
    cap.capture()

    def run_ours():
        ours.clear()
        ours.run()

    def run_ref():
        ref.clear()
        torch_head_and_loss(ref.net, ref.pool, ref.y).backward()

    variants = {'new_ops': run_ours, 'torch_reference_sequence': run_ref, 'new_ops_graph_replay': cap.replay}
    # eval-mode agreement of the two formulations on the same inputs (the yardstick computes what the kernels compute)
    ours.net.eval(), ref.net.eval()
    ours.clear()
    a = ours.run()
    ref.clear()
    b = torch_head_and_loss(ref.net, ref.pool, ref.y)
    b.backward()
    agree = dict(loss_rel=abs(a.item() - b.item()) / abs(b.item()),
                 dpool_rel=float((ours.pool.grad - ref.pool.grad).norm() / ref.pool.grad.norm()))
    ours.net.train(), ref.net.train()
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.samples):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.calls * 1e6)
    rows = []
    for name, ts in times.items():
        ts.sort()
        names = kernel_launches(variants[name])
        rows.append({'variant': name, 'median_us': round(ts[len(ts) // 2], 1), 'min_us': round(ts[0], 1), 'p90_us': round(ts[int(0.9 * len(ts))], 1),
                     'kernel_launches': None if names is None else sum(names.values()), 'launches_by_kernel': names})
    result = {'shape': {'B': G.N_CLASSES * G.N_SAMPLES, 'D': G.D, 'hidden': G.HIDDEN, 'C': 200}, 'samples': args.samples, 'calls': args.calls,
              'eval_agreement': agree, 'rows': rows}
    if args.step:
        result['model_step'] = model_step(dev)
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    return 0


def model_step(dev, steps=8):
    import hawkeye_amd.model.methods.APINet as plugin
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.loss import APINetLoss
    cfg = CfgNode.load_cfg(open(os.path.join(ROOT, 'configs', 'APINet_synthetic.yaml')))
    net = plugin.APINet(cfg.model).to(dev).train()
    crit = APINetLoss(None)
    opt = torch.optim.Adam(net.parameters(), lr=cfg.train.optimizer.lr, weight_decay=cfg.train.optimizer.weight_decay)
    b = cfg.dataset.n_classes * cfg.dataset.n_samples
    size = cfg.dataset.transformer.image_size
    x = torch.randn(b, 3, size, size, device=dev)
    y = torch.arange(cfg.dataset.n_classes, device=dev).repeat_interleave(cfg.dataset.n_samples)
    ts = []
    for i in range(3 + steps):
        t0 = time.perf_counter()
        opt.zero_grad()
        crit(net(x, y, flag='train'), y).backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {'images': b, 'size': size, 'median_ms': round(ts[len(ts) // 2], 2), 'min_ms': round(ts[0], 2), 'steps': steps}


if __name__ == '__main__':
    sys.exit(main())
