"""CrossX's head at the yaml's shapes (B = 8, P = 2, 448 x 448 images: a [8,1024,28,28] and a [8,2048,14,14] map, 200
classes), piece by piece, forward + backward, on one device in one process:

  me3    the layer3 multi-excitation tail with its max pools: (i) crossx_me; (ii) the reference's sequence in torch
         (CrossX.py:109-119, 225): a clone, P broadcast multiplies, P + 1 adds, P + 1 ReLUs, P adaptive max pools;
  me4    the same for the layer4 tail with average pools;
  up_add (i) crossx_up_add; (ii) F.interpolate(b, 28) + torch.add (CrossX.py:213-223), P times;
  loss   (i) crossx_loss; (ii) the reference's criterion restated in torch (CrossX_loss.py:13-64): the P x P matrix
         filled on the host, entry by entry; its device-to-host copies are counted.

(ii) is a yardstick only; nothing in the package calls it.  Every variant is forward + backward with fixed upstream
gradients.  Two clocks.  `median_us` / `min_us` / `p90_us`: host-clock time per call over `--samples` samples of `--calls`
eager calls, each sample ending in a device synchronise, the two variants of a piece taken in turn after a warm-up - for
work this short it is mostly the host's cost of enqueueing (Python, ctypes, the allocator).  `graph_*_us`: the same
call captured into a hipGraph and replayed between two device events - the device's time without the host; the
reference's loss cannot be captured (it copies to the host), so it has the host clock only.  For the ME pieces the bytes
the fused forward + backward must move (every operand once) over the graph time is reported as achieved bandwidth.

    python tools/crossx_rows.py [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, P, K = 8, 2, 200
GAMMA = (0.5, 0.25, 0.5)
PEAK_HBM = 8.0e12           # bytes / s, MI355X


def torch_me(out, res, gates, pool):
    outreach = out.clone()
    parts = [outreach * gates[p].view(*gates.shape[1:], 1, 1) for p in range(gates.shape[0])]
    main = torch.relu(out + res)
    parts = [torch.relu(part + res) for part in parts]
    pooled = [(F.adaptive_max_pool2d if pool == 'max' else F.adaptive_avg_pool2d)(part, 1) for part in parts]
    return main, parts, pooled


copies = [0]


def torch_regular(x, gamma):
    p = len(x)
    corr = torch.zeros(p, p)                                # on the host, as RegularLoss makes it
    x = [torch.div(v.squeeze(), v.squeeze().norm(dim=1, keepdim=True)) for v in x]
    for i in range(p):
        for j in range(p):
            corr[i, j] = torch.mean(torch.mm(x[i], x[j].t()))
            copies[0] += 1
            if i == j:
                corr[i, j] = 1.0 - corr[i, j]
    return torch.mul(torch.sum(torch.triu(corr)), gamma).to(x[0].device)


def torch_loss(ulti, plty, cmbn, fu, fp, fc, y):
    cls = F.cross_entropy(ulti + plty + cmbn, y, label_smoothing=0.1)
    regs = torch_regular(fc, GAMMA[2]), torch_regular(fu, GAMMA[0]), torch_regular(fp, GAMMA[1])
    target = F.softmax(ulti, 1)
    kl = (F.kl_div(F.log_softmax(plty, 1), target, reduction='sum') + F.kl_div(F.log_softmax(cmbn, 1), target, reduction='sum')) / y.size(0)
    return regs[1] + regs[2] + regs[0] + kl + cls


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


def graph_timed(variants, replays=50, repeats=9):
    """Device time without the host: each variant captured into a hipGraph once, then `repeats` windows of `replays`
    replays between two device events, the variants taken in turn."""
    graphs, keep = {}, {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in variants.values():
            for _ in range(3):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for name, fn in variants.items():
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            keep[name] = fn()
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / replays * 1e3)
    rows = {}
    for name, ts in times.items():
        ts.sort()
        rows[name] = {'graph_median_us': round(ts[len(ts) // 2], 1), 'graph_min_us': round(ts[0], 1), 'graph_max_us': round(ts[-1], 1)}
    return rows


def merge(rows, more):
    for name, r in more.items():
        rows[name].update(r)
    return rows


def me_piece(HF, dev, c, side, pool, use_main, samples, calls):
    rs = np.random.RandomState(c)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(dev)
    out, res, gates = t(B, c, side, side).requires_grad_(True), t(B, c, side, side).requires_grad_(True), torch.sigmoid(t(P, B, c)).requires_grad_(True)
    d_main, d_parts, d_pooled = t(B, c, side, side), t(P, B, c, side, side), t(P, B, c)

    def fused():
        main, parts, pooled = HF.crossx_me(out, res, gates, pool)
        outs, grads = [parts, pooled], [d_parts, d_pooled]
        if use_main:
            outs, grads = outs + [main], grads + [d_main]
        return torch.autograd.grad(outs, [out, res, gates], grads)

    def yardstick():
        main, parts, pooled = torch_me(out, res, gates, pool)
        outs = parts + pooled + ([main] if use_main else [])
        grads = [d_parts[p] for p in range(P)] + [d_pooled[p].view(B, c, 1, 1) for p in range(P)] + ([d_main] if use_main else [])
        return torch.autograd.grad(outs, [out, res, gates], grads)
    a, b = fused(), yardstick()
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    rows = merge(timed({'fused': fused, 'torch_sequence': yardstick}, samples, calls), graph_timed({'fused': fused, 'torch_sequence': yardstick}))
    maps = B * c * side * side * 4
    # forward: out, res read, main and P parts written; backward: out, main, P parts, P part gradients (and the main one) read, d_out and d_res written
    moved = maps * (2 + 1 + P) + maps * (2 + 2 * P + (1 if use_main else 0) + 2)
    rows['fused']['bytes_moved'] = moved
    rows['fused']['achieved_TBps'] = round(moved / (rows['fused']['graph_median_us'] * 1e-6) / 1e12, 3)
    rows['fused']['share_of_hbm_peak'] = round(moved / (rows['fused']['graph_median_us'] * 1e-6) / PEAK_HBM, 3)
    rows['max_relative_gradient_difference'] = worst
    return rows


def up_piece(HF, dev, samples, calls):
    rs = np.random.RandomState(5)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(dev)
    a = [t(B, 1024, 28, 28).requires_grad_(True) for _ in range(P)]
    b = [t(B, 1024, 14, 14).requires_grad_(True) for _ in range(P)]
    g = t(B, 1024, 28, 28)
    fused = lambda: [torch.autograd.grad(HF.crossx_up_add(a[i], b[i]), [a[i], b[i]], g) for i in range(P)]
    yardstick = lambda: [torch.autograd.grad(torch.add(a[i], F.interpolate(b[i], 28)), [a[i], b[i]], g) for i in range(P)]
    return merge(timed({'fused': fused, 'torch_sequence': yardstick}, samples, calls), graph_timed({'fused': fused, 'torch_sequence': yardstick}))


def loss_piece(HF, dev, samples, calls):
    rs = np.random.RandomState(9)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32)).to(dev)
    logits = [t(B, K).requires_grad_(True) for _ in range(3)]
    feats = [t(P, B, c).abs().add(0.1).requires_grad_(True) for c in (2048, 1024, 1024)]
    y = torch.from_numpy(rs.randint(0, K, B)).to(dev)
    lists = lambda: [[f[i].view(B, -1, 1, 1) for i in range(P)] for f in feats]
    fused = lambda: torch.autograd.grad(HF.crossx_loss(*logits, *lists(), y, GAMMA), logits + feats)
    yardstick = lambda: torch.autograd.grad(torch_loss(*logits, *lists(), y), logits + feats)
    a, b = fused(), yardstick()
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    copies[0] = 0
    yardstick()
    per_call = copies[0]
    rows = timed({'fused': fused, 'torch_sequence': yardstick}, samples, calls)
    rows['fused'].update(graph_timed({'fused': fused})['fused'])           # the yardstick cannot be captured: it copies to the host
    rows['fused']['host_copies_per_call'] = 0
    rows['torch_sequence']['host_copies_per_call'] = per_call
    rows['max_relative_gradient_difference'] = worst
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('crossx_rows needs an MI355X: nothing is measured without one')
        sys.exit(2)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    import hawkeye_amd.functional as HF
    result = {'shape': {'B': B, 'P': P, 'K': K, 'image': 448}, 'samples': args.samples, 'calls_per_sample': args.calls,
              'device': torch.cuda.get_device_name(0), 'unit': 'microseconds per forward + backward call: host clock around eager calls, and device events around hipGraph replays (graph_*)'}
    result['me3_max'] = me_piece(HF, dev, 1024, 28, 'max', True, args.samples, args.calls)
    result['me4_avg'] = me_piece(HF, dev, 2048, 14, 'avg', False, args.samples, args.calls)
    result['up_add'] = up_piece(HF, dev, args.samples, args.calls)
    result['loss'] = loss_piece(HF, dev, args.samples, args.calls)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
