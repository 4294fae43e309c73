"""Peer-learning loss on the GPU: hipGraph capture check and the timing table of DESIGN.md section 3.11.

    python tools/peer_graph_check.py                 # capture forward + backward at 64 x 200, replay three times
    python tools/peer_graph_check.py --time [--out FILE.json]

Check: forward plus backward of hawkeye_amd.functional.peer_learning_loss is captured with torch.cuda.graph on one
stream and replayed three times with fresh logits copied into the static inputs; every replay must be bit-identical to
the eager result for the same logits.  A host synchronisation inside the call would abort the capture.  Exit status 0
when all of that holds.

--time: at (8, 200), (16, 200), (64, 200), forward + backward of (a) the torch-op composition of the loss (softmax,
argmax, nonzero, gathers, argsort, cat, cross entropy - the reference's formulation), (b) the general form (peer_form 1),
(c) the resident form (peer_form 2), (d) the replay of the captured graph.  Median over 60 samples of 20 calls each, the
variants taken in turn, each sample ending in a device synchronise."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import hawkeye_amd.functional as HF  # noqa: E402
from graph_capture import Step, main, replays_match  # noqa: E402
from hawkeye_amd import _lib  # noqa: E402
from peer_inputs import peer_inputs  # noqa: E402


def aten_peer_loss(logits_1, logits_2, labels, drop_rate):
    """The loss as a composition of torch ops, formulated as model/loss/peer_learning_loss.py:5-65 formulates it:
    boolean-index gathers of the agreeing / disagreeing rows (host synchronisations), argsort of the agreeing rows' cross
    entropies, the crossed low-loss subsets concatenated behind the disagreeing rows, mean cross entropy of each."""
    ce = torch.nn.functional.cross_entropy
    pred_1 = torch.softmax(logits_1, 1).argmax(1)
    pred_2 = torch.softmax(logits_2, 1).argmax(1)
    dis = (pred_1 != pred_2).nonzero().squeeze(1)
    agr = (pred_1 == pred_2).nonzero().squeeze(1)
    a1, a2, ay = logits_1[agr], logits_2[agr], labels[agr]
    d1, d2, dy = logits_1[dis], logits_2[dis], labels[dis]
    if agr.shape[0] > 0:
        keep = int((1 - drop_rate) * agr.shape[0])
        by_1 = torch.argsort(ce(a1, ay, reduction='none').detach())[:keep]
        by_2 = torch.argsort(ce(a2, ay, reduction='none').detach())[:keep]
        f1, y1 = torch.cat((d1, a1[by_2])), torch.cat((dy, ay[by_2]))
        f2, y2 = torch.cat((d2, a2[by_1])), torch.cat((dy, ay[by_1]))
    else:
        f1, y1, f2, y2 = d1, dy, d2, dy
    return ce(f1, y1), ce(f2, y2)


def device_case(seed, n, c, dev):
    l1, l2, y = peer_inputs(seed, n, c, 'mixed')
    return torch.from_numpy(l1).to(dev), torch.from_numpy(l2).to(dev), torch.from_numpy(y).to(dev)


def eager(l1, l2, y, drop_rate, loss_fn=None):
    a, b = l1.clone().requires_grad_(True), l2.clone().requires_grad_(True)
    loss_1, loss_2 = (loss_fn or HF.peer_learning_loss)(a, b, y, drop_rate)
    (loss_1 + loss_2).backward()
    return loss_1.detach(), loss_2.detach(), a.grad, b.grad


class PeerStep(Step):
    """Forward + backward of the loss on static tensors; `capture()` turns it into one graph."""

    def __init__(self, n, c, drop_rate, dev):
        self.static = dict(l1=torch.zeros(n, c, device=dev, requires_grad=True), l2=torch.zeros(n, c, device=dev, requires_grad=True),
                           y=torch.zeros(n, dtype=torch.int64, device=dev))
        self.drop_rate = drop_rate

    def run(self):
        s = self.static
        loss_1, loss_2 = HF.peer_learning_loss(s['l1'], s['l2'], s['y'], self.drop_rate)
        (loss_1 + loss_2).backward()
        return [loss_1.detach(), loss_2.detach()]

    def results(self, out):
        return out + [self.static['l1'].grad, self.static['l2'].grad]


def check(dev):
    n, c, drop_rate = 64, 200, 0.35
    case = lambda seed: dict(zip(('l1', 'l2', 'y'), device_case(seed, n, c, dev)))      # noqa: E731
    if not replays_match(PeerStep(n, c, drop_rate, dev), PeerStep(n, c, drop_rate, dev), case, ('loss_1', 'loss_2', 'dl1', 'dl2')):
        return 1
    print('peer_graph_check ok: 3 replays bit-identical to eager')
    return 0


def timing(dev, out):
    calls, samples, drop_rate = 20, 60, 0.35
    rows = []
    for n, c in ((8, 200), (16, 200), (64, 200)):
        case = device_case(100 + n, n, c, dev)
        cap = PeerStep(n, c, drop_rate, dev)
        cap.load(dict(zip(('l1', 'l2', 'y'), case)))
        cap.capture()

        fused = lambda: eager(*case, drop_rate)                                           # noqa: E731
        variants = {'aten_us': (0, lambda: eager(*case, drop_rate, aten_peer_loss)), 'general_us': (1, fused),
                    'resident_us': (2, fused), 'graph_replay_us': (0, cap.replay)}
        times = {k: [] for k in variants}
        for form, fn in variants.values():
            with _lib.tuning(peer_form=form):
                for _ in range(10):
                    fn()
        torch.cuda.synchronize()
        for _ in range(samples):
            for name, (form, fn) in variants.items():
                with _lib.tuning(peer_form=form):                     # the knob is set outside the timed window
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / calls * 1e6)
        row = {'N': n, 'C': c}
        for name, ts in times.items():
            ts.sort()
            row[name] = round(ts[len(ts) // 2], 2)
            row[name.replace('_us', '_min_us')] = round(ts[0], 2)
        # the kernels alone: the C ABI on preallocated buffers, no autograd, no allocation
        lib = _lib.load()
        l1, l2, y = case[0].contiguous(), case[1].contiguous(), case[2].to(torch.int32)
        loss = torch.empty(2, device=dev)
        dl1, dl2 = torch.empty_like(l1), torch.empty_like(l2)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        nws = lib.hk_peer_loss_ws_bytes(n, c)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        abi = {}
        for form in (1, 2):
            with _lib.tuning(peer_form=form):
                def call():
                    _lib.check(lib.hk_peer_loss(_lib.ptr(l1), _lib.ptr(l2), _lib.ptr(y), drop_rate, _lib.ptr(loss), _lib.ptr(dl1),
                                                _lib.ptr(dl2), _lib.ptr(stats), n, c, _lib.ptr(ws), nws, _lib.stream()), 'hk_peer_loss')
                for _ in range(20):
                    call()
                torch.cuda.synchronize()
                ts = []
                for _ in range(samples):
                    t0 = time.perf_counter()
                    for _ in range(200):
                        call()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) / 200 * 1e6)
                ts.sort()
                abi[form] = round(ts[len(ts) // 2], 2)
        row['abi_general_us'], row['abi_resident_us'] = abi[1], abi[2]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    main('peer_graph_check', lambda device: timing(device, args.out) if args.time else check(device))
