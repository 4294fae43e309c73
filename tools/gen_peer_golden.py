"""Writes tests/golden/peer_loss.npz: the reference's PeerLearningLoss (model/loss/peer_learning_loss.py:5-65) on the
cases of tests/golden/peer_inputs.py, run in float32 and in float64, with both logit gradients.

    python tools/gen_peer_golden.py [--reference DIR] [--check]

The reference's loss file is loaded by path (it needs only torch; the package around it imports yacs).  Per case k the
archive holds the recipe (`c{k}_recipe` = seed, N, C and `c{k}_drop_rate`, `c{k}_mode`; the tensors come from
peer_inputs.peer_inputs), `c{k}_loss_f32` [2], `c{k}_dl1_f32`, `c{k}_dl2_f32` and the same with `_f64`, and from the
float64 run `c{k}_n`, `c{k}_m`, `c{k}_keep1`, `c{k}_keep2` (a row is kept by a net when the reference's gradient for it
is not zero).

A seed is accepted only when float32 rounding cannot flip a prediction or a selection, so that the masks can be compared
exactly: every top-1 margin and the gap between the m-th and (m+1)-th smallest agreeing cross entropy are at least 1e-3
in both nets, and a mixed case has 0.25 N <= n <= 0.85 N.  Otherwise the next seed is tried.  The archive is written with
fixed zip timestamps: the same inputs give the same bytes (--check compares instead of writing)."""
import argparse
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import peer_inputs  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'peer_loss.npz')
MARGIN = 1e-3


def load_reference_loss(ref_root):
    path = os.path.join(ref_root, 'model', 'loss', 'peer_learning_loss.py')
    spec = importlib.util.spec_from_file_location('_reference_peer_learning_loss', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PeerLearningLoss


def run_reference(loss_fn, l1, l2, y, drop_rate, dtype):
    a = torch.from_numpy(l1).to(dtype).requires_grad_(True)
    b = torch.from_numpy(l2).to(dtype).requires_grad_(True)
    loss_1, loss_2 = loss_fn(a, b, torch.from_numpy(y), drop_rate)
    loss_1.backward()                                            # Examples/PeerLearning.py:86-87
    loss_2.backward()
    g1 = a.grad if a.grad is not None else torch.zeros_like(a)
    g2 = b.grad if b.grad is not None else torch.zeros_like(b)
    return (torch.stack([loss_1.detach(), loss_2.detach()]).numpy(), g1.numpy(), g2.numpy())


def margins_ok(l1, l2, y, drop_rate, mode):
    """(ok, n, m) from a float64 restatement of the selection's inputs: top-1 margins and the gap at the cut."""
    n_rows = l1.shape[0]
    ces, preds = [], []
    for l in (l1.astype(np.float64), l2.astype(np.float64)):
        srt = np.sort(l, axis=1)
        if (srt[:, -1] - srt[:, -2]).min() < MARGIN:
            return False, 0, 0
        preds.append(l.argmax(1))
        mx = l.max(1, keepdims=True)
        ces.append(np.log(np.exp(l - mx).sum(1)) + mx[:, 0] - l[np.arange(n_rows), y])
    agree = preds[0] == preds[1]
    n = int(agree.sum())
    m = int((1 - drop_rate) * n)
    if mode == 'mixed' and not (0.25 * n_rows <= n <= 0.85 * n_rows):
        return False, n, m
    if mode == 'agree' and n != n_rows:
        return False, n, m
    if mode == 'disagree' and n != 0:
        return False, n, m
    if 0 < m < n:
        for ce in ces:
            s = np.sort(ce[agree])
            if s[m] - s[m - 1] < MARGIN:
                return False, n, m
    return True, n, m


def build(ref_root):
    loss_fn = load_reference_loss(ref_root)
    out = {}
    for k, (n_rows, c, drop_rate, mode) in enumerate(peer_inputs.CASES):
        for seed in range(100 * k, 100 * k + 100):
            l1, l2, y = peer_inputs.peer_inputs(seed, n_rows, c, mode)
            ok, n, m = margins_ok(l1, l2, y, drop_rate, mode)
            if ok:
                break
        else:
            raise RuntimeError(f'case {k}: no seed meets the margins')
        loss32, a32, b32 = run_reference(loss_fn, l1, l2, y, drop_rate, torch.float32)
        loss64, a64, b64 = run_reference(loss_fn, l1, l2, y, drop_rate, torch.float64)
        keep1, keep2 = (a64 != 0).any(1), (b64 != 0).any(1)
        agree = l1.argmax(1) == l2.argmax(1)
        assert np.array_equal(keep1 | agree, np.ones(n_rows, bool)) and int(keep1.sum()) == n_rows - n + m == int(keep2.sum())
        assert np.array_equal((a32 != 0).any(1), keep1) and np.array_equal((b32 != 0).any(1), keep2)   # float32 selects the same rows
        out[f'c{k}_recipe'] = np.array([seed, n_rows, c], dtype=np.int64)
        out[f'c{k}_drop_rate'] = np.array(drop_rate, dtype=np.float64)
        out[f'c{k}_mode'] = np.array(mode)
        out[f'c{k}_loss_f32'], out[f'c{k}_dl1_f32'], out[f'c{k}_dl2_f32'] = loss32, a32, b32
        out[f'c{k}_loss_f64'], out[f'c{k}_dl1_f64'], out[f'c{k}_dl2_f64'] = loss64, a64, b64
        out[f'c{k}_n'], out[f'c{k}_m'] = np.array(n, dtype=np.int64), np.array(m, dtype=np.int64)
        out[f'c{k}_keep1'], out[f'c{k}_keep2'] = keep1, keep2
        print(f'case {k}: N {n_rows} C {c} drop {drop_rate} {mode}: seed {seed}, n {n}, m {m}, loss {loss64}')
    out['cases'] = np.array(len(peer_inputs.CASES), dtype=np.int64)
    return out


def to_bytes(arrays):
    """An .npz (np.load reads it) with fixed member timestamps: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue(), compresslevel=9)
    return buf.getvalue()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', '/root/reference'))
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    blob = to_bytes(build(args.reference))
    if args.check:
        same = open(OUT, 'rb').read() == blob
        print('identical' if same else 'DIFFERENT', OUT)
        sys.exit(0 if same else 1)
    with open(OUT, 'wb') as f:
        f.write(blob)
    print(f'wrote {OUT} ({len(blob)} bytes)')
