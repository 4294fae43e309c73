"""Writes the NTS-Net fixtures under tests/golden/: the reference's anchor tables and hard_nms
(model/methods/NTS_Net/anchors.py), its pad + slice + F.interpolate crop (NTSNet.py:31,43-47), its criterion
(model/loss/NTS_loss.py) and one whole-model case, on the cases of tests/golden/nts_inputs.py in float32 and float64,
plus the reference model's state_dict keys.

    python tools/gen_nts_golden.py [--reference DIR] [--check]

The reference is imported at run time (with oracle/_stubs in front for the packages it imports and does not use here);
nothing of it is copied.  Files: nts_ops.npz (anchor tables, NMS, crop and loss cases), nts_model.npz (whole model) and
nts_state_dict.json.  Inputs and weights are stored as recipes only.

The reference model is never constructed with pretrained=True (that would ask model_zoo for a download): the instance
is made with __new__ + nn.Module.__init__ and the reference's own resnet50(pretrained=False), ProposalNet and anchor
generator, then filled by tests/golden/inputs.py:seeded_init.  Shims, in this process only: np.int = int (numpy 2),
Tensor.cuda as the identity, torch.cuda.FloatTensor = torch.FloatTensor, and for the whole-model run an identity in
place of nn.Dropout (the reference's trunk builds a fresh, always active Dropout in every forward).

A seed is accepted only if (1) the reference's float32 and float64 runs choose the same proposals / the same
indicators, (2) every compared gap - a chosen anchor's score above the best live rival, two part losses of one sample -
is at least 16 x the largest float32-versus-float64 difference of that quantity in the case, and (3) no hinge argument
is closer to zero than 1e-5; loss cases from (3, 6, 200) up must have active and inactive hinge terms behind a true
indicator.  Otherwise the next seed is tried.  The archives have fixed zip timestamps (--check compares instead of
writing)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nts_inputs as T  # noqa: E402
from inputs import seeded_init  # noqa: E402
from gen_apinet_golden import to_bytes  # noqa: E402

GAP = 16.0
HINGE = 1e-5
KEYS_FILE = 'nts_state_dict.json'


def load_reference(ref_root):
    np.int = int                                            # anchors.py, NTSNet.py (numpy < 1.24 spelling)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
    import importlib
    M = importlib.import_module('model.methods.NTS_Net.NTSNet')
    L = importlib.import_module('model.loss.NTS_loss')
    return M, L


def anchor_table(M, size):
    _, edge, _ = M.generate_default_anchor_maps(input_shape=(size, size))
    return (edge + 224).astype(np.int)


def build_nms(M):
    out = {}
    tables = {size: anchor_table(M, size) for size in (224, 448)}
    for size, table in tables.items():
        out[f'anchors_{size}'] = table.astype(np.int32)
    for k, (size, b, kind) in enumerate(T.NMS_CASES):
        anchors = tables[size]
        seed = 300 + k
        scores = T.nms_scores(seed, b, kind, anchors)
        index, boxes = [], []
        for row in scores:
            # as NTSNet.py:35-37 builds it: float32 scores next to integer columns make a float64 table
            cdds = np.concatenate((row.reshape(-1, 1), anchors.copy(), np.arange(len(row)).reshape(-1, 1)), axis=1)
            assert cdds.dtype == np.float64
            top = M.hard_nms(cdds, topn=T.TOPN, iou_thresh=T.IOU)
            assert top.shape == (T.TOPN, 6)
            own, gaps = T.nms_trace(row, anchors)
            assert np.array_equal(own, top[:, -1].astype(np.int64)) and gaps.min() > 0
            index.append(top[:, -1].astype(np.int64))
            boxes.append(top[:, 1:5].astype(np.int32))
        index, boxes = np.stack(index), np.stack(boxes)
        if kind == 'quarter':                               # the winner's exact-quarter partners hold the next scores and are gone
            for i, row in enumerate(scores):
                partners = T.quarter_partners(anchors, index[i, 0])
                assert len(partners) >= 2 and not np.isin(partners, index[i]).any()
                assert set(np.argsort(-row)[1:1 + len(partners)]) == set(partners)
        if kind == 'overlap':
            assert all(np.argsort(-row)[1] not in index[i] for i, row in enumerate(scores))
        out[f'n{k}_recipe'] = np.array([seed, size, b], dtype=np.int64)
        out[f'n{k}_index'], out[f'n{k}_boxes'] = index, boxes
        print(f'nms case {k}: {size} B {b} {kind}: index {index.tolist()}')
    return out


def build_crop():
    out = {}
    for k, c in enumerate(T.CROP_CASES):
        seed = 400 + k
        images = T.crop_images(seed, c['B'], c['C'], c['H'], c['W'])
        pad = c['pad']
        for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            x = torch.from_numpy(images).to(dtype)
            x_pad = F.pad(x, (pad, pad, pad, pad), mode='constant', value=0)
            parts = torch.zeros([c['B'], c['N'], c['C'], *c['out']], dtype=dtype)
            for i in range(c['B']):
                for j in range(c['N']):
                    y0, x0, y1, x1 = (int(v) + pad for v in T.CROP_BOXES[i][j])
                    assert y0 >= 0 and x0 >= 0                # a negative start would wrap in the slice
                    parts[i:i + 1, j] = F.interpolate(x_pad[i:i + 1, :, y0:y1, x0:x1], size=c['out'], mode='bilinear', align_corners=True)
            out[f'c{k}_out_{prec}'] = parts.view(c['B'] * c['N'], c['C'], *c['out']).numpy()
        out[f'c{k}_recipe'] = np.array([seed], dtype=np.int64)
        print(f'crop case {k}: out {c["out"]}: fp32 distance from fp64 {T.distance(out[f"c{k}_out_f32"], out[f"c{k}_out_f64"]):.2e}')
    return out


def run_loss(L, raw, cat, part, prob, y, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                          # ranking_loss starts from zeros(1) of the default dtype
    try:
        b, n, c = part.shape
        crit = L.NTSLoss(type('Cfg', (), {'proposal_num': n})())
        t = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (raw, cat, part, prob)]
        yt = torch.from_numpy(y)
        total = crit([t[0], t[1], t[2], None, t[3]], yt)
        total.backward()
        with torch.no_grad():                               # the terms, from the reference's members in the order it calls them
            yy = yt.unsqueeze(1).repeat(1, n).view(-1)
            part_loss = crit.list_loss(t[2].view(b * n, -1), yy).view(b, n)
            raw_loss = crit.ce_loss(t[0], yt)
            cat_loss = crit.ce_loss(t[1], yt)
            rank_loss = crit.rank_loss(t[3], part_loss, n)
            partcls_loss = crit.ce_loss(t[2].view(b * n, -1), yy)
    finally:
        torch.set_default_dtype(old)
    assert total.dtype == dtype and rank_loss.dtype == dtype
    pl, s = part_loss.numpy(), t[3].detach().numpy()
    indicator = pl[:, None, :] > pl[:, :, None]             # [b, i, j]: part_loss_bj > part_loss_bi
    hinge = 1 - s[:, :, None] + s[:, None, :]
    return dict(loss=np.array([total.item(), raw_loss.item(), cat_loss.item(), partcls_loss.item(), rank_loss.item()],
                              dtype=np.float32 if dtype == torch.float32 else np.float64),
                draw=t[0].grad.numpy(), dconcat=t[1].grad.numpy(), dpart=t[2].grad.numpy(), dprob=t[3].grad.numpy(),
                part_loss=pl, indicator=indicator, hinge=hinge)


def min_gap(v):
    """Smallest distance between two entries of one row of v [b, n]."""
    s = np.sort(np.asarray(v, dtype=np.float64), axis=1)
    return np.diff(s, axis=1).min() if s.shape[1] > 1 else np.inf


def build_loss(L):
    out = {}
    for k, (b, n, c) in enumerate(T.LOSS_CASES):
        for seed in range(500 + 100 * k, 600 + 100 * k):
            inputs = T.loss_inputs(seed, b, n, c)
            r64, r32 = run_loss(L, *inputs, torch.float64), run_loss(L, *inputs, torch.float32)
            off = ~np.eye(n, dtype=bool)[None]
            ok = np.array_equal(r32['indicator'], r64['indicator'])
            ok = ok and min_gap(r64['part_loss']) >= GAP * np.abs(r32['part_loss'] - r64['part_loss']).max()
            ok = ok and np.abs(r64['hinge'][np.broadcast_to(off, r64['hinge'].shape)]).min() >= HINGE
            ok = ok and np.array_equal(r32['hinge'] > 0, r64['hinge'] > 0)
            gated = r64['hinge'][r64['indicator']]
            if b * n >= 18:
                ok = ok and (gated > 0).any() and (gated <= 0).any()
            if ok:
                break
        else:
            raise RuntimeError(f'loss case {k}: no seed meets the margins')
        out[f'l{k}_recipe'] = np.array([seed, b, n, c], dtype=np.int64)
        out[f'l{k}_indicator'] = r64['indicator']
        for prec, r in (('f32', r32), ('f64', r64)):
            for name in T.LOSS_RESULTS:
                out[f'l{k}_{name}_{prec}'] = r[name]
        print(f'loss case {k}: B {b} N {n} C {c}: seed {seed}, active {int((gated > 0).sum())}/{gated.size} gated hinges, loss {r64["loss"]}, '
              f'fp32 distance dpart {T.distance(r32["dpart"], r64["dpart"]):.1e} rank {T.distance(r32["loss"][4], r64["loss"][4]):.1e}')
    return out


class _NoDropout(nn.Module):
    def __init__(self, *a, **k):
        super().__init__()

    def forward(self, x):
        return x


def reference_model(M, cfg):
    ref = M.NTSNet.__new__(M.NTSNet)
    nn.Module.__init__(ref)
    ref.topN = ref.proposal_num = cfg['proposal_num']
    ref.CAT_NUM = cfg['cat_num']
    ref.image_size = cfg['size']
    ref.pretrained_model = M.resnet50(pretrained=False)
    ref.pretrained_model.avgpool = nn.AdaptiveAvgPool2d(1)
    ref.pretrained_model.fc = nn.Linear(512 * 4, 200)
    ref.proposal_net = M.ProposalNet()
    ref.concat_net = nn.Linear(2048 * (ref.CAT_NUM + 1), 200)
    ref.partcls_net = nn.Linear(512 * 4, 200)
    ref.pad_side = 224
    ref.edge_anchors = anchor_table(M, cfg['size'])
    return ref


def build_model(M):
    c = T.MODEL_CASE
    net = reference_model(M, c)
    keys = {'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()],
            'children': [n for n, _ in net.named_children()], 'n_params': sum(p.numel() for p in net.parameters())}
    seeded_init(net, c['init_seed'])
    net.eval()
    real = nn.Dropout
    nn.Dropout = _NoDropout
    try:
        for seed in range(c['init_seed'] + 1, c['init_seed'] + 9):
            images = T.model_images(seed, c['B'], c['size'])
            runs = {}
            for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
                old = torch.get_default_dtype()
                torch.set_default_dtype(dtype)              # part_imgs is zeros() of the default dtype
                try:
                    net.to(dtype)
                    with torch.no_grad():
                        out = net(torch.from_numpy(images).to(dtype))
                        score = net.proposal_net(net.pretrained_model(torch.from_numpy(images).to(dtype))[1])
                finally:
                    torch.set_default_dtype(old)
                    net.float()
                assert out[0].dtype == dtype
                runs[prec] = dict(raw_logits=out[0].numpy(), concat_logits=out[1].numpy(), part_logits=out[2].numpy(),
                                  top_n_index=out[3].numpy(), top_n_prob=out[4].numpy(), score=score.numpy())
            s32, s64 = runs['f32']['score'], runs['f64']['score']
            traces = [T.nms_trace(row, net.edge_anchors, c['proposal_num']) for row in s64]
            gap = min(t[1].min() for t in traces)
            noise = np.abs(s32 - s64).max()
            ok = np.array_equal(runs['f32']['top_n_index'], runs['f64']['top_n_index']) and gap >= GAP * noise and \
                np.array_equal(np.stack([t[0] for t in traces]), runs['f64']['top_n_index'])
            print(f'model seed {seed}: score gap {gap:.2e}, fp32 score noise {noise:.2e}, index {runs["f64"]["top_n_index"].tolist()}: '
                  f'{"accepted" if ok else "rejected"}')
            if ok:
                break
        else:
            raise RuntimeError('model case: no seed meets the margins')
    finally:
        nn.Dropout = real
    arrays = dict(model_recipe=np.array([seed, c['B'], c['size'], c['init_seed']], dtype=np.int64), model_top_n_index=runs['f64']['top_n_index'])
    for prec in ('f32', 'f64'):
        for name in ('raw_logits', 'concat_logits', 'part_logits', 'top_n_prob'):
            arrays[f'model_{name}_{prec}'] = runs[prec][name]
    for name in ('raw_logits', 'concat_logits', 'part_logits', 'top_n_prob'):
        print(f'  model {name}: fp32 distance from fp64 {T.distance(arrays[f"model_{name}_f32"], arrays[f"model_{name}_f64"]):.2e}')
    return arrays, keys


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    M, L = load_reference(args.reference)
    ops = {**build_nms(M), **build_crop(), **build_loss(L)}
    model, keys = build_model(M)
    blobs = {'nts_ops.npz': to_bytes(ops), 'nts_model.npz': to_bytes(model), KEYS_FILE: (json.dumps(keys) + '\n').encode()}
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if f.endswith('.npz') and not f.startswith('nts_'))
    same = True
    for name, blob in blobs.items():
        assert len(blob) <= largest, (name, len(blob), largest)
        path = os.path.join(GOLDEN, name)
        if args.check:
            ok = os.path.isfile(path) and open(path, 'rb').read() == blob
            print('identical' if ok else 'DIFFERENT', path)
            same = same and ok
        else:
            with open(path, 'wb') as f:
                f.write(blob)
            print(f'wrote {path} ({len(blob)} bytes)')
    sys.exit(0 if same else 1)
