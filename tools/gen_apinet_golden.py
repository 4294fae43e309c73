"""Writes the APINet fixtures under tests/golden/: the reference's head (model/methods/APINet.py) and criterion
(model/loss/APINet_loss.py) on the cases of tests/golden/apinet_inputs.py in float32 and float64, the reference model's
state_dict keys, and one whole-model case.

    python tools/gen_apinet_golden.py [--reference DIR] [--check]

The reference is imported at run time (with oracle/_stubs in front for the packages it imports and does not use here);
nothing of it is copied.  Files: apinet_head.npz (the small head cases, and the float32 gradient of the yaml-sized
one), apinet_head_yaml.npz (logits and losses of the 10 x 4, D = 2048 case), apinet_head_yaml_grad.npz (its float64
gradient), apinet_model.npz (whole model) and apinet_state_dict.json.  Inputs and weights are stored as recipes only.

Head cases run a head-only instance (identity trunk, own map1 / map2 / fc) in eval() with flag='train': dropout is the
identity.  Per case k: `h{k}_recipe` = seed, classes, samples, D, hidden; `h{k}_partner` [2B]; `h{k}_labels1/2`;
`h{k}_active` (rows whose rank term is positive); and with `_f32` / `_f64`: `h{k}_self_logits`, `h{k}_other_logits`,
`h{k}_loss` (total, CE, rank), `h{k}_dpool` = 49 x d loss / d x at any map position (checked to be the same at all 49).

The float64 run is made under torch.set_default_dtype(torch.float64): the reference writes its logits into zeros() of
the default dtype.  A seed is accepted only if rounding cannot flip the selection - in float64 every row's gap between
its best and second-best candidate distance is at least 2e-5 x max_i |pool_i|^2 (intra and inter separately, rows with
two candidates or more), no rank term is closer than 1e-5 to zero, and the reference's own get_pairs on its float32 run
selects the same partners (and its float32 run the same active rows); the yaml-sized case must also have active and
inactive rank rows.  Otherwise the next seed is tried.  The archives have fixed zip timestamps: the same inputs give the
same bytes (--check compares instead of writing)."""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
import apinet_inputs as A  # noqa: E402
from inputs import seeded_init  # noqa: E402

GAP = 2e-5
HINGE = 1e-5
KEYS_FILE = 'apinet_state_dict.json'


def load_reference(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
    import importlib
    importlib.import_module('model.methods.APINet')
    M = sys.modules['model.methods.APINet']            # the module (the package re-exports the class under the same name)
    from model.loss.APINet_loss import APINetLoss
    return M, APINetLoss


def head_only(M, d, hidden, weights, dtype):
    ref = M.APINet.__new__(M.APINet)
    nn.Module.__init__(ref)
    ref.num_classes = A.CLASSES
    ref.backbone = nn.Identity()
    ref.avg = nn.AvgPool2d(kernel_size=A.MAP, stride=1)
    ref.map1, ref.map2, ref.fc = nn.Linear(2 * d, hidden), nn.Linear(hidden, d), nn.Linear(d, A.CLASSES)
    ref.drop, ref.sigmoid, ref.device = nn.Dropout(p=0.5), nn.Sigmoid(), None
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return ref.to(dtype).eval()


def loss_terms(crit, out):
    """total from the reference's call; CE and rank from its own member modules applied as APINet_loss.py:29-38 does."""
    self_logits, other_logits, labels1, labels2 = out
    total = crit(out, None)
    y = torch.cat([labels1, labels2])
    ce = crit.ce_loss(torch.cat([self_logits, other_logits]), torch.cat([y, y]))
    rows = torch.arange(y.numel())
    s, o = crit.softmax_layer(self_logits)[rows, y], crit.softmax_layer(other_logits)[rows, y]
    rank = crit.rank_loss(s, o, torch.ones_like(s))
    return total, ce, rank, (o - s + 0.05).detach()


def run_head(M, crit_cls, x, y, weights, d, hidden, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        ref = head_only(M, d, hidden, weights, dtype)
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        out = ref(xt, torch.from_numpy(y), flag='train')
        assert out[0].dtype == dtype and out[1].dtype == dtype, (out[0].dtype, dtype)
        total, ce, rank, hinge = loss_terms(crit_cls(None), out)
        total.backward()
    finally:
        torch.set_default_dtype(old)
    dx = xt.grad.numpy()
    dpool = dx[:, :, 0, 0] * (A.MAP * A.MAP)
    assert np.abs(dx - dx[:, :, :1, :1]).max() <= 1e-6 * np.abs(dx).max()           # the same at all 49 positions
    with torch.no_grad():                               # the reference's own selection on this run's pooled vectors, in this dtype
        pairs = ref.get_pairs(ref.avg(xt.detach()).squeeze(), torch.from_numpy(y))
    own = torch.cat([pairs[0][:, 1], pairs[1][:, 1]]).numpy()
    assert np.array_equal(pairs[0][:, 0].numpy(), np.arange(x.shape[0])) and np.array_equal(pairs[1][:, 0].numpy(), np.arange(x.shape[0]))
    return dict(self_logits=out[0].detach().numpy(), other_logits=out[1].detach().numpy(),
                loss=np.array([total.item(), ce.item(), rank.item()], dtype=np.float32 if dtype == torch.float32 else np.float64),
                dpool=dpool, labels1=out[2].numpy(), labels2=out[3].numpy(), hinge=hinge.numpy(), partner=own)


def partners_and_gaps(pool, y):
    """float64: partner [2B] by the reference's rules from exact squared distances, and the smallest relative gap."""
    pool = pool.astype(np.float64)
    b = pool.shape[0]
    dist = ((pool[:, None, :] - pool[None, :, :]) ** 2).sum(-1)
    scale = (pool ** 2).sum(1).max()
    same = y[:, None] == y[None, :]
    eye = np.eye(b, dtype=bool)
    partner, gap = np.zeros(2 * b, dtype=np.int64), np.inf
    for half, mask in enumerate((same & ~eye, ~same)):
        for i in range(b):
            cand = np.where(mask[i])[0]
            if len(cand) == 0:
                continue
            order = np.sort(dist[i, cand])
            partner[half * b + i] = cand[np.argmin(dist[i, cand])]
            if len(cand) > 1:
                gap = min(gap, (order[1] - order[0]) / scale)
    return partner, gap


def build_head(M, crit_cls):
    out = {}
    for k, (n_classes, n_samples, d, hidden) in enumerate(A.HEAD_CASES):
        b = n_classes * n_samples
        for seed in range(100 * k, 100 * k + 100):
            x, y = A.head_inputs(seed, n_classes, n_samples, d)
            partner, gap = partners_and_gaps(x.astype(np.float64).mean((2, 3)), y)
            if gap < GAP:
                continue
            w = A.head_weights(seed, d, hidden, x, y)
            r64 = run_head(M, crit_cls, x, y, w, d, hidden, torch.float64)
            r32 = run_head(M, crit_cls, x, y, w, d, hidden, torch.float32)
            assert np.array_equal(r64['labels1'], np.concatenate([y, y])) and np.array_equal(r64['labels2'], y[partner])
            assert np.array_equal(r64['partner'], partner)                            # the reference's float64 get_pairs
            active = r64['hinge'] > 0
            ok = np.abs(r64['hinge']).min() >= HINGE and np.array_equal(r32['partner'], partner) and \
                np.array_equal(r32['hinge'] > 0, active)                              # ... and its float32 get_pairs and active rows
            if k == len(A.HEAD_CASES) - 1:
                ok = ok and 0 < active.sum() < active.size                            # the yaml case: rank rows on both sides
            if ok:
                break
        else:
            raise RuntimeError(f'head case {k}: no seed meets the margins')
        out[f'h{k}_recipe'] = np.array([seed, n_classes, n_samples, d, hidden], dtype=np.int64)
        out[f'h{k}_partner'] = partner
        out[f'h{k}_labels1'], out[f'h{k}_labels2'] = r64['labels1'], r64['labels2']
        out[f'h{k}_active'] = r64['hinge'] > 0
        for prec, r in (('f32', r32), ('f64', r64)):
            for name in A.RESULTS:
                out[f'h{k}_{name}_{prec}'] = r[name]
        d32 = {name: A.distance(r32[name], r64[name]) for name in ('self_logits', 'dpool')}
        print(f'head case {k}: {n_classes}x{n_samples} D {d} H {hidden}: seed {seed}, gap {gap:.2e}, active {int((r64["hinge"] > 0).sum())}'
              f'/{4 * b}, loss {r64["loss"]}, fp32 distance logits {d32["self_logits"]:.1e} dpool {d32["dpool"]:.1e}')
    out['head_cases'] = np.array(len(A.HEAD_CASES), dtype=np.int64)
    return out


def build_model(M, crit_cls):
    """The whole model: weights from tests/golden/inputs.py:seeded_init on both sides (not stored), B = 4 at 224 x 224,
    flag='train' in eval mode and flag='val'; float32 and float64 (logits, the three loss terms, every 4th x 16th
    element of fc's weight gradient, every 16th x 64th of map1's, and the two gradients' norms)."""
    from yacs.config import CfgNode as CN
    real = M.resnet101
    M.resnet101 = lambda pretrained=True: real(pretrained=False)
    try:
        net = M.APINet(CN(dict(num_classes=A.CLASSES)))
    finally:
        M.resnet101 = real
    keys = {'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()],
            'children': [n for n, _ in net.named_children()], 'n_params': sum(p.numel() for p in net.parameters())}
    c = A.MODEL_CASE
    seeded_init(net, c['init_seed'])
    net.eval()
    b = c['classes'] * c['samples']
    for seed in range(c['init_seed'] + 1, c['init_seed'] + 41):
        images, y = A.model_images(seed, c['classes'], c['samples'], c['size'])
        xt = torch.from_numpy(images)
        with torch.no_grad():
            pool = net.avg(net.backbone(xt)).squeeze().double().numpy()
        partner, gap = partners_and_gaps(pool, y)
        if gap >= GAP:
            break
    else:
        raise RuntimeError('model case: no seed meets the margin')
    arrays = dict(model_recipe=np.array([seed, c['classes'], c['samples'], c['size'], c['init_seed']], dtype=np.int64),
                  model_partner=partner, model_pool=pool.astype(np.float32))
    for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)                # the reference's zeros() buffers take the default dtype
        try:
            net.to(dtype)
            xd = xt.to(dtype)
            out = net(xd, torch.from_numpy(y), flag='train')
            assert out[0].dtype == dtype
            total, ce, rank, hinge = loss_terms(crit_cls(None), out)
            g_fc, g_map1 = torch.autograd.grad(total, [net.fc.weight, net.map1.weight])
            with torch.no_grad():
                val = net(xd, flag='val')
        finally:
            torch.set_default_dtype(old)
            net.float()
        assert np.array_equal(out[3].numpy(), y[partner]) and np.abs(hinge.numpy()).min() >= HINGE
        arrays['model_labels1'], arrays['model_labels2'] = out[2].numpy(), out[3].numpy()
        arrays.update({f'model_self_logits_{prec}': out[0].detach().numpy(), f'model_other_logits_{prec}': out[1].detach().numpy(),
                       f'model_val_logits_{prec}': val.numpy(), f'model_loss_{prec}': np.array([total.item(), ce.item(), rank.item()]),
                       f'model_fc_grad_{prec}': g_fc.numpy()[::4, ::16].copy(), f'model_map1_grad_{prec}': g_map1.numpy()[::16, ::64].copy(),
                       f'model_grad_norms_{prec}': np.array([g_fc.norm().item(), g_map1.norm().item()], dtype=np.float64)})
    for name in ('self_logits', 'val_logits', 'fc_grad', 'map1_grad', 'grad_norms'):
        print(f'  model {name}: fp32 distance from fp64 {A.distance(arrays[f"model_{name}_f32"], arrays[f"model_{name}_f64"]):.2e}')
    print(f'model case: seed {seed}, gap {gap:.2e}, partner {partner.tolist()}, loss {arrays["model_loss_f64"]}')
    return arrays, keys


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


def split(head, model):
    """Which array goes into which file (every file stays below the largest fixture already in tests/golden/)."""
    big = len(A.HEAD_CASES) - 1
    files = {name: {} for name in A.FILES}
    for key, value in head.items():
        if key == f'h{big}_dpool_f64':
            files['apinet_head_yaml_grad.npz'][key] = value
        elif key.startswith(f'h{big}_') and key != f'h{big}_dpool_f32':
            files['apinet_head_yaml.npz'][key] = value
        else:
            files['apinet_head.npz'][key] = value
    files['apinet_model.npz'] = model
    return files


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    M, crit_cls = load_reference(args.reference)
    model, keys = build_model(M, crit_cls)
    blobs = {name: to_bytes(arrays) for name, arrays in split(build_head(M, crit_cls), model).items()}
    blobs[KEYS_FILE] = (json.dumps(keys) + '\n').encode()
    same = True
    for name, blob in blobs.items():
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
