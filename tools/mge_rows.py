"""MGE-CNN's four ops at the yaml's shapes, each next to the reference's op sequence in torch on the same device:

  partpool  (i) mge_partpool; (ii) conv2d(padding=1) + relu + adaptive_max_pool2d(1) - forward alone, and forward + backward to
            the weight and the bias - at B 4, 1024 x 14 x 14 -> 2000 (the yaml) and B 16 at 28 x 28; with the floor
            max(GEMM at 157.3 TF/s, bytes at 6.3 TB/s) of the forward;
  box       (i) mge_cam_bbox + nts_crop_resize; (ii) get_bbox restated in torch (MGE.py:48-72) with its per-image host loop
            (nonzero, min / max, the comparison in an `if`, slice, interpolate), the Grad-CAM weights given to both;
  loss      (i) mge_loss; (ii) ten CrossEntropyLoss(label_smoothing=0.1) calls and their mean - forward + backward;
  gradcam   what the class weights cost before: an eval-mode forward of a ResNet-50 layer4 and the backward of the one-hot sum to
            its output, against the plugin's cost without labels (that forward alone, under no_grad) - with labels it costs nothing.

The two sides are interleaved in one session.  Device events around hipGraph replays where both sides can be captured (21
windows of 20 replays, the median, the minimum and the maximum); the box rows, whose torch side synchronises with the host, on
the host clock around calls ending in a synchronise (21 samples).  Writes the rows as json.

    python tools/mge_rows.py [--out FILE.json]"""
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

from crossx_rows import graph_timed, timed  # noqa: E402

PEAK_F32_MFMA, STREAM_HBM = 157.3e12, 6.3e12
WINDOWS, REPLAYS = 21, 20


def torch_partpool(x, weight, bias):
    return F.adaptive_max_pool2d(F.relu(F.conv2d(x, weight, bias, 1, 1)), 1).flatten(1)


def partpool_piece(HF, dev, b, side):
    import mge_inputs as T
    cin, cout = 1024, 2000
    a = T.pool_arrays((b, cin, cout, side, side), 3)
    x, g = torch.from_numpy(a['x']).to(dev), torch.from_numpy(a['g']).to(dev)
    weight = torch.from_numpy(a['weight']).to(dev).view(cout, cin, 1, 1).requires_grad_(True)
    bias = torch.from_numpy(a['bias']).to(dev).requires_grad_(True)

    def step(fn):
        def run():
            weight.grad = bias.grad = None
            fn(x, weight, bias).backward(g)
            return weight.grad, bias.grad
        return run

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(x, weight, bias)
        return run
    rows = {}
    for tag, wrap in (('fwd', fwd), ('fwd_bwd', step)):
        r = graph_timed({'hip': wrap(HF.mge_partpool), 'torch': wrap(torch_partpool)}, replays=REPLAYS, repeats=WINDOWS)
        rows[tag] = r
    hw = side * side
    flops, nbytes = 2.0 * b * cout * cin * hw, 4.0 * (b * cin * hw + cout * cin + 2 * b * cout)
    rows['fwd_floor_us'] = round(max(flops / PEAK_F32_MFMA, nbytes / STREAM_HBM) * 1e6, 1)
    rows['shape'] = [b, cin, cout, side, side]
    return rows


def torch_get_bbox(x, conv5, layer_weights, rate, img_size):
    """get_bbox's op sequence (MGE.py:48-72), host loop included."""
    b, c = conv5.shape[:2]
    cam = (conv5.detach().view(b, c, -1) * layer_weights.unsqueeze(-1)).sum(1, keepdim=True).view(b, 1, conv5.shape[2], conv5.shape[3])
    up = F.interpolate(cam, size=(img_size, img_size), mode='bilinear', align_corners=True).view(b, -1)
    lo, hi = up.min(-1, keepdim=True)[0], up.max(-1, keepdim=True)[0]
    mask = torch.sign(torch.sign((up - lo) / (hi - lo) - rate) + 1).view(b, 1, img_size, img_size)
    out = torch.zeros_like(x)
    for k in range(b):
        hit = mask[k].nonzero()
        y1, x1 = hit.min(dim=0)[0][-2:]
        y2, x2 = hit.max(dim=0)[0][-2:]
        piece = x[k, :, y1:y2, x1:x2]
        if x1 == x2 or y1 == y2:
            piece = x[k]
        out[k] = F.interpolate(piece.unsqueeze(0), size=(img_size, img_size), mode='bilinear', align_corners=True)
    return out


def box_piece(HF, dev, b=4, s=224):
    import mge_inputs as T
    a = T.cam_arrays((b, 2048, s // 32, s // 32, s), 2)
    conv5, cls, index = (torch.from_numpy(a[k]).to(dev) for k in ('conv5', 'cls_weight', 'index'))
    images = torch.randn(b, 3, s, s, device=dev)
    weights = HF.mge_cam_weights(cls, index, conv5.shape[2] * conv5.shape[3])
    ours = lambda: HF.nts_crop_resize(images, HF.mge_cam_bbox(conv5, cls, index, 0.2, s), 0, s)
    theirs = lambda: torch_get_bbox(images, conv5, weights, 0.2, s)
    err = float((ours() - theirs()).abs().max())
    rows = timed({'hip': ours, 'torch': theirs}, WINDOWS, 10)
    rows['max_abs_difference'] = err
    rows['shape'] = [b, 2048, s // 32, s // 32, s]
    return rows


def loss_piece(HF, dev, k=10, b=4, c=200):
    rs = np.random.RandomState(4)
    logits = [torch.from_numpy((2 * rs.randn(b, c)).astype(np.float32)).to(dev).requires_grad_(True) for _ in range(k)]
    y = torch.from_numpy(rs.randint(0, c, b)).to(dev)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)

    def step(fn):
        def run():
            for t in logits:
                t.grad = None
            fn().backward()
            return [t.grad for t in logits]
        return run

    def ten():
        losses = [crit(t, y) for t in logits]
        return sum(losses) / len(losses)
    rows = graph_timed({'hip': step(lambda: HF.mge_loss(logits, y)), 'torch': step(ten)}, replays=REPLAYS, repeats=WINDOWS)
    rows['shape'] = [k, b, c]
    return rows


def gradcam_piece(dev, b=4, side=14):
    from hawkeye_amd.model.backbone import resnet50
    net = resnet50(pretrained=False).to(dev).eval()
    layer4, fc = net.layer4, torch.nn.Linear(2048, 200).to(dev)
    conv4 = torch.randn(b, 1024, side, side, device=dev)
    index = torch.randint(0, 200, (b,), device=dev)

    def before():
        x = conv4.detach().requires_grad_(True)
        feats = layer4(x)
        out = fc(feats.mean((2, 3)))
        one_hot = torch.zeros_like(out).scatter_(1, index.view(-1, 1), 1.0)
        feats.retain_grad()
        for q in list(layer4.parameters()) + list(fc.parameters()):
            q.grad = None
        (one_hot * out).sum().backward()
        return F.relu(feats.grad).mean((2, 3))

    def now():
        with torch.no_grad():
            return fc(layer4(conv4).mean((2, 3))).argmax(1)
    rows = graph_timed({'reference_forward_backward': before, 'plugin_without_labels': now}, replays=REPLAYS, repeats=WINDOWS)
    rows['plugin_with_labels'] = {'graph_median_us': 0.0}
    rows['shape'] = [b, 1024, side, side]
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mge_rows.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print('mge_rows needs an MI355X')
        sys.exit(2)
    from hawkeye_amd.miopen_cache import use_in_tree_cache
    use_in_tree_cache()
    import hawkeye_amd.functional as HF
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    rows = {'clock': f'device events around {REPLAYS} hipGraph replays, {WINDOWS} windows per side, the sides in turn; box: host clock, {WINDOWS} samples of 10 calls',
            'partpool_yaml': partpool_piece(HF, dev, 4, 14), 'partpool_b16_28': partpool_piece(HF, dev, 16, 28),
            'box_crop': box_piece(HF, dev), 'loss': loss_piece(HF, dev), 'gradcam': gradcam_piece(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    print(json.dumps(rows, indent=1))
