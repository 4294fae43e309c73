"""Writes the MGE-CNN fixtures under tests/golden/: the reference's own GradCam outputs (its autograd path) for a seeded short
model and the reference trainer's ten-criterion loss on the golden loss cases of tests/mge_inputs.py, in float32 and float64
(mge_ops.npz); one whole-model case of a short-trunk LocalCamNet in eval mode and one train-mode step with y=None
(mge_model.npz); and the reference model's state_dict keys (mge_state_dict.json).

    python tools/gen_mge_golden.py [--reference DIR] [--check]

The reference is imported at run time on the CPU; nothing of it is copied.  Inputs and weights are stored as recipes only.

What needs care.
  * model/methods/__init__.py imports every method and with them torchvision, which is not installed: `import torchvision`
    resolves to oracle/_stubs.
  * LocalCamNet asks its backbone for downloaded weights.  `MGE.resnet50` is rebound, before anything is constructed, to a
    function that builds the reference's own ResNet(Bottleneck, short layers) with pretrained=False: the download path never runs.
    The short trunk keeps three blocks in layer4, since Grad-CAM's target layer is the block named "2".
  * The boxes never leave LocalCamNet.forward and GradCam's class index is chosen inside it: `MGE.get_bbox` and `MGE.GradCam` are
    wrapped in this process to record what they return.
  * The train-mode gradients are taken with torch.autograd.grad, so the one-hot gradients that GradCam leaves in `.grad` during the
    forward are not in them.
A model seed is accepted only where the float32 and float64 runs agree on every argmax and every box.  The archives have fixed
zip timestamps (--check compares instead of writing)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mge_inputs as T  # noqa: E402
from inputs import seeded_init  # noqa: E402
from gen_apinet_golden import to_bytes  # noqa: E402

KEYS_FILE = 'mge_state_dict.json'
MAX_BYTES = 1 << 20


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
    M = importlib.import_module('model.methods.MGE_CNN.MGE')
    R = importlib.import_module('model.backbone.resnet')
    M.resnet50 = lambda pretrained=False, **kw: R.ResNet(R.Bottleneck, list(T.MODEL_CASE['layers']))     # never the hub
    return M


class Recorder:
    """Wraps MGE.get_bbox and MGE.GradCam for one forward."""

    def __init__(self, M):
        self.M, self.boxes, self.cams = M, [], []

    def __enter__(self):
        M, rec = self.M, self
        self.saved = (M.get_bbox, M.GradCam)
        get_bbox, GradCam = self.saved

        def recording_bbox(x, conv5, layer_weights, rate=0.3, img_size=448):
            out, xy = get_bbox(x, conv5, layer_weights, rate=rate, img_size=img_size)
            rows = []
            for x1, x2, y1, y2 in xy:
                x1, x2, y1, y2 = int(x1), int(x2), int(y1), int(y2)
                rows.append([0, 0, img_size, img_size] if x1 == x2 or y1 == y2 else [y1, x1, y2, x2])
            rec.boxes.append(np.array(rows, dtype=np.int32))
            return out, xy

        class RecordingGradCam(GradCam):
            def __call__(self, input, index=None):
                weights = GradCam.__call__(self, input, index)
                was = self.model.training                  # the map's size, and the class GradCam chose: its own eval-mode logits again
                self.model.eval()
                with torch.no_grad():
                    feats = input
                    for module in self.extractor.feature_extractor.feature_extractor._modules.values():
                        feats = module(feats)
                    if index is None:
                        index = torch.argmax(self.model.classifier(self.model.pool(feats).flatten(1)), dim=-1)
                self.model.train(was)
                rec.cams.append((weights.numpy().copy(), np.asarray(index).astype(np.int64), int(feats.shape[2] * feats.shape[3])))
                return weights
        M.get_bbox, M.GradCam = recording_bbox, RecordingGradCam
        return self

    def __exit__(self, *exc):
        self.M.get_bbox, self.M.GradCam = self.saved
        return False


def short_model(M, dtype=torch.float32):
    c = T.MODEL_CASE
    net = M.MGE_CNN(Cfg(num_classes=c['classes'], box_thred=c['box_thred'], image_size=c['size']))
    seeded_init(net, c['init_seed'])
    return net.to(dtype)


def state_dict_keys(M):
    net = short_model(M)
    extractor = {id(q) for q in net.get_params('extractor')}
    names = {id(q): n for n, q in net.named_parameters()}
    return {'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()], 'children': [n for n, _ in net.named_children()],
            'n_params': sum(q.numel() for q in net.parameters()),
            'extractor': [names[id(q)] for q in net.get_params('extractor')],
            'classifier': [names[id(q)] for q in net.get_params('classifier')], 'n_extractor': len(extractor)}


def run_model(M, images, mode, dtype, y=None):
    net = short_model(M, dtype).train(mode == 'train')
    x = torch.from_numpy(images).to(dtype)
    with Recorder(M) as rec:
        if mode == 'eval':
            with torch.no_grad():
                out = net(x, y)
        else:
            out = net(x, y)
    res = dict(logits=[t.detach().numpy() for t in out['logits']], pr_gate=out['pr_gate'].detach().numpy(), boxes=rec.boxes, cams=rec.cams,
               cls_weight=net.classifier.fc.weight.detach().numpy().copy())
    if mode == 'train':                                    # Examples/MGE_CNN.py:43-45
        crit = torch.nn.CrossEntropyLoss(label_smoothing=T.SMOOTHING)
        labels = torch.tensor(T.MODEL_CASE['labels'])
        losses = [crit(t, labels) for t in out['logits']]
        loss = sum(losses) / len(losses)
        params = dict(net.named_parameters())
        grads = torch.autograd.grad(loss, [params[n] for n in T.TRAIN_GRADS])
        res['loss'] = loss.detach().numpy()
        res['grads'] = {n: g.numpy() for n, g in zip(T.TRAIN_GRADS, grads)}
    return res


def build_model(M):
    c = T.MODEL_CASE
    for seed in range(c['init_seed'] + 1, c['init_seed'] + 17):
        images = T.model_images(seed, c['B'], c['size'])
        runs, ok = {}, True
        for mode in ('eval', 'train'):
            for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
                runs[mode, prec] = run_model(M, images, mode, dtype)
            a, b = runs[mode, 'f32'], runs[mode, 'f64']
            ok = ok and all(np.array_equal(p, q) for p, q in zip(a['boxes'], b['boxes']))
            ok = ok and all(p.argmax(1).tolist() == q.argmax(1).tolist() for p, q in zip(a['logits'] + [a['pr_gate']], b['logits'] + [b['pr_gate']]))
            ok = ok and all(np.array_equal(p[1], q[1]) for p, q in zip(a['cams'], b['cams']))
            ok = ok and any((bx != np.array([0, 0, c['size'], c['size']])).any() for bx in b['boxes'])     # a real box somewhere
        print(f'model seed {seed}: {"accepted" if ok else "rejected"}; boxes {[bx.tolist() for bx in runs["eval", "f64"]["boxes"]]}')
        if ok:
            break
    else:
        raise RuntimeError('model case: no seed meets the conditions')
    arrays = dict(model_recipe=np.array([seed, c['B'], c['size'], c['init_seed']], dtype=np.int64))
    for (mode, prec), r in runs.items():
        if mode == 'eval':
            for i, t in enumerate(r['logits']):
                arrays[f'eval_logits{i}_{prec}'] = t
            arrays[f'eval_pr_gate_{prec}'] = r['pr_gate']
        else:
            arrays[f'train_loss_{prec}'] = r['loss']
            for n, g in r['grads'].items():
                arrays[f'train_grad_{n}_{prec}'] = T.grad_sample(g)
    for mode in ('eval', 'train'):
        for k, bx in enumerate(runs[mode, 'f64']['boxes']):
            arrays[f'{mode}_boxes{k + 1}'] = bx
    return arrays


def build_ops(M):
    """GradCam's own outputs, both calls, y given and y=None, from the float32 eval-mode short model; and the golden loss cases."""
    c = T.MODEL_CASE
    images = T.model_images(c['init_seed'] + 1, c['B'], c['size'])
    out = {}
    for tag, y in (('given', torch.tensor(c['labels'])), ('none', None)):
        r = run_model(M, images, 'eval', torch.float32, y)
        assert len(r['cams']) == 2
        for k, (weights, index, hw) in enumerate(r['cams']):
            stem = f'cam_{tag}_{k + 1}'
            out[stem + '_weights'], out[stem + '_index'], out[stem + '_hw'] = weights, index, np.int64(hw)
        out['cam_cls_weight'] = r['cls_weight']
    for case in T.LOSS_GOLDEN_CASES:
        logits, labels = T.loss_arrays(case)
        stem = 'loss_' + T.loss_case_id(case)
        for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            r = T.loss_reference(logits, labels, dtype)
            out[f'{stem}_loss_{prec}'], out[f'{stem}_grads_{prec}'] = r['loss'], np.stack(r['grads'])
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    M = load_reference(args.reference)
    blobs = {'mge_ops.npz': to_bytes(build_ops(M)), 'mge_model.npz': to_bytes(build_model(M)),
             KEYS_FILE: (json.dumps(state_dict_keys(M)) + '\n').encode()}
    same = True
    for name, blob in blobs.items():
        assert len(blob) <= MAX_BYTES, (name, len(blob))
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
