"""MGE-CNN head and criterion on the GPU: hipGraph capture check.

    python tools/mge_graph_check.py

What MGE-CNN does around its trunks at the yaml's shapes - the part pool on a [4,1024,14,14] layer-3 map (2000 part
channels), the classifiers on the pooled vectors, the Grad-CAM box from the [4,2048,7,7] layer-4 map with the class taken from
the logits on the device, the crop of the 224 x 224 images, and MGELoss over ten logits tensors forward + backward - is captured
with torch.cuda.graph on one stream and replayed three times with fresh maps, weights and labels copied into the static inputs.
Every replay must be bit-identical to the eager result for the same inputs: the loss, its terms, the boxes, the crops and all
gradients.  A host synchronisation anywhere would abort the capture.  Exit status 0 when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mge_inputs as T  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

B, CIN, PARTS, H, W, FEATURES, CLASSES, S, RATE = 4, 1024, 2000, 14, 14, 2048, 200, 224, 0.2
SHAPES = dict(conv6=(PARTS, CIN, 1, 1), conv6_bias=(PARTS,), cls=(CLASSES, FEATURES), cls_bias=(CLASSES,), cls_part=(CLASSES, PARTS),
              cls_part_bias=(CLASSES,))
INPUTS = dict(conv4=(B, CIN, H, W), conv5=(B, FEATURES, H // 2, W // 2), images=(B, 3, S, S))


def device_case(seed, dev):
    a = T.pool_arrays((B, CIN, PARTS, H, W), seed)
    c = T.cam_arrays((B, FEATURES, H // 2, W // 2, S), seed)
    rs = np.random.RandomState(seed)
    case = dict(conv4=a['x'], conv6=a['weight'].reshape(PARTS, CIN, 1, 1), conv6_bias=a['bias'], conv5=c['conv5'],
                cls=(rs.randn(CLASSES, FEATURES) * 0.05).astype(np.float32), cls_bias=(rs.randn(CLASSES) * 0.1).astype(np.float32),
                cls_part=(rs.randn(CLASSES, PARTS) * 0.05).astype(np.float32), cls_part_bias=(rs.randn(CLASSES) * 0.1).astype(np.float32),
                images=rs.randn(B, 3, S, S).astype(np.float32), y=rs.randint(0, CLASSES, B).astype(np.int64))
    return {name: torch.from_numpy(v).to(dev) for name, v in case.items()}


class Step(_Step):
    def __init__(self, dev):
        import hawkeye_amd.functional as HF
        self.HF = HF
        self.static = {name: torch.zeros(*shape, device=dev).requires_grad_(True) for name, shape in SHAPES.items()}
        self.static.update({name: torch.zeros(*shape, device=dev) for name, shape in INPUTS.items()})
        self.static.update(y=torch.zeros(B, dtype=torch.int64, device=dev))

    def run(self):
        s, HF = self.static, self.HF
        pooled = s['conv5'].mean((2, 3))
        logits = HF.linear(pooled, s['cls'], s['cls_bias'])
        parts = HF.mge_partpool(s['conv4'], s['conv6'], s['conv6_bias'])
        logits_part = HF.linear(parts, s['cls_part'], s['cls_part_bias'])
        boxes = HF.mge_cam_bbox(s['conv5'], s['cls'], logits.detach().argmax(1), RATE, S)
        crops = HF.nts_crop_resize(s['images'], boxes, 0, S)
        total, terms = HF.mge_loss_with_terms([logits, logits_part] * 5, s['y'])
        total.backward()
        return [total.detach(), terms, boxes, crops]

    def results(self, out):
        return out + [self.static[name].grad for name in SHAPES]


NAMES = ('loss', 'loss terms', 'boxes', 'crops') + tuple('d ' + name for name in SHAPES)


def check(dev):
    if not replays_match(Step(dev), Step(dev), lambda seed: device_case(seed, dev), NAMES):
        return 1
    print('mge_graph_check ok: 3 replays bit-identical to eager (part pool, classifiers, Grad-CAM box, crop, loss, forward + backward)')
    return 0


if __name__ == '__main__':
    main('mge_graph_check', check)
