"""NTS-Net head on the GPU: hipGraph capture check.

    python tools/nts_graph_check.py

What NTS-Net does between its trunk passes and after them - proposal scores -> nts_nms -> gather of the chosen scores ->
nts_crop_resize, and NTSLoss forward + backward - is captured with torch.cuda.graph on one stream at the yaml's shape
(B = 4, 426 anchors, 6 proposals, 24 crops of 3 x 224 x 224, 200 classes) and replayed three times with fresh images,
scores, logits and labels copied into the static inputs.  Every replay must be bit-identical to the eager result for
the same inputs: indices, boxes, chosen scores, the crops, the loss terms and all four gradients.  A host
synchronisation anywhere - the reference copies the scores to the host and calls .item() per part row - would abort
the capture.  Exit status 0 when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nts_inputs as T  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

B, N, C, SIZE = 4, 6, 200, 224


def device_case(seed, anchors, dev):
    rs = np.random.RandomState(seed)
    raw, cat, part, _, y = T.loss_inputs(seed, B, N, C)
    return dict(images=torch.from_numpy(T.model_images(seed, B, SIZE)).to(dev),
                scores=torch.from_numpy(T.nms_scores(seed, B, 'random', anchors) + rs.rand(B, 1).astype(np.float32)).to(dev),
                raw=torch.from_numpy(raw).to(dev), cat=torch.from_numpy(cat).to(dev), part=torch.from_numpy(part).to(dev),
                y=torch.from_numpy(y).to(dev))


class Step(_Step):
    """The head on static tensors; `capture()` turns it into one graph."""

    def __init__(self, anchors, dev):
        import hawkeye_amd.functional as HF
        self.HF = HF
        self.anchors = torch.from_numpy(anchors - 224).to(dev)
        z = lambda *s: torch.zeros(*s, device=dev)
        self.static = dict(images=z(B, 3, SIZE, SIZE), scores=z(B, len(anchors)).requires_grad_(True), raw=z(B, C).requires_grad_(True),
                           cat=z(B, C).requires_grad_(True), part=z(B, N, C).requires_grad_(True), y=torch.zeros(B, dtype=torch.int64, device=dev))

    def run(self):
        s = self.static
        index, boxes = self.HF.nts_nms(s['scores'], self.anchors, N, T.IOU)
        prob = torch.gather(s['scores'], 1, index)
        crops = self.HF.nts_crop_resize(s['images'], boxes, 224, SIZE)
        total, parts = self.HF.nts_loss_with_parts(s['raw'], s['cat'], s['part'], prob, s['y'])
        total.backward()
        return [index, boxes, prob.detach(), crops, total.detach(), parts]

    def results(self, out):
        s = self.static
        return out + [s['scores'].grad, s['raw'].grad, s['cat'].grad, s['part'].grad]


NAMES = ('index', 'boxes', 'top_n_prob', 'crops', 'loss', 'loss terms', 'd scores', 'd raw', 'd concat', 'd part')


def check(dev):
    anchors = T.load()['anchors_224']
    if not replays_match(Step(anchors, dev), Step(anchors, dev), lambda seed: device_case(seed, anchors, dev), NAMES,
                         nonempty=('d scores', 'crops')):
        return 1
    print('nts_graph_check ok: 3 replays bit-identical to eager (nms, gather, crops, loss forward + backward)')
    return 0


if __name__ == '__main__':
    main('nts_graph_check', check)
