"""DCL head on the GPU: hipGraph capture check.

    python tools/dcl_graph_check.py

What DCL does around its trunk - the swap law of a uint8 batch (dcl_swap_law), the head on the last map (dcl_head on a
[2B,2048,14,14] map), the two classifiers and DCLLoss forward + backward - is captured with torch.cuda.graph on one
stream at the yaml's shape (B = 8 images and their swapped copies, 200 classes, a 7 x 7 grid) and replayed three times
with fresh images, maps, weights and labels copied into the static inputs.  Every replay must be bit-identical to the
eager result for the same inputs: the law, the four loss terms and all five gradients.  A host synchronisation anywhere
would abort the capture.  Exit status 0 when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dcl_inputs as T  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

B, K, SIDE, GRID = 8, 200, 448, (7, 7)
SHAPES = dict(x=(2 * B, 2048, 14, 14), w=(1, 2048, 1, 1), bias=(1,), cls=(K, 2048), swap=(2, 2048))


def device_case(seed, dev):
    rs = np.random.RandomState(seed)
    case = {name: torch.from_numpy((rs.randn(*shape) * (0.02 if name != 'x' else 1.0)).astype(np.float32)).to(dev) for name, shape in SHAPES.items()}
    img = T.smooth_image(rs, SIDE, SIDE, cells=14)
    un = np.stack([np.roll(img, 7 * i, axis=0) for i in range(B)])
    sw = np.stack([T.permute_patches(u, rs.permutation(49), GRID) for u in un])
    case.update(un=torch.from_numpy(un).to(dev), sw=torch.from_numpy(sw).to(dev), y=torch.from_numpy(np.repeat(rs.randint(0, K, B), 2)).to(dev),
                ys=torch.from_numpy(np.tile([1, 0], B)).to(dev))
    return case


class Step(_Step):
    """The head on static tensors; `capture()` turns it into one graph (its warm-up also uploads the patch bounds)."""

    def __init__(self, dev):
        import hawkeye_amd.functional as HF
        from hawkeye_amd.data import dcl_law_ramp
        self.HF = HF
        self.static = {name: torch.zeros(*shape, device=dev).requires_grad_(True) for name, shape in SHAPES.items()}
        self.static.update(un=torch.zeros(B, SIDE, SIDE, 3, dtype=torch.uint8, device=dev), sw=torch.zeros(B, SIDE, SIDE, 3, dtype=torch.uint8, device=dev),
                           y=torch.zeros(2 * B, dtype=torch.int64, device=dev), ys=torch.zeros(2 * B, dtype=torch.int64, device=dev))
        self.ramp = dcl_law_ramp(GRID[0] * GRID[1]).to(dev)

    def run(self):
        s, HF = self.static, self.HF
        law2, index = HF.dcl_swap_law(s['un'], s['sw'], GRID)
        law = torch.stack([self.ramp.expand_as(law2), law2], 1).reshape(2 * B, -1)
        pooled, mask = HF.dcl_head(s['x'], s['w'], s['bias'])
        total, terms = HF.dcl_loss_with_terms(HF.linear(pooled, s['cls']), HF.linear(pooled, s['swap']), mask, s['y'], s['ys'], law, *T.COEF)
        total.backward()
        return [index, total.detach(), terms]

    def results(self, out):
        return out + [self.static[name].grad for name in SHAPES]


NAMES = ('law index', 'loss', 'loss terms') + tuple('d ' + name for name in SHAPES)


def check(dev):
    def permutation(got):
        if sorted(got[0][0].tolist()) != list(range(49)):
            return 'the law of a patch permutation is no permutation'

    if not replays_match(Step(dev), Step(dev), lambda seed: device_case(seed, dev), NAMES, extra=permutation):
        return 1
    print('dcl_graph_check ok: 3 replays bit-identical to eager (swap law, head, two classifiers, loss, forward + backward)')
    return 0


if __name__ == '__main__':
    main('dcl_graph_check', check)
