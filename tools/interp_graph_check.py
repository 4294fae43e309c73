"""InterpParts head and criterion on the GPU: hipGraph capture check.

    python tools/interp_graph_check.py

What InterpParts does around its trunk and tail - the grouping unit on the layer-3 map (ip_group on a [16,1024,28,28] map,
5 parts), a classifier on the pooled region features and InterpPartsLoss forward + backward at the yaml's parameters - is
captured with torch.cuda.graph on one stream and replayed three times with fresh maps, weights and labels copied into the
static inputs.  Every replay must be bit-identical to the eager result for the same inputs: the three loss terms and all
five gradients.  A host synchronisation anywhere would abort the capture.  Exit status 0 when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import interp_inputs as T  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

N, C, K, H, W, CLASSES = 16, 1024, 5, 28, 28, 200
SHAPES = dict(x=(N, C, H, W), weight=(K, C, 1, 1), smooth=(K,), cls=(CLASSES, C), cls_bias=(CLASSES,))
CRITERION = dict(radius=2, std=0.4, alpha=1.0, beta=0.001, coeff=0.5)


def device_case(seed, dev):
    a = T.group_arrays(seed, (N, C, K, H, W))
    rs = np.random.RandomState(seed)
    case = dict(x=a['x'], weight=a['weight'].reshape(K, C, 1, 1), smooth=a['smooth'], cls=(rs.randn(CLASSES, C) * 0.05).astype(np.float32),
                cls_bias=(rs.randn(CLASSES) * 0.1).astype(np.float32), y=rs.randint(0, CLASSES, N).astype(np.int64))
    return {name: torch.from_numpy(v).to(dev) for name, v in case.items()}


class Step(_Step):
    """The head and the criterion on static tensors; `capture()` turns them into one graph (its warm-up also makes the window
    and the prior, once)."""

    def __init__(self, dev):
        import hawkeye_amd.functional as HF
        self.HF = HF
        self.static = {name: torch.zeros(*shape, device=dev).requires_grad_(True) for name, shape in SHAPES.items()}
        self.static.update(y=torch.zeros(N, dtype=torch.int64, device=dev))

    def run(self):
        s, HF = self.static, self.HF
        outputs_t, assign = HF.ip_group(s['x'], s['weight'], s['smooth'])
        logits = HF.linear(outputs_t.sum(2), s['cls'], s['cls_bias'])
        total, terms = HF.ip_loss_with_terms(logits, assign, s['y'], **CRITERION)
        total.backward()
        return [total.detach(), terms]

    def results(self, out):
        return out + [self.static[name].grad for name in SHAPES]


NAMES = ('loss', 'loss terms') + tuple('d ' + name for name in SHAPES)


def check(dev):
    if not replays_match(Step(dev), Step(dev), lambda seed: device_case(seed, dev), NAMES):
        return 1
    print('interp_graph_check ok: 3 replays bit-identical to eager (grouping unit, classifier, loss, forward + backward)')
    return 0


if __name__ == '__main__':
    main('interp_graph_check', check)
