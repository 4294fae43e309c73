"""CrossX head on the GPU: hipGraph capture check.

    python tools/crossx_graph_check.py

What CrossX does between its trunk's convolutions and the loss gradient - the two multi-excitation block tails
(crossx_me on a [B,1024,28,28] and a [B,2048,14,14] map), the combined branch's upsample + add and squeeze, and
CrossXLoss forward + backward - is captured with torch.cuda.graph on one stream at the yaml's shape (B = 8, P = 2,
200 classes) and replayed three times with fresh maps, gates, logits and labels copied into the static inputs.  The
1 x 1 convolution between the layer4 parts and the add is stood in for by the first 1024 channels.  Every replay must be
bit-identical to the eager result for the same inputs: the six loss terms and all nine gradients.  A host
synchronisation anywhere - the reference copies 3 P^2 correlations to the host - would abort the capture.  Exit status 0
when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import crossx_inputs as T  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

B, P, K = 8, 2, 200
SHAPES = dict(out3=(B, 1024, 28, 28), res3=(B, 1024, 28, 28), gates3=(P, B, 1024), out4=(B, 2048, 14, 14), res4=(B, 2048, 14, 14),
              gates4=(P, B, 2048), ulti=(B, K), plty=(B, K), cmbn=(B, K))


def device_case(seed, dev):
    rs = np.random.RandomState(seed)
    case = {}
    for name, shape in SHAPES.items():
        a = rs.randn(*shape).astype(np.float32)
        case[name] = torch.from_numpy(1 / (1 + np.exp(-a)) if name.startswith('gates') else a).to(dev)
    case['y'] = torch.from_numpy(rs.randint(0, K, B)).to(dev)
    return case


class Step(_Step):
    """The head on static tensors; `capture()` turns it into one graph."""

    def __init__(self, dev):
        import hawkeye_amd.functional as HF
        self.HF = HF
        self.static = {name: torch.zeros(*shape, device=dev).requires_grad_(True) for name, shape in SHAPES.items()}
        self.static['y'] = torch.zeros(B, dtype=torch.int64, device=dev)

    def run(self):
        s, HF = self.static, self.HF
        _, parts3, pool3 = HF.crossx_me(s['out3'], s['res3'], s['gates3'], 'max')
        _, parts4, pool4 = HF.crossx_me(s['out4'], s['res4'], s['gates4'], 'avg')
        cmbn = torch.stack([HF.osme_gap(HF.crossx_up_add(parts3[i], parts4[i][:, :1024])) for i in range(P)])
        total, terms = HF.crossx_loss_with_terms(s['ulti'], s['plty'], s['cmbn'], pool4, pool3, cmbn, s['y'], T.GAMMA)
        total.backward()
        return [total.detach(), terms]

    def results(self, out):
        return out + [self.static[name].grad for name in SHAPES]


NAMES = ('loss', 'loss terms') + tuple('d ' + name for name in SHAPES)


def check(dev):
    if not replays_match(Step(dev), Step(dev), lambda seed: device_case(seed, dev), NAMES):
        return 1
    print('crossx_graph_check ok: 3 replays bit-identical to eager (two ME blocks, upsample + add, loss, forward + backward)')
    return 0


if __name__ == '__main__':
    main('crossx_graph_check', check)
