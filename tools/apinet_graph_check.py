"""APINet head on the GPU: hipGraph capture check.

    python tools/apinet_graph_check.py

The head of hawkeye_amd.model.methods.APINet - pair selection, pair gather, map1, map2, the gated interaction, fc - and
APINetLoss behind it are captured, forward plus backward, with torch.cuda.graph on one stream at the yaml's shape
(B = 40, D = 2048, hidden 512, 200 classes) and replayed three times with fresh pooled vectors and labels copied into
the static inputs.  Every replay must be bit-identical to the eager result for the same inputs: the loss, the gradient
at the pooled vectors and the gradients of map1 / fc.  A host synchronisation anywhere in the head - the reference's
pair search copies the distance matrix to the host - would abort the capture.  The module is in eval() for the
comparison (dropout draws differ between a replay and an eager call); a second capture in train() checks that the
device-side mask draw is capturable too and gives finite results.  Exit status 0 when all of that holds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import apinet_inputs as A  # noqa: E402
from graph_capture import Step as _Step, main, replays_match  # noqa: E402

N_CLASSES, N_SAMPLES, D, HIDDEN = A.HEAD_CASES[-1]


def head_only(dev, seed=3):
    """The plugin with an identity trunk: only its head is used here."""
    import hawkeye_amd.model.methods.APINet as plugin
    from hawkeye_amd.config import CfgNode
    real = plugin.resnet101
    plugin.resnet101 = lambda pretrained=True: nn.Sequential(nn.Identity(), nn.Identity(), nn.Identity())
    try:
        net = plugin.APINet(CfgNode(dict(num_classes=A.CLASSES)))
    finally:
        plugin.resnet101 = real
    net.load_state_dict({k: torch.from_numpy(v) for k, v in A.head_weights(seed, D, HIDDEN).items()})
    return net.to(dev)


def device_case(seed, dev):
    x, y = A.head_inputs(seed, N_CLASSES, N_SAMPLES, D)
    return torch.from_numpy(x.mean((2, 3))).to(dev), torch.from_numpy(y).to(dev)


class Step(_Step):
    """Forward + backward of head and loss on static tensors; `capture()` turns it into one graph."""

    def __init__(self, net, dev):
        from hawkeye_amd.model.loss import APINetLoss
        self.net, self.crit = net, APINetLoss(None)
        self.pool = torch.zeros(N_CLASSES * N_SAMPLES, D, device=dev, requires_grad=True)
        self.y = torch.zeros(N_CLASSES * N_SAMPLES, dtype=torch.int64, device=dev)

    def load(self, pool, y):
        with torch.no_grad():
            self.pool.copy_(pool)
            self.y.copy_(y)

    def clear(self):
        self.pool.grad = None
        for p in self.net.parameters():
            p.grad = None

    def run(self):
        out = self.net.head(self.pool, self.y)
        loss = self.crit(out, self.y)
        loss.backward()
        return loss.detach()

    def results(self, loss):
        return [loss, self.pool.grad, self.net.map1.weight.grad, self.net.fc.weight.grad, self.net.fc.bias.grad]


def check(dev):
    names = ('loss', 'dpool', 'map1.weight.grad', 'fc.weight.grad', 'fc.bias.grad')
    if not replays_match(Step(head_only(dev).eval(), dev), Step(head_only(dev).eval(), dev), lambda seed: device_case(seed, dev), names,
                         load=lambda step, case: step.load(*case)):
        return 1
    train = Step(head_only(dev).train(), dev)
    train.load(*device_case(2, dev))
    train.capture()
    first = [t.clone() for t in train.replay()]
    second = train.replay()
    torch.cuda.synchronize()
    if not all(torch.isfinite(t).all() for t in first + second):
        print('train-mode replay: a result is not finite')
        return 1
    if torch.equal(first[1], second[1]):
        print('train-mode replay: two replays drew the same dropout masks')
        return 1
    print('apinet_graph_check ok: 3 replays bit-identical to eager; the train-mode head captures with fresh masks per replay')
    return 0


if __name__ == '__main__':
    main('apinet_graph_check', check)
