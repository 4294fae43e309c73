"""What the plugin heads' hipGraph capture checks share (tools/{peer,apinet,nts,crossx,dcl}_graph_check.py): a step on
static tensors that `capture()` turns into one graph, the comparison of three replays with eager runs on the same
inputs, and the command line's entry.  Each tool adds its shapes, its case generator, its static tensors and its run()."""
import sys

import torch


class Step:
    """A head on static tensors.  A subclass fills `self.static` (name -> tensor; the leaves require grad), gives `run()`
    (forward + backward; returns what it computed) and `results(out)` (that and the gradients, as one list)."""
    graph = None

    def load(self, case):
        with torch.no_grad():
            for k, v in case.items():
                self.static[k].copy_(v)

    def clear(self):
        for t in self.static.values():
            t.grad = None

    def capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # warm-up off the capture
            for _ in range(3):
                self.clear()
                self.run()
        torch.cuda.current_stream().wait_stream(side)
        self.clear()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self.run()

    def replay(self):
        self.graph.replay()
        return self.results(self.out)


def replays_match(cap, eager, case, names, nonempty=None, load=Step.load, extra=None):
    """`cap` is captured once on case(1); then for three seeds the replay on case(seed) must equal `eager`'s run on it bit
    for bit, every floating-point result finite and the results named in `nonempty` (default: all of `names`) not all
    zero.  load(step, case) copies a case into a step's static tensors; extra(got) may return a further complaint.
    Prints what fails and returns False, True otherwise."""
    load(cap, case(1))
    cap.capture()
    for seed in (11, 12, 13):
        inputs = case(seed)
        load(eager, inputs)
        eager.clear()
        want = [t.clone() for t in eager.results(eager.run())]
        load(cap, inputs)
        got = cap.replay()
        torch.cuda.synchronize()
        for name, w, g in zip(names, want, got):
            if not torch.equal(w, g) or (g.is_floating_point() and not torch.isfinite(g).all()):
                print(f'replay with seed {seed}: {name} differs from the eager result or is not finite')
                return False
            if name in (names if nonempty is None else nonempty) and not g.any():
                print(f'replay with seed {seed}: {name} is an empty result')
                return False
        complaint = extra(got) if extra else None
        if complaint:
            print(f'replay with seed {seed}: {complaint}')
            return False
    return True


def main(name, check):
    """check(device) -> exit status, on cuda:0; without a GPU: exit status 2."""
    if not torch.cuda.is_available():
        print(f'{name} needs an MI355X')
        sys.exit(2)
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    sys.exit(check(device))
