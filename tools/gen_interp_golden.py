"""Writes the InterpParts fixtures under tests/golden/: the reference's criterion (model/loss/InterpParts_loss.py) on the loss
cases of tests/golden/interp_inputs.py, in float32 and float64 (interp_ops.npz); one whole-model case of a short-`layers`
ResNet of model/methods/Interp_Parts.py in eval and train mode (interp_model.npz); and the reference model's state_dict keys
(interp_state_dict.json).

    python tools/gen_interp_golden.py [--reference DIR] [--check]

The reference is imported at run time; nothing of it is copied.  Inputs and weights are stored as recipes only.

Four things need care.
  * model/methods/Interp_Parts.py imports torchvision, which is not installed: `import torchvision` resolves to oracle/_stubs.
  * The reference's two factory functions ask for a download and are never called: ResNet(Bottleneck, layers, ..) is built
    directly, with short `layers` and the weights of tests/golden/inputs.py:seeded_init.
  * The reference's loss calls .cuda(device) on CPU tensors: torch.Tensor.cuda is the identity in this process only.
  * GroupingUnit's parameters are FloatTensors whatever the default dtype: for the float64 runs the module is cast with .double().

A loss seed is accepted by interp_inputs.loss_inputs only where the reference is well defined (no near ties, no |.| near 0).
The grouping unit's own cases are not stored: their largest gradient is beyond the size of a committed file, and the tests run
the reference's op sequence in torch on the CPU instead (tests/interp_ops.py).  The archives have fixed zip timestamps
(--check compares instead of writing)."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interp_inputs as T  # noqa: E402
from inputs import seeded_init  # noqa: E402
from gen_apinet_golden import to_bytes  # noqa: E402
from gen_crossx_golden import default_dtype  # noqa: E402

KEYS_FILE = 'interp_state_dict.json'
MAX_BYTES = 1 << 20


class Cfg(dict):
    """The reference reads its config both ways: `'radius' in config` and `config.radius`."""
    __getattr__ = dict.__getitem__


def load_reference(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
    torch.Tensor.cuda = lambda self, *a, **k: self          # this process only: the reference's loss moves CPU tensors "to the device"
    M = importlib.import_module('model.methods.Interp_Parts')
    L = importlib.import_module('model.loss.InterpParts_loss')
    return M, L


# ---------------------------------------------------------------------------------------------------------- loss
def run_loss(L, case, arrays, dtype):
    shape, radius, std, alpha, beta, coeff = case
    logits, assign, y = arrays
    with default_dtype(dtype):
        crit = L.InterpPartsLoss(Cfg(radius=radius, std=std, num_parts=shape[1], alpha=alpha, beta=beta, coeff=coeff))
        leaves = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (logits, assign)]
        yt = torch.from_numpy(y)
        total = crit((leaves[0], None, leaves[1]), yt)
        total.backward()
        with torch.no_grad():
            terms = [crit.ce_loss(leaves[0], yt), L.ShapingLoss(leaves[1], radius, std, shape[1], alpha, beta)]
    assert total.dtype == dtype
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    out = dict(loss=np.array([total.item()] + [t.item() for t in terms], dtype=np_dtype))
    for name, t in zip(T.LOSS_RESULTS[1:], leaves):
        out[name] = t.grad.numpy()
    return out


def build_loss(L):
    out = {}
    for k, case in enumerate(T.LOSS_CASES):
        arrays = T.loss_inputs(k)
        seed = arrays[3]
        r64, r32 = run_loss(L, case, arrays[:3], torch.float64), run_loss(L, case, arrays[:3], torch.float32)
        shape, radius = case[0], case[1]
        want = shape[0] * shape[1] * (2 * radius + 1) ** 2
        assert np.count_nonzero(r64['d_assign']) == want and np.count_nonzero(r32['d_assign']) == want
        assert np.array_equal(r64['d_assign'] != 0, r32['d_assign'] != 0)
        out[f'l{k}_recipe'] = np.array([seed, *shape, radius], dtype=np.int64)
        for prec, r in (('f32', r32), ('f64', r64)):
            for name in T.LOSS_RESULTS:
                out[f'l{k}_{name}_{prec}'] = r[name]
        print(f'loss case {k}: {case} seed {seed}: loss {r64["loss"]}, fp32 distance total '
              f'{T.distance(r32["loss"][0], r64["loss"][0]):.1e} d_assign {T.distance(r32["d_assign"], r64["d_assign"]):.1e}')
    for radius, std in T.WINDOWS:                          # the reference's own window and prior, for the functional layer's twins
        out[f'window_r{radius}'] = L.GaussianKernel(radius, std).numpy()
    for n, alpha, beta in T.PRIORS:
        L.update_prior_dist(n, alpha, beta)
        out[f'prior_n{n}_b{beta}'] = L.prior_dist.squeeze(1).numpy()
    return out


# --------------------------------------------------------------------------------------------------------- model
def short_model(M):
    c = T.MODEL_CASE
    net = M.ResNet(M.Bottleneck, list(c['layers']), c['classes'], c['parts'])       # never through the factory functions
    seeded_init(net, c['init_seed'])
    return net


def state_dict_keys(M):
    net = short_model(M)
    return {'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()], 'children': [n for n, _ in net.named_children()],
            'n_params': sum(q.numel() for q in net.parameters()), 'repr_grouping': repr(net.grouping)}


def build_model(M):
    c = T.MODEL_CASE
    for seed in range(c['init_seed'] + 1, c['init_seed'] + 9):
        images = T.model_images(seed, c['B'], c['size'])
        runs, ok = {}, True
        for mode in T.MODEL_MODES:
            for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
                net = short_model(M)                       # a fresh copy: train mode moves the running statistics
                net.train(mode == 'train')
                with default_dtype(dtype):
                    net.to(dtype)                          # GroupingUnit's FloatTensor parameters included
                    with torch.no_grad():
                        out = net(torch.from_numpy(images).to(dtype))
                assert out[0].dtype == dtype and len(out) == 3
                runs[mode, prec] = dict(zip(T.MODEL_OUTPUTS, (t.numpy() for t in out)))
            top = [runs[mode, q]['logits'].argmax(1).tolist() for q in ('f32', 'f64')]
            sums = runs[mode, 'f64']['assign'].sum((2, 3))
            ok = ok and top[0] == top[1] and not ((sums > T.EPS / T.S_FACTOR) & (sums < T.EPS * T.S_FACTOR)).any()
        print(f'model seed {seed}: {"accepted" if ok else "rejected"}')
        if ok:
            break
    else:
        raise RuntimeError('model case: no seed meets the conditions')
    arrays = dict(model_recipe=np.array([seed, c['B'], c['size'], c['init_seed']], dtype=np.int64))
    for (mode, prec), r in runs.items():
        for name in T.MODEL_OUTPUTS:
            arrays[f'model_{mode}_{name}_{prec}'] = r[name]
    for mode in T.MODEL_MODES:
        for name in T.MODEL_OUTPUTS:
            d = T.distance(arrays[f"model_{mode}_{name}_f32"], arrays[f"model_{mode}_{name}_f64"])
            print(f'  model {mode} {name}: fp32 distance from fp64 {d:.2e}')
    return arrays


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    M, L = load_reference(args.reference)
    blobs = {'interp_ops.npz': to_bytes(build_loss(L)), 'interp_model.npz': to_bytes(build_model(M)),
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
