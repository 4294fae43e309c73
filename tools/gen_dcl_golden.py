"""Writes the DCL fixtures under tests/golden/: the reference's criterion (model/loss/DCL_loss.py) on the loss cases of
tests/golden/dcl_inputs.py and one whole-model case (model/methods/DCL.py), in float32 and float64; the swap laws that
the reference's own DCLDataset.__getitem__ (dataset/dataset_DCL.py) returns for the law cases; the permutation and the
image its RandomSwap (dataset/transforms.py) makes under a fixed random.seed; the outputs of its two collate functions;
and the reference model's state_dict keys for the four cls_2 / cls_2xmul settings.

    python tools/gen_dcl_golden.py [--reference DIR] [--check]

The reference is imported at run time; nothing of it is copied.  Files: dcl_ops.npz, dcl_model.npz and
dcl_state_dict.json.  Inputs and weights are stored as recipes only (the swapped image of the RandomSwap case is a
result, and small).

Three things need care.
  * The reference's DCL.__init__ hard-codes resnet50(pretrained=True), which would ask for a download.  Before any model is
    constructed the name `resnet50` in the imported model.methods.DCL module is replaced by a wrapper that forces
    pretrained=False; the weights then come from tests/golden/inputs.py:seeded_init.  The model is never made another way.
  * The reference's dataset package imports torchvision, which is not installed, and its RandomSwap names
    PIL.Image.ANTIALIAS, which Pillow 10 dropped (it named LANCZOS).  dataset/dataset_DCL.py and dataset/transforms.py are
    loaded by file path, so that dataset/__init__.py does not run; in-memory stand-in modules answer the torchvision names
    that dataset/transforms.py imports; PIL.Image.ANTIALIAS is set to PIL.Image.LANCZOS first.  All in this process only.
  * L1 is not differentiable at 0: dcl_inputs.loss_inputs accepts a loss seed only if no mask element is within 1e-3 of its
    law, and a model seed is accepted here only if the float64 mask keeps that distance from the constant ramp.

The laws come from DCLDataset.__getitem__ in train mode on a temporary directory of PNGs and a meta file, with
common_aug=None, a `swap` that returns the prepared swapped image and a `train_totensor` that does nothing; `swap_law2`
is read back and turned into indices.  The archives have fixed zip timestamps (--check compares instead of writing)."""
import argparse
import importlib
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcl_inputs as T  # noqa: E402
from inputs import seeded_init  # noqa: E402
from gen_apinet_golden import to_bytes  # noqa: E402
from gen_crossx_golden import default_dtype  # noqa: E402

KEYS_FILE = 'dcl_state_dict.json'


class _Anything:
    """Answers any attribute with itself: default arguments such as InterpolationMode.BILINEAR evaluate, nothing runs."""

    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def _stand_in(name):
    m = types.ModuleType(name)
    m.__getattr__ = lambda attr: _Anything()
    m.__path__ = []
    return m


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
    M = importlib.import_module('model.methods.DCL')
    inner = M.resnet50

    def resnet50_offline(pretrained=False, **kwargs):       # the reference asks for pretrained=True: never honoured here
        return inner(pretrained=False, **kwargs)
    M.resnet50 = resnet50_offline
    L = importlib.import_module('model.loss.DCL_loss')
    import PIL.Image
    if not hasattr(PIL.Image, 'ANTIALIAS'):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    for name in ('torchvision', 'torchvision.transforms', 'torchvision.transforms.functional', 'torchvision.transforms.autoaugment',
                 'torchvision.transforms.transforms'):
        sys.modules[name] = _stand_in(name)
    D = _load_by_path('_reference_dataset_dcl', os.path.join(ref_root, 'dataset', 'dataset_DCL.py'))
    X = _load_by_path('_reference_dataset_transforms', os.path.join(ref_root, 'dataset', 'transforms.py'))
    return M, L, D, X


def cfg(**kw):
    return type('Cfg', (), kw)()


# ---------------------------------------------------------------------------------------------------------- loss
def run_loss(L, arrays, dtype):
    logits, swap, mask, y, ys, law = arrays
    with default_dtype(dtype):
        crit = L.DCLLoss(cfg(alpha=T.COEF[0], beta=T.COEF[1], gamma=T.COEF[2]))
        leaves = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (logits, swap, mask)]
        yt, yst, lawt = torch.from_numpy(y), torch.from_numpy(ys), torch.from_numpy(law).to(dtype)
        total = crit(leaves, yt, yst, lawt)
        total.backward()
        with torch.no_grad():
            terms = [crit.ce_loss(leaves[0], yt), crit.ce_loss(leaves[1], yst), crit.add_loss(leaves[2], lawt)]
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
        seed = arrays[6]
        r64, r32 = run_loss(L, arrays[:6], torch.float64), run_loss(L, arrays[:6], torch.float32)
        if k == T.TIE_CASE:
            for b, e in T.TIES:
                assert r64['d_mask'][b, e] == 0 and r32['d_mask'][b, e] == 0
        out[f'l{k}_recipe'] = np.array([seed, *case], dtype=np.int64)
        for prec, r in (('f32', r32), ('f64', r64)):
            for name in T.LOSS_RESULTS:
                out[f'l{k}_{name}_{prec}'] = r[name]
        print(f'loss case {k}: N K S M {case} seed {seed}: loss {r64["loss"]}, fp32 distance total '
              f'{T.distance(r32["loss"][0], r64["loss"][0]):.1e} d_logits {T.distance(r32["d_logits"], r64["d_logits"]):.1e}')
    return out


# ----------------------------------------------------------------------------------------------------------- law
def reference_law(D, unswap, swapped, grid):
    """The reference's DCLDataset.__getitem__ in train mode on one image -> the indices behind swap_law2."""
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        Image.fromarray(unswap).save(os.path.join(tmp, 'image.png'))
        meta = os.path.join(tmp, 'train.txt')
        with open(meta, 'w') as f:
            f.write('0 image.png\n')
        prepared = Image.fromarray(swapped)
        tf = {'common_aug': None, 'swap': lambda img: prepared, 'train_totensor': lambda img: img}
        ds = D.DCLDataset(tmp, meta, transforms=tf, swap_size=list(grid), mode='train', cls_2=True, cls_2xmul=False)
        img_unswap, img_swap, label, label_swap, law1, law2, name = ds[0]
    assert np.array_equal(np.array(img_unswap), unswap) and np.array_equal(np.array(img_swap), swapped)      # PNG is lossless
    parts = grid[0] * grid[1]
    index = [int(round(v * parts)) + parts // 2 for v in law2]
    assert [(i - parts // 2) / parts for i in index] == law2
    assert law1 == [(i - parts // 2) / parts for i in range(parts)]
    return np.array(index, dtype=np.int32)


def build_law(D):
    out = {}
    for name, make in T.LAW_CASES.items():
        unswap, swapped = make()
        index = reference_law(D, unswap, swapped, T.LAW_GRID)
        out[f'law_{name}_index'] = index
        print(f'law case {name}: {unswap.shape[0]} x {unswap.shape[1]}, {len(set(index.tolist()))} distinct indices')
    perm = T.law_permutation_case()[2]
    assert np.array_equal(out['law_permutation_index'], perm), 'a patch permutation must come back as the index'
    assert not out['law_constant_index'].any()
    assert out['law_equal_total_index'][12] == 30
    return out


# ---------------------------------------------------------------------------------------- RandomSwap and collates
def build_swap(X):
    import PIL
    from PIL import Image
    swap = X.RandomSwap((7, 7))
    random.seed(T.SWAP_SEED)
    probe = np.array(swap(Image.fromarray(T.probe_image())))
    perm = T.read_probe(probe)
    assert sorted(perm) == list(range(49)), perm
    random.seed(T.SWAP_SEED)
    image = np.array(swap(Image.fromarray(T.swap_image())))
    print(f'RandomSwap under seed {T.SWAP_SEED}: permutation {perm}')
    return dict(swap_perm=np.array(perm, dtype=np.int32), swap_image=image,
                swap_pil_version=np.frombuffer(PIL.__version__.encode(), dtype=np.uint8).copy())


def build_collate(D):
    train, val = T.collate_samples()
    as_t = lambda s, n: tuple(torch.from_numpy(v) if i < n else v for i, v in enumerate(s))
    out = {}
    for split, fn, samples, n_img in (('train', D.collate_fn4train, train, 2), ('val', D.collate_fn4val, val, 1)):
        imgs, label, label_swap, law, names = fn([as_t(s, n_img) for s in samples])
        assert label.dtype == torch.int64 and law.dtype == torch.float32
        out[f'collate_{split}_imgs'] = imgs.numpy()
        out[f'collate_{split}_label'] = label.numpy()
        out[f'collate_{split}_label_swap'] = label_swap.numpy()
        out[f'collate_{split}_law'] = law.numpy()
        assert names == [s[-1] for s in samples]
    return out


# --------------------------------------------------------------------------------------------------------- model
def state_dict_keys(M):
    keys = {}
    for cls_2 in (False, True):
        for cls_2xmul in (False, True):
            net = M.DCL(cfg(num_classes=T.CLASSES, cls_2=cls_2, cls_2xmul=cls_2xmul))
            keys[f'{int(cls_2)}{int(cls_2xmul)}'] = {'state_dict': [[k, list(v.shape)] for k, v in net.state_dict().items()],
                                                      'children': [n for n, _ in net.named_children()],
                                                      'n_params': sum(q.numel() for q in net.parameters())}
    return keys


def build_model(M):
    c = T.MODEL_CASE
    net = M.DCL(cfg(num_classes=T.CLASSES, cls_2=c['cls_2'], cls_2xmul=c['cls_2xmul']))
    seeded_init(net, c['init_seed'])
    net.eval()
    ramp = np.array([(i - 49 // 2) / 49 for i in range(49)])
    for seed in range(c['init_seed'] + 1, c['init_seed'] + 9):
        images = T.model_images(seed, c['B'], c['size'])
        runs = {}
        for prec, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            with default_dtype(dtype):
                net.to(dtype)
                try:
                    with torch.no_grad():
                        out = net(torch.from_numpy(images).to(dtype))
                finally:
                    net.float()
            assert out[0].dtype == dtype and len(out) == 3
            runs[prec] = dict(zip(T.MODEL_OUTPUTS, (t.numpy() for t in out)))
        margin = float(np.abs(runs['f64']['mask'] - ramp).min())
        top = [runs[q]['logits'].argmax(1).tolist() for q in ('f32', 'f64')]
        ok = margin >= T.L1_MARGIN and top[0] == top[1]
        print(f'model seed {seed}: min |mask - ramp| {margin:.2e}, classes {top}: {"accepted" if ok else "rejected"}')
        if ok:
            break
    else:
        raise RuntimeError('model case: no seed meets the conditions')
    arrays = dict(model_recipe=np.array([seed, c['B'], c['size'], c['init_seed']], dtype=np.int64))
    for prec in ('f32', 'f64'):
        for name in T.MODEL_OUTPUTS:
            arrays[f'model_{name}_{prec}'] = runs[prec][name]
    for name in T.MODEL_OUTPUTS:
        print(f'  model {name}: fp32 distance from fp64 {T.distance(arrays[f"model_{name}_f32"], arrays[f"model_{name}_f64"]):.2e}')
    return arrays


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('HAWKEYE_REFERENCE', os.path.join(os.path.dirname(ROOT), 'reference')))
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    torch.set_num_threads(1)                       # one thread: ATen's reduction order does not depend on the host
    M, L, D, X = load_reference(args.reference)
    ops = build_loss(L)
    ops.update(build_law(D))
    ops.update(build_swap(X))
    ops.update(build_collate(D))
    blobs = {'dcl_ops.npz': to_bytes(ops), 'dcl_model.npz': to_bytes(build_model(M)),
             KEYS_FILE: (json.dumps(state_dict_keys(M)) + '\n').encode()}
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if f.endswith('.npz') and not f.startswith('dcl_'))
    same = True
    for name, blob in blobs.items():
        assert len(blob) <= largest, (name, len(blob), largest)
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
