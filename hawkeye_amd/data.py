"""Datasets for the trainer: an on-the-fly synthetic dataset (what the metric is
quoted on: N(0,1) 448x448 images, uniform labels - SURVEY.md section 8d), an
image-folder dataset with the reference's `label relpath` meta format
(dataset/dataset.py:22-64) and the class-balanced batch sampler.  The image
presets live in hawkeye_amd/transforms.py."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset


class SyntheticDataset(Dataset):
    def __init__(self, n, image_size, num_classes, seed=0):
        self.n, self.size, self.k, self.seed = int(n), int(image_size), int(num_classes), seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        return {'img': torch.randn(3, self.size, self.size, generator=g),
                'label': int(torch.randint(0, self.k, (1,), generator=g))}

    @property
    def labels(self):
        # same draw order as __getitem__ (image first, then label) so that both agree
        out = []
        for i in range(self.n):
            g = torch.Generator().manual_seed(self.seed * 1000003 + i)
            torch.randn(3, self.size, self.size, generator=g)
            out.append(int(torch.randint(0, self.k, (1,), generator=g)))
        return out


class FGDataset(Dataset):
    """meta file lines: `<label> <relative/path.jpg>` (metadata/cub/train.txt:1)."""

    def __init__(self, root, meta_path, transform=None):
        self.root, self.transform, self.items = root, transform, []
        with open(meta_path) as f:
            for line in f:
                line = line.strip()
                if line:
                    lab, rel = line.split(' ', 1)
                    self.items.append((int(lab), rel))

    def __len__(self):
        return len(self.items)

    @property
    def labels(self):
        return [lab for lab, _ in self.items]

    def __getitem__(self, i):
        from PIL import Image
        lab, rel = self.items[i]
        img = Image.open(os.path.join(self.root, rel))
        if self.transform is not None:
            return {'img': self.transform(img), 'label': lab}
        from .transforms import to_float_tensor
        return {'img': to_float_tensor(img), 'label': lab}


class BalancedBatchSampler(torch.utils.data.Sampler):
    """Batches of `n_classes` distinct classes x `n_samples` images each - what the MAMC n-pairs loss needs to have
    same-class pairs in every batch (reference dataset/sampler.py:5-38, used by Examples/OSMENet.py:20-23).
    Own organisation: one shuffled queue per class that is refilled when it runs short; `seed`/`rank` make the
    stream reproducible and different on every data-parallel rank."""

    def __init__(self, labels, n_classes, n_samples, seed=0, rank=0):
        self.by_class = {}
        for idx, lab in enumerate(labels):
            self.by_class.setdefault(int(lab), []).append(idx)
        self.classes = sorted(c for c, v in self.by_class.items() if len(v) >= n_samples)
        if len(self.classes) < n_classes:
            raise ValueError(f'need {n_classes} classes with >= {n_samples} images, found {len(self.classes)}')
        self.n_classes, self.n_samples, self.total = int(n_classes), int(n_samples), len(labels)
        self.rng = np.random.RandomState(seed * 9973 + rank)
        self.queues = {c: [] for c in self.classes}

    def __len__(self):
        return self.total // (self.n_classes * self.n_samples)

    def _take(self, c):
        q = self.queues[c]
        if len(q) < self.n_samples:
            q[:] = [int(i) for i in self.rng.permutation(self.by_class[c])]
        out = q[:self.n_samples]
        del q[:self.n_samples]
        return out

    def __iter__(self):
        for _ in range(len(self)):
            batch = []
            for c in self.rng.choice(self.classes, self.n_classes, replace=False):
                batch.extend(self._take(int(c)))
            yield batch


# --------------------------------------------------------------------------- DCL
def subsample_per_class(paths, labels, rng=None, fraction=10):
    """The reference's validation subsample (dataset/dataset_DCL.py:100-115): per class, in the order the classes first
    appear, `len // fraction` images drawn without replacement by `random.sample` over the class's positions."""
    import random
    rng = rng or random
    by_class = {}
    for path, label in zip(paths, labels):
        by_class.setdefault(label, []).append(path)
    out_paths, out_labels = [], []
    for label, members in by_class.items():
        picked = rng.sample(list(range(len(members))), len(members) // fraction)
        out_paths.extend(members[k] for k in picked)
        out_labels.extend(label for _ in picked)
    return out_paths, out_labels


def _as_u8(img):
    return torch.from_numpy(np.array(img.convert('RGB'), dtype=np.uint8))


class DCLDataset(Dataset):
    """DCL's image-folder dataset (dataset/dataset_DCL.py:11-97) with the reference's `label relpath` meta format.  The
    swap law is not computed here: a training sample is the uint8 unswapped and swapped images [H,W,3], and the trainer
    takes the law from them on the device (functional.dcl_swap_law).
        train: (unswapped u8, swapped u8, label, label_swap, relpath) - label_swap is -1 for cls_2 (which wins when both
               are set, as in the reference), label + num_classes for cls_2xmul
        val  : (u8, label, label_swap = label, relpath)
        test : (u8, label, relpath)
    `transforms`: a dict with `common_aug` (PIL -> PIL or None), `swap` (PIL -> PIL, e.g. transforms.RandomSwap) and
    `{mode}_totensor` (PIL -> PIL of the final size, or None).  `subsample_val` (default True, the reference's behaviour)
    keeps a tenth of every class in val mode."""

    def __init__(self, root, meta_path, transforms=None, swap_size=(7, 7), mode='train', cls_2=True, cls_2xmul=False,
                 subsample_val=True):
        self.root, self.mode, self.swap_size = root, mode, tuple(swap_size)
        self.paths, self.labels = [], []
        with open(meta_path) as f:
            for line in f:
                line = line.strip()
                if line:
                    lab, rel = line.split(' ', 1)
                    self.labels.append(int(lab))
                    self.paths.append(rel)
        if mode == 'val' and subsample_val:
            self.paths, self.labels = subsample_per_class(self.paths, self.labels)
        self.use_cls_2, self.use_cls_mul = cls_2, cls_2xmul
        self.num_classes = len(set(self.labels))
        transforms = transforms or {}
        self.common_aug, self.swap = transforms.get('common_aug'), transforms.get('swap')
        self.finish = transforms.get(mode + '_totensor')

    def __len__(self):
        return len(self.paths)

    def _final(self, img):
        return _as_u8(self.finish(img) if self.finish is not None else img)

    def __getitem__(self, i):
        from PIL import Image
        with open(os.path.join(self.root, self.paths[i]), 'rb') as f:
            img = Image.open(f).convert('RGB')
        label = self.labels[i]
        if self.mode == 'test':
            return self._final(img), label, self.paths[i]
        unswap = self.common_aug(img) if self.common_aug is not None else img
        if self.mode == 'train':
            swapped = self.swap(unswap)
            label_swap = label + self.num_classes if self.use_cls_mul else None
            if self.use_cls_2:
                label_swap = -1
            if label_swap is None:
                raise ValueError('DCLDataset: train mode needs cls_2 or cls_2xmul')     # the reference: an UnboundLocalError
            return self._final(unswap), self._final(swapped), label, label_swap, self.paths[i]
        return self._final(unswap), label, label, self.paths[i]


class SyntheticDCLDataset(Dataset):
    """Seeded uint8 images [size,size,3] in DCLDataset's sample formats.  The image is smooth noise (a coarse random grid
    upsampled, plus fine noise), so that patch means differ; the swapped image is a patch permutation of it drawn by
    transforms.swap_permutation from the sample's own generator - whole patches move, nothing is resampled."""

    def __init__(self, n, image_size, num_classes, swap_size=(7, 7), mode='train', cls_2=True, cls_2xmul=False, seed=0):
        self.n, self.size, self.k, self.seed = int(n), int(image_size), int(num_classes), seed
        self.swap_size, self.mode, self.use_cls_2, self.use_cls_mul = tuple(swap_size), mode, cls_2, cls_2xmul
        self.num_classes = self.k

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        import random
        from .transforms import patch_bounds, swap_permutation
        rs = np.random.RandomState((self.seed * 1000003 + i) % (2 ** 31))
        gx, gy = self.swap_size
        coarse = rs.randint(0, 256, (gy * 2, gx * 2, 3)).astype(np.float32)
        reps = -(-self.size // (gy * 2)), -(-self.size // (gx * 2))
        img = np.repeat(np.repeat(coarse, reps[0], 0), reps[1], 1)[:self.size, :self.size]
        img = np.clip(0.75 * img + 0.25 * rs.randint(0, 256, img.shape), 0, 255).astype(np.uint8)
        label = int(rs.randint(0, self.k))
        name = f'synthetic/{i}'
        if self.mode != 'train':
            return torch.from_numpy(img), label, label, name
        xs, ys = patch_bounds(self.size, gx), patch_bounds(self.size, gy)
        pw, ph = self.size // gx, self.size // gy                    # whole patches of one size move; the rest stays
        swapped = img.copy()
        perm = swap_permutation(self.swap_size, random.Random(int(rs.randint(0, 2 ** 31 - 1))))
        for k, src in enumerate(perm):
            dj, di, sj, si = k // gx, k % gx, src // gx, src % gx
            swapped[ys[dj]:ys[dj] + ph, xs[di]:xs[di] + pw] = img[ys[sj]:ys[sj] + ph, xs[si]:xs[si] + pw]
        label_swap = -1 if self.use_cls_2 else label + self.k
        return torch.from_numpy(img), torch.from_numpy(swapped), label, label_swap, name


def dcl_collate_train(batch):
    """The reference's collate_fn4train (dataset/dataset_DCL.py:118-142) without the laws, which the device makes: images
    interleaved unswapped, swapped; each label twice; labels_swap 1, 0 per sample for cls_2 (label_swap == -1), else label,
    label_swap.  -> {'u8': uint8 [2B,H,W,3], 'label', 'label_swap': int64 [2B], 'name': list of B}"""
    imgs, label, label_swap, names = [], [], [], []
    for unswap, swapped, lab, lab_swap, name in batch:
        imgs += [unswap, swapped]
        label += [lab, lab]
        label_swap += [1, 0] if lab_swap == -1 else [lab, lab_swap]
        names.append(name)
    return {'u8': torch.stack(imgs, 0), 'label': torch.tensor(label, dtype=torch.int64),
            'label_swap': torch.tensor(label_swap, dtype=torch.int64), 'name': names}


def dcl_collate_val(batch):
    """The reference's collate_fn4val (dataset/dataset_DCL.py:145-164): one image per sample; label_swap is the sample's own
    (its label: the reference's test for -1 looks at the law list and never holds).  The law of a validation batch is the
    constant ramp."""
    imgs, label, label_swap, names = [], [], [], []
    for img, lab, lab_swap, name in batch:
        imgs.append(img)
        label.append(lab)
        label_swap.append(lab_swap)
        names.append(name)
    return {'u8': torch.stack(imgs, 0), 'label': torch.tensor(label, dtype=torch.int64),
            'label_swap': torch.tensor(label_swap, dtype=torch.int64), 'name': names}


def dcl_law_ramp(parts):
    """swap_law1 (dataset/dataset_DCL.py:51): (i - P // 2) / P for i in range(P), as float32."""
    return torch.tensor([(i - (parts // 2)) / parts for i in range(parts)], dtype=torch.float64).to(torch.float32)
