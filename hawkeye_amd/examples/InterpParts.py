"""InterpParts trainer (reference Examples/InterpPartsNet.py): its own transforms - Resize(resize_size), a horizontal flip,
ColorJitter(0.1) (brightness only), RandomCrop(image_size), normalise, RandomErasing(p_erasing) in training; Resize and
CenterCrop in validation -, SGD with momentum 0.9 over two parameter groups (`conv1`, `bn1`, `layer1..3` at `lr`, everything
else at 20 x `lr`), CosineAnnealingLR over iterations x epochs stepped per batch, and the InterpParts criterion on the HIP
kernels.

The workers ship uint8 crops and the erasing rectangle; the float conversion, the normalisation and the erasing run on the
device (`image_finalize`, its `erase` argument).  Model, criterion, backward and step have no host synchronisation; the
step's only read-back is the loss value for the meter."""
import random

import numpy as np
import torch
from PIL import Image, ImageEnhance

import hawkeye_amd.model.methods.InterpParts  # noqa: F401  (opt-in registration of the plugin)

from .. import transforms as T
from ..model.loss import InterpPartsLoss
from ..train import Trainer
from ..utils import accuracy

FINETUNE_LAYERS = ('conv1', 'bn1', 'layer1', 'layer2', 'layer3')
SCRATCH_LR_RATIO = 20


def _resize_shorter(img, size):
    w, h = img.size
    if w <= h:
        return img.resize((size, int(size * h / w)), Image.BILINEAR)
    return img.resize((int(size * w / h), size), Image.BILINEAR)


def _shipped(img, box=None):
    return {'u8': torch.from_numpy(np.array(img, dtype=np.uint8)),
            'erase': torch.tensor(box if box is not None else (0, 0, 0, 0), dtype=torch.int32)}


class TrainTransform:
    """Shorter side to `resize`, flip with probability one half, brightness by a uniform factor in [1 - jitter, 1 + jitter],
    a random crop x crop cut (zero padding where the image is smaller), and with probability `p_erasing` an erasing
    rectangle for the device: PIL in, {'u8', 'erase'} out."""

    def __init__(self, resize, crop, p_erasing, jitter=0.1):
        self.resize, self.crop, self.p_erasing, self.jitter = int(resize), int(crop), float(p_erasing), float(jitter)

    def __call__(self, img):
        img = _resize_shorter(img.convert('RGB'), self.resize)
        if random.random() < 0.5:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        img = ImageEnhance.Brightness(img).enhance(random.uniform(max(0.0, 1 - self.jitter), 1 + self.jitter))
        w, h = img.size
        left, top = random.randint(0, max(w - self.crop, 0)), random.randint(0, max(h - self.crop, 0))
        img = img.crop((left, top, left + self.crop, top + self.crop))
        box = T.random_erasing_box(self.crop, self.crop) if random.random() < self.p_erasing else None
        return _shipped(img, box)


class InterpPartsTrainer(Trainer):
    def get_transformers(self, config):
        resize = config['resize_size'] if 'resize_size' in config else 512
        p_erasing = config['p_erasing'] if 'p_erasing' in config else 0.05
        return {'train': TrainTransform(resize, config['image_size'], p_erasing),
                'val': T.ClassificationPresetEval(crop_size=config['image_size'], resize_size=resize, device_finalize=True)}

    def get_criterion(self, config):
        return InterpPartsLoss(config)

    def get_optimizer(self, config):
        finetune, scratch = [], []
        for name, p in self.get_model_module().named_parameters():
            (finetune if name.split('.')[0] in FINETUNE_LAYERS else scratch).append(p)
        return torch.optim.SGD([{'params': finetune, 'lr': config.lr}, {'params': scratch, 'lr': SCRATCH_LR_RATIO * config.lr}],
                               weight_decay=config.weight_decay, momentum=0.9)

    def get_scheduler(self, config):
        return torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, len(self.dataloaders['train']) * self.config.train.epoch)

    def do_scheduler_step(self):
        pass                                               # stepped in every batch

    def batch_training(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        outputs = self.model(images)
        loss = self.criterion(outputs, labels)
        acc = accuracy(outputs[0], labels, 1)
        self.backward_and_step(loss)
        self.scheduler.step()
        self.average_meters['acc'].update(acc, labels.size(0))
        self.average_meters['loss'].update(loss.item(), labels.size(0))

    def batch_validate(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        self.average_meters['acc'].update(accuracy(self.model(images)[0], labels, 1), labels.size(0))


if __name__ == '__main__':
    InterpPartsTrainer().train()
