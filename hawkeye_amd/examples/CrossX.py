"""CrossX trainer (reference Examples/CrossX.py): its own transforms - Resize(600 x 600), RandomCrop / CenterCrop(448),
a horizontal flip in training, normalise -, SGD with momentum, MultiStepLR, the CrossX criterion on the HIP kernel, and
accuracy taken from the sum of the three classifiers' logits.  The model's forward and the criterion have no host
synchronisation; the step's only read-back is the loss value for the meter."""
import random

import torch
from PIL import Image

import hawkeye_amd.model.methods.CrossX  # noqa: F401  (opt-in registration of the plugin)

from .. import transforms as T
from ..model.loss import CrossXLoss
from ..train import Trainer
from ..utils import accuracy


class ResizeCrop:
    """Resize to resize x resize (both sides, the aspect ratio is not kept), cut crop x crop - at a random place with a
    random flip in training, from the centre in validation -, to a float tensor, normalise."""

    def __init__(self, resize, crop, train):
        self.resize, self.crop, self.train = int(resize), int(crop), train

    def __call__(self, img):
        img = img.convert('RGB').resize((self.resize, self.resize), Image.BILINEAR)
        room = self.resize - self.crop
        if self.train:
            top, left = random.randint(0, room), random.randint(0, room)
        else:
            top = left = int(round(room / 2.0))
        img = img.crop((left, top, left + self.crop, top + self.crop))
        if self.train and random.random() < 0.5:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return T.normalize(T.to_float_tensor(img))


class CrossXTrainer(Trainer):
    def get_transformers(self, config):
        resize = config['resize_size'] if 'resize_size' in config else 600
        return {'train': ResizeCrop(resize, config['image_size'], True), 'val': ResizeCrop(resize, config['image_size'], False)}

    def get_criterion(self, config):
        return CrossXLoss(config)

    def get_optimizer(self, config):
        return torch.optim.SGD(self.model.parameters(), lr=config.lr, momentum=config.momentum, weight_decay=config.weight_decay)

    def get_scheduler(self, config):
        return torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=config.milestones, gamma=config.gamma)

    def summed_logits(self, outputs):
        return outputs if self.config.model.num_parts == 1 else outputs[0] + outputs[1] + outputs[2]

    def batch_training(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        outputs = self.model(images)
        loss = self.criterion(outputs, labels)
        acc = accuracy(self.summed_logits(outputs), labels, 1)
        self.backward_and_step(loss)
        self.average_meters['acc'].update(acc, images.size(0))
        self.average_meters['loss'].update(loss.item(), images.size(0))

    def batch_validate(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        self.average_meters['acc'].update(accuracy(self.summed_logits(self.model(images)), labels, 1), images.size(0))


if __name__ == '__main__':
    CrossXTrainer().train()
