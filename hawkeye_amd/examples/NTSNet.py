"""NTS-Net trainer (reference Examples/NTSNet.py): Adam over every parameter, linear warm-up + cosine annealing stepped
per epoch, the NTS criterion on the HIP kernel, and accuracy taken from `concat_logits` - the scrutinizer's verdict -
in training and validation alike.  The model's forward and the criterion have no host synchronisation; the step's
only read-back is the loss value for the meter."""
import torch

import hawkeye_amd.model.methods.NTSNet  # noqa: F401  (opt-in registration of the plugin)

from ..model.loss import NTSLoss
from ..train import Trainer
from ..utils import accuracy
from .common import warmup_cosine


class NTSTrainer(Trainer):
    def get_optimizer(self, config):
        return torch.optim.Adam(self.model.parameters(), lr=config.lr, weight_decay=config.weight_decay)

    def get_criterion(self, config):
        return NTSLoss(config)

    def get_scheduler(self, config):
        return warmup_cosine(self.optimizer, config)

    def batch_training(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        output = self.model(images)
        loss = self.criterion(output, labels)
        self.backward_and_step(loss)
        self.average_meters['acc'].update(accuracy(output[1], labels, 1), images.size(0))
        self.average_meters['loss'].update(loss.item(), images.size(0))

    def batch_validate(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        output = self.model(images)
        self.average_meters['acc'].update(accuracy(output[1], labels, 1), images.size(0))


if __name__ == '__main__':
    NTSTrainer().train()
