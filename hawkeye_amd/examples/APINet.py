"""APINet trainer (reference Examples/APINet.py): class-balanced batches of `n_classes` x `n_samples` images for
training and plain batches for validation, the APINet criterion on the HIP kernel, Adam with a backbone group and a
group of everything else, and linear warm-up + cosine annealing stepped per epoch.  Accuracy is taken over
`cat(self_logits, other_logits)` against the fourfold targets; the meters are weighted as the reference weights them
(4 x 2B for the accuracy, 2 x 2B for the loss, B the number of images).

Kept from the reference, quirks included: at the start of epoch 0 the backbone group's lr is set to 0
("Freeze conv").  LinearLR steps in its chained form - it multiplies the group's CURRENT lr - so the zero survives all
`warmup_epochs` warm-up epochs; the trunk thaws when SequentialLR reaches its milestone and starts the cosine schedule
from the base lr.  With the yaml's `warmup_epochs: 8` that is epoch 8, where the reference's "Unfreeze conv" line merely
assigns the lr to itself.

Under hawkeye_amd.ddp every rank draws its own balanced batches (`BalancedBatchSampler(rank=...)`) and chooses the
pairs on its local batch; no collective is added for the selection, gradients are all-reduced as usual."""
import torch

import hawkeye_amd.model.methods.APINet  # noqa: F401  (opt-in registration of the plugin)

from ..model.loss import APINetLoss
from ..utils import accuracy
from .common import PairBatchTrainer, lr_groups


class APINetTrainer(PairBatchTrainer):
    def get_criterion(self, config):
        return APINetLoss(config)

    def get_optimizer(self, config):
        groups = lr_groups(self.get_model_module(), 'backbone', config.lr, 1.0)     # group 0: the trunk, group 1: the head
        return torch.optim.Adam(groups, weight_decay=config.weight_decay)

    def batch_training(self, data):
        images, labels = self._batch(data)
        outputs = self.model(images, labels, flag='train')
        self_logits, other_logits, labels1, labels2 = outputs
        loss = self.criterion(outputs, labels)
        self.backward_and_step(loss)
        logits = torch.cat([self_logits, other_logits], dim=0)
        targets = torch.cat([labels1, labels2, labels1, labels2], dim=0)
        pairs = self_logits.shape[0] // 2                                           # 2B
        self.average_meters['acc'].update(accuracy(logits, targets, 1), 4 * pairs)
        self.average_meters['loss'].update(loss.item(), 2 * pairs)

    def batch_validate(self, data):
        images, labels = self._batch(data)
        logits = self.model(images, flag='val')
        self.average_meters['acc'].update(accuracy(logits, labels, 1), logits.size(0))

    def on_start_epoch(self, config):
        group = self.optimizer.param_groups[0]
        if self.epoch == 0:
            group['lr'] = 0
            self.logger.info('Freeze conv')
        elif self.epoch == 8:
            group['lr'] = group['lr']                   # Examples/APINet.py:91 - a no-op there too
            self.logger.info('Unfreeze conv')
        super().on_start_epoch(config)


if __name__ == '__main__':
    APINetTrainer().train()
