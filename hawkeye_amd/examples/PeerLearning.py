"""Peer-learning trainer (reference Examples/PeerLearning.py): two BCNNs, the peer-learning criterion on the HIP kernel,
Adam with linear warm-up + cosine annealing, and the drop-rate schedule of the paper's equation 2 - `drop_rate` from
the `T_k`-th epoch on, a linear ramp from 0 over the first `T_k` epochs.  Meters: acc (the better of the two nets per
batch), acc1, acc2, loss1, loss2.  One backward of loss1 + loss2 through `backward_and_step`: loss1 depends on the
first net only and loss2 on the second, so this equals the reference's two backward calls.

The one deliberate deviation: in stage 1 the reference asks for `model.classifier`, which a PeerLearningNet does not
have (it would raise there); here stage 1 optimises both `base_model.classifier` and `base_model2.classifier`.

Under hawkeye_amd.ddp every rank selects on its local batch (the reference's single-process DataParallel run gathers
the logits and selects over the whole batch); no collective is added for the selection, gradients are all-reduced as
usual."""
import numpy as np
import torch

import hawkeye_amd.model.methods.PeerLearningNet  # noqa: F401  (opt-in registration of the plugin)

from ..model.loss import PeerLearningLoss
from ..train import Trainer
from ..utils import AverageMeter, PerformanceMeter, accuracy
from .common import warmup_cosine

METERS = ('acc', 'acc1', 'acc2', 'loss1', 'loss2')


def drop_rate_schedule(epochs, t_k, drop_rate):
    """d(T) per epoch (Examples/PeerLearning.py:20-23)."""
    rates = np.ones(epochs) * drop_rate
    rates[:t_k] = np.linspace(0, drop_rate, t_k)[:epochs]
    return rates


class PLTrainer(Trainer):
    def __init__(self, config=None):
        super().__init__(config)
        model = self.config.model
        self.rate_scheduler = drop_rate_schedule(self.config.train.epoch, model.T_k, model.drop_rate)

    def get_performance_meters(self):
        return {'train': {m: PerformanceMeter(higher_is_better=not m.startswith('loss')) for m in METERS},
                'val': {m: PerformanceMeter() for m in ('acc', 'acc1', 'acc2')},
                'val_first': {'acc': PerformanceMeter()}}

    def get_average_meters(self):
        return {m: AverageMeter() for m in METERS}

    def get_dataset(self, config):
        if config.name == 'synthetic':                   # the class count lives in the base model's section
            from .. import data
            n_cls, size = self.config.model.base_model.num_classes, config.transformer.image_size
            return {s: data.SyntheticDataset(config.samples if 'samples' in config else 64 * config.batch_size,
                                             size, n_cls, seed=i) for i, s in enumerate(('train', 'val'))}
        return super().get_dataset(config)

    def get_optimizer(self, config):
        cfg = self.config.model
        stage = cfg.stage if 'stage' in cfg else (cfg.base_model.stage if 'stage' in cfg.base_model else None)
        model = self.get_model_module()
        if stage == 1:
            params = list(model.base_model.classifier.parameters()) + list(model.base_model2.classifier.parameters())
        elif stage is None or stage == 2:
            params = model.parameters()
        else:
            raise NotImplementedError()
        return torch.optim.Adam(params, lr=config.lr, weight_decay=config.weight_decay)

    def get_scheduler(self, config):
        return warmup_cosine(self.optimizer, config)

    def get_criterion(self, config):
        return PeerLearningLoss

    def batch_training(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        logits1, logits2 = self.model(images)
        loss1, loss2 = self.criterion(logits1, logits2, labels, drop_rate=float(self.rate_scheduler[self.epoch]))
        self.backward_and_step(loss1 + loss2)
        count = images.size(0)
        acc1, acc2 = accuracy(logits1, labels, 1), accuracy(logits2, labels, 1)
        for name, value in (('acc', max(acc1, acc2)), ('acc1', acc1), ('acc2', acc2), ('loss1', loss1.item()),
                            ('loss2', loss2.item())):
            self.average_meters[name].update(value, count)

    def batch_validate(self, data):
        images, labels = self.to_device(data['img']), self.to_device(data['label'])
        logits1, logits2 = self.model(images)
        acc1, acc2 = accuracy(logits1, labels, 1), accuracy(logits2, labels, 1)
        for name, value in (('acc', max(acc1, acc2)), ('acc1', acc1), ('acc2', acc2)):
            self.average_meters[name].update(value, images.size(0))

    def update_performance_meter(self, split):
        for name, meter in self.performance_meters[split].items():
            meter.update(self.average_meters[name].avg)


if __name__ == '__main__':
    PLTrainer().train()
