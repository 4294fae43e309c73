"""Peer-learning plugin (mirrors model/methods/PeerLearningNet.py:8-20): two copies of a registered base model - the
yaml's `model.base_model`, BCNN in the reference's configs - that teach each other through
`hawkeye_amd.model.loss.PeerLearningLoss`.  The second net is a deep copy of the first (same trunk weights, own
storage) with a freshly initialised classifier; `forward` returns both nets' logits in training and evaluation.

Registration is opt-in: `import hawkeye_amd.model.methods.PeerLearningNet` puts it into MODEL (importing
`hawkeye_amd.model` alone does not), after which `MODEL.get('PeerLearningNet')` and `install_into` carry it like the
other plugins.  `hawkeye_amd.examples.PeerLearning` does that import."""
import copy

import torch.nn as nn

from ..registry import MODEL
from ..utils import initialize_weights


@MODEL.register
class PeerLearningNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.base_model = MODEL.get(config.base_model.name)(config.base_model)
        self.base_model2 = copy.deepcopy(self.base_model)
        self.base_model2.classifier.apply(initialize_weights)

    def forward(self, x):
        return self.base_model(x), self.base_model2(x)
