"""MGE-CNN's criterion on the MI355X path.  The reference has no loss module for this method: its trainer calls
`nn.CrossEntropyLoss(label_smoothing=0.1)` on each of the model's ten logits tensors and backpropagates their mean
(Examples/MGE_CNN.py:15-16,43-45).  `MGELoss(config)(outputs, targets)` takes the model's output as it is returned
(`{'logits': [ten], 'pr_gate': ..}`, or the list itself) and gives that mean from one launch of the HIP library, which also returns
every gradient (`hawkeye_amd.functional.mge_loss`).  Optional `config.label_smoothing` (0.1).  `terms(outputs, targets)` also
returns the device tensor of the single cross entropies."""
import torch.nn as nn

from ... import functional as HF

LABEL_SMOOTHING = 0.1


class MGELoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.label_smoothing = config.label_smoothing if 'label_smoothing' in config else LABEL_SMOOTHING

    @staticmethod
    def _logits(outputs):
        logits = outputs['logits'] if isinstance(outputs, dict) else outputs
        if not isinstance(logits, (list, tuple)) or not logits:
            raise ValueError("MGELoss: outputs must be the model's {'logits': [..], 'pr_gate': ..} or the list of logits")
        return logits

    def forward(self, outputs, targets):
        return HF.mge_loss(self._logits(outputs), targets, self.label_smoothing)

    def terms(self, outputs, targets):
        return HF.mge_loss_with_terms(self._logits(outputs), targets, self.label_smoothing)
