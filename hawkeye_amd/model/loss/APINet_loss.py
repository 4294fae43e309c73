"""APINet's criterion on the MI355X path - the reference's `model/loss/APINet_loss.py:5-40` contract:
`APINetLoss(config)(outputs, target)` with `outputs = (self_logits, other_logits, labels1, labels2)` as the model
returns them in training.  Cross entropy with label smoothing 0.1 over `cat(self, other)` against the fourfold targets,
plus a margin ranking term that wants each image's own gate to score its class at least 0.05 above its partner's gate.
One call into the HIP library returns the loss and both logit gradients (`hawkeye_amd.functional.apinet_loss`): no host
synchronisation.  `target` is unused, as in the reference (the labels travel inside `outputs`)."""
import torch.nn as nn

from ... import functional as HF

LABEL_SMOOTHING = 0.1
MARGIN = 0.05


class APINetLoss(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        self.label_smoothing = LABEL_SMOOTHING
        self.margin = MARGIN

    def forward(self, output, target=None):
        self_logits, other_logits, labels1, labels2 = output
        return HF.apinet_loss(self_logits, other_logits, labels1, labels2, self.label_smoothing, self.margin)
