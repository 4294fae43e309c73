"""CrossX's criterion on the MI355X path - the reference's `model/loss/CrossX_loss.py:31-64` contract:
`CrossXLoss(config)(outputs, target)` with `config.num_parts` and `config.gamma` (three weights: ulti, plty, cmbn) and
`outputs` as the model returns them.  With one part it is the label-smoothed (0.1) cross entropy of the plain logits.
Otherwise: that cross entropy on the sum of the three classifiers' logits, the KL divergence from the last layer's
prediction to the other two (over the batch size; the target carries gradient, as in the reference), and per feature
list gamma x the upper triangle of the parts' correlation matrix - which the reference fills on the host, one
device-to-host copy per entry.  One call into the HIP library returns the loss and all six gradients
(`hawkeye_amd.functional.crossx_loss`).  The batch must hold at least two samples: the reference's `squeeze()` drops the
batch axis of a single one and fails."""
import torch.nn as nn
import torch.nn.functional as F

from ... import functional as HF

LABEL_SMOOTHING = 0.1


class CrossXLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_parts = config.num_parts
        self.gamma = list(config.gamma)
        if len(self.gamma) != 3:
            raise ValueError(f'CrossXLoss: gamma must hold three weights (ulti, plty, cmbn), got {self.gamma}')

    def forward(self, outputs, target):
        if self.num_parts == 1:
            return F.cross_entropy(outputs, target, label_smoothing=LABEL_SMOOTHING)
        ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs = outputs
        for name, ftrs in (('ulti', ulti_ftrs), ('plty', plty_ftrs), ('cmbn', cmbn_ftrs)):
            if len(ftrs) != self.num_parts:
                raise ValueError(f'CrossXLoss: {len(ftrs)} {name} features for num_parts = {self.num_parts}')
        return HF.crossx_loss(ulti, plty, cmbn, ulti_ftrs, plty_ftrs, cmbn_ftrs, target, self.gamma)
