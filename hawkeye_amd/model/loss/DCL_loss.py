"""DCL's criterion on the MI355X path - the reference's `model/loss/DCL_loss.py:4-21` contract:
`DCLLoss(config)(outputs, labels, labels_swap, swap_law)` with `config.alpha`, `config.beta` and `config.gamma` and
`outputs = [logits, swap_logits, mask]` as the model returns them: alpha x the label-smoothed (0.1) cross entropy of the
class logits, beta x that of the swap logits against `labels_swap`, gamma x the mean absolute difference of the mask and
the swap law.  One call into the HIP library returns the loss and the three gradients
(`hawkeye_amd.functional.dcl_loss`)."""
import torch.nn as nn

from ... import functional as HF

LABEL_SMOOTHING = 0.1


class DCLLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.alpha, self.beta, self.gamma = config.alpha, config.beta, config.gamma

    def forward(self, outputs, labels, labels_swap, swap_law):
        if len(outputs) != 3:
            raise ValueError(f'DCLLoss: outputs must be [logits, swap_logits, mask], got {len(outputs)} entries')
        return HF.dcl_loss(outputs[0], outputs[1], outputs[2], labels, labels_swap, swap_law, self.alpha, self.beta, self.gamma,
                           LABEL_SMOOTHING)
