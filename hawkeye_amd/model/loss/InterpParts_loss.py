"""InterpParts' criterion on the MI355X path - the reference's `model/loss/InterpParts_loss.py:12-31` contract:
`InterpPartsLoss(config)(output, target)` with `output = (logits, att, assign)` as the model returns them and the optional
`config.radius` (2), `config.std` (0.4), `config.num_parts` (5), `config.alpha` (1), `config.beta` (0.001) and
`config.coeff` (0.5): the mean cross entropy of the logits plus coeff x the shaping loss of the assignment maps (each map
blurred with a Gaussian window, its maximum taken, the batch's maxima of a part sorted and compared in log space with the
inverse CDF of Beta(alpha, beta)).  Two launches of the HIP library return the loss and both gradients
(`hawkeye_amd.functional.ip_loss`).

Where the reference goes through `.cpu().numpy()` and scipy on every call (its `prev_bs` is never updated), the prior here
is made once per batch size and kept on the device: a step has no host synchronisation.  Ties, which the reference leaves
to its library's kernels: the lowest flat index holds a tied maximum, the lower sample takes the lower rank."""
import torch.nn as nn

from ... import functional as HF


class InterpPartsLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.radius = config.radius if 'radius' in config else 2
        self.std = config.std if 'std' in config else 0.4
        self.num_parts = config.num_parts if 'num_parts' in config else 5
        self.alpha = config.alpha if 'alpha' in config else 1
        self.beta = config.beta if 'beta' in config else 0.001
        self.coeff = config.coeff if 'coeff' in config else 0.5

    def forward(self, output, target):
        if len(output) != 3:
            raise ValueError(f'InterpPartsLoss: output must be (logits, att, assign), got {len(output)} entries')
        logits, _att, assign = output
        if assign.dim() == 4 and assign.shape[1] != self.num_parts:           # the reference's grouped conv2d fails there
            raise ValueError(f'InterpPartsLoss: assign holds {assign.shape[1]} parts, the criterion was made for {self.num_parts}')
        return HF.ip_loss(logits, assign, target, self.radius, self.std, self.alpha, self.beta, self.coeff)
