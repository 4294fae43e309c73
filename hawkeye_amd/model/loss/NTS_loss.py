"""NTS-Net's criterion on the MI355X path - the reference's `model/loss/NTS_loss.py:6-47` contract:
`NTSLoss(config)(outputs, targets)` with `config.proposal_num` and `outputs = [raw_logits, concat_logits, part_logits,
top_n_index, top_n_prob]` as the model returns them.  Three label-smoothed (0.1) cross entropies - the image's own
logits, the concatenated feature's, and every part's - plus the navigator's ranking hinge: a proposal whose part the
teacher finds easier (a smaller unsmoothed part loss) should carry the higher score, by a margin of 1.  One call into
the HIP library returns the loss and all four gradients (`hawkeye_amd.functional.nts_loss`); the reference calls
`.item()` once per part row and loops over the proposals in Python."""
import torch.nn as nn

from ... import functional as HF

LABEL_SMOOTHING = 0.1


class NTSLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.PROPOSAL_NUM = config.proposal_num
        self.label_smoothing = LABEL_SMOOTHING

    def forward(self, outputs, targets):
        raw_logits, concat_logits, part_logits, _, top_n_prob = outputs
        if part_logits.dim() != 3 or part_logits.shape[1] != self.PROPOSAL_NUM:
            raise ValueError(f'NTSLoss: part_logits must be [B, proposal_num = {self.PROPOSAL_NUM}, C], got {tuple(part_logits.shape)}')
        return HF.nts_loss(raw_logits, concat_logits, part_logits, top_n_prob, targets, self.label_smoothing)
