"""Peer-learning loss (Webly Supervised Fine-Grained Recognition, ICCV 2021) on the MI355X path - the reference's
`model/loss/peer_learning_loss.py:5-65` contract: `PeerLearningLoss(logits_1, logits_2, labels, drop_rate)` ->
`(loss_1, loss_2)`.  Rows on which the two nets' predictions disagree always count; of the rows on which they agree,
each net learns from the `int((1 - drop_rate) * n)` its PEER finds easiest.  One call into the HIP library returns both
losses and both gradients (`hawkeye_amd.functional.peer_learning_loss`): no host synchronisation, so a step that uses
it can be captured into a hipGraph.  Under hawkeye_amd.ddp the selection is per rank, on the local batch."""
from ... import functional as HF


def PeerLearningLoss(logits_1, logits_2, labels, drop_rate):
    """logits_1, logits_2 [N, C]; labels [N]; drop_rate: this epoch's drop rate (a host float in [0, 1])."""
    return HF.peer_learning_loss(logits_1, logits_2, labels, drop_rate)
