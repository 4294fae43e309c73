"""APINet plugin (attentive pairwise interaction; mirrors model/methods/APINet.py:9-113): a ResNet-101 trunk, a 7 x 7
average pool, and a head that compares every image with its nearest same-class and its nearest other-class image of
the batch.  A "mutual" vector `map2(drop(map1([f1 | f2])))` gates both members of a pair; the classifier sees each
feature gated by its own and by its partner's gate.

Interface kept from the reference: `APINet(config)` with `config.num_classes`; attributes `backbone`, `avg`, `map1`,
`map2`, `fc`, `drop`, `sigmoid` (the state_dict keys are `backbone.*`, `map1.*`, `map2.*`, `fc.*`, in that order);
`forward(images, targets=None, flag='train')` -> `(self_logits [4B,C], other_logits [4B,C], labels1 [2B], labels2 [2B])`
with long labels, `forward(images, flag='val')` -> `fc(pool)`.

What runs where: the trunk is PyTorch-ROCm; the pooling is `hk_osme_gap`; pair selection, pair gather, the gated
interaction (with its four dropouts) and the scatter of their backward are csrc/apinet.hip; `map1`, `map2` and `fc` run
on `hk_linear_fwd / bwd`.  Between the trunk's output and the logits nothing synchronises with the host: the pairs and
`labels1` / `labels2` are chosen and built on the device, so the head (and `APINetLoss` behind it) can be captured into
a hipGraph.  The reference copies the distance matrix to the host and searches it with numpy (APINet.py:76-113).

Deviations from the reference:
  * the logits are `num_classes` wide (APINet.py:63-64 hard-codes 200);
  * a batch of one image works (the reference's `.squeeze()` drops the batch dimension);
  * the trunk's map must be 7 x 7 - what `AvgPool2d(7, 1)` + `squeeze` effectively requires - anything else raises;
  * the pair distance is sum (a - b)^2 instead of -2ab + |a|^2 + |b|^2 (no cancellation); ties go to the lowest index
    and a row without a candidate is paired with row 0, as numpy's argmin does;
  * the dropout masks come from torch's device generator, one draw for the four blocks: the same distribution, not the
    reference's random stream;
  * the `pretrained=True` trunk weights are looked up offline by the backbone, like the other plugins'.

Registration is opt-in: `import hawkeye_amd.model.methods.APINet` puts it into MODEL (importing `hawkeye_amd.model`
alone does not); `hawkeye_amd.examples.APINet` does that import."""
import torch
import torch.nn as nn

from ... import functional as HF
from ..backbone import resnet101
from ..registry import MODEL

FEATURES = 2048         # width of the pooled vector (ResNet-101, layer4)
HIDDEN = 512            # width of map1's output
MAP_SIDE = 7            # the trunk's map at a 224 x 224 input


@MODEL.register
class APINet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_classes = config.num_classes
        trunk = resnet101(pretrained=True)
        self.backbone = nn.Sequential(*list(trunk.children())[:-2])
        self.avg = nn.AvgPool2d(kernel_size=MAP_SIDE, stride=1)            # attribute parity; the pooling is hk_osme_gap
        self.map1 = nn.Linear(FEATURES * 2, HIDDEN)
        self.map2 = nn.Linear(HIDDEN, FEATURES)
        self.fc = nn.Linear(FEATURES, self.num_classes)
        self.drop = nn.Dropout(p=0.5)
        self.sigmoid = nn.Sigmoid()
        self.device = None

    def pool(self, images):
        conv_out = self.backbone(images)
        if conv_out.dim() != 4 or tuple(conv_out.shape[2:]) != (MAP_SIDE, MAP_SIDE):
            raise ValueError(f'APINet: the trunk must give a {MAP_SIDE} x {MAP_SIDE} map (a 224 x 224 input), got '
                             f'{tuple(conv_out.shape)}')
        return HF.osme_gap(conv_out)                                       # [B, D]

    def head(self, pool_out, targets):
        """pool_out [B,D], targets [B] -> (self_logits, other_logits, labels1, labels2); everything on the device."""
        b, d = pool_out.shape
        partner = HF.api_pairs(pool_out, targets)                          # int32 [2B]: intra partners, inter partners
        targets = targets.to(device=pool_out.device, dtype=torch.long)
        labels1 = torch.cat([targets, targets])
        labels2 = targets.index_select(0, partner.long())
        mutual = HF.api_pair_features(pool_out, partner)                   # [2B, 2D]
        map1_out = HF.linear(mutual, self.map1.weight, self.map1.bias)
        m = HF.linear(self.drop(map1_out), self.map2.weight, self.map2.bias)
        masks = None
        if self.training and self.drop.p > 0:
            masks = torch.empty(8 * b, d, dtype=torch.bool, device=pool_out.device).bernoulli_(1.0 - self.drop.p)
        feats = HF.api_interact(pool_out, partner, m, masks, self.drop.p)  # [8B, D]: 1-self, 2-self, 1-other, 2-other
        logits = HF.linear(feats, self.fc.weight, self.fc.bias)
        return logits[:4 * b], logits[4 * b:], labels1, labels2

    def forward(self, images, targets=None, flag='train'):
        self.device = images.device
        pool_out = self.pool(images)
        if flag == 'train':
            if targets is None:
                raise ValueError("APINet: flag='train' needs the batch's targets (the pairs are chosen by label)")
            return self.head(pool_out, targets)
        if flag == 'val':
            return HF.linear(pool_out, self.fc.weight, self.fc.bias)
        raise ValueError(f"APINet: flag must be 'train' or 'val', got {flag!r}")
