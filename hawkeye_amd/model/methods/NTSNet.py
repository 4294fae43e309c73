"""NTS-Net plugin (navigator - teacher - scrutinizer; mirrors model/methods/NTS_Net/NTSNet.py:9-78): a ResNet-50 trunk
scores a fixed set of anchors on its own layer4 map (the navigator), the `proposal_num` best anchors that survive a
greedy NMS are cut out of the zero-padded image and resized to 224 x 224, the same trunk looks at those parts (the
teacher's `partcls_net`), and `concat_net` classifies the image from its own feature and the first `cat_num` part
features (the scrutinizer).

Interface kept from the reference: `NTSNet(config)` with `config.proposal_num`, `config.cat_num`, `config.image_size`;
attributes `pretrained_model` (with `avgpool = AdaptiveAvgPool2d(1)`, `fc = Linear(2048, 200)`), `proposal_net`
(`down1..3`, `ReLU`, `tidy1..3`), `concat_net`, `partcls_net`, `topN`, `proposal_num`, `CAT_NUM`, `image_size`,
`pad_side = 224` and `edge_anchors` (numpy, padded by +224 and truncated to integers); the state_dict keys and their
order; `forward(x)` -> `[raw_logits, concat_logits, part_logits [B,topN,200], top_n_index int64 [B,topN],
top_n_prob [B,topN]]`.

What runs where: the trunk and the proposal convolutions are PyTorch-ROCm (MIOpen); the plugin calls the trunk's
submodules itself to get the reference's three outputs (logits, the layer4 map, the pooled feature); the NMS
(`hk_nts_nms`) and the part crops (`hk_nts_crop_resize`) are csrc/nts.hip; the three linears run on `hk_linear_fwd /
bwd`.  Between the images and the logits nothing synchronises with the host, so the forward (and `NTSLoss` behind it)
can be captured into a hipGraph.  The reference copies all scores to the host, runs a numpy NMS per image, builds a
padded copy of the batch and calls F.interpolate B x topN times (NTSNet.py:31-47).

The anchor table is computed here from the published setting (three pyramid levels with strides 32 / 64 / 128 and base
sizes 48 / 96 / 192, scales 2^(1/3), 2^(2/3) - and 1 on the last level -, aspect ratios 0.667 / 1 / 1.5; level by level,
scale by scale, ratio by ratio, then the map row-major), in float32 like the published generator, so that the truncated
corners are the same integers.

Deviations from the reference:
  * the reference's trunk builds a fresh `nn.Dropout(p=0.5)` in every forward, which is therefore active in eval() too;
    here the pooled feature is dropped only while `self.training`;
  * the dropout masks come from torch's device generator: the same distribution, not the reference's random stream;
  * the `pretrained=True` trunk weights are looked up offline by the backbone, like the other plugins';
  * `np.int` and `.cuda()` are gone (tensors are made on the input's device);
  * NMS ties go to the highest index, an unfillable slot repeats the last pick, and hard_nms's `res.any()` stop is not
    reproduced (see `hawkeye_amd.functional.nts_nms`); with the default anchors neither can occur.

Registration is opt-in: `import hawkeye_amd.model.methods.NTSNet` puts it into MODEL (importing `hawkeye_amd.model`
alone does not); `hawkeye_amd.examples.NTSNet` does that import."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import functional as HF
from ..backbone import resnet50
from ..registry import MODEL

FEATURES = 2048          # width of the pooled vector (ResNet-50, layer4)
CLASSES = 200            # NTSNet.py:21-24 hard-codes 200 logits
PAD_SIDE = 224           # zero padding around the image, and the side of a part crop
DROP_P = 0.5

# (stride, base size, scales); every level has the aspect ratios below
LEVELS = ((32, 48, (2 ** (1. / 3.), 2 ** (2. / 3.))),
          (64, 96, (2 ** (1. / 3.), 2 ** (2. / 3.))),
          (128, 192, (1, 2 ** (1. / 3.), 2 ** (2. / 3.))))
ASPECT_RATIOS = (0.667, 1, 1.5)


def default_edge_anchors(image_size):
    """-> float32 [A, 4] = y0, x0, y1, x1 of every default anchor on an image_size x image_size image."""
    rows = []
    for stride, size, scales in LEVELS:
        side = int(np.ceil(np.float32(image_size) / stride))
        centre = (stride / 2. + stride * np.arange(side)).astype(np.float32)
        cy, cx = np.meshgrid(centre, centre, indexing='ij')
        for scale in scales:
            for ratio in ASPECT_RATIOS:
                h = np.float32(size * scale / float(ratio) ** 0.5)
                w = np.float32(size * scale * float(ratio) ** 0.5)
                half_h, half_w = h / np.float32(2.), w / np.float32(2.)
                rows.append(np.stack([cy - half_h, cx - half_w, cy + half_h, cx + half_w], -1).reshape(-1, 4))
    return np.concatenate(rows).astype(np.float32)


class ProposalNet(nn.Module):
    """The navigator: three strided 3 x 3 convolutions on the layer4 map, a 1 x 1 convolution per level whose channels
    are that level's (scale, ratio) anchors - [B, A] scores in the anchor table's order (NTSNet.py:63-85)."""

    def __init__(self):
        super().__init__()
        self.down1 = nn.Conv2d(FEATURES, 128, 3, 1, 1)
        self.down2 = nn.Conv2d(128, 128, 3, 2, 1)
        self.down3 = nn.Conv2d(128, 128, 3, 2, 1)
        self.ReLU = nn.ReLU()
        self.tidy1 = nn.Conv2d(128, 6, 1, 1, 0)
        self.tidy2 = nn.Conv2d(128, 6, 1, 1, 0)
        self.tidy3 = nn.Conv2d(128, 9, 1, 1, 0)

    def forward(self, x):
        b = x.size(0)
        d1 = self.ReLU(self.down1(x))
        d2 = self.ReLU(self.down2(d1))
        d3 = self.ReLU(self.down3(d2))
        return torch.cat((self.tidy1(d1).reshape(b, -1), self.tidy2(d2).reshape(b, -1), self.tidy3(d3).reshape(b, -1)), dim=1)


@MODEL.register
class NTSNet(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.topN = config.proposal_num
        self.proposal_num = config.proposal_num
        self.CAT_NUM = config.cat_num
        self.image_size = config.image_size
        if not 1 <= self.CAT_NUM <= self.topN:
            raise ValueError(f'NTSNet: cat_num {self.CAT_NUM} must lie in [1, proposal_num = {self.topN}]')
        self.pretrained_model = resnet50(pretrained=True)
        self.pretrained_model.avgpool = nn.AdaptiveAvgPool2d(1)
        self.pretrained_model.fc = nn.Linear(FEATURES, CLASSES)
        self.proposal_net = ProposalNet()
        self.concat_net = nn.Linear(FEATURES * (self.CAT_NUM + 1), CLASSES)
        self.partcls_net = nn.Linear(FEATURES, CLASSES)
        self.pad_side = PAD_SIDE
        self.edge_anchors = (default_edge_anchors(self.image_size) + np.float32(PAD_SIDE)).astype(int)
        # the device copy, in image coordinates (IoU does not see the shift): what hk_nts_nms returns feeds the crop as it is
        self.register_buffer('_anchors', torch.from_numpy((self.edge_anchors - PAD_SIDE).astype(np.int32)), persistent=False)

    def trunk(self, x):
        """-> (logits, the layer4 map, the pooled feature after dropout): the three outputs of the reference's trunk."""
        t = self.pretrained_model
        x = t.maxpool(t.relu(t.bn1(t.conv1(x))))
        fmap = t.layer4(t.layer3(t.layer2(t.layer1(x))))
        feature = F.dropout(HF.osme_gap(fmap), DROP_P, self.training)
        return HF.linear(feature, t.fc.weight, t.fc.bias), fmap, feature

    def forward(self, x):
        batch = x.size(0)
        raw_logits, rpn_feature, feature = self.trunk(x)
        rpn_score = self.proposal_net(rpn_feature.detach())
        if rpn_score.shape[1] != self._anchors.shape[0]:
            raise ValueError(f'NTSNet: {rpn_score.shape[1]} proposal scores for {self._anchors.shape[0]} anchors: the input must be '
                             f'{self.image_size} x {self.image_size} (config.image_size), got {tuple(x.shape)}')
        top_n_index, boxes = HF.nts_nms(rpn_score, self._anchors, self.topN, 0.25)
        top_n_prob = torch.gather(rpn_score, dim=1, index=top_n_index)
        part_imgs = HF.nts_crop_resize(x, boxes, self.pad_side, PAD_SIDE)                    # [B topN, 3, 224, 224], detached
        _, _, part_features = self.trunk(part_imgs)
        part_feature = part_features.view(batch, self.topN, -1)[:, :self.CAT_NUM].reshape(batch, -1)
        concat_out = torch.cat([part_feature, feature], dim=1)
        concat_logits = HF.linear(concat_out, self.concat_net.weight, self.concat_net.bias)
        part_logits = HF.linear(part_features, self.partcls_net.weight, self.partcls_net.bias).view(batch, self.topN, -1)
        return [raw_logits, concat_logits, part_logits, top_n_index, top_n_prob]
