"""MGE-CNN plugin (mixture of granularity-specific experts; mirrors model/methods/MGE_CNN/MGE.py:75-245 and grad_cam.py): three
ResNet-50 experts look at the image, at the box its class activation map selects, and at the box inside that box; each expert
has a part branch (`conv6*`: a padded 1 x 1 convolution, ReLU and a global max pool on the detached layer-3 map) and a classifier on
the normalised concatenation; a fourth trunk gates the three concatenated verdicts.

Interface kept from the reference: `LocalCamNet(config)` and the factory `MGE_CNN(config)` with `config.num_classes`,
`config.box_thred`, `config.image_size`; the attributes `conv4`, `conv5`, `pool`, `classifier` and their `_box`, `_box_2`, `_gate`
copies, `conv6`, `conv6_1`, `conv6_2`, `cls_part*`, `cls_cat*`, `cls_cat_a`, `cls_gate`, `pool_max`; the `Classifier` wrapper; the
state_dict keys and their order; `get_params(prefix)`; `forward(x, y=None, is_vis=False, vis_idx=None, gt_top=None)` ->
`{'logits': [logits, logits_max, logits_cat, logits_box, logits_max_1, logits_cat_1, logits_box_2, logits_max_2, logits_cat_2,
logits_gate], 'pr_gate': [B,3]}`.

What runs where.  Grad-CAM: the reference runs an eval-mode forward of `conv5` and an autograd backward through it twice per
step, only to average the gradient at the last block's output; that output feeds AdaptiveAvgPool2d(1) and a Linear, so the
gradient at every pixel is W[idx,c] / (h w) and the CAM weight relu(W[idx,c]) / (h w) - no backward at all.  W is the MAIN
classifier's for both boxes: ModelOutputs.__call__ uses `self.model.classifier`, not its `classifier` argument (grad_cam.py:43-48).
The class index is `y` when given (or `gt_top` under `is_vis` with the matching `vis_idx`); otherwise the argmax of the main
classifier on the branch's pooled conv5 features in eval mode - in eval mode the features in hand, in training mode one extra
no-grad forward of that branch's `conv5` with its BatchNorms in eval mode (running statistics untouched).  The CAM, its
upsampling, the threshold and the box are one launch (`hk_mge_cam_bbox`), the crop is `hk_nts_crop_resize`, the part branch is
`hk_mge_partpool_fwd / bwd` (the [B, 10 classes, H + 2, W + 2] map is never written and its backward is a gather), every
classifier runs on `hk_linear_fwd / bwd`.  Nothing between the images and the logits synchronises with the host; the reference's
get_bbox loops over the images with nonzero() and a tensor comparison in an `if`.  Left on PyTorch ops (out of scope): the four
trunks, the average pools, the `l2_norm_v2` concatenations, and the gate's softmax mix.

Deviations from the reference:
  * GradCam calls `model.zero_grad()` and leaves its one-hot gradients in `.grad` during the forward; the reference's trainer
    clears both with `optimizer.zero_grad()` before `loss.backward()`.  Here `.grad` is left alone.
  * A constant class activation map, or one without a pixel >= box_thred, gives the whole image; the reference divides by a zero
    range and raises on the empty nonzero().
  * The `pretrained=True` trunk weights are looked up offline by the backbone, like the other plugins'.

Registration is opt-in: `import hawkeye_amd.model.methods.MGE_CNN` puts `MGE_CNN` into MODEL (importing `hawkeye_amd.model`
alone does not); `hawkeye_amd.examples.MGE_CNN` does that import."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import functional as HF
from ..backbone import resnet50
from ..registry import MODEL

FEATURES = 2048          # layer4's width
PART_IN = 1024           # layer3's width: what conv6* read
PARTS_PER_CLASS = 10


def l2_norm_v2(input):
    input_size = input.size()
    _output = input / (torch.norm(input, p=2, dim=-1, keepdim=True))
    return _output.view(input_size)


class Classifier(nn.Module):
    def __init__(self, in_panel, out_panel, bias=False):
        super().__init__()
        self.fc = nn.Linear(in_panel, out_panel, bias=bias)

    def forward(self, input):
        logit = HF.linear(input if input.dim() > 1 else input.unsqueeze(0), self.fc.weight, self.fc.bias)
        return logit


def eval_features(conv5, conv4_map):
    """conv5(conv4_map) as the module computes it in eval mode, without touching its mode, its running statistics or autograd."""
    norms = [m for m in conv5.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training]
    for m in norms:
        m.training = False
    try:
        with torch.no_grad():
            return conv5(conv4_map)
    finally:
        for m in norms:
            m.training = True


class LocalCamNet(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        self.config = config
        self.num_classes = config.num_classes
        self.box_thred = config.box_thred
        self.image_size = config.image_size
        parts = PARTS_PER_CLASS * self.num_classes

        basenet = resnet50(pretrained=True)
        self.conv4 = nn.Sequential(*list(basenet.children())[:-3])
        self.conv5 = nn.Sequential(*list(basenet.children())[-3])
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.classifier = Classifier(FEATURES, self.num_classes, bias=True)

        self.conv4_box = copy.deepcopy(self.conv4)
        self.conv5_box = copy.deepcopy(self.conv5)
        self.classifier_box = Classifier(FEATURES, self.num_classes, bias=True)
        self.conv4_box_2 = copy.deepcopy(self.conv4)
        self.conv5_box_2 = copy.deepcopy(self.conv5)
        self.classifier_box_2 = Classifier(FEATURES, self.num_classes, bias=True)

        self.conv6_1 = nn.Conv2d(PART_IN, parts, 1, 1, 1)
        self.conv6_2 = nn.Conv2d(PART_IN, parts, 1, 1, 1)
        self.conv6 = nn.Conv2d(PART_IN, parts, 1, 1, 1)
        self.cls_part_1 = Classifier(parts, self.num_classes, bias=True)
        self.cls_part_2 = Classifier(parts, self.num_classes, bias=True)
        self.cls_part = Classifier(parts, self.num_classes, bias=True)
        self.cls_cat_1 = Classifier(FEATURES + parts, self.num_classes, bias=True)
        self.cls_cat_2 = Classifier(FEATURES + parts, self.num_classes, bias=True)
        self.cls_cat = Classifier(FEATURES + parts, self.num_classes, bias=True)
        self.pool_max = nn.AdaptiveMaxPool2d(1)
        self.cls_cat_a = Classifier(3 * (FEATURES + parts), self.num_classes, bias=True)

        self.conv4_gate = copy.deepcopy(self.conv4)
        self.conv5_gate = copy.deepcopy(self.conv5)
        self.cls_gate = nn.Sequential(Classifier(FEATURES, 512, bias=True), Classifier(512, 3, bias=True))

    def cam_index(self, given, conv5, conv4_map, pooled):
        """The class whose activation map selects the box: `given`, or the main classifier's verdict on the branch's eval-mode
        features (`pooled` [B, 2048]: this forward's, which are those in eval mode)."""
        if given is not None:
            return given
        if self.training:
            pooled = self.pool(eval_features(conv5, conv4_map.detach())).flatten(1)
        with torch.no_grad():
            return torch.argmax(self.classifier(pooled.detach()), dim=-1)

    def expert(self, images, conv4, conv5, classifier, conv6, cls_part, cls_cat):
        b = images.size(0)
        conv4_map = conv4(images)
        conv5_map = conv5(conv4_map)
        pooled = self.pool(conv5_map).view(b, -1)
        logits = classifier(pooled)
        pool_conv6 = HF.mge_partpool(conv4_map.detach(), conv6.weight, conv6.bias)
        pool_cat = torch.cat((10 * l2_norm_v2(pooled.detach()), 10 * l2_norm_v2(pool_conv6.detach())), dim=1)
        return conv4_map, conv5_map, pooled, [logits, cls_part(pool_conv6), cls_cat(pool_cat)]

    def box_images(self, images, given, conv5, conv4_map, conv5_map, pooled):
        index = self.cam_index(given, conv5, conv4_map, pooled)
        boxes = HF.mge_cam_bbox(conv5_map, self.classifier.fc.weight, index, self.box_thred, self.image_size)
        return HF.nts_crop_resize(images, boxes, 0, self.image_size), boxes

    def forward(self, x, y=None, is_vis=False, vis_idx=None, gt_top=None):
        if x.dim() != 4 or x.shape[2] != self.image_size or x.shape[3] != self.image_size:
            raise ValueError(f'MGE_CNN: the input must be [B, 3, {self.image_size}, {self.image_size}] (config.image_size), got {tuple(x.shape)}')
        b = x.size(0)
        targets = [gt_top if is_vis and vis_idx == k else y for k in (1, 2)]
        conv4, conv5, pooled, logits_list = self.expert(x, self.conv4, self.conv5, self.classifier, self.conv6, self.cls_part, self.cls_cat)
        input_box, boxes = self.box_images(x, targets[0], self.conv5, conv4, conv5, pooled)
        conv4_box, conv5_box, pooled_box, out = self.expert(input_box, self.conv4_box, self.conv5_box, self.classifier_box, self.conv6_1,
                                                            self.cls_part_1, self.cls_cat_1)
        logits_list += out
        input_box_2, boxes_2 = self.box_images(input_box, targets[1], self.conv5_box, conv4_box, conv5_box, pooled_box)
        out = self.expert(input_box_2, self.conv4_box_2, self.conv5_box_2, self.classifier_box_2, self.conv6_2, self.cls_part_2,
                          self.cls_cat_2)[3]
        logits_list += out

        pool_gate = self.pool(self.conv5_gate(self.conv4_gate(x))).view(b, -1)
        pr_gate = F.softmax(self.cls_gate(pool_gate), dim=1)
        logits_gate = torch.stack([logits_list[2].detach(), logits_list[5].detach(), logits_list[8].detach()], dim=-1)
        logits_gate = (logits_gate * pr_gate.view(pr_gate.size(0), 1, pr_gate.size(1))).sum(-1)
        self.boxes = (boxes, boxes_2)                      # int32 [B,1,4] y0, x0, y1, x1 on the device: for visualisation and the tests
        return {'logits': logits_list + [logits_gate], 'pr_gate': pr_gate}

    def get_params(self, prefix='extractor'):
        """'extractor' / 'extract': the four trunks' parameters (conv5 before conv4, branch by branch, as the reference lists
        them); 'classifier': an iterator over everything else, in parameters() order."""
        trunks = [getattr(self, stage + branch) for branch in ('', '_box', '_box_2', '_gate') for stage in ('conv5', 'conv4')]
        extractor = [q for m in trunks for q in m.parameters()]
        if prefix in ('extractor', 'extract'):
            return extractor
        if prefix == 'classifier':
            ids = {id(q) for q in extractor}
            return (q for q in self.parameters() if id(q) not in ids)
        return None


@MODEL.register
def MGE_CNN(config):
    return LocalCamNet(config)
