"""DCL plugin (Destruction and Construction Learning; mirrors model/methods/DCL.py:8-46): a ResNet-50 trunk whose last map
feeds three readers - the class classifier and the swap classifier on its spatial mean, and the region-alignment mask
`tanh(avgpool2x2(Convmask(map)))`, which the loss compares with the swap law of the batch.

Interface kept from the reference: `DCL(config)` with `config.num_classes`, `config.cls_2` and `config.cls_2xmul` (plus
the optional `pretrained`, True when absent); attributes `num_classes`, `cls_2`, `cls_2xmul`, `backbone` (the `Sequential`
of the ResNet-50 children without the last two), `Convmask` (`Conv2d(2048, 1, 1)` with bias), `avgpool2`, `avgpool`,
`classifier` (`Linear(2048, num_classes)`, no bias) and `classifier_swap` (`Linear(2048, 2)` for `cls_2`,
`Linear(2048, 2 num_classes)` for `cls_2xmul`, which wins when both are set); the state_dict keys; `forward(x)` ->
`[logits, swap_logits, mask]`.  With neither `cls_2` nor `cls_2xmul` there is no `classifier_swap` and `forward` fails
with an AttributeError, as the reference's does.

What runs where: the trunk is PyTorch-ROCm (MIOpen); the head is one autograd node (`hk_dcl_head_fwd / _bwd`,
csrc/dcl.hip) that reads the last map once forward and once backward; the two classifiers run on `hk_linear_fwd / bwd`.
Nothing synchronises with the host.

Deviations from the reference:
  * the `pretrained=True` trunk weights are looked up offline by the backbone (`backbone/pretrained.py`), like the other
    plugins'; a missing file leaves the initialisation in place, with one warning;
  * `avgpool2` and `avgpool` are kept as modules (parameter-free, callable on their own) but `forward` does not go through
    them: a forward hook on either never fires;
  * the spatial mean and the 1 x 1 convolution are summed in the kernel's fixed order, not ATen's.

Registration is opt-in: `import hawkeye_amd.model.methods.DCL` puts it into MODEL (importing `hawkeye_amd.model` alone
does not); `hawkeye_amd.examples.DCL` does that import."""
import torch.nn as nn

from ... import functional as HF
from ..backbone.resnet import resnet50
from ..registry import MODEL

FEATURES = 2048


@MODEL.register
class DCL(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.num_classes = config.num_classes
        self.cls_2 = config.cls_2
        self.cls_2xmul = config.cls_2xmul
        pretrained = config.pretrained if 'pretrained' in config else True

        trunk = resnet50(pretrained=pretrained)
        self.backbone = nn.Sequential(*list(trunk.children())[:-2])
        self.Convmask = nn.Conv2d(FEATURES, 1, 1, stride=1, padding=0, bias=True)
        self.avgpool2 = nn.AvgPool2d(2, stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(output_size=1)
        self.classifier = nn.Linear(FEATURES, self.num_classes, bias=False)
        if self.cls_2:
            self.classifier_swap = nn.Linear(FEATURES, 2, bias=False)
        if self.cls_2xmul:                                 # set after cls_2: the 2 K classifier wins when both are asked for
            self.classifier_swap = nn.Linear(FEATURES, 2 * self.num_classes, bias=False)

    def forward(self, x):
        swap = self.classifier_swap                        # neither cls_2 nor cls_2xmul: an AttributeError, as in the reference
        pooled, mask = HF.dcl_head(self.backbone(x), self.Convmask.weight, self.Convmask.bias)
        return [HF.linear(pooled, self.classifier.weight), HF.linear(pooled, swap.weight), mask]
