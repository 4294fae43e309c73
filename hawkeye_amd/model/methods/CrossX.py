"""CrossX plugin (mirrors model/methods/CrossX.py:47-270): a ResNet-50 whose last `layer3` and `layer4` bottlenecks end
in a one-squeeze multi-excitation ("ME") block - one global average of the block's bn3 output, `num_parts` gate MLPs
(`Linear(C, C / 256)`, ReLU, `Linear(C / 256, C)`, sigmoid), and a part map `relu(out * gate_p + residual)` per gate
next to the ordinary `relu(out + residual)`.  Three classifiers read the parts: `fc_plty` the spatial maxima of the
`layer3` parts, `fc_ulti` the spatial means of the `layer4` parts, `fc_cmbn` the means of
`bn3_i(conv3_i(layer3 part i + upsample(conv2_i(layer4 part i))))`.

Interface kept from the reference: `CrossX(config)` with `config.num_parts` (1 to 3) and the optional `num_classes`
(200) and `pretrained` (True); attributes `nparts`, `nclass`, `meflag`, `adpavgpool`, `fc_ulti` and, for more than one
part, `adpmaxpool`, `fc_plty`, `fc_cmbn`, `conv2_i`, `conv3_i`, `bn3_i`; the ME bottlenecks' `me.avg_pool` and
`me.parts.{p}.{0..3}`; the state_dict keys and their order; the initialisation (normal(0, sqrt(2 / (k k out))) for every
convolution, BatchNorm at 1 / 0, the Linears' defaults); `forward(x)` -> `(ulti_logits, plty_logits, cmbn_logits,
ulti_parts, plty_parts, cmbn_ftres)` with each list holding `num_parts` features `[B,C,1,1]`.  With one part there is no
ME block and `forward` returns plain logits.

What runs where: the trunk's convolutions and BatchNorm are PyTorch-ROCm (MIOpen), and so are the gate MLPs (four tiny
GEMMs per block); the squeeze is `hk_osme_gap`; the tail of an ME bottleneck - the main map, the P part maps and their
pooled features - is one pass (`hk_crossx_me_fwd`, csrc/crossx.hip), and so is its backward; the combined branch's
upsample + add is `hk_crossx_up_add_fwd` (the upsampled map is never written); the classifiers run on `hk_linear_fwd /
bwd`.  Nothing synchronises with the host.

Deviations from the reference:
  * a `layer3` map that is not 28 x 28 (an input that is not 448 x 448) raises a ValueError; the reference fails there
    too, inside `torch.add`, because it upsamples to a fixed 28;
  * the `pretrained=True` trunk weights are looked up offline by the backbone (`backbone/pretrained.py`), like the other
    plugins', and loaded non-strictly; a missing file leaves the initialisation in place, with one warning;
  * the part maps are views of one `[P,B,C,H,W]` tensor and the pooled features views of one `[P,B,C]` tensor;
  * the mean over a part map is summed in the kernel's fixed order, not ATen's.

Registration is opt-in: `import hawkeye_amd.model.methods.CrossX` puts it into MODEL (importing `hawkeye_amd.model`
alone does not); `hawkeye_amd.examples.CrossX` does that import."""
import math

import torch
import torch.nn as nn

from ... import functional as HF
from ..backbone import pretrained as _pre
from ..backbone.resnet import Bottleneck
from ..registry import MODEL
from ..utils import load_state_dict

LAYERS = (3, 4, 6, 3)
REDUCTION = 256          # the gate MLPs' hidden width is C / 256: 4 on layer3, 8 on layer4
PLTY_SIDE = 28           # the side of the layer3 map that the combined branch upsamples to (a 448 x 448 input)


class MELayer(nn.Module):
    """One squeeze, `nparts` excitations (CrossX.py:47-70)."""

    def __init__(self, channel, reduction=16, nparts=1):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.nparts = nparts
        self.parts = nn.Sequential(*[nn.Sequential(nn.Linear(channel, channel // reduction), nn.ReLU(inplace=True),
                                                   nn.Linear(channel // reduction, channel), nn.Sigmoid()) for _ in range(nparts)])

    def gates(self, x):
        """x [N,C,H,W] -> [P,N,C]"""
        z = HF.osme_gap(x)
        return torch.stack([part(z) for part in self.parts])


class MEBottleneck(Bottleneck):
    """A bottleneck that ends in an ME block (CrossX.py:73-123 with meflag)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None, nparts=1, reduction=1):
        super().__init__(inplanes, planes, stride, downsample)
        self.meflag = True
        self.me = MELayer(planes * self.expansion, nparts=nparts, reduction=reduction)

    def me_forward(self, x, pool):
        """-> main [N,C,H,W], parts [P,N,C,H,W], pooled [P,N,C] ('max' or 'avg' over each part map)"""
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return HF.crossx_me(y, idt, self.me.gates(y), pool)

    def forward(self, x):
        main, parts, _ = self.me_forward(x, 'avg')
        return main, list(parts.unbind(0))


class CrossXNet(nn.Module):
    def __init__(self, nparts=1, meflag=False, num_classes=1000):
        super().__init__()
        self.nparts = nparts
        self.nclass = num_classes
        self.meflag = meflag
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, LAYERS[0])
        self.layer2 = self._make_layer(128, LAYERS[1], stride=2)
        self.layer3 = self._make_layer(256, LAYERS[2], stride=2, meflag=meflag)
        self.layer4 = self._make_layer(512, LAYERS[3], stride=2, meflag=meflag)
        self.adpavgpool = nn.AdaptiveAvgPool2d(1)
        wide, narrow = 512 * Bottleneck.expansion, 256 * Bottleneck.expansion
        self.fc_ulti = nn.Linear(wide * nparts, num_classes)
        if nparts > 1:
            self.adpmaxpool = nn.AdaptiveMaxPool2d(1)
            self.fc_plty = nn.Linear(narrow * nparts, num_classes)
            self.fc_cmbn = nn.Linear(narrow * nparts, num_classes)
            # the reference's order: conv2_1, conv2_2, conv3_1, conv3_2, bn3_1, bn3_2, then the third part's three
            for i in (1, 2):
                setattr(self, f'conv2_{i}', nn.Conv2d(wide, narrow, kernel_size=1, bias=False))
            for i in (1, 2):
                setattr(self, f'conv3_{i}', nn.Conv2d(narrow, narrow, kernel_size=3, padding=1, bias=False))
            for i in (1, 2):
                setattr(self, f'bn3_{i}', nn.BatchNorm2d(narrow))
            if nparts == 3:
                self.conv2_3 = nn.Conv2d(wide, narrow, kernel_size=1, bias=False)
                self.conv3_3 = nn.Conv2d(narrow, narrow, kernel_size=3, padding=1, bias=False)
                self.bn3_3 = nn.BatchNorm2d(narrow)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                nn.init.normal_(m.weight, 0, math.sqrt(2. / fan))
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1, meflag=False):
        down = None
        out = planes * Bottleneck.expansion
        if stride != 1 or self.inplanes != out:
            down = nn.Sequential(nn.Conv2d(self.inplanes, out, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(out))
        layers = [Bottleneck(self.inplanes, planes, stride, down)]
        self.inplanes = out
        for i in range(1, blocks):
            if meflag and i == blocks - 1:
                layers.append(MEBottleneck(out, planes, nparts=self.nparts, reduction=REDUCTION))
            else:
                layers.append(Bottleneck(out, planes))
        return nn.Sequential(*layers)

    @staticmethod
    def _me_stage(layer, x, pool):
        for block in list(layer)[:-1]:
            x = block(x)
        return layer[-1].me_forward(x, pool)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer2(self.layer1(x))
        if not self.meflag:
            x = self.adpavgpool(self.layer4(self.layer3(x))).flatten(1)
            return HF.linear(x, self.fc_ulti.weight, self.fc_ulti.bias)
        x, plty_maps, plty_pool = self._me_stage(self.layer3, x, 'max')
        if tuple(x.shape[2:]) != (PLTY_SIDE, PLTY_SIDE):
            raise ValueError(f'CrossX: the layer3 map is {tuple(x.shape[2:])}, the combined branch needs {PLTY_SIDE} x {PLTY_SIDE}: '
                             f'the input must be {PLTY_SIDE * 16} x {PLTY_SIDE * 16}')
        _, ulti_maps, ulti_pool = self._me_stage(self.layer4, x, 'avg')
        b = x.size(0)
        cmbn_ftres = []
        for i in range(self.nparts):
            conv2, conv3, bn3 = (getattr(self, f'{name}_{i + 1}') for name in ('conv2', 'conv3', 'bn3'))
            both = HF.crossx_up_add(plty_maps[i], conv2(ulti_maps[i]))
            cmbn_ftres.append(HF.osme_gap(bn3(conv3(both))).view(b, -1, 1, 1))
        xp = HF.linear(plty_pool.permute(1, 0, 2).reshape(b, -1), self.fc_plty.weight, self.fc_plty.bias)
        xf = HF.linear(ulti_pool.permute(1, 0, 2).reshape(b, -1), self.fc_ulti.weight, self.fc_ulti.bias)
        xc = HF.linear(torch.cat(cmbn_ftres, 1).view(b, -1), self.fc_cmbn.weight, self.fc_cmbn.bias)
        ulti_parts = [ulti_pool[i].view(b, -1, 1, 1) for i in range(self.nparts)]
        plty_parts = [plty_pool[i].view(b, -1, 1, 1) for i in range(self.nparts)]
        return xf, xp, xc, ulti_parts, plty_parts, cmbn_ftres


@MODEL.register
def CrossX(config):
    nparts = int(config.num_parts)
    if not 1 <= nparts <= 3:
        raise ValueError(f'CrossX: num_parts must be 1, 2 or 3, got {config.num_parts}')
    pretrained = config.pretrained if 'pretrained' in config else True
    num_classes = config.num_classes if 'num_classes' in config else 200
    model = CrossXNet(nparts=nparts, meflag=nparts > 1, num_classes=num_classes)
    if pretrained:
        sd = _pre.load('resnet50')
        if sd is not None:
            load_state_dict(model, sd)
    return model
