"""InterpParts plugin (interpretable region grouping; mirrors model/methods/Interp_Parts.py:9-371): a ResNet trunk up to
layer 3, a grouping unit that assigns every pixel of the layer-3 map softly to `num_parts` learned centres and codes each
part as the normalised residual of its assignment-weighted mean feature, and a tail of 1 x 1 bottlenecks over the part
axis - an attention per part, a post-processing block, the attention-weighted sum, a BatchNorm and the classifier.  The
criterion (`model/loss/InterpParts_loss.py`) shapes the assignment maps' occurrence statistics.

Interface kept from the reference: `IP_ResNet50(config)` / `IP_ResNet101(config)` with `config.num_classes` and
`config.num_parts`; the class `ResNet(block, layers, num_classes=1000, num_parts=32)` with the attributes `inplanes`,
`n_parts`, `num_classes`, `conv1`, `bn1`, `relu`, `maxpool`, `layer1..3`, `grouping`, `post_block`, `attconv`, `groupingbn`
and `mylinear`; `GroupingUnit(in_channels, num_parts)` with `weight` [K,C,1,1], `smooth_factor` [K], `reset_parameters`
and the reference's `__repr__`; `Bottleneck1x1`; the state_dict keys; the initialisation (kaiming fan-out for every
convolution, BatchNorm at 1 / 0, the last BatchNorm of every block zeroed, the centres MSRA-initialised and clamped at
1e-5, the smooth factors 0); `forward(x)` -> `(logits, att, assign)`.

What runs where: the trunk is PyTorch-ROCm (MIOpen); the grouping unit is one autograd node (`hk_ip_group_fwd / _bwd`,
csrc/interp.hip) that reads the layer-3 map once forward and once backward; the classifier runs on `hk_linear_fwd / bwd`.
Nothing synchronises with the host.

Deviations from the reference:
  * the tail (`attconv`, `post_block`, the softmax over parts, the weighted sum, `groupingbn`) works on N x num_parts
    positions: it stays on PyTorch ops, and fusing it is out of scope;
  * the sums of the grouping unit (over channels, pixels and tiles) are taken in the kernel's fixed order, not ATen's;
  * the pretrained trunk weights are looked up offline (`backbone/pretrained.py`) and copied where name and shape agree,
    as the reference's `load_state_dict(strict=False)` does; a missing file leaves the initialisation in place, with one
    warning.  `config.pretrained: False` skips the lookup;
  * the grouping unit serves 1 to 32 parts and a multiple of 64 channels up to 1024 (the plugin's 1024) and raises otherwise.

Registration is opt-in: `import hawkeye_amd.model.methods.InterpParts` puts `IP_ResNet50` and `IP_ResNet101` into MODEL
(importing `hawkeye_amd.model` alone does not); `hawkeye_amd.examples.InterpParts` does that import."""
import torch
import torch.nn as nn
import torch.nn.functional as TF

from ... import functional as HF
from ..backbone import pretrained as _pre
from ..backbone.resnet import Bottleneck
from ..registry import MODEL
from ..utils import load_state_dict


class GroupingUnit(nn.Module):
    def __init__(self, in_channels, num_parts):
        super().__init__()
        self.num_parts = num_parts
        self.in_channels = in_channels
        self.weight = nn.Parameter(torch.empty(num_parts, in_channels, 1, 1, dtype=torch.float32))
        self.smooth_factor = nn.Parameter(torch.empty(num_parts, dtype=torch.float32))

    def reset_parameters(self, init_weight=None, init_smooth_factor=None):
        if init_weight is None:
            nn.init.kaiming_normal_(self.weight)           # msra
            self.weight.data.clamp_(min=1e-5)
        else:                                              # centres from a clustering
            assert init_weight.shape == (self.num_parts, self.in_channels)
            with torch.no_grad():
                self.weight.copy_(init_weight.unsqueeze(2).unsqueeze(3))
        if init_smooth_factor is None:
            nn.init.constant_(self.smooth_factor, 0)       # before the sigmoid
        else:
            assert init_smooth_factor.shape == (self.num_parts,)
            with torch.no_grad():
                self.smooth_factor.copy_(init_smooth_factor)

    def forward(self, inputs):
        assert inputs.dim() == 4 and inputs.size(1) == self.in_channels
        return HF.ip_group(inputs, self.weight, self.smooth_factor)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_channels) + ' -> ' + str(self.num_parts) + ')'


class Bottleneck1x1(nn.Module):
    """The ResNet bottleneck with a 1 x 1 convolution in the middle: the tail works on [N, C, num_parts, 1] maps."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=1, stride=stride, padding=0, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        residual = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out += residual
        return self.relu(out)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, num_parts=32):
        super().__init__()
        self.inplanes = 64
        self.n_parts = num_parts
        self.num_classes = num_classes

        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)

        self.grouping = GroupingUnit(256 * block.expansion, num_parts)
        self.grouping.reset_parameters(init_weight=None, init_smooth_factor=None)

        self.post_block = nn.Sequential(
            Bottleneck1x1(1024, 512, stride=1, downsample=nn.Sequential(
                nn.Conv2d(1024, 2048, kernel_size=1, stride=1, bias=False),
                nn.BatchNorm2d(2048))),
            Bottleneck1x1(2048, 512, stride=1),
            Bottleneck1x1(2048, 512, stride=1),
            Bottleneck1x1(2048, 512, stride=1),
        )
        self.attconv = nn.Sequential(
            Bottleneck1x1(1024, 256, stride=1),
            Bottleneck1x1(1024, 256, stride=1),
            nn.Conv2d(1024, 1, kernel_size=1, stride=1, padding=0, bias=True),
            nn.BatchNorm2d(1),
            nn.ReLU(),
        )
        self.groupingbn = nn.BatchNorm2d(2048)
        self.mylinear = nn.Linear(2048, num_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        for m in self.modules():                           # the last BatchNorm of every residual block starts at zero
            if isinstance(m, (Bottleneck, Bottleneck1x1)):
                nn.init.constant_(m.bn3.weight, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer3(self.layer2(self.layer1(x)))

        region_feature, assign = self.grouping(x)          # [N, C, K], [N, K, H, W]
        region_feature = region_feature.contiguous().unsqueeze(3)

        att = TF.softmax(self.attconv(region_feature), dim=2)
        region_feature = self.post_block(region_feature)

        out = (region_feature * att).contiguous().squeeze(3)
        out = TF.avg_pool1d(out, self.n_parts) * self.n_parts      # the attention-weighted sum over the parts
        out = self.groupingbn(out.contiguous().unsqueeze(3))
        out = out.contiguous().view(out.size(0), -1)
        return HF.linear(out, self.mylinear.weight, self.mylinear.bias), att, assign


def _build(arch, layers, config):
    net = ResNet(Bottleneck, layers, config.num_classes, config.num_parts)
    if config.pretrained if 'pretrained' in config else True:
        sd = _pre.load(arch)
        if sd is not None:
            load_state_dict(net, sd)                       # the trunk's entries; `layer4.*` and `fc.*` have no counterpart
    return net


@MODEL.register
def IP_ResNet50(config):
    return _build('resnet50', [3, 4, 6, 3], config)


@MODEL.register
def IP_ResNet101(config):
    return _build('resnet101', [3, 4, 23, 3], config)
