"""ResNet encoder + FPN decoder + segmentation head with segmentation_models_pytorch-compatible
module / parameter names.

The reference builds these from `segmentation_models_pytorch` (call sites
F/lib/pose_regressor.py:608-666), which is NOT vendored in /root/reference and is not installed
in this image, so the graph below is re-derived from upstream knowledge of smp at the commit the
reference cites (F/lib/pose_regressor.py:578-580) and could not be cross-checked here
("parity unpinned" for the conv stack — SURVEY.md section 7.2).  What IS checked: every op
against torch.nn.functional on the same tensors (tests/).

Structure (encoder_depth = 5, FPN, merge "add"):
  encoder(x) -> [x, relu(bn1(conv1 x)), layer1(maxpool .), layer2, layer3, layer4]
  FPNDecoder: p5 = 1x1(c5); p4 = up2_nearest(p5) + 1x1(c4); p3; p2;
              seg_blocks[i] = n_i x [conv3x3(no bias) -> GroupNorm(32) -> ReLU (-> up2 bilinear,
              align_corners=True)] with n = 3,2,1,0 upsamples (at least one conv);
              sum of the four 1/4-scale maps; Dropout2d(0.2)
  SegmentationHead: conv 1x1 -> UpsamplingBilinear2d(x4) (align_corners=True) -> Identity
The SE-ResNet encoders (se_resnet50 / 101 / 152) are smp's SENetEncoder over pretrainedmodels.senet, restated the same way
(neither package is here: parity unpinned): encoder.layer0.{conv1,bn1,relu1,pool}, SEResNetBottleneck blocks with
se_module.fc1 / fc2, the same six feature levels.
The MobileNetV2 encoder (mobilenet_v2) is smp's MobileNetV2Encoder over torchvision.models.mobilenet_v2, restated the same way
(neither package is here: parity unpinned): encoder.features.0 .. 18 without the classifier, InvertedResidual blocks with a `conv`
Sequential, ReLU6, the six feature levels behind the input, features.1 / 3 / 6 / 13 / 18.
The EfficientNet-B0 encoder (efficientnet-b0) is smp's EfficientNetEncoder over efficientnet_pytorch.EfficientNet, restated the same
way (neither package is here: parity unpinned): encoder._conv_stem / _bn0, 16 MBConv blocks encoder._blocks.N with the static "same"
pads of the declared 224 image, swish and the squeeze-and-excitation gate, _conv_head / _bn1 kept and not run, the feature levels
behind the stem and blocks 2 / 4 / 8 / 15.
The DenseNet encoders (densenet121 / 169 / 201) are smp's DenseNetEncoder over torchvision.models.densenet, restated the same way
(parity unpinned): encoder.features.conv0 / norm0 / relu0 / pool0, dense blocks of pre-activated 1x1 + 3x3 layers whose outputs are
concatenated, transitions whose post-ReLU tensor is the feature level, norm5 without a ReLU as the last level.  densenet161 is not built.
The VGG encoders (vgg11 / 13 / 16 / 19 and each with _bn) are smp's VGGEncoder over torchvision.models.vgg.make_layers, restated the
same way (neither package is here: parity unpinned): one Sequential encoder.features indexed as torchvision's, 3x3 / pad 1
convolutions with a bias, [BatchNorm,] ReLU, MaxPool2d(2, 2) behind each of five blocks, no classifier; the six feature levels are
the five blocks' outputs IN FRONT of their pools and the last pool's output alone (the first level is not the input image).
state_dict names follow smp: encoder.conv1.weight, encoder.layer1.0.conv1.weight, ...,
<dec>.p5.weight, <dec>.p4.skip_conv.weight, <dec>.seg_blocks.0.block.0.block.0.weight (conv),
...block.1.weight (GroupNorm), <head>.0.weight.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _train_conv():
    """lib/train_conv.py, imported when a training step first needs it."""
    from fastposecnn_amd.lib import train_conv
    return train_conv


def _train_native(ok, front_end, *args, **kw):
    """The one dispatch of the training step's native ops: while `ok` — the caller's own pre-conditions — holds, the front end
    lib/train_conv.<front_end>(*args), an attribute of the module looked up at call time; None when `ok` fails or the front end
    refuses its operands, and the caller runs torch's modules."""
    return getattr(_train_conv(), front_end)(*args, **kw) if ok else None


class Conv2d(nn.Conv2d):
    """nn.Conv2d whose TRAINING-mode forward on a GPU runs on the native kernels, forward and backward
    (lib/train_conv.py); evaluation goes through the engine's plan (or torch, on CPU) as before.  Same parameters and
    state_dict names as nn.Conv2d."""

    def forward(self, x):
        ok = self.training and x.is_cuda and self.dilation == (1, 1) and self.padding_mode == "zeros" \
            and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1] and not isinstance(self.padding, str) \
            and _train_conv().ENABLED      # (groups > 1: torch's grouped convolution on the channel-last tensor)
        y = _train_native(ok, "conv2d", x, self.weight, self.bias, self.stride[0], self.padding[0], self.groups)
        return super().forward(x) if y is None else y


def _upsample_bilinear(x, scale, out_nchw=False):
    """Bilinear, align_corners=True.  Under autograd on a GPU (the training step) the native forward / backward kernels of
    lib/train_conv.py; plain torch otherwise (inference goes through the engine's plan and never gets here)."""
    y = _train_native(x.is_cuda and torch.is_grad_enabled() and x.requires_grad, "upsample_bilinear", x, scale, out_nchw)
    return F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True) if y is None else y


class UpsamplingBilinear2d(nn.UpsamplingBilinear2d):
    """nn.UpsamplingBilinear2d of the heads; the training step's forward / backward run natively (NCHW result)."""

    def forward(self, x):
        if float(self.scale_factor) in (2.0, 4.0):
            return _upsample_bilinear(x, int(self.scale_factor), out_nchw=True)
        return super().forward(x)


class BatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d whose TRAINING-mode forward on a channel-last GPU tensor under autograd runs on the native kernels, forward
    and backward (csrc/batchnorm.hip, lib/train_conv.batchnorm_act); everything else — evaluation mode, CPU tensors, a no_grad
    forward, whatever the front end refuses — is nn.BatchNorm2d's own forward.  Same parameters, buffers and state_dict names;
    the engine folds it at plan build like any nn.BatchNorm2d."""

    def forward(self, x):
        y = _train_native(x.is_cuda and torch.is_grad_enabled(), "batchnorm_act", x, self, relu=False)
        return super().forward(x) if y is None else y


class MaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d whose 3x3 / stride-2 / pad-1 forward on a dense channel-last f32 GPU tensor that requires grad runs on the
    native kernels, forward and backward, when FPC_TRAIN_NATIVE_STEM=1 (lib/train_conv.maxpool3x3s2, csrc/stem_train.hip);
    everything else — another geometry, return_indices, ceil_mode, CPU tensors, a no_grad forward, the switch off (its default) —
    is nn.MaxPool2d's own forward.  No parameters: state_dicts are untouched."""

    def forward(self, x):
        ok = x.is_cuda and torch.is_grad_enabled() and x.requires_grad and not self.return_indices and not self.ceil_mode \
            and self.kernel_size in (3, (3, 3)) and self.stride in (2, (2, 2)) and self.padding in (1, (1, 1)) \
            and self.dilation in (1, (1, 1))
        y = _train_native(ok, "maxpool3x3s2", x)
        return super().forward(x) if y is None else y


def _bn_act(x, bn, act, res=None):
    """act(bn(x) + res) at a block's BatchNorm.  In the training step BatchNorm, the add and the ReLU are one native op; the
    ReLU (and with it the add) is fused only while `act` is an nn.ReLU — a test may have swapped it for a smooth activation,
    and then the BatchNorm runs native and plain (its own forward), the add and the activation stay torch."""
    ok = isinstance(act, nn.ReLU) and isinstance(bn, BatchNorm2d) and bn.training and x.is_cuda and torch.is_grad_enabled()
    y = _train_native(ok, "batchnorm_act", x, bn, res, relu=True, count_refusal=False)      # (refused: bn(x) below asks again, plain)
    if y is not None:
        return y
    y = bn(x)
    if res is not None:
        y = y + res
    return act(y)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = _bn_act(self.conv1(x), self.bn1, self.relu)
        out = self.conv2(out)
        identity = x if self.downsample is None else self.downsample(x)
        return _bn_act(out, self.bn2, self.relu, identity)


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (ResNet V1.5, which smp's ResNetEncoder subclasses): 1x1 -> 3x3 (the stride) -> 1x1 x 4.
    ResNeXt: the 3x3 in `groups` groups over a middle of int(planes * base_width / 64) * groups channels."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * base_width / 64) * groups
        self.conv1 = Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = BatchNorm2d(width)
        self.conv2 = Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = BatchNorm2d(width)
        self.conv3 = Conv2d(width, planes * self.expansion, 1, bias=False)
        self.bn3 = BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = _bn_act(self.conv1(x), self.bn1, self.relu)
        out = _bn_act(self.conv2(out), self.bn2, self.relu)
        out = self.conv3(out)
        identity = x if self.downsample is None else self.downsample(x)
        return _bn_act(out, self.bn3, self.relu, identity)


class SEModule(nn.Module):
    """pretrainedmodels.senet.SEModule: x * sigmoid(fc2(relu(fc1(avgpool(x))))), fc1 / fc2 1x1 convolutions WITH bias.  Its own
    forward is plain torch modules; the engine's plan runs the gate on k_se_pool / k_se_excite (csrc/se.hip) at inference, and in the
    training step with FPC_TRAIN_NATIVE_SE=1 SEResNetBottleneck runs it, fused with its add and ReLU, on the same kernels and on
    csrc/se_train.hip (lib/train_conv.se_gate_add_relu) — from these parameters, whose names and shapes stay as they are."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        g = self.sigmoid(self.fc2(self.relu(self.fc1(self.avg_pool(x)))))
        return x * g


class SEResNetBottleneck(nn.Module):
    """pretrainedmodels.senet.SEResNetBottleneck (the Caffe-style ResNet: the stride on conv1, a 1x1) with the squeeze-and-
    excitation gate between bn3 and the residual add: relu(se_module(bn3(conv3(.))) + residual).  bn3 therefore never fuses the
    add or the ReLU.  Gate, add and ReLU are torch ops by default; under autograd on a GPU with FPC_TRAIN_NATIVE_SE=1 they are one
    native op each way (lib/train_conv.se_gate_add_relu), which whatever it refuses — another layout or dtype, a swapped
    activation, the switch off — hands back to the torch lines."""
    expansion = 4

    def __init__(self, inplanes, planes, reduction, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1, stride, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = _bn_act(self.conv1(x), self.bn1, self.relu)
        out = _bn_act(self.conv2(out), self.bn2, self.relu)
        out = self.bn3(self.conv3(out))
        residual = x if self.downsample is None else self.downsample(x)
        y = _train_native(out.is_cuda and torch.is_grad_enabled(), "se_gate_add_relu", out, self.se_module, residual, self.relu)
        return self.relu(self.se_module(out) + residual) if y is None else y


# name -> (block, blocks per stage, groups, width per group, squeeze-and-excitation reduction: 0 without the gate), as torchvision /
# smp for the ResNets and ResNeXts, smp's SENetEncoder over pretrainedmodels.senet for the SE-ResNets
_ENCODERS = {"resnet18": (BasicBlock, [2, 2, 2, 2], 1, 64, 0), "resnet34": (BasicBlock, [3, 4, 6, 3], 1, 64, 0),
             "resnet50": (Bottleneck, [3, 4, 6, 3], 1, 64, 0), "resnet101": (Bottleneck, [3, 4, 23, 3], 1, 64, 0),
             "resnet152": (Bottleneck, [3, 8, 36, 3], 1, 64, 0),
             "resnext50_32x4d": (Bottleneck, [3, 4, 6, 3], 32, 4, 0), "resnext101_32x4d": (Bottleneck, [3, 4, 23, 3], 32, 4, 0),
             "resnext101_32x8d": (Bottleneck, [3, 4, 23, 3], 32, 8, 0),
             "se_resnet50": (SEResNetBottleneck, [3, 4, 6, 3], 1, 64, 16), "se_resnet101": (SEResNetBottleneck, [3, 4, 23, 3], 1, 64, 16),
             "se_resnet152": (SEResNetBottleneck, [3, 8, 36, 3], 1, 64, 16)}


def encoder_family(name):
    """The one look-up the engine switches on: "mobilenet_v2", "efficientnet", "densenet" and "vgg" for the encoders fpc_net_create builds by
    their names, "resnet" for every encoder that encoder_layout / encoder_groups / encoder_reduction describe; KeyError for a name this
    package does not build."""
    if name == MobileNetV2Encoder.NAME:
        return "mobilenet_v2"
    if name in EfficientNetEncoder.VARIANTS:
        return "efficientnet"
    if name in DenseNetEncoder.VARIANTS:
        return "densenet"
    if name in VGGEncoder.VARIANTS:
        return "vgg"
    _ENCODERS[name]
    return "resnet"


def encoder_layout(name):
    """(block expansion, blocks per stage) of encoder `name`: the descriptor fpc_net_create_encoder takes."""
    block, layers = _ENCODERS[name][:2]
    return block.expansion, list(layers)


def encoder_groups(name):
    """(groups, width per group) of encoder `name`: what fpc_net_create_encoder_ex takes beside encoder_layout's pair."""
    return _ENCODERS[name][2:4]


def encoder_reduction(name):
    """The squeeze-and-excitation reduction of encoder `name` (16 for the SE-ResNets: what fpc_net_create_encoder_se takes), 0 for
    every encoder without the gate."""
    return _ENCODERS[name][4]


def _available():
    """The encoder names this package builds, for the KeyError of an unknown one."""
    return sorted(_ENCODERS) + [MobileNetV2Encoder.NAME] + sorted(EfficientNetEncoder.VARIANTS) + sorted(DenseNetEncoder.VARIANTS) \
        + sorted(VGGEncoder.VARIANTS)


def _make_stage(block, inplanes, planes, blocks, stride, **kw):
    """One stage: `blocks` blocks of `planes`, the first with the stride and, where the shape changes, a 1x1 downsample."""
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(Conv2d(inplanes, planes * block.expansion, 1, stride, bias=False),
                                   BatchNorm2d(planes * block.expansion))
    layers = [block(inplanes, planes, stride=stride, downsample=downsample, **kw)]
    layers += [block(planes * block.expansion, planes, **kw) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


class _Encoder(nn.Module):
    """What the encoder classes share: the descriptor look-up, the four stages, the initialisation and the walk over the six
    feature levels.  A subclass says which descriptors are its own (`_gated`), builds its stem and names the stem's four modules."""

    def __init__(self, name, in_channels, depth):
        super().__init__()
        if name not in _ENCODERS or bool(_ENCODERS[name][4]) != self._gated:
            raise KeyError(f"encoder {name!r} not available (have {_available()})")
        block, layers, groups, width, reduction = _ENCODERS[name]
        self.name = name
        self._depth = depth
        e = block.expansion
        self.out_channels = (in_channels, 64, 64 * e, 128 * e, 256 * e, 512 * e)
        self._make_stem(in_channels)
        kw = dict(reduction=reduction) if reduction else dict(groups=groups, base_width=width) if groups > 1 else {}
        inplanes = 64
        for i, planes in enumerate((64, 128, 256, 512)):
            setattr(self, f"layer{i + 1}", _make_stage(block, inplanes, planes, layers[i], 1 if i == 0 else 2, **kw))
            inplanes = planes * e
        # (pretrainedmodels leaves torch's default initialisation; the bias-free convolutions and the BatchNorms of the SE-ResNets
        # start as the ResNet encoders' here, fc1 / fc2 — the only biased ones — keep nn.Conv2d's default.  A checkpoint or a weights
        # file overwrites all of it.)
        for m in self.modules():
            if isinstance(m, nn.Conv2d) and m.bias is None:
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        conv1, bn1, relu, pool = self._stem()
        feats = [x]
        x = _bn_act(conv1(x), bn1, relu)
        feats.append(x)
        x = pool(x)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = layer(x)
            feats.append(x)
        return feats


class ResNetEncoder(_Encoder):
    """torchvision-style ResNet (BasicBlock or Bottleneck) without avgpool/fc, returning 6 feature levels."""
    _gated = False

    def __init__(self, name="resnet18", in_channels=3, depth=5):
        super().__init__(name, in_channels, depth)

    def _make_stem(self, in_channels):
        self.conv1 = Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = MaxPool2d(3, 2, 1)

    def _stem(self):
        return self.conv1, self.bn1, self.relu, self.maxpool


class SENetEncoder(_Encoder):
    """smp's SENetEncoder for the SE-ResNets (pretrainedmodels.senet.SENet with groups = 1, inplanes = 64, a 7x7 stem and 1x1
    downsamples, without avg_pool / last_linear), returning 6 feature levels.  layer0 is the stem as a Sequential of named
    children; its pool is MaxPool2d(3, stride=2, ceil_mode=True) WITHOUT padding (windows start at 0, the last one is clipped),
    a plain nn.MaxPool2d in every mode: the native training pool kernels are pad-1 kernels."""
    _gated = True

    def __init__(self, name="se_resnet50", in_channels=3, depth=5):
        super().__init__(name, in_channels, depth)

    def _make_stem(self, in_channels):
        from collections import OrderedDict
        self.layer0 = nn.Sequential(OrderedDict([
            ("conv1", Conv2d(in_channels, 64, 7, 2, 3, bias=False)), ("bn1", BatchNorm2d(64)), ("relu1", nn.ReLU(inplace=True)),
            ("pool", nn.MaxPool2d(3, stride=2, ceil_mode=True))]))

    def _stem(self):
        return self.layer0.conv1, self.layer0.bn1, self.layer0.relu1, self.layer0.pool


class ConvBNReLU6(nn.Sequential):
    """torchvision's ConvBNReLU / Conv2dNormActivation as MobileNetV2 uses it: conv (no bias, padding (k - 1) / 2) -> BatchNorm ->
    ReLU6, children 0 / 1 / 2.  The activation is a child module: a test may swap it.  In the training step, with
    FPC_TRAIN_NATIVE_MBV2=1 and FPC_TRAIN_NATIVE_BN=1 both set, the BatchNorm and the ReLU6 are one native op each way
    (lib/train_conv.batchnorm_act(relu6=True)) while child 1 is a training BatchNorm2d and child 2 an nn.ReLU6; whatever the front end
    refuses, and every other case, is nn.Sequential's own forward, child by child."""

    def __init__(self, inp, oup, kernel_size=3, stride=1, groups=1):
        super().__init__(Conv2d(inp, oup, kernel_size, stride, (kernel_size - 1) // 2, groups=groups, bias=False),
                         BatchNorm2d(oup), nn.ReLU6(inplace=True))

    def forward(self, x):
        if len(self) == 3 and x.is_cuda and torch.is_grad_enabled():
            conv, bn, act = self[0], self[1], self[2]
            tc = _train_conv()
            if isinstance(act, nn.ReLU6) and isinstance(bn, BatchNorm2d) and bn.training and tc.NATIVE_MBV2 and tc.NATIVE_BN:
                x = conv(x)
                y = _train_native(True, "batchnorm_act", x, bn, relu=False, relu6=True, count_refusal=False)      # (refused: bn(x) asks again, plain)
                return act(bn(x)) if y is None else y
        return super().forward(x)


class InvertedResidual(nn.Module):
    """torchvision.models.mobilenetv2.InvertedResidual: `conv` = [expand 1x1 + BN + ReLU6 (absent where expand_ratio = 1)], the
    depthwise 3x3 with the stride (groups = hidden) + BN + ReLU6, the project 1x1 without bias, its BN; the input is added where the
    stride is 1 and inp = oup, with no activation behind the add.  In the training step the dense 1x1 sites and the BatchNorms run
    on the native kernels lib/train_conv.py already has (Conv2d / BatchNorm2d above); the depthwise convolution and ReLU6 are torch's
    by default and, with FPC_TRAIN_NATIVE_MBV2=1, native too: the convolution on csrc/depthwise.hip, forward and backward (Conv2d above
    reaches lib/train_conv._DepthwiseConv2dFn), ReLU6 as the activation of the native BatchNorm (ConvBNReLU6.forward, with
    FPC_TRAIN_NATIVE_BN=1)."""

    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"stride should be 1 or 2 instead of {stride}")
        self.stride = stride
        hidden = int(round(inp * expand_ratio))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(ConvBNReLU6(inp, hidden, kernel_size=1))
        layers += [ConvBNReLU6(hidden, hidden, stride=stride, groups=hidden), Conv2d(hidden, oup, 1, 1, 0, bias=False), BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)
        self.out_channels = oup

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


class MobileNetV2Encoder(nn.Module):
    """smp's MobileNetV2Encoder: torchvision's MobileNetV2 (width 1.0, round_nearest 8) without its classifier, returning 6 feature
    levels: the input and the outputs of features[:2], [2:4], [4:7], [7:14], [14:].  state_dict names are torchvision's
    (features.0.0.weight, features.2.conv.1.1.running_var, features.18.1.bias)."""
    NAME = "mobilenet_v2"
    # (t, c, n, s): expansion, output channels, blocks, stride of the first block
    SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
    STAGES = (2, 4, 7, 14, 19)      # smp: the feature level i + 1 is the output of features[STAGES[i] - 1]

    def __init__(self, name="mobilenet_v2", in_channels=3, depth=5):
        super().__init__()
        if name != self.NAME:
            raise KeyError(f"encoder {name!r} not available (have {_available()})")
        self.name = name
        self._depth = depth
        self.out_channels = (in_channels, 16, 24, 32, 96, 1280)
        features = [ConvBNReLU6(in_channels, 32, stride=2)]
        inp = 32
        for t, c, n, s in self.SETTING:
            for i in range(n):
                features.append(InvertedResidual(inp, c, s if i == 0 else 1, t))
                inp = c
        features.append(ConvBNReLU6(inp, 1280, kernel_size=1))
        self.features = nn.Sequential(*features)
        # torchvision's initialisation (a checkpoint or a weights file overwrites it)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        feats = [x]
        for i, f in enumerate(self.features):
            x = f(x)
            if i + 1 in self.STAGES:
                feats.append(x)
        return feats


class Swish(nn.Module):
    """efficientnet_pytorch's swish, x * sigmoid(x), as a child module without parameters: a test may swap it."""

    def forward(self, x):
        return x * torch.sigmoid(x)


class Conv2dStaticSamePadding(Conv2d):
    """efficientnet_pytorch's Conv2dStaticSamePadding: a pad-0 convolution behind `static_padding`, the TensorFlow "same" pads worked
    out once from the DECLARED image size at this site (not from the tensor it gets): per axis max((ceil(i / s) - 1) s + k - i, 0)
    cells, the smaller half before.  nn.ZeroPad2d where there is any, nn.Identity otherwise; no parameters, so the state_dict is
    nn.Conv2d's.  Behind the pad the convolution is Conv2d above: in the training step a dense one reaches the native front end
    where that accepts its shape, a depthwise one (k = 5 included) runs on torch's grouped kernels."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, image_size=None, **kw):
        super().__init__(in_channels, out_channels, kernel_size, stride, 0, **kw)
        ih, iw = (image_size, image_size) if isinstance(image_size, int) else image_size
        k, s = self.kernel_size[0], self.stride[0]
        pad_h = max((-(-ih // s) - 1) * s + k - ih, 0)
        pad_w = max((-(-iw // s) - 1) * s + k - iw, 0)
        if pad_h or pad_w:
            self.static_padding = nn.ZeroPad2d((pad_w // 2, pad_w - pad_w // 2, pad_h // 2, pad_h - pad_h // 2))
        else:
            self.static_padding = nn.Identity()

    def forward(self, x):
        return super().forward(self.static_padding(x))


class MBConvBlock(nn.Module):
    """efficientnet_pytorch's MBConvBlock with the gate (se_ratio 0.25 of the block's INPUT width) and the identity skip:
        x1 = swish(bn0(expand(x)))            (absent where expand_ratio = 1: x1 = x)
        x2 = swish(bn1(depthwise(x1)))        (k x k with the block's stride)
        g  = sigmoid(se_expand(swish(se_reduce(mean_hw(x2)))))
        y  = bn2(project(x2 * g));  y = drop_connect(y) + x where the stride is 1 and inp = oup
    drop_connect runs in training only, at `drop_connect_rate` (the encoder sets it per call).  Every BatchNorm has eps 1e-3 and
    momentum 0.01.  The native engine runs all of it at inference (csrc/efficientnet.hip); in the training step the dense 1x1
    sites and the BatchNorms reach the native front ends through Conv2d / BatchNorm2d above, the rest is torch."""

    def __init__(self, inp, oup, kernel_size, stride, expand_ratio, image_size, se_ratio=0.25, bn_mom=0.01, bn_eps=1e-3):
        super().__init__()
        hidden = inp * expand_ratio
        self.stride = stride
        self.use_skip = stride == 1 and inp == oup
        self.drop_connect_rate = 0.0
        if expand_ratio != 1:
            self._expand_conv = Conv2dStaticSamePadding(inp, hidden, 1, image_size=image_size, bias=False)
            self._bn0 = BatchNorm2d(hidden, momentum=bn_mom, eps=bn_eps)
        self._depthwise_conv = Conv2dStaticSamePadding(hidden, hidden, kernel_size, stride, image_size=image_size, groups=hidden, bias=False)
        self._bn1 = BatchNorm2d(hidden, momentum=bn_mom, eps=bn_eps)
        squeezed = max(1, int(inp * se_ratio))
        self._se_reduce = Conv2dStaticSamePadding(hidden, squeezed, 1, image_size=(1, 1))
        self._se_expand = Conv2dStaticSamePadding(squeezed, hidden, 1, image_size=(1, 1))
        self._project_conv = Conv2dStaticSamePadding(hidden, oup, 1, image_size=-(-image_size // stride), bias=False)
        self._bn2 = BatchNorm2d(oup, momentum=bn_mom, eps=bn_eps)
        self._swish = Swish()

    def forward(self, x):
        inputs = x
        if hasattr(self, "_expand_conv"):
            x = self._swish(self._bn0(self._expand_conv(x)))
        x = self._swish(self._bn1(self._depthwise_conv(x)))
        g = self._se_expand(self._swish(self._se_reduce(F.adaptive_avg_pool2d(x, 1))))
        x = self._bn2(self._project_conv(torch.sigmoid(g) * x))
        if self.use_skip:
            p = self.drop_connect_rate
            if self.training and p:
                keep = torch.floor(1 - p + torch.rand([x.shape[0], 1, 1, 1], dtype=x.dtype, device=x.device))
                x = x / (1 - p) * keep
            x = x + inputs
        return x


class EfficientNetEncoder(nn.Module):
    """smp's EfficientNetEncoder: efficientnet_pytorch's EfficientNet without _fc, returning 6 feature levels: the input, the stem
    and the outputs of the blocks in front of smp's stage indices.  `_conv_head` and the top-level `_bn1` stay in the module and in
    the state_dict, as in smp, and forward does not run them.  One row of VARIANTS per encoder: the declared image size, the block
    arguments (repeat, kernel, stride, expand ratio, input, output — only a group's first block has the stride and the input width),
    smp's stage indices and the head width.  Only B0 is here: its declared 224 stays even down to 14, so every stride-2 site pads
    (0, 1) for k = 3 and (1, 2) for k = 5; B1 and up declare sizes that reach odd extents and need their own pads per site in the
    native kernels."""
    VARIANTS = {"efficientnet-b0": dict(
        image_size=224, stem=32, head=1280, stages=(3, 5, 9, 16), out_channels=(32, 24, 40, 112, 320),
        blocks=((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112),
                (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)))}

    def __init__(self, name="efficientnet-b0", in_channels=3, depth=5):
        super().__init__()
        if name not in self.VARIANTS:
            raise KeyError(f"encoder {name!r} not available (have {_available()})")
        v = self.VARIANTS[name]
        self.name = name
        self._depth = depth
        self._stage_idxs = v["stages"]
        self.out_channels = (in_channels,) + v["out_channels"]
        self.drop_connect_rate = 0.2
        size = v["image_size"]
        self._conv_stem = Conv2dStaticSamePadding(in_channels, v["stem"], 3, 2, image_size=size, bias=False)
        self._bn0 = BatchNorm2d(v["stem"], momentum=0.01, eps=1e-3)
        size = -(-size // 2)
        blocks = []
        for repeat, k, stride, expand, inp, oup in v["blocks"]:
            for i in range(repeat):
                blocks.append(MBConvBlock(inp if i == 0 else oup, oup, k, stride if i == 0 else 1, expand, size))
                if i == 0:
                    size = -(-size // stride)
        self._blocks = nn.ModuleList(blocks)
        self._conv_head = Conv2dStaticSamePadding(v["blocks"][-1][5], v["head"], 1, image_size=size, bias=False)
        self._bn1 = BatchNorm2d(v["head"], momentum=0.01, eps=1e-3)
        self._swish = Swish()
        # (efficientnet_pytorch leaves torch's default initialisation; a checkpoint or a weights file overwrites it)

    def forward(self, x):
        feats = [x]
        x = self._swish(self._bn0(self._conv_stem(x)))
        feats.append(x)
        for i, block in enumerate(self._blocks):
            block.drop_connect_rate = self.drop_connect_rate * i / len(self._blocks)
            x = block(x)
            if i + 1 in self._stage_idxs:
                feats.append(x)
        return feats


class DenseLayer(nn.Module):
    """torchvision.models.densenet._DenseLayer: conv2(relu2(norm2(conv1(relu1(norm1(x)))))) of the concatenated input, conv1 a 1x1
    to bn_size * growth channels, conv2 a 3x3 / pad 1 to `growth`; no dropout (drop_rate 0).  Both ReLUs are named children: a test
    may swap them."""

    def __init__(self, inp, growth, bn_size):
        super().__init__()
        self.norm1 = BatchNorm2d(inp)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = Conv2d(inp, bn_size * growth, 1, bias=False)
        self.norm2 = BatchNorm2d(bn_size * growth)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = Conv2d(bn_size * growth, growth, 3, 1, 1, bias=False)

    def forward(self, x):
        y = self.conv1(_bn_act(x, self.norm1, self.relu1))
        return self.conv2(_bn_act(y, self.norm2, self.relu2))


class DenseBlock(nn.ModuleDict):
    """torchvision's _DenseBlock: children denselayer1 .. N; every layer's output is concatenated behind its input."""

    def __init__(self, layers, inp, growth, bn_size):
        super().__init__()
        for j in range(layers):
            self["denselayer%d" % (j + 1)] = DenseLayer(inp + j * growth, growth, bn_size)

    def forward(self, x):
        for layer in self.values():
            x = torch.cat([x, layer(x)], 1)
        return x


class Transition(nn.Sequential):
    """torchvision's _Transition (norm, relu, conv 1x1 to half the channels, AvgPool2d(2, 2)) as smp's TransitionWithSkip walks it:
    returns the pooled tensor and the tensor behind the ReLU, which is the stage's feature level."""

    def __init__(self, inp, oup):
        super().__init__()
        self.norm = BatchNorm2d(inp)
        self.relu = nn.ReLU(inplace=True)
        self.conv = Conv2d(inp, oup, 1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)

    def forward(self, x):
        skip = _bn_act(x, self.norm, self.relu)
        return self.pool(self.conv(skip)), skip


class DenseNetEncoder(nn.Module):
    """smp's DenseNetEncoder: torchvision's DenseNet.features without the classifier, restated the same way as the other encoders
    (neither package is here: parity unpinned), returning 6 feature levels: the input, relu0's output, the tensor behind the ReLU
    of transitions 1 .. 3 (in front of their conv) and norm5's output WITHOUT a ReLU.  state_dict names and order are torchvision's
    (features.conv0.weight, features.denseblock1.denselayer1.norm1.weight, features.transition1.conv.weight, features.norm5.bias).
    VARIANTS: the dense layers per block; all three have a 64-channel stem, growth 32 and bn_size 4.  densenet161 (stem 96, growth
    48) is NOT built: the native 7x7 stem and the native 3x3 are made for 64 and 32 channels; it raises KeyError like any unknown
    name.  In the training step the convolutions and BatchNorms reach the native front ends through Conv2d / BatchNorm2d / _bn_act
    above where those accept the shape; the concatenation and the average pool are torch's."""
    VARIANTS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}
    STEM, GROWTH, BN_SIZE = 64, 32, 4

    def __init__(self, name="densenet121", in_channels=3, depth=5):
        super().__init__()
        if name not in self.VARIANTS:
            raise KeyError(f"encoder {name!r} not available (have {_available()})")
        from collections import OrderedDict
        self.name = name
        self._depth = depth
        f = OrderedDict([("conv0", Conv2d(in_channels, self.STEM, 7, 2, 3, bias=False)), ("norm0", BatchNorm2d(self.STEM)),
                         ("relu0", nn.ReLU(inplace=True)), ("pool0", MaxPool2d(3, 2, 1))])
        c, skips = self.STEM, []
        for i, layers in enumerate(self.VARIANTS[name]):
            f["denseblock%d" % (i + 1)] = DenseBlock(layers, c, self.GROWTH, self.BN_SIZE)
            c += layers * self.GROWTH
            if i < 3:
                skips.append(c)
                f["transition%d" % (i + 1)] = Transition(c, c // 2)
                c //= 2
        f["norm5"] = BatchNorm2d(c)
        self.features = nn.Sequential(f)
        self.out_channels = (in_channels, self.STEM, *skips, c)
        # torchvision's initialisation (a checkpoint or a weights file overwrites it)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        f = self.features
        feats = [x]
        x = _bn_act(f.conv0(x), f.norm0, f.relu0)
        feats.append(x)
        x = f.pool0(x)
        for i in (1, 2, 3):
            x, skip = getattr(f, "transition%d" % i)(getattr(f, "denseblock%d" % i)(x))
            feats.append(skip)
        feats.append(f.norm5(f.denseblock4(x)))
        return feats

    @staticmethod
    def remap_legacy_keys(sd):
        """torchvision's released DenseNet checkpoints name a dense layer's children norm.1 / relu.1 / conv.1 / norm.2 ...; smp's
        DenseNetEncoder.load_state_dict rewrites them to norm1 / conv1 ... before loading.  The same rewrite."""
        import re
        pat = re.compile(r"^(.*denselayer\d+\.(?:norm|relu|conv))\.((?:[12])\.(?:weight|bias|running_mean|running_var|num_batches_tracked))$")
        out = type(sd)()
        for k, v in sd.items():
            m = pat.match(k)
            out[m.group(1) + m.group(2) if m else k] = v
        return out


class VGGEncoder(nn.Module):
    """smp's VGGEncoder: torchvision's vgg.make_layers(cfg, batch_norm) without avgpool and classifier, restated the same way as the
    other encoders (neither package is here: parity unpinned).  `features` is ONE nn.Sequential indexed exactly as torchvision's: per
    convolution Conv2d(3x3, pad 1, bias=True), [BatchNorm2d,] ReLU(inplace), and MaxPool2d(2, 2) behind each of the five blocks of
    64 / 128 / 256 / 512 / 512 channels; state_dict names are features.N.weight / .bias (and the BatchNorm's five).  smp splits the
    Sequential at every max-pool, the pool OPENING the next stage, and returns one tensor per stage: six feature levels, the five
    blocks' outputs in front of their pools (scales 1/1 .. 1/16; the first is NOT the input image) and the last pool's output alone
    (1/32).  The FPN reads the last four.  VARIANTS: (convolutions per block, BatchNorm) of configurations A / B / D / E.  In the
    training step the convolutions and BatchNorms reach the native front ends through Conv2d / BatchNorm2d / _bn_act above where
    those accept the shape; features.0 (3 -> 64 channels) and the 2x2 pools are torch's unless FPC_TRAIN_NATIVE_VGG=1 — then
    lib/train_conv's _VggConv0Fn (through Conv2d) and maxpool2x2 (asked here for a pool that is exactly MaxPool2d(2, 2)), on
    csrc/vgg.hip and csrc/vgg_train.hip —; whatever the front ends refuse is torch's."""
    CHANNELS = (64, 128, 256, 512, 512)
    CONFIGS = {"vgg11": (1, 1, 2, 2, 2), "vgg13": (2, 2, 2, 2, 2), "vgg16": (2, 2, 3, 3, 3), "vgg19": (2, 2, 4, 4, 4)}
    VARIANTS = {n + s: (c, bool(s)) for n, c in CONFIGS.items() for s in ("", "_bn")}

    def __init__(self, name="vgg16", in_channels=3, depth=5):
        super().__init__()
        if name not in self.VARIANTS:
            raise KeyError(f"encoder {name!r} not available (have {_available()})")
        self.name = name
        self._depth = depth
        convs, self.batch_norm = self.VARIANTS[name]
        self.out_channels = self.CHANNELS + (512,)
        layers, c = [], in_channels
        for n, v in zip(convs, self.CHANNELS):
            for _ in range(n):
                layers.append(Conv2d(c, v, 3, padding=1))
                if self.batch_norm:
                    layers.append(BatchNorm2d(v))
                layers.append(nn.ReLU(inplace=True))
                c = v
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        self.features = nn.Sequential(*layers)
        # torchvision's initialisation (a checkpoint or a weights file overwrites it)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        feats, mods, i = [], list(self.features), 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.MaxPool2d):      # a pool closes a stage and opens the next
                feats.append(x)
                # exactly MaxPool2d(2, 2) in the training step: one native op each way (FPC_TRAIN_NATIVE_VGG=1); refused: the module
                ok = x.is_cuda and torch.is_grad_enabled() and x.requires_grad and not m.return_indices and not m.ceil_mode \
                    and m.kernel_size in (2, (2, 2)) and m.stride in (2, (2, 2)) and m.padding in (0, (0, 0)) and m.dilation in (1, (1, 1))
                y = _train_native(ok, "maxpool2x2", x)
                x = m(x) if y is None else y
            elif isinstance(m, nn.BatchNorm2d):  # (BatchNorm + ReLU: one native op in the training step)
                x = _bn_act(x, m, mods[i + 1])
                i += 1
            else:
                x = m(x)
            i += 1
        feats.append(x)
        return feats


_WARNED_WEIGHTS = set()


def get_encoder(name, in_channels=3, depth=5, weights=None):
    """smp.encoders.get_encoder stand-in (call site F/lib/pose_regressor.py:608-613).

    smp downloads the torchvision ImageNet checkpoint for weights='imagenet' (every HPARAM preset asks for it,
    F/config.py).  There is no network here, so pretrained weights come from a local file:
    `FPC_ENCODER_WEIGHTS_DIR/<name>.pth` (or `FPC_ENCODER_WEIGHTS=<file>`) holding the torchvision ResNet state
    dict (keys conv1.weight, bn1.*, layer1.0.conv1.weight, ...; fc.* is dropped, as smp does) or, for an SE-ResNet, the
    pretrainedmodels one (layer0.conv1.weight, ..., layerN.i.se_module.fc1.bias; last_linear.* is dropped) or, for mobilenet_v2,
    torchvision's (features.0.0.weight, ..., features.18.1.running_var; classifier.* is dropped) or, for efficientnet-b0,
    efficientnet_pytorch's (_conv_stem.weight, ..., _conv_head.weight, _bn1.*; _fc.* is dropped) or, for densenet121 / 169 / 201,
    torchvision's (features.conv0.weight, ..., features.norm5.running_var, with the released files' legacy norm.1 / conv.2 keys
    rewritten; classifier.* is dropped) or, for a VGG, torchvision's (features.0.weight, features.0.bias, ...; classifier.* is
    dropped).  When `weights` is
    requested and no file is configured the encoder stays randomly initialised and a warning says so once per
    encoder — a checkpoint loaded afterwards (load_from_ckpt) overwrites the encoder anyway."""
    import logging
    import os
    cls = MobileNetV2Encoder if name == MobileNetV2Encoder.NAME else EfficientNetEncoder if name in EfficientNetEncoder.VARIANTS \
        else DenseNetEncoder if name in DenseNetEncoder.VARIANTS else VGGEncoder if name in VGGEncoder.VARIANTS else SENetEncoder if name in _ENCODERS and _ENCODERS[name][4] else ResNetEncoder
    enc = cls(name, in_channels=in_channels, depth=depth)
    enc.requested_weights = weights
    enc.loaded_weights = None
    if weights is not None:
        path = os.environ.get("FPC_ENCODER_WEIGHTS")
        if not path and os.environ.get("FPC_ENCODER_WEIGHTS_DIR"):
            path = os.path.join(os.environ["FPC_ENCODER_WEIGHTS_DIR"], f"{name}.pth")
        if path:
            import torch
            sd = torch.load(path, map_location="cpu")
            sd = {k: v for k, v in sd.items() if not k.startswith(("fc.", "last_linear.", "classifier.", "_fc."))}
            if cls is DenseNetEncoder:
                sd = DenseNetEncoder.remap_legacy_keys(sd)      # (norm.1 -> norm1 ...: as smp's load_state_dict)
            enc.load_state_dict(sd)                  # strict: a wrong file fails loudly
            enc.loaded_weights = path
        elif (name, weights) not in _WARNED_WEIGHTS:
            _WARNED_WEIGHTS.add((name, weights))
            logging.getLogger('fastposecnn').warning(
                "encoder %s: ENCODER_WEIGHTS=%r requested but no local file is configured "
                "(FPC_ENCODER_WEIGHTS / FPC_ENCODER_WEIGHTS_DIR): the encoder is RANDOMLY initialised, unlike "
                "smp.get_encoder, until a checkpoint is loaded", name, weights)
    return enc


class Conv3x3GNReLU(nn.Module):
    def __init__(self, in_channels, out_channels, upsample=False):
        super().__init__()
        self.upsample = upsample
        self.block = nn.Sequential(
            Conv2d(in_channels, out_channels, (3, 3), stride=1, padding=1, bias=False),
            nn.GroupNorm(32, out_channels),
            nn.ReLU(inplace=True),
        )

    def forward(self, x):
        if self.training and x.is_cuda and torch.is_grad_enabled() and isinstance(self.block[2], nn.ReLU):
            # the training step: GroupNorm + ReLU as one native channel-last op behind the native convolution
            x = _train_native(True, "groupnorm_relu", self.block[0](x), self.block[1])
        else:
            x = self.block(x)
        if self.upsample:
            x = _upsample_bilinear(x, 2)
        return x


class FPNBlock(nn.Module):
    def __init__(self, pyramid_channels, skip_channels):
        super().__init__()
        self.skip_conv = Conv2d(skip_channels, pyramid_channels, kernel_size=1)

    def forward(self, x, skip=None):
        c = self.skip_conv
        # the training step: lateral convolution + merge in one launch
        y = _train_native(c.training and x.is_cuda and torch.is_grad_enabled(), "conv2d_up_add", skip, c.weight, c.bias, x, c.padding[0])
        if y is not None:
            return y
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        skip = self.skip_conv(skip)
        return x + skip


class SegmentationBlock(nn.Module):
    def __init__(self, in_channels, out_channels, n_upsamples=0):
        super().__init__()
        blocks = [Conv3x3GNReLU(in_channels, out_channels, upsample=bool(n_upsamples))]
        if n_upsamples > 1:
            for _ in range(1, n_upsamples):
                blocks.append(Conv3x3GNReLU(out_channels, out_channels, upsample=True))
        self.block = nn.Sequential(*blocks)

    def forward(self, x):
        return self.block(x)


class MergeBlock(nn.Module):
    def __init__(self, policy):
        super().__init__()
        if policy not in ("add", "cat"):
            raise ValueError(f"`merge_policy` must be one of: ['add', 'cat'], got {policy}")
        self.policy = policy

    def forward(self, x):
        if self.policy == "add":
            return sum(x)
        return torch.cat(x, dim=1)


class FPNDecoder(nn.Module):
    def __init__(self, encoder_channels, encoder_depth=5, pyramid_channels=256, segmentation_channels=128,
                 dropout=0.2, merge_policy="add"):
        super().__init__()
        self.out_channels = segmentation_channels if merge_policy == "add" else segmentation_channels * 4
        if encoder_depth < 3:
            raise ValueError(f"Encoder depth for FPN decoder cannot be less than 3, got {encoder_depth}.")
        encoder_channels = encoder_channels[::-1]
        encoder_channels = encoder_channels[:encoder_depth + 1]
        self.p5 = Conv2d(encoder_channels[0], pyramid_channels, kernel_size=1)
        self.p4 = FPNBlock(pyramid_channels, encoder_channels[1])
        self.p3 = FPNBlock(pyramid_channels, encoder_channels[2])
        self.p2 = FPNBlock(pyramid_channels, encoder_channels[3])
        self.seg_blocks = nn.ModuleList([
            SegmentationBlock(pyramid_channels, segmentation_channels, n_upsamples=n) for n in [3, 2, 1, 0]
        ])
        self.merge = MergeBlock(merge_policy)
        self.dropout = nn.Dropout2d(p=dropout, inplace=True)

    def forward(self, *features):
        c2, c3, c4, c5 = features[-4:]
        p5 = self.p5(c5)
        p4 = self.p4(p5, c4)
        p3 = self.p3(p4, c3)
        p2 = self.p2(p3, c2)
        feature_pyramid = [seg_block(p) for seg_block, p in zip(self.seg_blocks, [p5, p4, p3, p2])]
        x = self.merge(feature_pyramid)
        x = self.dropout(x)
        return x


class SegmentationHead(nn.Sequential):
    def __init__(self, in_channels, out_channels, kernel_size=3, activation=None, upsampling=1):
        conv2d = Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=kernel_size // 2)
        up = UpsamplingBilinear2d(scale_factor=upsampling) if upsampling > 1 else nn.Identity()
        if activation is not None:
            raise ValueError("only activation=None is used by FastPoseCNN (pose_regressor.py:596)")
        super().__init__(conv2d, up, nn.Identity())
