"""MobileNetV3-Large feature tower of the reference (models/mobilenetv3.py), MI355X-native.

Same module tree, state_dict keys, parameter order and initialisation as the reference (`features.N.conv.M`,
`conv`, `classifier`), every forward on the HIP kernels:

  * a pointwise convolution + BatchNorm + activation is one conv_bn_act node (1x1 MFMA convolution, statistics in its
    epilogue, finalize + normalise + activate in one pass; the pw-linear one adds the identity skip in that pass);
  * a depthwise convolution + BatchNorm (+ activation) is one node of its own kernels (csrc/mobilenet.hip) whose
    epilogue also pools per image for the SELayer behind it; the SELayer then costs one launch for its MLP and one
    elementwise pass that multiplies and activates (conv -> BN -> SE -> act, models/mobilenetv3.py:108-112);
  * both towers run as one batch of two statistics groups, as the DenseNet tower does.

The reference's tail (`conv` 1x1 160 -> 960 + BN + h_swish, avgpool, classifier) is computed and discarded upstream: its
parameters never receive a gradient, but in train mode it moves the running statistics of `conv.1` — the native tower
runs that 1x1 convolution with statistics (no backward) and nothing else of the tail.
"""
import math

import torch
import torch.nn as nn

from . import ops


def _make_divisible(v, divisor, min_value=None):
    """models/mobilenetv3.py:20-38."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class h_sigmoid(nn.Module):
    """models/mobilenetv3.py:41-47."""

    def __init__(self, inplace=True):
        super().__init__()
        self.relu = nn.ReLU6(inplace=inplace)

    def forward(self, x):
        return ops.affine_act(x, act=ops.ACT_HSIGMOID)


class h_swish(nn.Module):
    """models/mobilenetv3.py:50-56."""

    def __init__(self, inplace=True):
        super().__init__()
        self.sigmoid = h_sigmoid(inplace=inplace)

    def forward(self, x):
        return ops.affine_act(x, act=ops.ACT_HSWISH)


class SELayer(nn.Module):
    """models/mobilenetv3.py:59-77.  Stand-alone forward: the pool comes from the depthwise node in front
    (InvertedResidual passes it on); see ops.se_scale_act."""

    def __init__(self, channel, reduction=4):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        hidden = _make_divisible(channel // reduction, 8)
        self.fc = nn.Sequential(nn.Linear(channel, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, channel), h_sigmoid())

    def forward(self, x, side, act=0):
        return ops.se_scale_act(x, self.fc[0], self.fc[2], side, act)


def conv_3x3_bn(inp, oup, stride):
    return nn.Sequential(nn.Conv2d(inp, oup, 3, stride, 1, bias=False), nn.BatchNorm2d(oup), h_swish())


def conv_1x1_bn(inp, oup):
    return nn.Sequential(nn.Conv2d(inp, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup), h_swish())


def _act_code(mod):
    return ops.ACT_HSWISH if isinstance(mod, h_swish) else 1


class InvertedResidual(nn.Module):
    """models/mobilenetv3.py:80-124."""

    def __init__(self, inp, hidden_dim, oup, kernel_size, stride, use_se, use_hs):
        super().__init__()
        assert stride in [1, 2]
        self.identity = stride == 1 and inp == oup
        self.stride, self.use_se = stride, bool(use_se)
        self.expand = inp != hidden_dim
        act = lambda: h_swish() if use_hs else nn.ReLU(inplace=True)
        dw = nn.Conv2d(hidden_dim, hidden_dim, kernel_size, stride, (kernel_size - 1) // 2, groups=hidden_dim, bias=False)
        se = lambda: SELayer(hidden_dim) if use_se else nn.Identity()
        if not self.expand:
            self.conv = nn.Sequential(dw, nn.BatchNorm2d(hidden_dim), act(), se(),
                                      nn.Conv2d(hidden_dim, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup))
        else:
            self.conv = nn.Sequential(nn.Conv2d(inp, hidden_dim, 1, 1, 0, bias=False), nn.BatchNorm2d(hidden_dim), act(),
                                      dw, nn.BatchNorm2d(hidden_dim), se(), act(),
                                      nn.Conv2d(hidden_dim, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup))

    def forward(self, x, groups=1):
        c = self.conv
        res = x if self.identity else None
        if not self.expand:
            # dw -> BN -> act -> pw -> BN.  An SELayer here would pool the ACTIVATED map (models/mobilenetv3.py:97-104):
            # only MobileNetV3-Small has one, and it is not on the native path
            if self.use_se:
                raise NotImplementedError("InvertedResidual without expansion and with an SELayer (MobileNetV3-Small)")
            h = ops.dw_conv_bn_act(x, c[0].weight, c[1], self.stride, _act_code(c[2]), groups)
            return ops.conv_bn_act(h, c[4].weight, c[5], act=0, residual=res, groups=groups)
        h = ops.conv_bn_act(x, c[0].weight, c[1], act=_act_code(c[2]), groups=groups)
        if self.use_se:
            side = ops.SESide()
            h = ops.dw_conv_bn_act(h, c[3].weight, c[4], self.stride, 0, groups, side)
            h = c[5](h, side, _act_code(c[6]))
        else:
            h = ops.dw_conv_bn_act(h, c[3].weight, c[4], self.stride, _act_code(c[6]), groups)
        return ops.conv_bn_act(h, c[7].weight, c[8], act=0, residual=res, groups=groups)


TAPS = (1, 3, 6, 12, 15)


class MobileNetV3(nn.Module):
    """models/mobilenetv3.py:127-194: returns the outputs of blocks 1, 3, 6, 12 and 15."""

    def __init__(self, cfgs, mode, num_classes=1000, width_mult=1.):
        super().__init__()
        self.cfgs = cfgs
        assert mode in ['large', 'small']
        input_channel = _make_divisible(16 * width_mult, 8)
        layers = [conv_3x3_bn(3, input_channel, 2)]
        for k, t, c, use_se, use_hs, s in self.cfgs:
            output_channel = _make_divisible(c * width_mult, 8)
            exp_size = _make_divisible(input_channel * t, 8)
            layers.append(InvertedResidual(input_channel, exp_size, output_channel, k, s, use_se, use_hs))
            input_channel = output_channel
        self.features = nn.ModuleList(layers)
        self.conv = conv_1x1_bn(input_channel, exp_size)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        output_channel = {'large': 1280, 'small': 1024}
        output_channel = _make_divisible(output_channel[mode] * width_mult, 8) if width_mult > 1.0 else output_channel[mode]
        self.classifier = nn.Sequential(nn.Linear(exp_size, output_channel), h_swish(), nn.Dropout(0.2),
                                        nn.Linear(output_channel, num_classes))
        self._initialize_weights()

    def forward(self, x, groups=1):
        stem = self.features[0]
        # the image may arrive zero-padded to 8 channels (nn._stereo_buffer): the stem reads the weight's channels only
        f = ops.conv_bn_act(x[:, :stem[0].weight.shape[1]], stem[0].weight, stem[1], stride=2, padding=1, act=ops.ACT_HSWISH,
                            groups=groups)
        taps = []
        for i in range(1, len(self.features)):
            f = self.features[i](f, groups)
            if i in TAPS:
                taps.append(f)
        if self.training:
            # the reference's tail: its output is discarded, but the train-mode BatchNorm of conv.1 updates its running
            # statistics (left tower, then right: one statistics group each)
            with torch.no_grad():
                ops.conv_bn_act(f.detach(), self.conv[0].weight, self.conv[1], act=ops.ACT_HSWISH, groups=groups)
        return taps

    def _initialize_weights(self):
        """models/mobilenetv3.py:196-210 (same module order, hence the same draws for a seeded generator)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.weight.data.normal_(0, 0.01)
                m.bias.data.zero_()


LARGE_CFGS = [
    # k, t, c, SE, HS, s  (models/mobilenetv3.py:217-233)
    [3, 1, 16, 0, 0, 1],
    [3, 4, 24, 0, 0, 2],
    [3, 3, 24, 0, 0, 1],
    [5, 3, 40, 1, 0, 2],
    [5, 3, 40, 1, 0, 1],
    [5, 3, 40, 1, 0, 1],
    [3, 6, 80, 0, 1, 2],
    [3, 2.5, 80, 0, 1, 1],
    [3, 2.3, 80, 0, 1, 1],
    [3, 2.3, 80, 0, 1, 1],
    [3, 6, 112, 1, 1, 1],
    [3, 6, 112, 1, 1, 1],
    [5, 6, 160, 1, 1, 2],
    [5, 6, 160, 1, 1, 1],
    [5, 6, 160, 1, 1, 1],
]


def mobilenetv3_large(**kwargs):
    """models/mobilenetv3.py:213-245.  Upstream also torch.load()s 'weights/mobilenetv3-large-1cd25616.pth' and then
    only rebinds entries of a state_dict copy it never loads: the constructed model keeps its random initialisation.
    The native constructor neither needs nor reads that file."""
    return MobileNetV3(LARGE_CFGS, mode='large', **kwargs)
