"""DeepLabV3+ on Xception-65 in its stereo form (`-net deeplab_mod`, models_deeplab_mod/{net,encoder,xception,spp,common}.py),
MI355X-native: same module tree, state_dict keys and parameter order as the reference, every forward on the HIP kernels.

  * SeparableConv2d is two autograd nodes: depthwise 3x3 (stride, dilation) + bn_depth (+ relu1) on the dilated depthwise
    kernels of csrc/mobilenet.hip — relu_first is applied in that kernel's load, so the un-rectified input stays available
    to the 'sum' skip — and pointwise + bn_point (+ relu2, + the skip of XceptionBlock) as one conv_bn_act node;
  * both images go through the encoder as one batch of two statistics groups (left | right), as the other towers here do:
    the batch statistics are per image side and the running statistics move once per side, as two calls upstream do;
  * the 1-D correlation (patch (1, 17)) is the project's own kernel.

`SPPNet(..., harness=True)` (keyword-only, not in the reference) adds the steps the reference's training harness wraps
around the network (torch_implementation.py:123-131,163-166): left <- left*2 - 1 (the right image is NOT rescaled
upstream, and is not here), one zero row and column appended bottom / right of both images, every output resized
bilinear align_corners=True to (h+1, w+1) and cropped to h x w, returned as (seg1, disp1, seg2, disp1) — the tuple
TrainStep's loss, metrics, optimisers and checkpoints take.  The module tree and keys do not change.

Only what `-net deeplab_mod` builds by default is implemented: enc_type 'xception65', dec_type 'aspp'.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops
from .aspp import _layer_ids      # one counter for the dropout stream ids of every ASPP head in the process
from .nn import SpatialCorrelationSampler


class SeparableConv2d(nn.Module):
    """models_deeplab_mod/common.py:24-50."""

    def __init__(self, inplanes, planes, kernel_size=3, stride=1, dilation=1, relu_first=True):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError("SeparableConv2d: kernel_size 3 only (the depthwise kernels are 3x3)")
        depthwise = nn.Conv2d(inplanes, inplanes, kernel_size, stride=stride, padding=dilation, dilation=dilation, groups=inplanes,
                              bias=False)
        bn_depth = nn.BatchNorm2d(inplanes)
        pointwise = nn.Conv2d(inplanes, planes, 1, bias=False)
        bn_point = nn.BatchNorm2d(planes)
        self.relu_first = relu_first
        if relu_first:
            self.block = nn.Sequential(OrderedDict([('relu', nn.ReLU()), ('depthwise', depthwise), ('bn_depth', bn_depth),
                                                    ('pointwise', pointwise), ('bn_point', bn_point)]))
        else:
            self.block = nn.Sequential(OrderedDict([('depthwise', depthwise), ('bn_depth', bn_depth), ('relu1', nn.ReLU()),
                                                    ('pointwise', pointwise), ('bn_point', bn_point), ('relu2', nn.ReLU())]))

    def forward(self, x, residual=None, groups=1):
        b = self.block
        act = 0 if self.relu_first else 1
        h = ops.dw_dil_conv_bn_act(x, b.depthwise.weight, b.bn_depth, b.depthwise.stride[0], b.depthwise.dilation[0],
                                   in_relu=self.relu_first, act=act, groups=groups)
        return ops.conv_bn_act(h, b.pointwise.weight, b.bn_point, act=act, residual=residual, groups=groups)


class XceptionBlock(nn.Module):
    """models_deeplab_mod/xception.py:7-49."""

    def __init__(self, channel_list, stride=1, dilation=1, skip_connection_type='conv', relu_first=True, low_feat=False):
        super().__init__()
        assert len(channel_list) == 4
        if skip_connection_type not in ('conv', 'sum', 'none'):
            raise ValueError('Unsupported skip connection type.')
        self.skip_connection_type = skip_connection_type
        self.relu_first = relu_first
        self.low_feat = low_feat
        if skip_connection_type == 'conv':
            self.conv = nn.Conv2d(channel_list[0], channel_list[-1], 1, stride=stride, bias=False)
            self.bn = nn.BatchNorm2d(channel_list[-1])
        self.sep_conv1 = SeparableConv2d(channel_list[0], channel_list[1], dilation=dilation, relu_first=relu_first)
        self.sep_conv2 = SeparableConv2d(channel_list[1], channel_list[2], dilation=dilation, relu_first=relu_first)
        self.sep_conv3 = SeparableConv2d(channel_list[2], channel_list[3], dilation=dilation, relu_first=relu_first, stride=stride)

    def forward(self, inputs, groups=1):
        sc1 = self.sep_conv1(inputs, groups=groups)
        sc2 = self.sep_conv2(sc1, groups=groups)
        if self.skip_connection_type == 'conv':
            skip = ops.conv_bn_act(inputs, self.conv.weight, self.bn, stride=self.conv.stride[0], act=0, groups=groups)
        elif self.skip_connection_type == 'sum':
            skip = inputs
        else:
            skip = None
        outputs = self.sep_conv3(sc2, residual=skip, groups=groups)     # the skip is added in bn_point's pass
        return (outputs, sc2) if self.low_feat else outputs


class Xception65(nn.Module):
    """models_deeplab_mod/xception.py:52-136: returns (x, block2's sc2, block8's sc2, block14's sc2)."""

    def __init__(self, output_stride=8):
        super().__init__()
        if output_stride == 16:
            entry_block3_stride, middle_block_dilation, exit_block_dilations = 2, 1, (1, 2)
        elif output_stride == 8:
            entry_block3_stride, middle_block_dilation, exit_block_dilations = 1, 2, (2, 4)
        else:
            raise NotImplementedError
        self.conv1 = nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv2d(32, 64, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        self.block1 = XceptionBlock([64, 128, 128, 128], stride=2)
        self.block2 = XceptionBlock([128, 256, 256, 256], stride=2, low_feat=True)
        self.block3 = XceptionBlock([256, 728, 728, 728], stride=entry_block3_stride)
        for i in range(4, 20):      # middle flow: 16 units
            setattr(self, "block%d" % i, XceptionBlock([728, 728, 728, 728], dilation=middle_block_dilation,
                                                       skip_connection_type='sum', low_feat=i in (8, 14)))
        self.block20 = XceptionBlock([728, 728, 1024, 1024], dilation=exit_block_dilations[0])
        self.block21 = XceptionBlock([1024, 1536, 1536, 2048], dilation=exit_block_dilations[1], skip_connection_type='none',
                                     relu_first=False)

    def forward(self, x, groups=1):
        # the image may arrive zero-padded to 8 channels (one pixel = one 16-byte chunk): the stem reads the weight's channels
        x = ops.conv_bn_act(x[:, :3], self.conv1.weight, self.bn1, stride=2, padding=1, act=1, groups=groups)
        x = ops.conv_bn_act(x, self.conv2.weight, self.bn2, stride=1, padding=1, act=1, groups=groups)
        x = self.block1(x, groups)
        x, low = self.block2(x, groups)
        x = self.block3(x, groups)
        mid = {}
        for i in range(4, 20):
            x = getattr(self, "block%d" % i)(x, groups)
            if i in (8, 14):
                x, mid[i] = x
        x = self.block20(x, groups)
        x = self.block21(x, groups)
        return x, low, mid[8], mid[14]


def _conv_bn_relu(cin, cout, gap=False):
    mods = [('gap', nn.AdaptiveAvgPool2d((1, 1)))] if gap else []
    return nn.Sequential(OrderedDict(mods + [('conv', nn.Conv2d(cin, cout, 1, bias=False)), ('bn', nn.BatchNorm2d(cout)),
                                             ('relu', nn.ReLU(inplace=True))]))


class ASPP(nn.Module):
    """models_deeplab_mod/spp.py:35-100 (small_net = False)."""

    def __init__(self, in_channels=2048, out_channels=256, output_stride=8):
        super().__init__()
        self.small_net = False
        if output_stride == 16:
            dilations = [6, 12, 18]
        elif output_stride == 8:
            dilations = [12, 24, 36]
        else:
            raise NotImplementedError
        self.aspp0 = _conv_bn_relu(in_channels, out_channels)
        self.aspp1 = SeparableConv2d(in_channels, out_channels, dilation=dilations[0], relu_first=False)
        self.aspp2 = SeparableConv2d(in_channels, out_channels, dilation=dilations[1], relu_first=False)
        self.aspp3 = SeparableConv2d(in_channels, out_channels, dilation=dilations[2], relu_first=False)
        self.image_pooling = _conv_bn_relu(in_channels, out_channels, gap=True)
        self.conv = nn.Conv2d(out_channels * 5, out_channels, 1, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout2d(p=0.1)
        self._drop_id = _layer_ids[0]
        _layer_ids[0] += 1

    def forward(self, x):
        ip = self.image_pooling
        pool = ops.conv_bn_act(ops.global_avg_pool(x), ip.conv.weight, ip.bn, act=1)
        pool = ops.interpolate(pool, size=x.shape[2:], mode='bilinear', align_corners=True)
        x0 = ops.conv_bn_act(x, self.aspp0.conv.weight, self.aspp0.bn, act=1)
        y = ops.concat([pool, x0, self.aspp1(x), self.aspp2(x), self.aspp3(x)])
        y = ops.conv_bn_act(y, self.conv.weight, self.bn, act=1)
        return ops.dropout_channels(y, self.dropout.p, self.training, self._drop_id)


class SPPDecoder(nn.Module):
    """models_deeplab_mod/spp.py:131-160: returns (x, middle_feat)."""

    def __init__(self, in_channels, sep_channel=256, concat_prev=False, reduced_layer_num=48):
        super().__init__()
        self.concat_prev = concat_prev
        inplane_int_feat = 0
        if self.concat_prev:
            inplane_int_feat = 64
            self.conv_int_feat = nn.Conv2d(self.concat_prev, inplane_int_feat, 1, bias=False)
        self.conv = nn.Conv2d(in_channels, reduced_layer_num, 1, bias=False)
        self.bn = nn.BatchNorm2d(reduced_layer_num)
        self.relu = nn.ReLU(inplace=True)
        self.sep1 = SeparableConv2d(sep_channel + reduced_layer_num + inplane_int_feat, 256, relu_first=False)
        self.sep2 = SeparableConv2d(256, 256, relu_first=False)

    def forward(self, x, low_level_feat, other_feat=None):
        x = ops.interpolate(x, size=low_level_feat.shape[2:], mode='bilinear', align_corners=True)
        low = ops.conv_bn_act(low_level_feat, self.conv.weight, self.bn, act=1)
        parts = [x, low]
        if self.concat_prev:
            parts.append(ops.conv2d(other_feat, self.conv_int_feat.weight))
        middle_feat = ops.concat(parts)
        return self.sep2(self.sep1(middle_feat)), middle_feat


def create_spp(dec_type, in_channels=2048, middle_channels=256, sep_channel=256, concat_prev=False, output_stride=8):
    """models_deeplab_mod/spp.py:163-175; 'aspp' only."""
    if dec_type != 'aspp':
        raise NotImplementedError("dec_type %r: only 'aspp' is built" % (dec_type,))
    return ASPP(in_channels, middle_channels, output_stride), SPPDecoder(middle_channels, sep_channel, concat_prev)


def create_encoder(enc_type, output_stride=8, pretrained=False):
    """models_deeplab_mod/encoder.py:86-98; 'xception65' only."""
    if enc_type != 'xception65':
        raise NotImplementedError("enc_type %r: only 'xception65' is built" % (enc_type,))
    return Xception65(output_stride)


class SegmentatorTTA(object):
    """models_deeplab_mod/tta.py: test-time augmentation is not built."""

    def _no_tta(self, *a, **k):
        raise NotImplementedError("test-time augmentation (SegmentatorTTA) is not built")

    hflip = vflip = trans = staticmethod(_no_tta)
    pred_resize = tta = _no_tta


def pad_bottom_right(x, scale=None, shift=None):
    """x (B, 3, h, w), optionally x*scale + shift, with one zero row and column appended (F.pad(x, [0, 1, 0, 1])), in an NHWC
    buffer zero-padded to 8 channels: one pixel = one 16-byte chunk for the stem."""
    B, C, h, w = x.shape
    buf = torch.zeros((B, h + 1, w + 1, 8), dtype=x.dtype, device=x.device)
    buf[:, :h, :w, :C] = (x if scale is None else x * scale + shift).permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)


def resize_crop(y, h, w):
    """F.interpolate(y, (h+1, w+1), bilinear, align_corners=True)[..., :h, :w] of the reference's harness."""
    return ops.interpolate(y, size=(h + 1, w + 1), mode='bilinear', align_corners=True)[..., :h, :w]


class _SPPNetBase(nn.Module, SegmentatorTTA):
    def update_bn_eps(self):
        for m in self.encoder.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eps = 1e-3

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.eval()

    def get_1x_lr_params(self):
        for p in self.encoder.parameters():
            yield p

    def get_10x_lr_params(self):
        modules = [self.spp, self.logits]
        if hasattr(self, 'decoder'):
            modules.append(self.decoder)
        for module in modules:
            for p in module.parameters():
                yield p


class SPPNet(_SPPNetBase):
    """models_deeplab_mod/net.py:82-169: forward(inputsL, inputsR) -> (x, disp_out, seg_out), all at 1/4 resolution."""

    def __init__(self, output_channels=19, enc_type='xception65', dec_type='aspp', output_stride=8, *, harness=False):
        super().__init__()
        self.output_channels = output_channels
        self.enc_type = enc_type
        self.dec_type = dec_type
        self.harness = harness
        self.encoder = create_encoder(enc_type, output_stride=output_stride, pretrained=False)
        self.conv2 = nn.Conv2d(728, 256, 1, bias=False)
        self.conv3 = nn.Conv2d(728, 256, 1, bias=False)
        self.correlation_sampler = SpatialCorrelationSampler(kernel_size=1, patch_size=(1, 8 * 2 + 1), stride=1, padding=0,
                                                             dilation_patch=1)
        self.corrConv2d = nn.Sequential(nn.Conv2d(17, 44, 1, bias=False), nn.ReLU(inplace=True))
        self.spp, self.decoder = create_spp(dec_type, output_stride=output_stride)
        _, self.decoder2 = create_spp(dec_type, sep_channel=300, concat_prev=304, output_stride=output_stride)
        _, self.decoder3 = create_spp(dec_type, sep_channel=256, concat_prev=412, output_stride=output_stride)
        self.logits = nn.Conv2d(256, output_channels, 1)
        self.logits_seg = nn.Conv2d(256, output_channels, 1)
        self.logits_disp = nn.Conv2d(256, 1, 1)

    def forward(self, inputsL, inputsR):
        B, _, h, w = inputsL.shape
        if self.harness:
            both = torch.cat([pad_bottom_right(inputsL, 2.0, -1.0), pad_bottom_right(inputsR)])
        else:
            both = torch.cat([inputsL, inputsR])
        x, low, mid2, high3 = self.encoder(both, groups=2)          # batch = [left | right]
        x = ops.split_batch(x, B)[0]
        low = ops.split_batch(low, B)[0]
        high3 = ops.split_batch(high3, B)[0]
        x = self.spp(x)
        x, int_seg = self.decoder(x, low)
        m2 = ops.conv2d(mid2, self.conv2.weight)                     # conv2 of both sides in one launch
        m2a, m2b = ops.split_batch(m2, B)
        corr = self.correlation(m2a, m2b)
        m2a = ops.concat([m2a, corr])
        high3 = ops.conv2d(high3, self.conv3.weight)
        disp_out, int_disp = self.decoder2(m2a, low, int_seg)
        seg_out, _ = self.decoder3(high3, low, int_disp)
        x = ops.conv2d(x, self.logits.weight, self.logits.bias)
        disp_out = ops.conv2d(disp_out, self.logits_disp.weight, self.logits_disp.bias)
        seg_out = ops.conv2d(seg_out, self.logits_seg.weight, self.logits_seg.bias)
        if self.harness:
            seg1, disp1, seg2 = resize_crop(x, h, w), resize_crop(disp_out, h, w), resize_crop(seg_out, h, w)
            return seg1, disp1, seg2, disp1
        return x, disp_out, seg_out

    def correlation(self, a, b):
        y = torch.squeeze(self.correlation_sampler(a, b), 1)
        return ops.conv2d(y, self.corrConv2d[0].weight, act=1)


def getNetwork(net, harness=False):
    """The two DeepLab entries of the reference's `-net` registry (util/utilLoadNetwork.py:24-25,47-50): the constructor's
    defaults, then update_bn_eps()."""
    if net == 'deeplab_mod':
        m = SPPNet(harness=harness)
    elif net == 'deeplab':
        from .deeplab import SPPNet as Mono
        m = Mono(harness=harness)
    else:
        raise NotImplementedError("getNetwork: %r is not a DeepLab entry" % (net,))
    m.update_bn_eps()
    return m
