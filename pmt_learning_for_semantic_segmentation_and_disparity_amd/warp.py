"""The warp networks of the reference (models/dsnet_t2_warp.py; `-net dsnet_warp` / `dsnet_warp_soft`,
util/utilLoadNetwork.py, output type `ThreeOutPuts`): the segmentation decoder runs on BOTH images, the right image's class
scores are warped into the left view with the predicted disparity (ops.warp_blend, models/torch_dsnet.py apply_disparity)
and blended with the left scores by a learnt gate, so the disparity head receives gradient from the segmentation loss.

The `*_disp` variants (`-net dsnet_warp_disp` / `dsnet_warp_disp_consist`, output types `ThreeOutPutsDisp` /
`ThreeOutPutsDispConsist`; _WarpDispNet below) run the tower a third time on the right image moved into the left view and
blend the two segmentation maps without a warp.

Same class names, constructor signatures, output tuples and state_dict keys as the reference.  The file's pyramid is NOT
nn.piramidNet2: it has a fourth level on the 1/16 tap and returns nine tensors (piramidNet2Warp below).
"""
import torch
import torch.nn as nn

from . import ops
from .nn import (BACKBONES, Conv2DownUp, ConvTranspose2dSame, SpatialCorrelationSampler, _c1x1, _const, _img_conv, _pool_branch,
                 _pyramid_branches, _stereo_buffer, conv2dSame, densenet121, mobilenetv3_large)


class piramidNet2Warp(nn.Module):
    """`piramidNet2` of models/dsnet_t2_warp.py:339-480: the three pyramids of nn.piramidNet2 plus `branch3_0`, `branch3_1` on
    the 1/16 tap.  Upstream runs branch3_1 and then discards its output: the third entry of the 1/16 pyramid is the
    (already upsampled) 1/8 branch `b2_1` resized bilinearly DOWN to the 1/16 size (:476).  Reproduced as is: branch3_1's
    BatchNorm moves its running statistics in train mode and its parameters never receive a gradient.
    forward -> (tap0..tap4, b0, b1, b2, b3)."""

    def __init__(self, pretrained=False, backbone='densenet'):
        super().__init__()
        if backbone not in BACKBONES:
            raise NotImplementedError("backbone %r: only %s are on the native path" % (backbone, " and ".join(BACKBONES)))
        self.backbone = backbone
        if backbone == 'mobilenet':
            self.resnet_features = mobilenetv3_large()
            cin = [16, 24, 40, 112]
        else:
            self.resnet_features = densenet121(pretrained)
            cin = [64, 128, 256, 512]
        pv = [128, 64, 32, 16, 8]
        for lvl, n in enumerate((5, 4, 3, 2)):
            for j in range(n):
                setattr(self, 'branch%d_%d' % (lvl, j), _pool_branch(pv[lvl + j], cin[lvl]))

    def _level(self, lvl, n, x, groups):
        return _pyramid_branches([getattr(self, 'branch%d_%d' % (lvl, j)) for j in range(n)], x, groups)

    def forward(self, x, groups=1):
        o = self.resnet_features(x, groups)
        b0 = ops.concat([o[0]] + self._level(0, 5, o[0], groups))
        b1 = ops.concat([o[1]] + self._level(1, 4, o[1], groups))
        l2 = self._level(2, 3, o[2], groups)
        b2 = ops.concat([o[2]] + l2)
        l3 = self._level(3, 2, o[3], groups)          # l3[1] (branch3_1) is computed and dropped, as upstream
        b3 = ops.concat([o[3], l3[0], ops.interpolate(l2[1], size=o[3].shape[2:], mode='bilinear')])
        return o[0], o[1], o[2], o[3], o[4], b0, b1, b2, b3


class SmallsegNet(nn.Module):
    """models/dsnet_t2_warp.py:144-167: nn.segNet without the two x2 upsamplings and without log_softmax (raw scores).
    forward(x, size, xleft) -> (x, x1_1, seg): the 32-channel decoder map, the 1x1-fused map at xleft's resolution and the
    scores resized (nearest) to `size`."""

    def __init__(self, in_channels, feature_channel, labels=8, pretrained=False):
        super().__init__()
        self.conv1d_1 = _c1x1(in_channels, 64)
        self.Conv2DownUp1 = Conv2DownUp(64, 32, 3)
        self.conv1d_2 = _c1x1(32 + feature_channel, 32)
        self.Conv2DownUp2 = nn.Sequential(Conv2DownUp(32, 32, 3, lastLayer=False),
                                          ConvTranspose2dSame(32, labels, 3, 1, padding='same', init_he=False))

    def forward(self, x, size, xleft, groups=1):
        x = self.Conv2DownUp1(self.conv1d_1[0].run(x, act=1), groups)
        s = ops.upcat_conv1x1(x, xleft, self.conv1d_2[0].c2d.weight, act=1)
        if s is None:
            s = self.conv1d_2[0].run(ops.concat([ops.interpolate(x, size=xleft.shape[2:], mode='nearest'), xleft]), act=1)
        seg = self.Conv2DownUp2[1](self.Conv2DownUp2[0](s, groups))
        return x, s, ops.interpolate(seg, size=size, mode='nearest')


class segNetB2(nn.Module):
    """models/dsnet_t2_warp.py:310-337.  Constructed by both warp networks and never called (upstream's call is commented
    out): it exists for its state_dict keys."""

    def __init__(self, inplane_seg2, labels):
        super().__init__()
        self.conv1d_1 = _c1x1(inplane_seg2, 128)
        self.Conv2DownUp1 = Conv2DownUp(128, 64, 3)
        self.Conv2DownUp2 = Conv2DownUp(32, 64, 3)
        self.Conv2DownUp3 = Conv2DownUp(128, 64, 3)
        self.conv1d_2 = _c1x1(65, 32)
        self.Conv2DownUp5 = nn.Sequential(Conv2DownUp(32, 32, 3, lastLayer=False),
                                          ConvTranspose2dSame(32, labels, 3, 1, padding='same', init_he=False))


class _WarpNet(nn.Module):
    """What minidsnetDivide and minidsnetDivideSoftmax share (models/dsnet_t2_warp.py:577-633 and :169-215 are the same
    constructor up to the gate head).  Members upstream builds and never calls (conv2d_ba2, conv2d_ba3, conv1d_3,
    segNetB2, aspp) are kept for their keys; conv2d_ba0 is RUN on both images with its output unused, so its running
    statistics move twice per training step, as upstream."""
    three_outputs = True       # train.TrainStep: loss of the `ThreeOutPuts` type, CE(outs[0]) + [CFG.loss](outs[2]) + CE(outs[4]) + L1(outs[1])

    def _build(self, CFG, labels, pretrained, patch_type, include_edges, backbone, aspp_name, segnet_in, segnet_feat):
        self.patch_type, self.include_edges, self.aspp_mod = patch_type, include_edges, CFG.aspp
        self.resnet_features = piramidNet2Warp(pretrained=pretrained, backbone=backbone)
        if self.aspp_mod:
            from .aspp import build_aspp
            self.aspp = build_aspp(aspp_name, 32)
        for j in range(4):
            setattr(self, 'conv2d_ba%d' % j, _img_conv(4 if include_edges else 3))
        patch = (1, 17) if patch_type == '1dcorr' else (17, 17)
        self.correlation_sampler = SpatialCorrelationSampler(1, patch, 1, 0, dilation_patch=1)
        self.corrConv2d = _c1x1(patch[0] * patch[1], 128)
        self.Conv2DownUp3 = Conv2DownUp(32, 128, 3)
        self.Conv2DownUp4 = Conv2DownUp(256, 64, 3)
        self.segNet = SmallsegNet(segnet_in, segnet_feat, labels)
        self.conv1d_2 = _c1x1(65, 64)
        self.Conv2DownUp5 = Conv2DownUp(64, 64, 5, lastLayer=False)
        self.dispoutConv = ConvTranspose2dSame(64, 1, 5, padding='same', init_he=False)
        self.conv1d_3 = _c1x1(96, 64)
        self.segNetB2 = segNetB2(256, labels)

    def _trunk(self, input_a, input_b, feature_of):
        """Everything up to the gate: returns (seg_left, seg_right, disp, s2_d input of the gate head).
        feature_of(taps, B) -> the full-batch feature map SmallsegNet concatenates ([left | right] halves)."""
        B = input_a.shape[0]
        size = input_a.shape[2:]
        both, img_a = _stereo_buffer(input_a, input_b, self.include_edges)
        if self.include_edges:      # conv2d_ba0 sees the right image's edge map too (the towers' weights have no 4th column)
            both[B:, 3] = input_b[:, 3]
        t = self.resnet_features(both, groups=2)              # batch = [left | right], one statistics group per image side
        xl2 = self.conv2d_ba1[0].fused(img_a, act=1)
        self.conv2d_ba0[0].fused(both, act=1, groups=2)       # computed on both images and unused, exactly as upstream
        # the two SmallsegNet calls of upstream share weights and normalise each with its own batch statistics: one batched
        # pass with two statistics groups
        x, x1_1, seg = self.segNet(t[8], size, feature_of(t, B), groups=2)
        x, x1_1 = ops.split_batch(x, B)[0], ops.split_batch(x1_1, B)[0]
        seg_l, seg_r = ops.split_batch(seg, B)
        pa, pb = ops.split_batch(t[7], B)
        y, disp = self._disparity(x, xl2, pa, pb, size)
        s2_d = ops.concat([x1_1, ops.interpolate(y, size=x1_1.shape[2:])])
        return seg_l, seg_r, disp, s2_d

    def _disparity(self, x, xl2, pa, pb, size):
        """The disparity branch: correlation of the 1/8 pyramids, Conv2DownUp3/4, the x8 head.  Returns (y, disp): the
        64-channel 1/8 map the gate heads read as well, and the full-resolution disparity."""
        y = self.correlation_sampler(pa, pb)
        if self.patch_type == '1dcorr':
            y = self.corrConv2d[0].run(torch.squeeze(y, 1), act=1)
        else:
            n, ph, pw, h, w = y.shape
            y = self.corrConv2d[0].run(ops.affine_act(y.reshape(n, ph * pw, h, w), _const(1.0 / pa.size(1), ph * pw, y.device), None), act=1)
        y1 = ops.interpolate(self.Conv2DownUp3(x), size=y.shape[2:], mode='bilinear')
        y = self.Conv2DownUp4(ops.concat([y1, y]))
        xl2 = ops.interpolate(xl2, size=(8 * y.shape[2], 8 * y.shape[3]), mode='bilinear')
        d0 = ops.upcat_conv1x1(y, xl2, self.conv1d_2[0].c2d.weight, act=1)
        if d0 is None:
            d0 = self.conv1d_2[0].run(ops.concat([ops.interpolate(y, scale_factor=8), xl2]), act=1)
        return y, ops.interpolate(self.dispoutConv(self.Conv2DownUp5(d0)), size=size, mode='bilinear')


class minidsnetDivide(_WarpNet):
    """models/dsnet_t2_warp.py:577-700 (`-net dsnet_warp`).  SmallsegNet reads the 1/4 pyramid of the matching image; the
    gate is one sigmoid channel.  forward(left, right) -> (both, disp, seg_left, disp, warped_right, gate)."""

    def __init__(self, CFG, labels=8, pretrained=False, patch_type='', include_edges=False, backbone='densenet'):
        super().__init__()
        if backbone not in BACKBONES:
            raise NotImplementedError("backbone %r: only %s are on the native path" % (backbone, " and ".join(BACKBONES)))
        segnet_in, segnet_feat = (176, 152) if backbone == 'mobilenet' else (576, 256)
        self._build(CFG, labels, pretrained, patch_type, include_edges, backbone, 'densenet', segnet_in, segnet_feat)
        self.Conv2DownUp7 = Conv2DownUp(96, 64, 3)
        self.conv1d_at_d = nn.Sequential(conv2dSame(64, 1, 1, padding='same'), nn.Sigmoid())

    def forward(self, input_a, input_b):
        seg_l, seg_r, disp, s2_d = self._trunk(input_a, input_b, lambda t, B: t[6])
        at_d = self.conv1d_at_d[0].run(self.Conv2DownUp7(s2_d), act=2)
        at_d = ops.interpolate(at_d, size=seg_l.shape[2:], mode='nearest')
        both, warped = ops.warp_blend(seg_l, seg_r, disp, at_d)
        return both, disp, seg_l, disp, warped, at_d


class minidsnetDivideSoftmax(_WarpNet):
    """models/dsnet_t2_warp.py:169-308 (`-net dsnet_warp_soft`).  Always DenseNet (the `backbone` argument is ignored, as
    upstream); SmallsegNet reads the LEFT image's 1/2 pyramid in both calls; the gate has one channel per class and a
    softmax over them.  forward(left, right) -> (seg_left, disp, both, disp, warped_right, gate)."""

    def __init__(self, CFG, labels=8, pretrained=False, patch_type='', include_edges=False, backbone='densenet'):
        super().__init__()
        self._build(CFG, labels, pretrained, patch_type, include_edges, 'densenet', 'densenet_a1', 576, 224)
        self.Conv2DownUp7 = nn.Sequential(Conv2DownUp(96, 64, 3, lastLayer=False),
                                          ConvTranspose2dSame(64, labels, 3, 1, padding='same', init_he=False))

    def forward(self, input_a, input_b):
        seg_l, seg_r, disp, s2_d = self._trunk(input_a, input_b, lambda t, B: ops.repeat_batch(ops.split_batch(t[5], B)[0]))
        at_d = self.Conv2DownUp7[1](self.Conv2DownUp7[0](s2_d))
        at_d = ops.interpolate(at_d, size=seg_l.shape[2:], mode='nearest')
        both, warped, prob = ops.warp_blend(seg_l, seg_r, disp, at_d, softmax_gate=True)
        return seg_l, disp, both, disp, warped, prob


class _WarpDispNet(_WarpNet):
    """What minidsnetDivideDisp and minidsnetDivideDisp2 share (models/dsnet_t2_warp.py:704-972: one constructor, one forward up
    to the image of the third tower pass).  minidsnetDivide's members in its order, then Conv2DownUp7 over 128 channels (both
    decoder maps and the disparity features) and the sigmoid gate.  The tower runs THREE times in sequence - left, right (only
    its 1/8 pyramid is used), the right image moved into the left view - and SmallsegNet twice, on the first and the third
    pass: the third depends on the disparity, so nothing is batched and every BatchNorm of the tower moves its running
    statistics three times per training step, in upstream's order.  The two segmentation maps are blended WITHOUT a warp
    (upstream's warp line is commented out): ops.gate_blend.  DenseNet only."""

    def __init__(self, CFG, labels=8, pretrained=False, patch_type='', include_edges=False, backbone='densenet'):
        super().__init__()
        if backbone != 'densenet':
            raise NotImplementedError("backbone %r: %s is on the native path with 'densenet' only" % (backbone, type(self).__name__))
        self._build(CFG, labels, pretrained, patch_type, include_edges, 'densenet', 'densenet', 576, 256)
        self.Conv2DownUp7 = Conv2DownUp(128, 64, 3)
        self.conv1d_at_d = nn.Sequential(conv2dSame(64, 1, 1, padding='same'), nn.Sigmoid())

    def _run(self, input_a, input_b, third_image):
        """third_image(right, disp_out) -> the (B,3,H,W) input of the third tower pass.
        Returns (both, disp_out, seg_left, seg_right, gate, third image)."""
        B = input_a.shape[0]
        size = input_a.shape[2:]
        both, img_a = _stereo_buffer(input_a, input_b, self.include_edges)
        if self.include_edges:      # conv2d_ba0 sees the right image's edge map too (the tower's weights have no 4th column)
            both[B:, 3] = input_b[:, 3]
        ta = self.resnet_features(both[:B])
        tb = self.resnet_features(both[B:])
        xl2 = self.conv2d_ba1[0].fused(img_a, act=1)
        self.conv2d_ba0[0].fused(both, act=1, groups=2)       # computed on both images and unused, exactly as upstream
        x, x1_1, seg_l = self.segNet(ta[8], size, ta[6])
        y, disp = self._disparity(x, xl2, ta[7], tb[7], size)
        third = third_image(both[B:, :3], disp)
        tc = self.resnet_features(third)
        _, x2_1, seg_r = self.segNet(tc[8], size, tc[6])
        s2_d = ops.concat([x1_1, x2_1, ops.interpolate(y, size=x1_1.shape[2:])])
        at_d = self.conv1d_at_d[0].run(self.Conv2DownUp7(s2_d), act=2)
        at_d = ops.interpolate(at_d, size=seg_l.shape[2:], mode='nearest')
        return ops.gate_blend(seg_l, seg_r, at_d), disp, seg_l, seg_r, at_d, third


class minidsnetDivideDisp(_WarpDispNet):
    """models/dsnet_t2_warp.py:704-836 (`-net dsnet_warp_disp`, output type `ThreeOutPutsDisp`).  The third tower pass reads the
    right image warped by the GROUND-TRUTH disparity and cut where that is not positive (ops.warp_image_masked): a constant,
    no gradient flows through it.  forward(left, right, disp) -> (both, disp_out, seg_left, disp_out, seg_right, gate)."""
    disp_input = True          # step.model_outputs: called as model(left, right, disp) with the f32 disparity target

    def forward(self, input_a, input_b, disp):
        both, disp_out, seg_l, seg_r, at_d, _ = self._run(input_a, input_b, lambda right, _d: ops.warp_image_masked(right, disp))
        return both, disp_out, seg_l, disp_out, seg_r, at_d


class minidsnetDivideDisp2(_WarpDispNet):
    """models/dsnet_t2_warp.py:839-972 (`-net dsnet_warp_disp_consist`, output type `ThreeOutPutsDispConsist`).  The third tower
    pass reads warped_right = apply_disparity(right, -disp_out), the right image warped by the PREDICTED disparity: the
    gradient of the segmentation losses flows back through the whole tower (densenet._Stem's data gradient) into the
    disparity head, and the step compares warped_right with the left image (ops.photo_loss) instead of disp_out with a
    disparity target.  forward(left, right) -> (both, disp_out, seg_left, disp_out, seg_right, warped_right)."""
    photo_outputs = True       # step.default_loss: three segmentation terms + MSE(outs[5], left), no L1

    def forward(self, input_a, input_b):
        both, disp_out, seg_l, seg_r, _, warped = self._run(input_a, input_b, lambda right, d: ops.apply_disparity(right, d, sign=-1.0))
        return both, disp_out, seg_l, disp_out, seg_r, warped
