"""The Ext_small networks of the reference (models/dsnet_t2_ext_small.py; `-net sdnet_mini_ext_small`,
`sdnet_mini_ext_small_edge`, `sdnet_mini_ext_small_edgev2` of util/utilLoadNetwork.py:16-18) on the HIP kernels: same class
names, constructor signatures, state_dict keys, parameter order and output tuples.

They are minidsnetExt with three-convolution residual units (RCU) in place of Conv2DownUp, one attention gate instead of two
(`cat(s2_d * g, s2_s * (1 - g))`, ops.gate_pair) and, in Ext_small, the gradient-magnitude edge map of the left image
(ops.grad_mag) as the auxiliary input of the heads.  Ext_small and Ext_smallv2 are the `edgeOut` networks: their first output
is a one-channel edge logit map, trained with the balanced BCE of ops.edge_loss (`edge_outputs`, step.default_loss,
train.EdgeStepLoss).

Only what upstream can run is built: backbone='densenet' with CFG.aspp == 0.  With aspp 1 or 2 upstream's forward fails in
conv1d_4 (built for inplane_seg2 // 2 channels, fed 256 / 273), and Ext_smallv0 / Ext_smallv2 with 'mobilenet' feed segNet a
16-channel tap where it expects 64; Ext_small with 'mobilenet' would fit upstream's channel table and is not built yet.
"""
import torch
import torch.nn as nn

from . import ops
from .nn import (ConvTranspose2dSame, SpatialCorrelationSampler, _c1x1, _const, _img_conv, _stereo_buffer, conv2dSame, convbn,
                 deconvbn, piramidNet2, run_act_block)


class RCU(nn.Module):
    """models/dsnet_t2_ext_small.py:43-64: c1 -> c2 -> d3 (transposed) or c3 -> + c1's output; the skip add is fused into the
    BatchNorm+ReLU pass of the last layer.  With use_deconv=False upstream resizes c3's output to its own size before the
    add: the identity."""

    def __init__(self, in_channels, out_channels=3, kernel_size=3, lastLayer=True, use_deconv=True):
        super().__init__()
        self.lastLayer, self.use_deconv = lastLayer, use_deconv
        o, k = out_channels, kernel_size
        self.c1 = nn.Sequential(convbn(in_channels, o, k, 1, 'same', 1), nn.ReLU(inplace=True))
        self.c2 = nn.Sequential(convbn(o, o, k, 1, 'same', 1), nn.ReLU(inplace=True))
        if use_deconv:
            self.d3 = nn.Sequential(deconvbn(o, o, k, 1, 'same', 1), nn.ReLU(inplace=True))
        else:
            self.c3 = nn.Sequential(convbn(o, o, k, 1, 'same', 1), nn.ReLU(inplace=True))

    def forward(self, x):
        x = run_act_block(self.c1, x)
        x1 = run_act_block(self.c2, x)
        return run_act_block(self.d3 if self.use_deconv else self.c3, x1, residual=x)


class segNet(nn.Module):
    """models/dsnet_t2_ext_small.py:1072-1095: the file's own coarse head (RCU blocks, a plain convolution at the end)."""

    def __init__(self, in_channels, feature_channel, labels=8, pretrained=False, RCU_deconv=True):
        super().__init__()
        self.conv1d_1 = _c1x1(in_channels, 64)
        self.Conv2DownUp1 = RCU(64, 32, 3, use_deconv=RCU_deconv)
        self.conv1d_2 = _c1x1(32 + feature_channel, 32)
        self.Conv2DownUp2 = nn.Sequential(RCU(32, 32, 3, lastLayer=False, use_deconv=RCU_deconv),
                                          conv2dSame(32, labels, 3, 1, padding='same'))

    def forward(self, x, input_a, input_b, xleft):
        x = ops.interpolate(x, scale_factor=2, mode='nearest')
        x = self.Conv2DownUp1(self.conv1d_1[0].run(x, act=1))
        x1 = ops.interpolate(x, scale_factor=2, mode='nearest')
        s = ops.upcat_conv1x1(x, xleft, self.conv1d_2[0].c2d.weight, act=1)
        if s is None:
            s = self.conv1d_2[0].run(ops.concat([ops.interpolate(x, size=xleft.shape[2:], mode='nearest'), xleft]), act=1)
        s = self.Conv2DownUp2[1](self.Conv2DownUp2[0](s))
        return x, x1, ops.interpolate(s, size=input_a.shape[2:], mode='nearest')


class _ExtSmallBase(nn.Module):
    """What the three classes share: the constructor's member list (in upstream's order) and the forward up to the heads."""
    _deconv = True            # RCU(use_deconv=...) of every block
    _aux_from_edges = False   # the auxiliary input of the heads: the edge map's convolutions (Ext_small) or the towers' taps
    _head_labels = None       # labels of segNet's head; None: the network's `labels`

    def __init__(self, CFG, labels=8, pretrained=False, patch_type='', include_edges=False, backbone='densenet'):
        super().__init__()
        name = type(self).__name__
        if CFG.aspp != 0:
            raise NotImplementedError("%s with CFG.aspp = %r: upstream's forward fails in conv1d_4 (built for inplane_seg2 // 2 "
                                      "channels, fed the ASPP's 256 / 273); only aspp = 0 runs" % (name, CFG.aspp))
        if backbone != 'densenet':
            why = ("it would fit upstream's channel table and is left for a follow-up" if self._aux_from_edges and backbone == 'mobilenet'
                   else "upstream cannot run it (segNet expects the 64-channel 1/2 tap of densenet)")
            raise NotImplementedError("%s with backbone %r: %s; only 'densenet' is on the native path" % (name, backbone, why))
        self.aspp_mod, self.backbone = CFG.aspp, backbone
        self.patch_type, self.include_edges = patch_type, include_edges
        rd = self._deconv
        edge = self._aux_from_edges
        self.resnet_features = piramidNet2(pretrained, backbone)
        for j in range(3):   # Ext_smallv0 / Ext_smallv2 build them and never call them: they exist for their keys
            setattr(self, 'conv2d_ba%d' % j, _img_conv(4 if include_edges else 3))
        patch = (1, 17) if patch_type == '1dcorr' else (17, 17)
        self.correlation_sampler = SpatialCorrelationSampler(1, patch, 1, 0, dilation_patch=1)
        self.s2_corr_sampler = SpatialCorrelationSampler(1, patch, 1, 0, dilation_patch=1)
        self.corrConv2d = _c1x1(patch[0] * patch[1], 128)
        self.Conv2DownUp3 = RCU(32, 64, 3, use_deconv=rd)
        self.Conv2DownUp4 = RCU(128 + 64, 64, 3, use_deconv=rd)
        head = labels if self._head_labels is None else self._head_labels
        self.segNet = segNet(1024 * 2, 1, head, RCU_deconv=False) if edge else segNet(1024 * 2, 64, head)
        self.conv1d_2 = _c1x1(64 + (1 if edge else 64), 64)
        self.Conv2DownUp5 = RCU(64, 64, 5, lastLayer=False, use_deconv=rd)
        self.dispoutConv = ConvTranspose2dSame(64, 1, 5, padding='same', init_he=False)
        self.conv1d_3 = _c1x1(96, 64)          # never called upstream either: kept for the state_dict
        self.conv1d_4 = _c1x1(512 // 2, 128)
        self.Conv2DownUp6 = RCU(128, 64, 3, use_deconv=rd)
        self.Conv2DownUp7 = RCU(128, 64, 3, use_deconv=rd)
        self.Conv2DownUp8 = RCU(32, 64, 3, use_deconv=rd)
        self.Conv2DownUp9 = RCU(128, 64, 3, use_deconv=rd)
        self.conv1d_at = nn.Sequential(conv2dSame(64, 1, 1, padding='same'), nn.Sigmoid())
        self.Conv2DownUp10 = RCU(128, 64, 3, use_deconv=rd)
        self.conv1d_5 = _c1x1(64 + (1 if edge else 224), 32)
        self.Conv2DownUp11 = nn.Sequential(RCU(32, 32, 3, lastLayer=False, use_deconv=rd), conv2dSame(32, labels, 3, 1, padding='same'))

    def _edge_map(self, input_a, left_e):
        """The (B, 3 | 4, H, W) edge map: the caller's, or ops.grad_mag of the left image as the network receives it (with
        include_edges all four channels, as netForward computes it after the concat, torch_implementation.py:136,263)."""
        if left_e is None:
            return ops.grad_mag(input_a.detach())
        if tuple(left_e.shape) != tuple(input_a.shape):
            raise ValueError("left_e must have the left image's shape %s, got %s" % (tuple(input_a.shape), tuple(left_e.shape)))
        return left_e.to(input_a.dtype)

    def _forward(self, input_a, input_b, left_e):
        B = input_a.shape[0]
        size = input_a.shape[2:]
        both, _ = _stereo_buffer(input_a, input_b, self.include_edges)
        t = self.resnet_features(both, groups=2)          # taps of both towers, batch = [left | right]
        halves = [ops.split_batch(u, B) for u in t]
        a = [h[0] for h in halves]
        b = [h[1] for h in halves]
        if self._aux_from_edges:
            e = self._edge_map(input_a, left_e)
            e2 = ops.interpolate(e, size=(size[0] // 2, size[1] // 2), mode='bilinear')     # upstream's edge_1 and edge_2: one tensor
            xl2 = self.conv2d_ba1[0].fused(e2, act=1)
            xl1 = self.conv2d_ba2[0].fused(e, act=1)
            xl0 = self.conv2d_ba0[0].fused(e2, act=1)
        else:
            xl0 = xl2 = a[0]
        x, x1, seg1 = self.segNet(ops.concat([a[4], b[4]]), input_a, input_b, xl0)

        y = self.correlation_sampler(a[5], b[5])
        if self.patch_type == '1dcorr':
            y = self.corrConv2d[0].run(torch.squeeze(y, 1), act=1)
        else:
            n, ph, pw, h, w = y.shape
            # the reference divides the 2-D correlation by C (:300): folded into the input of the 1x1 convolution
            y = self.corrConv2d[0].run(ops.affine_act(y.reshape(n, ph * pw, h, w), _const(1.0 / a[5].size(1), ph * pw, y.device), None), act=1)
        y1 = ops.interpolate(self.Conv2DownUp3(x1), size=y.shape[2:], mode='bilinear')
        y = self.Conv2DownUp4(ops.concat([y1, y]))
        xl2 = ops.interpolate(xl2, size=(8 * y.shape[2], 8 * y.shape[3]), mode='bilinear')
        d0 = ops.upcat_conv1x1(y, xl2, self.conv1d_2[0].c2d.weight, act=1)
        if d0 is None:
            d0 = self.conv1d_2[0].run(ops.concat([ops.interpolate(y, scale_factor=8), xl2]), act=1)
        disp = ops.interpolate(self.dispoutConv(self.Conv2DownUp5(d0)), size=size, mode='bilinear')

        s2 = self.Conv2DownUp6(self.conv1d_4[0].run(b[6], act=1))      # aspp 0: the RIGHT tower's 1/4 pyramid alone (:342)
        y3 = ops.interpolate(y, size=s2.shape[2:])
        s2_d = self.Conv2DownUp7(ops.concat([s2, y3]))
        x3 = ops.interpolate(self.Conv2DownUp8(x1), size=s2.shape[2:])
        s2_s = self.Conv2DownUp9(ops.concat([s2, x3]))
        s2_at = self.conv1d_at[0].run(s2, act=2)
        s2 = self.Conv2DownUp10(ops.gate_pair(s2_d, s2_s, s2_at))
        aux = xl1 if self._aux_from_edges else a[7]
        seg2 = ops.upcat_conv1x1(s2, aux, self.conv1d_5[0].c2d.weight, act=1)
        if seg2 is None:
            seg2 = self.conv1d_5[0].run(ops.concat([ops.interpolate(s2, size=aux.shape[2:]), aux]), act=1)
        seg2 = self.Conv2DownUp11[1](self.Conv2DownUp11[0](seg2))
        if not self._aux_from_edges:
            seg2 = ops.interpolate(seg2, size=size, mode='nearest')
        return seg1, disp, seg2, disp


class Ext_smallv0(_ExtSmallBase):
    """models/dsnet_t2_ext_small.py:639-892 (`-net sdnet_mini_ext_small`): an ordinary four-output network,
    forward(left, right) -> (seg_branch, disp_out, seg_branch2, disp_out); it trains under the default step."""

    def forward(self, input_a, input_b):
        return self._forward(input_a, input_b, None)


class Ext_smallv2(_ExtSmallBase):
    """models/dsnet_t2_ext_small.py:382-636 (`-net sdnet_mini_ext_small_edgev2`): Ext_smallv0 with a one-channel first head,
    the edge logits.  Upstream resizes `left_e` twice and discards both results: the argument is ignored and nothing is
    computed for it.  forward(left, right, left_e=None) -> (edge logits, disp_out, seg_branch2, disp_out)."""
    _head_labels = 1
    edge_outputs = True

    def forward(self, input_a, input_b, left_e=None):
        return self._forward(input_a, input_b, None)


class Ext_small(_ExtSmallBase):
    """models/dsnet_t2_ext_small.py:130-378 (`-net sdnet_mini_ext_small_edge`): the heads read convolutions of the edge map
    instead of the towers' taps, every RCU ends in a plain convolution, the first head gives the edge logits.
    forward(left, right, left_e=None) -> (edge logits, disp_out, seg_branch2, disp_out).  left_e: the edge map
    compute_grad_mag(left, True, False) of the harness; None (the one deviation from upstream's signature, so that a training
    step needs no fifth input): ops.grad_mag of the left image, computed here."""
    _deconv = False
    _aux_from_edges = True
    _head_labels = 1
    edge_outputs = True

    def forward(self, input_a, input_b, left_e=None):
        return self._forward(input_a, input_b, left_e)
