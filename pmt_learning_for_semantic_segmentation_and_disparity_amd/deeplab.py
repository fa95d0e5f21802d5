"""DeepLabV3+ on Xception-65 (`-net deeplab`, models_deeplab/{net,encoder,xception,spp,common}.py), MI355X-native: the mono
baseline of the reference.  Same module tree, state_dict keys and parameter order; encoder, ASPP and SeparableConv2d are
those of deeplab_mod.py (upstream the two packages differ in the taps the encoder returns and in SPPDecoder only).

forward(inputs) -> logits at 1/4 resolution.  `SPPNet(..., harness=True)` (keyword-only, not in the reference) wraps the
steps of the reference's harness around it (torch_implementation.py:123-131,163): inputs*2 - 1, one zero row and column
appended bottom / right, logits resized bilinear align_corners=True to (h+1, w+1) and cropped to h x w.  Upstream this
network has no disparity head: a TrainStep on it needs a loss of the caller's (`loss_fn=`).
"""
import torch.nn as nn

from . import ops
from .deeplab_mod import (ASPP, SeparableConv2d, XceptionBlock, Xception65, _SPPNetBase,  # noqa: F401  (the shared pieces)
                          create_encoder, pad_bottom_right, resize_crop)
from .deeplab_mod import SPPDecoder as _SPPDecoderMod


class SPPDecoder(_SPPDecoderMod):
    """models_deeplab/spp.py:111-129: no concat_prev, returns x alone."""

    def __init__(self, in_channels, reduced_layer_num=48):
        super().__init__(in_channels, 256, False, reduced_layer_num)

    def forward(self, x, low_level_feat):
        return super().forward(x, low_level_feat)[0]


def create_spp(dec_type, in_channels=2048, middle_channels=256, output_stride=8):
    """models_deeplab/spp.py:131-141; 'aspp' only."""
    if dec_type != 'aspp':
        raise NotImplementedError("dec_type %r: only 'aspp' is built" % (dec_type,))
    return ASPP(in_channels, middle_channels, output_stride), SPPDecoder(middle_channels)


class SPPNet(_SPPNetBase):
    """models_deeplab/net.py:82-135."""

    def __init__(self, output_channels=19, enc_type='xception65', dec_type='aspp', output_stride=8, *, harness=False):
        super().__init__()
        self.output_channels = output_channels
        self.enc_type = enc_type
        self.dec_type = dec_type
        self.harness = harness
        self.encoder = create_encoder(enc_type, output_stride=output_stride, pretrained=False)
        self.spp, self.decoder = create_spp(dec_type, output_stride=output_stride)
        self.logits = nn.Conv2d(256, output_channels, 1)

    def forward(self, inputs):
        h, w = inputs.shape[2:]
        if self.harness:
            inputs = pad_bottom_right(inputs, 2.0, -1.0)
        x, low, _, _ = self.encoder(inputs)
        x = self.decoder(self.spp(x), low)
        x = ops.conv2d(x, self.logits.weight, self.logits.bias)
        return resize_crop(x, h, w) if self.harness else x
