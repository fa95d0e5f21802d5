"""Uncertainty-weighted multitask loss (`-multaskloss 1|2`): the reference's `multiTask_loss`
(util/utilTorchLoss.py:521-540) on the HIP kernels of csrc/multitask.hip."""
import torch
import torch.nn as nn

from . import ops


class multiTask_loss(nn.Module):
    """Same constructor, parameter names and forward contract as the reference.  three_out == 1: disparity + two
    segmentation terms; three_out == 2: disparity + one segmentation term, loss_seg2 is the (1,) zero tensor.
    forward(disp, disp_gt, seg1, seg2, seg_gt) -> (loss_disp (B,1,H,W), loss_seg1 (B,H,W), loss_seg2 (B,H,W) or (1,)),
    per-pixel f32 maps (reduction='none'); seg_gt holds int64 labels, 19 is ignored (and so is any label outside
    [0, C), which the reference rejects).  Each map carries the mean its forward pass computed (ops.loss_map_mean)."""

    def __init__(self, three_out=1):
        super().__init__()
        self.three_out = three_out
        self.log_var_disp = nn.Parameter(torch.zeros(1,))
        self.log_var_seg1 = nn.Parameter(torch.zeros(1,))
        if self.three_out == 1:
            self.log_var_seg2 = nn.Parameter(torch.zeros(1,))

    def forward(self, disp, disp_gt, seg1, seg2, seg_gt):
        loss_disp = ops.multitask_l1_loss(disp, disp_gt, self.log_var_disp)
        loss_seg1 = ops.multitask_seg_loss(seg1, seg_gt, self.log_var_seg1)
        if self.three_out == 1:
            loss_seg2 = ops.multitask_seg_loss(seg2, seg_gt, self.log_var_seg2)
        else:
            loss_seg2 = torch.zeros((1,), device=disp.device)
        return loss_disp, loss_seg1, loss_seg2


def step_loss(loss_disp, loss_seg1, loss_seg2):
    """mean(loss_disp) + mean(loss_seg1) + mean(loss_seg2): the step loss of the reference harness
    (torch_implementation.py:173-176,285,291,305,325), from the means the loss kernels produced.  A loss_seg2 without a
    mean is the constant zero placeholder of three_out == 2."""
    total = ops.loss_map_mean(loss_disp) + ops.loss_map_mean(loss_seg1)
    if getattr(loss_seg2, "sdhip_mean", None) is not None:
        total = total + ops.loss_map_mean(loss_seg2)
    elif loss_seg2.requires_grad or loss_seg2.numel() != 1:
        raise ops._lib.SdhipError("step_loss: loss_seg2 is neither a multitask loss map nor the zero placeholder")
    return total
