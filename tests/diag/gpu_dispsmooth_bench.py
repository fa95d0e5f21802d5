"""Timings of the `smooth_grad` disparity regulariser (csrc/dispsmooth.hip) on one GPU, in one process, alternating rounds
(medians printed as one JSON line).  On a bf16 disparity of B=8 256x512 with a 2-channel target and B=4 512x1024 with a
20-channel target (f32 image and target, labels constant over 32 x 32 blocks):
  * entry_us   sdhip_disp_smooth alone: the stencil and the fold, value and gradient (what a captured step replays);
  * floor_us   the same entry on a 3 x 3 image: its two launches with nothing to do;
  * fused_us   ops.disp_smooth_loss + backward, eager: the entry plus the autograd node's small ATen launches;
  * aten_us    the reference's formula composed from ATen (conv2d, pad, products over (B, L, H, W)) + backward on the same GPU:
               what a user of the package would run without the kernel;
  * the bytes the entry must move (3 image channels and C target channels in f32, the disparity read and its gradient
    written) and the GB/s of entry_us against them.

Usage:  python tests/diag/gpu_dispsmooth_bench.py [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / iters      # us


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _gauss():
    y, x = np.ogrid[-3:4, -3:4]
    h = np.exp(-(x * x + y * y) / 8.0)
    return torch.from_numpy((h / h.sum()).astype(np.float32)).view(1, 1, 7, 7)


def _diff(img, down):
    m, n = img.shape[2:]
    if down:
        return F.pad((img[:, :, :m - 1] - img[:, :, 1:]).abs(), (0, 0, 0, 1))
    return F.pad((img[:, :, :, :n - 1] - img[:, :, :, 1:]).abs(), (0, 1, 0, 0))


def aten_smooth(left, disp, seg, gauss, ones):
    """The formula of util/utilTorchLoss.py:41-101, op for op, on the tensors' device (disp in its own dtype up to the division)."""
    L = seg.shape[1]
    Y = (0.2126 * left[:, 0] + 0.7152 * left[:, 1] + 0.0722 * left[:, 2]).unsqueeze(1)
    Ys = F.conv2d(F.pad(Y, (3, 3, 3, 3)), gauss)
    mask = F.conv2d(F.pad(seg, (1, 1, 1, 1)), ones, groups=L) == 9
    d = disp.float() / 128
    reg_down = _diff(d, True) * seg * mask * torch.exp(1.0 - _diff(Ys, True) * seg)
    reg_right = _diff(d, False) * seg * mask * torch.exp(1.0 - _diff(Ys, False) * seg)
    return torch.mean(reg_down.sum(1) + reg_right.sum(1)) * 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, dtype_code, ptr, stream_ptr
    out = {}
    for B, H, W, C in ((8, 256, 512, 2), (4, 512, 1024, 20)):
        g = torch.Generator(device="cuda").manual_seed(3)
        left = torch.rand(B, 3, H, W, device="cuda", generator=g)
        lab = torch.randint(0, C, (B, H // 32, W // 32), device="cuda", generator=g)
        lab = lab.repeat_interleave(32, 1).repeat_interleave(32, 2)
        seg = F.one_hot(lab, C).float().permute(0, 3, 1, 2)                       # channels-last memory, pixel stride C
        disp = (torch.rand(B, 1, H, W, device="cuda", generator=g) * 8).bfloat16().requires_grad_(True)
        gauss, ones = _gauss().cuda(), torch.ones(C, 1, 3, 3, device="cuda")
        tv, ldt = ops.nhwc_view(seg)
        grad = torch.empty_like(disp)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        ws = torch.empty(_lib.disp_smooth_workspace_bytes(B, H, W) // 8, dtype=torch.float64, device="cuda")
        sb, sc, _, sw = left.stride()
        tiny = [torch.zeros(s, device="cuda") for s in ((1, 3, 3, 3), (1, 3, 3, 2), (1, 1, 3, 3), (1, 1, 3, 3))]

        def entry():
            call("sdhip_disp_smooth", ptr(left), sb, sc, sw, ptr(tv), ldt, ptr(disp), dtype_code(disp), ptr(grad), ptr(loss), B, H, W, C, 1.0,
                 ptr(ws), ws.numel() * 8, stream_ptr())

        def floor():
            call("sdhip_disp_smooth", ptr(tiny[0]), 27, 9, 1, ptr(tiny[1]), 2, ptr(tiny[2]), _lib.F32, ptr(tiny[3]), ptr(loss), 1, 3, 3, 2, 1.0,
                 ptr(ws), 8, stream_ptr())

        def fused():
            disp.grad = None
            ops.disp_smooth_loss(left, disp, seg).backward()

        def aten():
            disp.grad = None
            aten_smooth(left, disp, seg, gauss, ones).backward()

        # same answer first (the composition runs the disparity in f32 after the cast; the kernel rounds its gradient to bf16 once)
        fused()
        gf, vf = disp.grad.float().clone(), float(ops.disp_smooth_loss(left, disp.detach(), seg))
        aten()
        ga, va = disp.grad.float().clone(), float(aten_smooth(left, disp.detach(), seg, gauss, ones))
        fns = {"entry_us": entry, "floor_us": floor, "fused_us": fused, "aten_us": aten}
        for f in fns.values():
            _time(f, 5)
        res = {k: [] for k in fns}
        iters = {"entry_us": 400, "floor_us": 400, "fused_us": 100, "aten_us": 20}      # windows of 10 ms and more
        for _ in range(a.rounds):
            for k, f in fns.items():
                res[k].append(_time(f, iters[k]))
        r = {k: _median(v) for k, v in res.items()}
        r["spread"] = {k: [min(v), max(v)] for k, v in res.items()}
        nbytes = B * H * W * (3 * 4 + C * 4 + 2 * 2)
        r["bytes_MB"] = nbytes / 1e6
        r["entry_GBps"] = nbytes / r["entry_us"] / 1e3
        r["aten_over_fused"] = r["aten_us"] / r["fused_us"]
        r["aten_over_entry"] = r["aten_us"] / r["entry_us"]
        r["value_fused"], r["value_aten"] = vf, va
        r["grad_maxdiff_over_max"] = float((gf - ga).abs().max() / ga.abs().max())
        out["B%d_%dx%d_C%d" % (B, H, W, C)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
