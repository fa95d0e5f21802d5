"""Timings of the segmentation loss terms (csrc/segloss.hip) on one GPU, in one process, alternating rounds (medians printed
as one JSON line).  On bf16 logits of B=8 256x512 C=2 and B=4 512x1024 C=19, with every term switched on
(cross-entropy with class weights + Tversky + diceEntropy; the kernels do the same work whatever the list):
  * each of the three launches alone (sdhip_seg_sums, sdhip_seg_finish, sdhip_seg_terms_bwd) and the three together;
  * the GB/s of the three against the bytes they must move: logits and target read twice, gradient written once;
  * sdhip_ce_loss (forward + gradient in ONE pass) on the same tensors: the existing baseline, expected near half.

Usage:  python tests/diag/gpu_segloss_bench.py [--rounds 5]"""
import argparse
import json
import os
import sys

import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, dtype_code, ptr, stream_ptr
    out = {}
    for B, H, W, C in ((8, 256, 512, 2), (4, 512, 1024, 19)):
        g = torch.Generator(device="cuda").manual_seed(3)
        x = torch.randn(B, H, W, C, device="cuda", generator=g).bfloat16()                       # NHWC, ld = C
        lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        onehot = torch.nn.functional.one_hot(lab, C).float().contiguous()                         # NHWC f32 target
        cw = torch.rand(C, device="cuda", generator=g) + 0.5
        grad = torch.empty_like(x)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        ws = torch.empty(_lib.seg_terms_workspace_bytes(B, H * W, C), dtype=torch.uint8, device="cuda")
        dt, terms = dtype_code(x), _lib.SEG_TVERSKY | _lib.SEG_DICE_ENTROPY

        def sums():
            call("sdhip_seg_sums", ptr(x), C, ptr(onehot), C, B, H * W, C, ptr(ws), ws.numel(), dt, stream_ptr())

        def finish():
            call("sdhip_seg_finish", ptr(ws), ws.numel(), ptr(cw), ptr(loss), B, H * W, C, 0.5, terms, stream_ptr())

        def bwd():
            call("sdhip_seg_terms_bwd", ptr(x), C, ptr(onehot), C, ptr(grad), C, ptr(ws), ws.numel(), B, H * W, C, dt, stream_ptr())

        def three():
            sums(); finish(); bwd()

        def ce():
            call("sdhip_ce_loss", ptr(x), C, ptr(onehot), C, ptr(grad), C, ptr(loss), B * H * W, C, 1.0, dt, stream_ptr())

        fns = {"sums_us": sums, "finish_us": finish, "bwd_us": bwd, "three_us": three, "ce_loss_us": ce}
        for f in fns.values():
            _time(f, 5)
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                res[k].append(_time(f, 20))
        r = {k: _median(v) for k, v in res.items()}
        nbytes = 2 * (x.numel() * 2 + onehot.numel() * 4) + grad.numel() * 2
        r["bytes_MB"] = nbytes / 1e6
        r["three_GBps"] = nbytes / r["three_us"] / 1e3
        r["ce_loss_GBps"] = (x.numel() * 2 + onehot.numel() * 4 + grad.numel() * 2) / r["ce_loss_us"] / 1e3
        r["ratio_to_ce_loss"] = r["three_us"] / r["ce_loss_us"]
        out["B%d_%dx%d_C%d" % (B, H, W, C)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
