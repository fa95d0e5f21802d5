"""Multitask loss timings on one GPU, in one process, alternating A/B rounds (medians printed as one JSON line):
  * fwd + bwd of one segmentation term (sdhip_mt_seg_fwd/bwd through ops.multitask_seg_loss, mean upstream) against
    sdhip_ce_loss (forward + gradient in one pass) on the same bf16 logits: B=4 512x1024 C=19 and B=8 256x512 C=2;
  * the captured bf16 step of minidsnetExt(multaskloss=1) against the ordinary step, B=8 256x512.

Usage:  python tests/diag/gpu_multitask_bench.py [--rounds 5] [--skip-steps]"""
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


def loss_terms(rounds):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, dtype_code, ptr, stream_ptr
    out = {}
    for B, H, W, C in ((4, 512, 1024, 19), (8, 256, 512, 2)):
        g = torch.Generator(device="cuda").manual_seed(3)
        x = torch.randn(B, H, W, C, device="cuda", generator=g).bfloat16().permute(0, 3, 1, 2)   # NHWC, ld = C
        lab = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        onehot = torch.nn.functional.one_hot(lab, C).float().contiguous()                         # NHWC f32 target
        lv = torch.nn.Parameter(torch.zeros(1, device="cuda"))
        grad = torch.empty_like(x)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        xr = x.detach().requires_grad_(True)

        def mt():
            xr.grad = None
            lv.grad = None
            ops.loss_map_mean(ops.multitask_seg_loss(xr, lab, lv)).backward()

        def ce():
            call("sdhip_ce_loss", ptr(x), C, ptr(onehot), C, ptr(grad), C, ptr(loss), B * H * W, C, 1.0, dtype_code(x), stream_ptr())

        for f in (mt, ce):
            _time(f, 5)
        a, b = [], []
        for _ in range(rounds):
            a.append(_time(mt, 20))
            b.append(_time(ce, 20))
        key = "B%d_%dx%d_C%d" % (B, H, W, C)
        out[key] = {"mt_seg_fwd_bwd_us": _median(a), "ce_loss_us": _median(b), "ratio": _median(a) / _median(b)}
    return out


def steps(rounds):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(8, 256, 512)
    ts = {}
    for name, mode in (("plain", 0), ("multitask", 1)):
        torch.manual_seed(0)
        m = N.minidsnetExt(N.CFG(multaskloss=mode), labels=2, patch_type='1dcorr').cuda().train()
        ts[name] = TrainStep(m, dtype=torch.bfloat16, use_graph=True)
        ts[name](*batch)                        # warm-up + capture
        ops.set_step_context(None)
    res = {k: [] for k in ts}
    for _ in range(rounds):
        for k, t in ts.items():
            res[k].append(_time(lambda: t(*batch), 10) / 1000.0)
    out = {"%s_step_ms" % k: _median(v) for k, v in res.items()}
    out["ratio"] = out["multitask_step_ms"] / out["plain_step_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    r = {"loss_terms": loss_terms(a.rounds)}
    if not a.skip_steps:
        r["steps_B8_256x512_bf16"] = steps(a.rounds)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
