"""Timings of the `*_disp` warp networks and their kernels on one GPU, in one process, alternating rounds (medians printed as one
JSON line):
  * sdhip_warp_image_masked, sdhip_gate_blend_fwd / _bwd and sdhip_photo_mse (both launches), called through the C ABI on
    preallocated bf16 buffers at B=8 256x512, so the figures are kernel time.  Algorithmic bytes per pixel: masked warp reads the
    f32 disparity and two pixels of C channels and writes one (4 + 3 C es; the two source pixels mostly share cache lines, so
    4 + 2 C es is what has to cross HBM); gate blend forward (3C + 1) es, backward (5C + 2) es; photometric MSE reads w and the
    f32 image and writes the gradient (2 C es + 4 C);
  * the captured bf16 step of warp.minidsnetDivideDisp and warp.minidsnetDivideDisp2 beside warp.minidsnetDivide, the nearest
    network that existed before them, B=8 256x512.

Usage:  python tests/diag/gpu_warp_disp_bench.py [--rounds 5] [--skip-steps]"""
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


def kernels(rounds):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import BF16, call, ptr, stream_ptr
    B, H, W, es = 8, 256, 512, 2
    npix = B * H * W
    g = torch.Generator(device="cuda").manual_seed(3)
    nhwc = lambda c, ld, dt=torch.bfloat16: torch.rand(B, H, W, ld, device="cuda", generator=g).to(dt)[..., :c]
    img = nhwc(3, 8)                                    # the right half of the stereo buffer: 3 channels at a pixel stride of 8
    left = torch.rand(B, 3, H, W, device="cuda", generator=g)      # the f32 NCHW image a step is fed
    gt = torch.rand(B, 1, H, W, device="cuda", generator=g) * 16 - 4
    out, w, grad = nhwc(3, 8), nhwc(3, 3), torch.empty(B, H, W, 3, device="cuda", dtype=torch.bfloat16)
    loss = torch.zeros(1, device="cuda", dtype=torch.float64)
    nws = _lib.photo_mse_workspace_bytes(npix)
    ws = torch.empty(nws // 8, device="cuda", dtype=torch.float64)
    res = {}
    fns = {"warp_image_masked": (lambda: call("sdhip_warp_image_masked", ptr(img), H * W * 8, 1, 8, BF16, ptr(gt), ptr(out), 8, BF16, B, H, W, 3,
                                              stream_ptr()), npix * (4 + 2 * 3 * es)),
           "photo_mse": (lambda: call("sdhip_photo_mse", ptr(w), 3, BF16, ptr(left), 3 * H * W, H * W, 1, ptr(grad), ptr(loss), 1.0, B, H, W, 3,
                                      ptr(ws), nws, stream_ptr()), npix * (2 * 3 * es + 4 * 3))}
    for C in (2, 19):
        a, b, y, gy, ga, gb = (nhwc(C, C) for _ in range(6))
        gate, gg = nhwc(1, 1), nhwc(1, 1)
        fns["gate_blend_fwd_C%d" % C] = (lambda a=a, b=b, gate=gate, y=y, C=C: call(
            "sdhip_gate_blend_fwd", ptr(a), C, ptr(b), C, ptr(gate), 1, ptr(y), C, npix, C, BF16, stream_ptr()), npix * (3 * C + 1) * es)
        fns["gate_blend_bwd_C%d" % C] = (lambda a=a, b=b, gate=gate, gy=gy, ga=ga, gb=gb, gg=gg, C=C: call(
            "sdhip_gate_blend_bwd", ptr(gy), C, ptr(a), C, ptr(b), C, ptr(gate), 1, ptr(ga), C, ptr(gb), C, ptr(gg), 1, npix, C, BF16,
            stream_ptr()), npix * (5 * C + 2) * es)
    for f, _ in fns.values():
        _time(f, 5)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (f, _) in fns.items():
            t[k].append(_time(f, 20))
    for k, (_, nbytes) in fns.items():
        us = _median(t[k])
        res[k] = {"us": us, "bytes": nbytes, "TBps": nbytes / us * 1e-6}
    return res


def _step(name):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, ops, warp
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(8, 256, 512)
    torch.manual_seed(0)
    m = getattr(warp, name)(N.CFG(), labels=2, patch_type='1dcorr').cuda().train()
    t = TrainStep(m, dtype=torch.bfloat16, use_graph=True)
    t(*batch)                        # warm-up + capture
    ops.set_step_context(None)
    assert t.graph is not None, name + ": the step was not captured"
    return t, batch


def steps(rounds):
    ts = {k: _step(k) for k in ("minidsnetDivide", "minidsnetDivideDisp", "minidsnetDivideDisp2")}
    res = {k: [] for k in ts}
    for _ in range(rounds):
        for k, (t, batch) in ts.items():
            res[k].append(_time(lambda: t(*batch), 10) / 1000.0)
    out = {"%s_step_ms" % k: _median(v) for k, v in res.items()}
    for k in ("minidsnetDivideDisp", "minidsnetDivideDisp2"):
        out[k + "_ratio"] = out[k + "_step_ms"] / out["minidsnetDivide_step_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    r = {"kernels_B8_256x512_bf16": kernels(a.rounds)}
    if not a.skip_steps:
        r["steps_B8_256x512_bf16"] = steps(a.rounds)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
