"""Cost of the dilated depthwise kernels at deeplab_mod's shapes, and of its captured training step ("DeepLab"):
run on the GPU box, one part per process:

    python tools/gpu_deeplab_cost.py kernels          # B=8, 257x513 input (output stride 8), bf16
    python tools/gpu_deeplab_cost.py step [B]         # captured deeplab_mod(harness=True) step at B x 256 x 512, bf16

kernels: median of 20 launches after warm-up, one event pair per launch; bytes = the source read once + the output written
once (forward, data gradient; + x once more where the data gradient masks with it) or both tensors read once (weight gradient), against the 8000 GB/s HBM roof bench.py's
roofline_hbm uses.  Prints one JSON line per part.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, deeplab_mod, ops
from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch

HBM_GBS = 8000.0
# (C, H, W, stride, dilation, input ReLU): middle flow, ASPP branches, entry flow block2 sep_conv3, decoder sep2
SHAPES = [(728, 33, 65, 1, 2, 1), (2048, 33, 65, 1, 12, 0), (2048, 33, 65, 1, 24, 0), (2048, 33, 65, 1, 36, 0), (256, 129, 257, 2, 1, 1),
          (256, 65, 129, 1, 1, 0)]


def median_us(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def kernels(B=8):
    out = []
    for C, H, W, s, d, relu in SHAPES:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn(B, H, W, C, device="cuda").bfloat16()
        gy = torch.randn(B, Ho, Wo, C, device="cuda").bfloat16()
        y, gx = torch.empty_like(gy), torch.empty_like(x)
        w = torch.randn(C, 1, 3, 3, device="cuda") * 0.3
        gw = torch.zeros_like(w)
        st = torch.zeros(ops.NREP, 1, 2, C, dtype=torch.float64, device="cuda")
        nparts = ops.dw_dil_wgrad_parts(B, H, W, C, s)
        part = torch.empty(nparts * 9 * C, device="cuda")
        fwd = lambda: call("sdhip_dw_dil_conv_fwd", ptr(x), C, ptr(w), ptr(y), C, ptr(st), C, ops.NREP, B, H, W, C, s, d, relu, 1,
                           _lib.BF16, stream_ptr())
        dg = lambda: call("sdhip_dw_dil_conv_dgrad", ptr(gy), C, ptr(w), ptr(x) if relu else None, C, ptr(gx), C, B, H, W, C, s, d,
                          _lib.BF16, stream_ptr())
        wg = lambda: call("sdhip_dw_dil_conv_wgrad", ptr(x), C, ptr(gy), C, ptr(gw), ptr(part), nparts, B, H, W, C, s, d, relu,
                          _lib.BF16, stream_ptr())
        nin, nout = 2 * B * H * W * C, 2 * B * Ho * Wo * C
        row = {"C": C, "H": H, "W": W, "stride": s, "dil": d}
        for name, fn, nbytes in (("fwd", fwd, nin + nout), ("dgrad", dg, nin + nout + (nin if relu else 0)), ("wgrad", wg, nin + nout)):
            us = median_us(fn)
            gbs = nbytes / (us * 1e-6) / 1e9
            row[name] = {"us": round(us, 1), "GBs": round(gbs, 1), "hbm_frac": round(gbs / HBM_GBS, 3)}
        out.append(row)
    print(json.dumps({"kernels": out, "batch": B, "dtype": "bf16"}))


def step(B):
    torch.manual_seed(0)
    m = deeplab_mod.getNetwork('deeplab_mod', harness=True).cuda().train()
    ts = TrainStep(m, dtype=torch.bfloat16, use_graph=True)
    batch = synthetic_batch(B, 256, 512, labels=19)
    ts.capture(*batch, warmup=2)
    for _ in range(3):
        ts(*batch)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 10
    a.record()
    for _ in range(n):
        loss = ts(*batch)
    b.record()
    b.synchronize()
    print(json.dumps({"step": {"batch": B, "H": 256, "W": 512, "dtype": "bf16", "ms_per_step": round(a.elapsed_time(b) / n, 2),
                               "loss": round(float(loss), 4), "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "step":
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    else:
        kernels()
