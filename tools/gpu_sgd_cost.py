"""Cost of the fused SGD launch beside the fused Adam launch ("SGD with momentum"): run on the GPU box,
`python tools/gpu_sgd_cost.py`.

On the flat parameter buffer of minidsnetExt and of warp.minidsnetDivide: sdhip_adam_step, sdhip_sgd_step with a NULL table
and - on the warp network, whose loss leaves parameters unreached - sdhip_sgd_step with that network's live table.  Median of
20 launches after warm-up, one event pair per launch, one process.  Prints one JSON line.
"""
import json
import statistics
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, ops, warp
from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch


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


def measure(n, live):
    p = torch.randn(n, device="cuda") * 0.05
    g = torch.randn(n, device="cuda") * 1e-3
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    bp = torch.ones(2, device="cuda")
    lr = torch.full((1,), 0.005, device="cuda")
    adam = lambda: call("sdhip_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(bp), n, 0.0015, 0.9, 0.999, 1e-7, 0.0, 1.0, stream_ptr())
    sgd = lambda t: (lambda: call("sdhip_sgd_step", ptr(p), ptr(g), ptr(buf), ptr(lr), n, 0.9, 1e-4, 1.0, ptr(t),
                                  0 if t is None else t.shape[0], stream_ptr()))
    out = {"elements": n, "adam_us": median_us(adam), "sgd_null_us": median_us(sgd(None))}
    if live is not None:
        out["live_rows"] = live.shape[0]
        out["live_elements"] = int((live[:, 1] - live[:, 0]).sum())
        out["sgd_live_us"] = median_us(sgd(live))
    return {k: (round(x, 2) if isinstance(x, float) else x) for k, x in out.items()}


def main():
    torch.manual_seed(0)
    res = {}
    m = N.minidsnetExt(N.CFG(), labels=2, patch_type='1dcorr').cuda().train()
    res["minidsnetExt"] = measure(TrainStep(m, dtype=torch.float32, use_graph=False).flat_p.numel(), None)
    # the warp network's table is found by its first step (the parameters its loss does not reach)
    ts = TrainStep(warp.minidsnetDivide(N.CFG(), labels=2, patch_type='1dcorr').cuda().train(), dtype=torch.float32, use_graph=False,
                   optimizer="sgd")
    ts(*synthetic_batch(2, 256, 256))
    ops.set_step_context(None)
    res["minidsnetDivide"] = measure(ts.flat_p.numel(), ts.live)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
