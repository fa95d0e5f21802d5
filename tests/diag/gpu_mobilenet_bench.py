"""MobileNetV3 backbone timings on one GPU, in one process, alternating rounds (medians printed as one JSON line):
the captured bf16 training step of minidsnetExt(backbone='mobilenet') against the DenseNet step at B=8 256x512, and the
kernel-node count of each captured step (sdhip_graph_node_counts).

Usage:  python tests/diag/gpu_mobilenet_bench.py [--rounds 5]"""
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
    return s.elapsed_time(e) / iters      # ms


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, ops, _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(8, 256, 512)
    ts, nodes = {}, {}
    for name in ("densenet", "mobilenet"):
        torch.manual_seed(0)
        m = N.minidsnetExt(N.CFG(), labels=2, patch_type='1dcorr', backbone=name).cuda().train()
        t = TrainStep(m, dtype=torch.bfloat16, use_graph=True)
        t.debug_graph = True
        t(*batch)                               # warm-up + capture
        nodes[name] = _lib.graph_node_counts(t.graph)
        ts[name] = t
        ops.set_step_context(None)
    res = {k: [] for k in ts}
    for _ in range(a.rounds):
        for k, t in ts.items():
            res[k].append(_time(lambda: t(*batch), 10))
    out = {"%s_step_ms" % k: _median(v) for k, v in res.items()}
    out["ratio"] = out["mobilenet_step_ms"] / out["densenet_step_ms"]
    out.update({"%s_nodes" % k: v for k, v in nodes.items()})
    print(json.dumps({"steps_B8_256x512_bf16": out}))


if __name__ == "__main__":
    main()
