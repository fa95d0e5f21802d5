"""Cost of one evaluation step: run on the GPU box,
`python tools/gpu_eval_cost.py --baseline --unfolded --folded [--steps 50] [--models minidsnetExt,psmnet]`.

  --baseline   eager eval forward under torch.no_grad() through the public modules only (what a user had before EvalStep; this
               mode imports nothing newer, so the same file runs on an older checkout)
  --unfolded   EvalStep(fold_bn=False): the same arithmetic, captured as one hipGraph
  --folded     EvalStep(fold_bn=True): BatchNorm folded into the packs, captured

minidsnetExt bf16 B = 8 256x512 and PSMNet(192) bf16 B = 8 256x512.  Every step is timed with a device event pair after a
warm-up; the selected modes alternate in rounds of 10 steps inside one process, so that clock and thermal drift hit them
alike.  Prints one JSON line: ms per step (median, mean) and, for the captured modes, the node inventory of the graph.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, nn as N
from pmt_learning_for_semantic_segmentation_and_disparity_amd.psmnet import PSMNet
from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch

ROUND = 10


def build(name):
    torch.manual_seed(0)
    if name == "minidsnetExt":
        return N.minidsnetExt(N.CFG(), labels=2, patch_type='1dcorr').cuda().eval()
    if name == "psmnet":
        return PSMNet(192).cuda().eval()
    raise SystemExit("unknown model %r" % name)


def runner(mode, name, left, right):
    """(callable running one step, callable returning the node inventory or None)."""
    m = build(name)
    if mode == "baseline":
        a, b = left.bfloat16(), right.bfloat16()

        def step():
            with torch.no_grad():
                return m(a, b)
        return step, lambda: None
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    ev = EvalStep(m, dtype=torch.bfloat16, fold_bn=(mode == "folded"))
    ev.debug_graph = True
    return (lambda: ev(left, right)), (lambda: dict(_lib.graph_node_counts(ev.graph), folded_calls=ev.folded_calls))


def main():
    ap = argparse.ArgumentParser()
    for mode in ("baseline", "unfolded", "folded"):
        ap.add_argument("--" + mode, action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="minidsnetExt,psmnet")
    args = ap.parse_args()
    modes = [k for k in ("baseline", "unfolded", "folded") if getattr(args, k)]
    if not modes:
        raise SystemExit("select at least one of --baseline --unfolded --folded")
    steps = max(50, args.steps)
    res = {}
    for name in args.models.split(","):
        left, right = synthetic_batch(8, 256, 512)[:2]
        run = {k: runner(k, name, left, right) for k in modes}
        for k in modes:
            for _ in range(max(3, args.warmup)):     # builds and captures the step on the way
                run[k][0]()
        torch.cuda.synchronize()
        times = {k: [] for k in modes}
        while len(times[modes[0]]) < steps:
            for k in modes:
                for _ in range(ROUND):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run[k][0]()
                    b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b))
        res[name] = {k: {"ms_median": round(statistics.median(times[k]), 4), "ms_mean": round(statistics.fmean(times[k]), 4),
                         "steps": len(times[k]), "nodes": run[k][1]()} for k in modes}
        del run
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
