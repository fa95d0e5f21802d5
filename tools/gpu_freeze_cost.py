"""Cost of a training step with frozen BatchNorm ("Frozen BatchNorm in the training step"): run on the GPU box,
`python tools/gpu_freeze_cost.py [--steps 50] [--models minidsnetExt,cfg5]`, or `--baseline` on a checkout of the parent commit.

  unfrozen   TrainStep(model): the step as it was (the only mode of --baseline, which passes no keyword the parent lacks, so the
             same file runs there)
  tables     TrainStep(model, freeze_bn=True, fold_bn=False): running statistics, scale / shift from the step's tables, no
             BatchNorm reductions, finalizes or statistics
  folded     TrainStep(model, freeze_bn=True): the norms of the skip-free conv + BatchNorm layers folded into the packs

minidsnetExt bf16 B = 8 256x512 and BASELINE config 5 (aspp 2, HANet, 19 classes) bf16 B = 4 512x1024, built and fed as bench.py
does.  Every captured step is timed with a device event pair after a warm-up; the modes alternate in rounds of 10 steps inside
one process, so that clock and thermal drift hit them alike.  Prints one JSON line: ms per step (median, mean) and the node
inventory of each graph.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, nn as N, ops
from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch

ROUND = 10
MODES = {"unfrozen": {}, "tables": dict(freeze_bn=True, fold_bn=False), "folded": dict(freeze_bn=True)}
SHAPES = {"minidsnetExt": (8, 256, 512, 2), "cfg5": (4, 512, 1024, 19)}


def build(name):
    torch.manual_seed(0)
    if name == "minidsnetExt":
        return N.minidsnetExt(N.CFG(dropout=0.0, aspp=0, use_att=1), labels=2, pretrained=False, patch_type='1dcorr',
                              backbone='densenet').cuda().train(), None
    if name == "cfg5":
        m = N.minidsnetExt(N.CFG(dropout=0.0, aspp=2, use_att=1, hanet=1), labels=19, pretrained=False, patch_type='1dcorr',
                           backbone='densenet').cuda().train()
        return m, (lambda outs, seg, disp: ops.train_loss(outs[0], outs[1], outs[2], seg, disp, True, True, True))
    raise SystemExit("unknown model %r" % name)


def runner(mode, name, batch):
    model, loss_fn = build(name)
    ts = TrainStep(model, dtype=torch.bfloat16, use_graph=True, loss_fn=loss_fn, **MODES[mode])
    ts.debug_graph = True
    return ts, (lambda: ts(*batch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true", help="the unfrozen step alone (runs on the parent commit too)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="minidsnetExt,cfg5")
    args = ap.parse_args()
    modes = ["unfrozen"] if args.baseline else list(MODES)
    steps = max(50, args.steps)
    res = {}
    for name in args.models.split(","):
        B, H, W, labels = SHAPES[name]
        batch = synthetic_batch(B, H, W, labels=labels)
        run = {k: runner(k, name, batch) for k in modes}
        for k in modes:
            for _ in range(max(3, args.warmup)):     # measuring pass, warm-up and capture happen on the way
                run[k][1]()
        torch.cuda.synchronize()
        times = {k: [] for k in modes}
        while len(times[modes[0]]) < steps:
            for k in modes:
                for _ in range(ROUND):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run[k][1]()
                    b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b))
        res[name] = {}
        for k in modes:
            ts = run[k][0]
            fold = getattr(ts.ctx, "fold", None)
            res[name][k] = {"ms_median": round(statistics.median(times[k]), 4), "ms_mean": round(statistics.fmean(times[k]), 4),
                            "ms_min": round(min(times[k]), 4), "steps": len(times[k]), "nodes": _lib.graph_node_counts(ts.graph),
                            "folded_layers": len(fold.layers) if fold is not None else 0,
                            "table_norms": len(fold.tables) if fold is not None else 0}
        ops.set_step_context(None)
        del run
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
