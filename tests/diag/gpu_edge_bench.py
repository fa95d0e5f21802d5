"""Timings of the three operators of the Ext_small edge networks (csrc/edge.hip) on one GPU, in one process, alternating rounds
(medians printed as one JSON line), in bf16 at B=8 256x512 and B=4 512x1024:
  * grad_mag   ops.grad_mag of a planar 3-channel bf16 image against the same formula composed from ATen (two padded
               differences, squares, sqrt, the channels-last copy a conv node would need);
  * edge_loss  ops.edge_loss + backward on a one-channel bf16 logit map against F.binary_cross_entropy_with_logits with the
               balancing weight built by ATen (two counts, two masked fills) + backward;
  * gate_pair  ops.gate_pair + backward at 64 channels on the 1/4-resolution map against torch.cat((a * g, b * (1 - g)), 1) +
               backward in channels-last memory;
  each with the bytes the operator must move and the GB/s of the kernel time against them; and, with --steps, the captured
  training step of Ext_small (EdgeStepLoss) and Ext_smallv0 beside minidsnetExt at B=8 256x512 bf16.

Usage:  python tests/diag/gpu_edge_bench.py [--rounds 5] [--steps 20]"""
import argparse
import json
import os
import sys

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


def _rounds(fns, iters, rounds):
    for f in fns.values():
        _time(f, 5)
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            res[k].append(_time(f, iters[k]))
    r = {k: _median(v) for k, v in res.items()}
    r["spread"] = {k: [min(v), max(v)] for k, v in res.items()}
    return r


def aten_grad_mag(img):
    P = F.pad(img.float(), (1, 1, 1, 1))
    ox = 0.5 * (P[:, :, 1:-1, 2:] - P[:, :, 1:-1, :-2])
    oy = 0.5 * (P[:, :, 2:, 1:-1] - P[:, :, :-2, 1:-1])
    return torch.sqrt(ox * ox + oy * oy + 1e-6).to(img.dtype).contiguous(memory_format=torch.channels_last)


def aten_edge_loss(z, t):
    pos, neg = (t == 1).sum(), (t == 0).sum()
    w = torch.zeros_like(t)
    w[t == 1] = (neg * 1.0 / (pos + neg)).float()
    w[t == 0] = (pos * 1.0 / (pos + neg)).float()
    return F.binary_cross_entropy_with_logits(z.float(), t, w)


def kernels(rounds):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, dtype_code, ptr, stream_ptr
    out = {}
    for B, H, W in ((8, 256, 512), (4, 512, 1024)):
        g = torch.Generator(device="cuda").manual_seed(3)
        img = torch.rand(B, 3, H, W, device="cuda", generator=g).bfloat16()
        z = (torch.randn(B, 1, H, W, device="cuda", generator=g) * 3).bfloat16().requires_grad_(True)
        t = (torch.rand(B, 1, H, W, device="cuda", generator=g) > 0.9).float()
        h, w, C = H // 4, W // 4, 64
        a, b = [torch.randn(B, h, w, C, device="cuda", generator=g).bfloat16().permute(0, 3, 1, 2).requires_grad_(True) for _ in range(2)]
        gate = torch.rand(B, h, w, 1, device="cuda", generator=g).bfloat16().permute(0, 3, 1, 2).requires_grad_(True)
        gy = torch.randn(B, h, w, 2 * C, device="cuda", generator=g).bfloat16().permute(0, 3, 1, 2)
        n = B * H * W
        ws = torch.empty(_lib.edge_bce_workspace_bytes(n) // 8, dtype=torch.float64, device="cuda")
        gz, loss = torch.empty_like(z), torch.zeros(1, dtype=torch.float64, device="cuda")
        y, ga, gb = torch.empty(B, h, w, 2 * C, device="cuda", dtype=torch.bfloat16), torch.empty_like(a), torch.empty_like(b)
        gg = torch.empty_like(gate)
        np_ = B * h * w

        def bce_entry():
            call("sdhip_edge_bce", ptr(z), 1, dtype_code(z), ptr(t), ptr(gz), ptr(loss), n, ptr(ws), ws.numel() * 8, stream_ptr())

        def gate_entry():
            call("sdhip_gate_pair_fwd", ptr(a), C, ptr(b), C, ptr(gate), 1, ptr(y), 2 * C, np_, C, dtype_code(a), stream_ptr())
            call("sdhip_gate_pair_bwd", ptr(gy), 2 * C, ptr(a), C, ptr(b), C, ptr(gate), 1, ptr(ga), C, ptr(gb), C, ptr(gg), 1, np_, C,
                 dtype_code(a), stream_ptr())

        def clear():
            z.grad = a.grad = b.grad = gate.grad = None

        def edge_fused():
            clear()
            ops.edge_loss(z, t).backward()

        def edge_aten():
            clear()
            aten_edge_loss(z, t).backward()

        def gate_fused():
            clear()
            ops.gate_pair(a, b, gate).backward(gy)

        def gate_aten():
            clear()
            torch.cat((a * gate, b * (1 - gate)), 1).backward(gy)

        fns = {"grad_mag_us": lambda: ops.grad_mag(img), "grad_mag_aten_us": lambda: aten_grad_mag(img),
               "edge_entry_us": bce_entry, "edge_fused_us": edge_fused, "edge_aten_us": edge_aten,
               "gate_entry_us": gate_entry, "gate_fused_us": gate_fused, "gate_aten_us": gate_aten}
        iters = {k: (40 if "aten" in k else 200) for k in fns}
        r = _rounds(fns, iters, rounds)
        # same answers first: against ATen in f32 on the same bf16 inputs
        r["grad_mag_maxdiff"] = float((ops.grad_mag(img).float() - aten_grad_mag(img).float()).abs().max())
        r["edge_value"], r["edge_value_aten"] = float(ops.edge_loss(z.detach(), t)), float(aten_edge_loss(z.detach(), t))
        nb = {"grad_mag": n * (3 * 2 + 8 * 2), "edge_entry": n * (4 + 4 + 2 + 2), "gate_entry": np_ * 2 * (2 * C + 1 + 2 * C) + np_ * 2 * (4 * C + 1 + 2 * C + 1)}
        for k, v in nb.items():
            r[k + "_MB"] = v / 1e6
            r[k + "_GBps"] = v / r[k + "_us"] / 1e3
        out["B%d_%dx%d" % (B, H, W)] = r
    return out


def steps(n):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ext_small, nn as N, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import EdgeStepLoss, TrainStep, synthetic_batch
    batch = synthetic_batch(8, 256, 512)
    edges = (torch.rand(8, 1, 32, 64, device="cuda") < 0.15).float().repeat_interleave(8, 2).repeat_interleave(8, 3).contiguous()
    ts = {}
    for name, cls in (("minidsnetExt", N.minidsnetExt), ("Ext_smallv0", ext_small.Ext_smallv0), ("Ext_small", ext_small.Ext_small)):
        torch.manual_seed(0)
        m = cls(N.CFG(), labels=2, patch_type='1dcorr').cuda().train()
        fn = EdgeStepLoss(m).set_edges(edges) if name == "Ext_small" else None
        t = TrainStep(m, dtype=torch.bfloat16, use_graph=True, use_lovasz=False, loss_fn=fn)
        t(*batch)
        ops.set_step_context(None)
        ts[name] = t
    res = {k: [] for k in ts}
    for _ in range(5):
        for k, t in ts.items():
            res[k].append(_time(lambda: t(*batch), n) / 1000.0)
    return {k + "_ms": _median(v) for k, v in res.items()} | {"spread_ms": {k: [min(v), max(v)] for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    out = kernels(a.rounds)
    if a.steps:
        out["step_B8_256x512_bf16"] = steps(a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
