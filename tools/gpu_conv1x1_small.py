"""The 1x1 bottleneck convolutions (conv1) of the DenseNet-121 tower on its small maps: the pointwise split-K kernel of
csrc/conv_point.h against the halo-tile kernel it replaces (SDHIP_CONV_NO_POINT=1).

  python tools/gpu_conv1x1_small.py [reps]

Shapes of the headline step (both towers as one batch of 16 images, two statistics groups, 512x256 input): every conv1 of
dense blocks 2, 3 and 4 as it runs there (sdhip_conv2d_fwd_bnpro on the prefix of the block's slab, the previous layer's
statistics pending in two replicas, output statistics in two replicas), transitions 2 and 3 (sdhip_conv2d_fwd with
in_scale / in_shift) and, as the yardstick, the 3x3 conv2 of each block (same finalize, epilogue and atomics, two chunks).
Per layer both kernels are captured as graphs of 20 launches in ONE process and replayed in turn `reps` (default 7) times;
the table holds the medians in us per launch against Cin, the block totals and a least-squares line us = base + slope *
(Cin / 64) per block and kernel.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops  # noqa: E402
from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr  # noqa: E402

dtype = torch.bfloat16
B, G, N = 16, 2, 20
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def switch(old):
    if old:
        os.environ["SDHIP_CONV_NO_POINT"] = "1"
    else:
        os.environ.pop("SDHIP_CONV_NO_POINT", None)
    _lib.reload_diag()


def bnpro_layer(slab, Ct, H, W, Cin, Cout, k, first):
    """One conv (k x k, Cin -> Cout) with the BatchNorm finalize inside, as _DenseBlockFn launches it."""
    dev = slab.device
    w = torch.randn(Cout, Cin, k, k, device=dev) * (2.0 / (Cin * k * k) ** 0.5)
    wp = ops.packed_weight(w, 'conv', 'fwd', dtype)
    y = torch.empty(B, H, W, Cout, dtype=dtype, device=dev)
    x = slab.float()[..., :Cin].reshape(G, -1, Cin)
    S = torch.stack([x.sum(1), (x * x).sum(1)], 1).double().reshape(1, G, 2, Cin).contiguous()
    pend = None if first else (S[0, :, :, Cin - 32:] / 2).expand(2, G, 2, 32).contiguous()
    S2 = torch.zeros(2, G, 2, Cout, dtype=torch.float64, device=dev)
    gam, bet, rm, rv = torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev)
    outs = [torch.empty(G, Cin, device=dev) for _ in range(4)]
    keep = (w, wp, y, S, pend, S2, gam, bet, rm, rv, outs)

    def go():
        call("sdhip_conv2d_fwd_bnpro", ptr(slab), ptr(wp), ptr(y), ptr(S2), Cout, 2, ptr(S), Cin, 1,
             ptr(pend), 32 if pend is not None else 0, 2 if pend is not None else 0, Cin - 32 if pend is not None else 0, 32 if pend is not None else 0,
             ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
             float(B // G * H * W), 1e-5, 0.1, B, H, W, Cin, Ct, H, W, Cout, Cout, k, k, k // 2, k // 2, G, _lib.BF16, stream_ptr())
    return go, y, keep


def scale_layer(slab, Ct, H, W, Cin, Cout):
    """A transition: given in_scale / in_shift, statistics of the output in NREP replicas."""
    dev = slab.device
    w = torch.randn(Cout, Cin, 1, 1, device=dev) * (2.0 / Cin ** 0.5)
    wp = ops.packed_weight(w, 'conv', 'fwd', dtype)
    y = torch.empty(B, H, W, Cout, dtype=dtype, device=dev)
    st = torch.zeros(ops.NREP, G, 2, Cout, dtype=torch.float64, device=dev)
    sc, sh = torch.rand(G, Cin, device=dev) + 0.5, torch.rand(G, Cin, device=dev) - 0.5

    def go():
        ops._conv_launch(slab.permute(0, 3, 1, 2)[:, :Cin], Ct, wp, y, Cout, None, sc, sh, st, B, H, W, Cin, H, W, Cout, 1, 1, 1, 1, 0, 0, True, G, 0, False, ops.NREP)
    return go, y, (w, wp, st, sc, sh)


def graph_of(go, old):
    switch(old)
    for _ in range(2):
        go()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(N):
            go()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / N


def ab(go, y):
    """-> (old us, new us, max |difference| of the outputs); one kernel only (no switch to flip) -> the same time twice."""
    graphs, ys = [], []
    for old in (True, False):
        graphs.append(graph_of(go, old))
        ys.append(y.float().clone())
    switch(False)
    t = ([], [])
    for _ in range(REPS):
        for i in (0, 1):
            t[i].append(time_us(graphs[i]))
    return statistics.median(t[0]), statistics.median(t[1]), (ys[0] - ys[1]).abs().max().item()


def fit(xs, ys):
    n, mx, my = len(xs), sum(xs) / len(xs), sum(ys) / len(ys)
    sxx = sum((x - mx) ** 2 for x in xs)
    slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sxx if sxx else 0.0
    return my - slope * mx, slope


def main():
    towers = [("block2", 32, 64, 512, [128 + 32 * i for i in range(12)]), ("block3", 16, 32, 1024, [256 + 32 * i for i in range(24)]),
              ("block4", 8, 16, 1024, [512 + 32 * i for i in range(16)])]
    for name, H, W, Ct, cins in towers:
        slab = torch.randn(B, H, W, Ct, device="cuda").to(dtype)
        rows = []
        for i, Cin in enumerate(cins):
            go, y, keep = bnpro_layer(slab, Ct, H, W, Cin, 128, 1, i == 0)
            o, n, diff = ab(go, y)
            rows.append((Cin, o, n))
            print("%s %dx%d conv1 %4d -> 128: old %6.2f us  new %6.2f us  maxdiff %.3g" % (name, H, W, Cin, o, n, diff), flush=True)
        go, y, keep = bnpro_layer(torch.randn(B, H, W, 128, device="cuda").to(dtype), 128, H, W, 128, 32, 3, True)
        o, n, _ = ab(go, y)
        print("%s %dx%d conv2 3x3 128 -> 32 (yardstick): %6.2f us" % (name, H, W, min(o, n)), flush=True)
        ch = [r[0] / 64.0 for r in rows]
        (bo, so), (bn_, sn) = fit(ch, [r[1] for r in rows]), fit(ch, [r[2] for r in rows])
        print("%s total: old %7.1f us  new %7.1f us | us = base + slope * chunks: old %.2f + %.3f  new %.2f + %.3f" % (
            name, sum(r[1] for r in rows), sum(r[2] for r in rows), bo, so, bn_, sn), flush=True)
    for name, H, W, Ct, Cout in (("transition2", 32, 64, 512, 256), ("transition3", 16, 32, 1024, 512)):
        slab = torch.randn(B, H, W, Ct, device="cuda").to(dtype)
        go, y, keep = scale_layer(slab, Ct, H, W, Ct, Cout)
        o, n, diff = ab(go, y)
        print("%s %dx%d %4d -> %3d: old %6.2f us  new %6.2f us  maxdiff %.3g" % (name, H, W, Ct, Cout, o, n, diff), flush=True)


if __name__ == "__main__":
    main()
