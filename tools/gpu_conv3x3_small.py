"""The 3x3 growth convolutions (conv2, 128 -> 32 with norm2 + ReLU on load) of the DenseNet-121 tower: the split-K kernel
of csrc/conv_grow.h against the halo-tile kernel it replaces (SDHIP_CONV_NO_GROW=1).

  python tools/gpu_conv3x3_small.py [reps]

Shapes of the headline step (both towers as one batch of 16 images, two statistics groups, 512x256 input): conv2 of dense
blocks 1 to 4 as it runs there, the output a 32-channel slice of the block's slab (ldy = Ct) with the statistics epilogue:
blocks 2 to 4 in the finalize form (sdhip_conv2d_fwd_bnpro, norm2's statistics in two replicas), block 1 with given
in_scale / in_shift (sdhip_conv2d_fwd).  Next to them the plain launch of the same shape (no prologue: LDS-DMA staging),
which is what the layer would cost without its dependent round trips.
Every block runs in a child process of its own under a time limit; the first failure ends the run.  In a child the
launches are captured as graphs of 20 and replayed in turn `reps` (default 7) times; the table holds the medians in us per
launch and the spread (max - min) of the `reps` values.  A shape that the dispatch does not hand to the new kernel (past
kGrowMaxMap / kGrowMaxWG of conv_grow.h) shows the same kernel twice.
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [("block1", 64, 128, 256, False), ("block2", 32, 64, 512, True), ("block3", 16, 32, 1024, True), ("block4", 8, 16, 1024, True)]
B, G, N, MID, GROWTH = 16, 2, 20, 128, 32
STEP_TIMEOUT = 120


def child(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    dtype = torch.bfloat16
    _, H, W, Ct, bnpro = [b for b in BLOCKS if b[0] == name][0]
    dev = "cuda"
    nrep_in, nrep_out = (2, 2) if bnpro else (ops.NREP, ops.NREP)
    c0 = Ct - GROWTH                                  # the last layer's slice of the slab
    slab = torch.zeros(B, H, W, Ct, dtype=dtype, device=dev)
    y = slab[..., c0:]
    y1 = torch.randn(B, H, W, MID, device=dev).to(dtype)
    w = torch.randn(GROWTH, MID, 3, 3, device=dev) * (2.0 / (MID * 9) ** 0.5)
    wp = ops.packed_weight(w, 'conv', 'fwd', dtype)
    xf = y1.float().reshape(G, -1, MID)
    S2 = (torch.stack([xf.sum(1), (xf * xf).sum(1)], 1).double() / nrep_in).expand(nrep_in, G, 2, MID).contiguous()
    S3 = torch.zeros(nrep_out, G, 2, GROWTH, dtype=torch.float64, device=dev)
    gam, bet = torch.rand(MID, device=dev) + 0.5, torch.rand(MID, device=dev) - 0.5
    rm, rv = torch.zeros(MID, device=dev), torch.ones(MID, device=dev)
    outs = [torch.empty(G, MID, device=dev) for _ in range(4)]
    count = float(B // G * H * W)
    mu = S2.sum(0)[:, 0] / count
    inv = 1.0 / torch.sqrt(S2.sum(0)[:, 1] / count - mu * mu + 1e-5)
    sc, sh = (gam * inv).float().contiguous(), (bet - mu * gam * inv).float().contiguous()

    def pro():
        if bnpro:
            call("sdhip_conv2d_fwd_bnpro", ptr(y1), ptr(wp), ptr(y), ptr(S3), GROWTH, nrep_out, ptr(S2), MID, nrep_in,
                 None, 0, 0, 0, 0, ptr(gam), ptr(bet), ptr(rm), ptr(rv), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                 count, 1e-5, 0.1, B, H, W, MID, MID, H, W, GROWTH, Ct, 3, 3, 1, 1, G, _lib.BF16, stream_ptr())
        else:
            call("sdhip_conv2d_fwd", ptr(y1), ptr(wp), ptr(y), None, ptr(sc), ptr(sh), ptr(S3), GROWTH, nrep_out,
                 B, H, W, MID, MID, H, W, GROWTH, Ct, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, G, 0, 0, _lib.BF16, stream_ptr())

    def plain():
        call("sdhip_conv2d_fwd", ptr(y1), ptr(wp), ptr(y), None, None, None, ptr(S3), GROWTH, nrep_out,
             B, H, W, MID, MID, H, W, GROWTH, Ct, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, G, 0, 0, _lib.BF16, stream_ptr())

    def switch(old):
        if old:
            os.environ["SDHIP_CONV_NO_GROW"] = "1"
        else:
            os.environ.pop("SDHIP_CONV_NO_GROW", None)
        _lib.reload_diag()

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
        out = y.float().clone()
        switch(False)
        return g, out

    def time_us(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N

    graphs = [graph_of(pro, True), graph_of(pro, False), graph_of(plain, True)]
    t = [[] for _ in graphs]
    for _ in range(reps):
        for i, (g, _) in enumerate(graphs):
            t[i].append(time_us(g))
    med = [statistics.median(v) for v in t]
    spr = [max(v) - min(v) for v in t]
    diff = (graphs[0][1] - graphs[1][1]).abs().max().item()
    print("%s %dx%d conv2 3x3 %d -> %d (%s): old %6.2f us (spread %.2f)  new %6.2f us (spread %.2f)  plain LDS-DMA %6.2f us (spread %.2f)  maxdiff %.3g" % (
        name, H, W, MID, GROWTH, "finalize form" if bnpro else "given prologue", med[0], spr[0], med[1], spr[1], med[2], spr[2], diff), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    for name, *_ in BLOCKS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(reps)], timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, STEP_TIMEOUT), flush=True)
            return 1
        if r.returncode:
            print("%s: exit status %d; stopping" % (name, r.returncode), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(main())
