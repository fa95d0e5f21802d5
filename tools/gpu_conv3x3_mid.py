"""The 3x3 64 -> 64 convolutions of the decoder blocks on the mid-size maps (Conv2DownUp6 / 7 / 9 / 10 at 1/4 resolution,
Conv2DownUp4 / 8 at 1/8): the whole-weight-set kernel of csrc/conv_mid.h against the halo-tile kernel it replaces
(SDHIP_CONV_NO_MID=1), and that kernel with the 8x32 tile (SDHIP_CONV_BIG=1: a quarter of the weight copies).

  python tools/gpu_conv3x3_mid.py [reps]

Shapes of the headline step (bf16, 8 images, one statistics group, 3x3 / pad 1): 64 -> 64 at 64x128 and at 32x64 in the
four forms the step and its tests launch — forward with the statistics epilogue, the data gradient through
sdhip_conv2d_fwd_bnbwd mode 0 without and with an addend, the plain launch — and the 128 -> 64 `c1` layers at 64x128,
forward only.
Every shape runs in a child process of its own under a time limit; the first failure ends the run.  In a child the
launches are captured as graphs of 20 and replayed in turn `reps` (default 7) times; the table holds the medians in us per
launch and the spread (max - min) of the `reps` values.  A shape that the dispatch does not hand to the new kernel (outside
kMidMinMap .. kMidMaxMap / kMidMaxWG of conv_mid.h, or a library without the kernel) shows the same kernel as `old` and `new`;
the last column is the new kernel with the limits lifted (SDHIP_TUNE_MID_MIN_MAP=1), which is how a shape outside them is
measured before it is let in or kept out.
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("quarter", 64, 128, 64, True), ("eighth", 32, 64, 64, True), ("c1", 64, 128, 128, False)]   # name, H, W, Cin, with the backward forms
B, G, N, COUT = 8, 1, 20, 64
STEP_TIMEOUT = 120
SWITCHES = ("SDHIP_CONV_NO_MID", "SDHIP_CONV_BIG", "SDHIP_TUNE_MID_MIN_MAP")


def child(name, reps):
    sys.path.insert(0, ROOT)
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    dtype = torch.bfloat16
    _, H, W, Cin, backward = [s for s in SHAPES if s[0] == name][0]
    dev = "cuda"
    nrep = ops.NREP
    x = torch.randn(B, H, W, Cin, device=dev).to(dtype)
    y = torch.zeros(B, H, W, COUT, dtype=dtype, device=dev)
    u = torch.randn(B, H, W, COUT, device=dev).to(dtype)
    add = torch.randn(B, H, W, COUT, device=dev).to(dtype)
    w = torch.randn(COUT, Cin, 3, 3, device=dev) * (2.0 / (Cin * 9) ** 0.5)
    wp = ops.packed_weight(w, 'conv', 'fwd', dtype)
    S = torch.zeros(nrep, G, 2, COUT, dtype=torch.float64, device=dev)
    sc, sh = (torch.rand(G, COUT, device=dev) + 0.5).contiguous(), (torch.randn(G, COUT, device=dev) * 0.3).contiguous()

    def fwd(stats):
        call("sdhip_conv2d_fwd", ptr(x), ptr(wp), ptr(y), None, None, None, ptr(S) if stats else None, COUT, nrep,
             B, H, W, Cin, Cin, H, W, COUT, COUT, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, G, 0, 0, _lib.BF16, stream_ptr())

    def dgrad(addend):
        call("sdhip_conv2d_fwd_bnbwd", ptr(x), ptr(wp), ptr(y), ptr(S), COUT, nrep, ptr(u), COUT, ptr(sc), ptr(sh),
             ptr(add) if addend else None, COUT if addend else 0,
             B, H, W, Cin, Cin, H, W, COUT, COUT, 3, 3, 1, 1, 1, G, 0, _lib.BF16, stream_ptr())

    forms = [("forward + statistics", lambda: fwd(True))]
    if backward:
        forms += [("data gradient (bnbwd mode 0)", lambda: dgrad(False)), ("data gradient + addend", lambda: dgrad(True)), ("plain", lambda: fwd(False))]

    def switch(on):
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k in on:
            os.environ[k] = "1"
        _lib.reload_diag()

    def graph_of(go, on):
        switch(on)
        for _ in range(2):
            go()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(N):
                go()
        g.replay()
        torch.cuda.synchronize()
        out = y.clone()
        switch(())
        return g, out

    def time_us(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N

    for label, go in forms:
        graphs = [graph_of(go, ("SDHIP_CONV_NO_MID",)), graph_of(go, ("SDHIP_CONV_NO_MID", "SDHIP_CONV_BIG")), graph_of(go, ()),
                  graph_of(go, ("SDHIP_TUNE_MID_MIN_MAP",))]
        t = [[] for _ in graphs]
        for _ in range(reps):
            for i, (g, _) in enumerate(graphs):
                t[i].append(time_us(g))
        med = [statistics.median(v) for v in t]
        spr = [max(v) - min(v) for v in t]
        same = torch.equal(graphs[0][1], graphs[2][1]) and torch.equal(graphs[0][1], graphs[3][1])
        print("%-8s %3dx%-3d %3d -> %d %-30s old %6.2f us (spread %.2f)  old 8x32 %6.2f us (spread %.2f)  new %6.2f us (spread %.2f)  "
              "new, limits lifted %6.2f us (spread %.2f)  y bits %s" % (
                  name, H, W, Cin, COUT, label, med[0], spr[0], med[1], spr[1], med[2], spr[2], med[3], spr[3], "equal" if same else "DIFFER"), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    for name, *_ in SHAPES:
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
