"""The persistent whole-CU convolution with the BatchNorm-backward sums in its epilogue (conv_band_bx_kernel of
csrc/conv_band.h, entry point sdhip_conv2d_fwd_bnbwd mode 0) at the full-resolution shapes of the headline step, against
the route it replaces: the data gradient on the plain kernel, then the reductions-only sdhip_affine_act_bwd pass.

  python tools/gpu_band_bx.py OTHER_TREE [reps [TABLE.json]]   # the A/B: prints a table (and writes it as JSON if asked)
  python tools/gpu_band_bx.py --child TREE OUT.json            # one measurement of one build (what the A/B starts, in turn)

One process per build (the package, and with it libsdhip.so, is imported from the tree given), the two builds alternating
`reps` (default 7) times; per case a graph of 20 launches is replayed, the table holds the medians over the processes in us
per launch and the spread (max - min).  Per shape (8 images of 256 x 512; 5x5 64 -> 64 and 3x3 32 -> 32; with and without
an addend) each build times
  dgrad   the data gradient alone (sdhip_conv2d_fwd / _add: the plain persistent kernel)
  pass    the reductions-only sdhip_affine_act_bwd pass alone
  fused   sdhip_conv2d_fwd_bnbwd — on OTHER_TREE (the parent) the halo-tile kernel takes it, on this tree the persistent one
A form is a gain if this tree's `fused` median is below the parent's dgrad + pass by more than the sum of the spreads."""
import json
import os
import statistics
import subprocess
import sys
import tempfile

N = 20
# name, images, H, W, k, channels
SHAPES = [("5x5 64->64", 8, 256, 512, 5, 64), ("3x3 32->32", 8, 256, 512, 3, 32)]


def child(tree, out_path):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    dt, BF, dev, NREP = torch.bfloat16, _lib.BF16, "cuda", ops.NREP
    res = {}

    def timed(go):
        go()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(N):
                go()
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / N)
        return min(ts)

    for name, B, H, W, k, C in SHAPES:
        gen = torch.Generator().manual_seed(1000 * k + C)
        npix, pad = B * H * W, k // 2
        x = torch.randn(npix, C, generator=gen).to(dev).to(dt)
        u = (torch.randn(npix, C, generator=gen) * 1.3).to(dev).to(dt)
        a = torch.randn(npix, C, generator=gen).to(dev).to(dt)
        w = (torch.randn(C, C, k, k, generator=gen) * 0.1).to(dev)
        sc = (torch.rand(1, C, generator=gen) + 0.5).to(dev)
        sh = (torch.randn(1, C, generator=gen) * 0.3).to(dev)
        wd = ops.packed_weight(w, 'conv', 'dgrad', dt)
        y = torch.empty(npix, C, device=dev, dtype=dt)
        sums = torch.zeros(NREP, 1, 2, C, dtype=torch.float64, device=dev)
        both = torch.zeros(2, NREP, 1, C, dtype=torch.float32, device=dev)

        def dgrad():
            ops._conv_launch(x, C, wd, y, C, None, None, None, None, B, H, W, C, H, W, C, k, k, 1, 1, pad, pad, False, 1, 0, False)

        def dgrad_add():
            call("sdhip_conv2d_fwd_add", ptr(x), ptr(wd), ptr(y), ptr(a), C, B, H, W, C, C, H, W, C, C, k, k, pad, pad, BF, stream_ptr())

        def red_pass():
            call("sdhip_affine_act_bwd", ptr(y), C, ptr(u), C, None, 0, ptr(sc), ptr(sh), ptr(both[0]), ptr(both[1]), NREP,
                 npix, C, 1, 1, 0, 0, BF, stream_ptr())

        def fused(addend):
            def go():
                call("sdhip_conv2d_fwd_bnbwd", ptr(x), ptr(wd), ptr(y), ptr(sums), C, NREP, ptr(u), C, ptr(sc), ptr(sh),
                     ptr(addend), (C if addend is not None else 0), B, H, W, C, C, H, W, C, C, k, k, 1, pad, pad, 1, 0, BF, stream_ptr())
            return go

        res[name + " dgrad"] = timed(dgrad)
        res[name + " pass"] = timed(red_pass)
        res[name + " fused"] = timed(fused(None))
        res[name + " +addend dgrad"] = timed(dgrad_add)
        res[name + " +addend fused"] = timed(fused(a))
        del x, u, a, y
    with open(out_path, "w") as f:
        json.dump(res, f)


def main(argv):
    if argv and argv[0] == "--child":
        return child(argv[1], argv[2])
    if not argv:
        sys.exit(__doc__)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    other, reps = argv[0], int(argv[1]) if len(argv) > 1 else 7
    table_path = argv[2] if len(argv) > 2 else None
    runs = {"other": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(reps):
            for who, tree in (("other", other), ("this", here)):
                out = os.path.join(tmp, "band_bx_%s_%d.json" % (who, r))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, out], check=True, timeout=300)   # the first failure ends the run
                with open(out) as f:
                    runs[who].append(json.load(f))

    def stat(who, key):
        ts = [r[key] for r in runs[who]]
        return statistics.median(ts), max(ts) - min(ts)

    table = {}
    print("%-28s %9s %7s %9s %7s" % ("launch", "other us", "spread", "this us", "spread"))
    for key in runs["this"][0]:
        (a, sa), (b, sb) = stat("other", key), stat("this", key)
        table[key] = {"other_us": a, "other_spread": sa, "this_us": b, "this_spread": sb}
        print("%-28s %9.2f %7.2f %9.2f %7.2f" % (key, a, sa, b, sb), flush=True)
    print("%-28s %9s %7s %9s %7s  %s" % ("form", "two us", "spread", "fused us", "spread", "verdict"))
    for name, *_ in SHAPES:
        for add in ("", " +addend"):
            (d, sd), (p, sp), (f, sf) = stat("other", name + add + " dgrad"), stat("other", name + " pass"), stat("this", name + add + " fused")
            two, s2 = d + p, sd + sp
            verdict = "gain" if f < two - (s2 + sf) else ("SLOWER" if f > two + (s2 + sf) else "even")
            table[name + add] = {"parent_two_launch_us": two, "parent_spread": s2, "fused_us": f, "fused_spread": sf, "verdict": verdict}
            print("%-28s %9.2f %7.2f %9.2f %7.2f  %s" % (name + add, two, s2, f, sf, verdict), flush=True)
    if table_path:
        with open(table_path, "w") as f:
            json.dump(table, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
