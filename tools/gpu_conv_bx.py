"""The halo-tile convolution with the BatchNorm-backward epilogue (conv_fast_kernel<.., DMA, BX> of csrc/conv_fast.h, entry
point sdhip_conv2d_fwd_bnbwd), launch by launch at the shapes the headline step calls it with: this tree against another
checkout of the repository (the parent commit, built).

  python tools/gpu_conv_bx.py OTHER_TREE [reps [TABLE.json]]   # the A/B: prints a table (and writes it as JSON if asked)
  python tools/gpu_conv_bx.py --child TREE OUT.json            # one measurement of one build (what the A/B starts, in turn)

One process per build (the package, and with it libsdhip.so, is imported from the tree given), the two builds alternating
`reps` (default 7) times; per case a graph of 20 launches is replayed, the table holds the medians over the processes in us
per launch and the spread (max - min) of each build.  A case is a gain if this build's median is below the other's by more
than the sum of the two spreads.

Cases (data-gradient form: x = the gradient that comes in, y = the gradient that goes out, u = the BatchNorm input):
  dense 3x3   the conv2 data gradient of DenseNet blocks 1 - 4, 32 -> 128, 16 images in two statistics groups, mode 0
  dense 1x1   the conv1 data gradient of blocks 2 - 4 in mode 1 (mask, scale, add into the slab gradient in place), 128 -> C
              at the narrowest and the widest slab of the block
  decoder     the BNSlot data gradients of Conv2DownUp3 / 4 / 8 on the 1/8-resolution map (32 x 64, 8 images), mode 0, with
              and without the parked skip gradient as addend
  (record)    two launches the step does NOT fuse, each next to its two-launch form (convolution, then sdhip_affine_act_bwd):
              block 1's 1x1 in mode 1 (above the 32768-pixel switch of densenet.py) and a mode-0 launch on a 1/2-resolution
              64-channel map (above SDHIP_TUNE_BN_SLOT_MAX_MB)
Every fused case also hashes y after ONE launch on fresh inputs — equal bit for bit between the builds, or the run fails —
and compares the two sums as totals over the replicas, within the bounds of tests/test_conv.py (2e-4 max|ref| in mode 0,
2e-2 max|ref| in mode 1)."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

N = 20
# name, images, H, W, k, K (channels of x), C (channels of y / u), Ct (pixel stride of u and, in mode 1, of y), mode, addend, groups
CASES = [
    ("dense1 3x3 32->128 64x128", 16, 64, 128, 3, 32, 128, 128, 0, False, 2),
    ("dense2 3x3 32->128 32x64", 16, 32, 64, 3, 32, 128, 128, 0, False, 2),
    ("dense3 3x3 32->128 16x32", 16, 16, 32, 3, 32, 128, 128, 0, False, 2),
    ("dense4 3x3 32->128 8x16", 16, 8, 16, 3, 32, 128, 128, 0, False, 2),
    ("dense2 1x1 m1 128->160 of 512", 16, 32, 64, 1, 128, 160, 512, 1, True, 2),
    ("dense2 1x1 m1 128->352 of 512", 16, 32, 64, 1, 128, 352, 512, 1, True, 2),
    ("dense2 1x1 m1 128->480 of 512", 16, 32, 64, 1, 128, 480, 512, 1, True, 2),
    ("dense3 1x1 m1 128->288 of 1024", 16, 16, 32, 1, 128, 288, 1024, 1, True, 2),
    ("dense3 1x1 m1 128->992 of 1024", 16, 16, 32, 1, 128, 992, 1024, 1, True, 2),
    ("dense4 1x1 m1 128->544 of 1024", 16, 8, 16, 1, 128, 544, 1024, 1, True, 2),
    ("dense4 1x1 m1 128->992 of 1024", 16, 8, 16, 1, 128, 992, 1024, 1, True, 2),
    ("decoder 3x3 128->128 32x64", 8, 32, 64, 3, 128, 128, 128, 0, False, 1),
    ("decoder 3x3 128->128 32x64 +addend", 8, 32, 64, 3, 128, 128, 128, 0, True, 1),
    ("decoder 3x3 64->64 32x64", 8, 32, 64, 3, 64, 64, 64, 0, False, 1),
    ("decoder 3x3 64->64 32x64 +addend", 8, 32, 64, 3, 64, 64, 64, 0, True, 1),
]
RECORD = [
    ("(record) dense1 1x1 m1 128->224 of 256 64x128", 16, 64, 128, 1, 128, 224, 256, 1, True, 2),
    ("(record) 3x3 64->64 128x256", 8, 128, 256, 3, 64, 64, 64, 0, False, 1),
]
TWO = " [two launches]"


def child(tree, out_path):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    dt, BF, dev, NREP = torch.bfloat16, _lib.BF16, "cuda", ops.NREP
    res = {}

    def digest(t):
        return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]

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

    for record, cases in ((False, CASES), (True, RECORD)):
        for name, B, H, W, k, K, C, Ct, mode, add, G in cases:
            gen = torch.Generator().manual_seed(1000 * H + C)
            npix, pad = B * H * W, k // 2
            x = torch.randn(npix, K, generator=gen).to(dev).to(dt)
            u = (torch.randn(npix, Ct, generator=gen) * 1.3).to(dev).to(dt)
            a0 = torch.randn(npix, Ct, generator=gen).to(dev).to(dt) if add else None
            w = (torch.randn(K, C, k, k, generator=gen) * 0.1).to(dev)        # the forward convolution C -> K; this is its data gradient
            sc = (torch.rand(G, C, generator=gen) + 0.5).to(dev)
            sh = (torch.randn(G, C, generator=gen) * 0.3).to(dev)
            wd = ops.packed_weight(w, 'conv', 'dgrad', dt)
            ldy = Ct if mode == 1 else C
            y = torch.empty(npix, ldy, device=dev, dtype=dt)
            a = a0.clone() if add else None
            if mode == 1:
                sums = torch.zeros(2, NREP, G, C, dtype=torch.float32, device=dev)
            else:
                sums = torch.zeros(NREP, G, 2, C, dtype=torch.float64, device=dev)

            def fresh():
                sums.zero_()
                if mode == 1:
                    y.copy_(a0)
                else:
                    y.zero_()

            def fused():
                addend = y if mode == 1 else a
                call("sdhip_conv2d_fwd_bnbwd", ptr(x), ptr(wd), ptr(y), ptr(sums), C, NREP, ptr(u), Ct, ptr(sc), ptr(sh),
                     ptr(addend), (Ct if addend is not None else 0), B, H, W, K, K, H, W, C, ldy, k, k, 1, pad, pad, G, mode, BF, stream_ptr())

            fresh()
            fused()
            torch.cuda.synchronize()
            tot = sums.double().sum(1) if mode == 1 else sums.sum(0).permute(1, 0, 2)      # [2][G][C]
            rec = {"hash": digest(y[:, :C]), "sums": tot.flatten().tolist(), "mode": mode}
            rec["us"] = timed(fused)
            res[name] = rec
            if record:
                gp = torch.empty(npix, C, device=dev, dtype=dt)
                both = torch.zeros(2, NREP, G, C, dtype=torch.float32, device=dev)

                def two():
                    ops._conv_launch(x, K, wd, gp, C, None, None, None, None, B, H, W, K, H, W, C, k, k, 1, 1, pad, pad, False, 1, 0, False)
                    call("sdhip_affine_act_bwd", ptr(gp), C, ptr(u), Ct, ptr(y) if mode == 1 else None, Ct if mode == 1 else 0,
                         ptr(sc), ptr(sh), ptr(both[0]), ptr(both[1]), NREP, npix, C, G, 1, int(mode == 1), 0, BF, stream_ptr())
                fresh()
                res[name + TWO] = {"us": timed(two)}
            del x, u, a0, a, y
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
                out = os.path.join(tmp, "conv_bx_%s_%d.json" % (who, r))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, out], check=True, timeout=300)   # the first failure ends the run
                with open(out) as f:
                    runs[who].append(json.load(f))
    table, ok = {}, True
    print("%-50s %9s %7s %9s %7s %7s  %s" % ("case", "other us", "spread", "this us", "spread", "ratio", "verdict / outputs"))
    for name in runs["this"][0]:
        ta = [r[name]["us"] for r in runs["other"]]
        tb = [r[name]["us"] for r in runs["this"]]
        a, b, sa, sb = statistics.median(ta), statistics.median(tb), max(ta) - min(ta), max(tb) - min(tb)
        verdict = "gain" if b < a - (sa + sb) else ("SLOWER" if b > a + (sa + sb) else "even")
        ra, rb = runs["other"][0][name], runs["this"][0][name]
        note = ""
        if "hash" in rb:
            same = ra["hash"] == rb["hash"]
            ref = max(abs(v) for v in ra["sums"]) or 1.0
            worst = max(abs(va - vb) for va, vb in zip(ra["sums"], rb["sums"])) / ((2e-2 if rb["mode"] == 1 else 2e-4) * ref)
            note = "y %s, sums differ by %.3g of the bound" % ("same" if same else "DIFFERENT", worst)
            ok = ok and same and worst <= 1.0
        table[name] = {"other_us": a, "other_spread": sa, "this_us": b, "this_spread": sb, "verdict": verdict, "outputs": note}
        print("%-50s %9.2f %7.2f %9.2f %7.2f %7.3f  %s%s" % (name, a, sa, b, sb, b / a, verdict, "; " + note if note else ""), flush=True)
    if table_path:
        with open(table_path, "w") as f:
            json.dump(table, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
