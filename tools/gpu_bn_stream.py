"""The BatchNorm elementwise kernels of csrc/bn_act.hip, one by one, at the shapes the headline step calls them with: this
tree against another checkout of the repository (the parent commit, built), launch by launch.

  python tools/gpu_bn_stream.py OTHER_TREE [reps [TABLE.json]]   # the A/B: prints a table (and writes it as JSON if asked)
  python tools/gpu_bn_stream.py --child TREE OUT.json    # one measurement of one build (what the A/B starts, in turn)

One process per build (the package, and with it libsdhip.so, is imported from the tree given), the two builds alternating
`reps` (default 7) times; per case a graph of 20 launches is replayed, the table holds the medians in us per launch.  Shapes
(pixels, C, statistics groups): the stem and the decoder maps of one tower pass (8 images) and the DenseNet maps of both
towers as one batch (16 images, two groups), NREP = 32 replicas, outputs in place where the step has them in place
(stats_fix).  Every case also hashes its outputs after ONE launch on fresh inputs: elementwise outputs and per-channel
outputs (scale, shift, mean, invstd, running statistics, dgamma, dbeta, dS) must be equal bit for bit between the builds
(`same`); the atomically summed dscale / dshift replicas are compared as sums, within the bound tests/test_bn_kernels.py
uses for them ((L + 1) u sum |terms|, L the links of the f32 chain)."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

N, NREP = 20, 32
SHAPES = [(8 * 256 * 512, 64, 1), (8 * 256 * 512, 32, 1), (8 * 64 * 128, 64, 1), (8 * 32 * 64, 128, 1),
          (16 * 64 * 128, 128, 2), (16 * 32 * 64, 128, 2), (16 * 16 * 32, 128, 2), (16 * 8 * 16, 128, 2)]
SLICES = [(16 * 64 * 128, 256, 128, 2), (16 * 32 * 64, 512, 256, 2), (16 * 16 * 32, 1024, 512, 2), (16 * 8 * 16, 1024, 512, 2)]   # pixels, Ct, Cf, groups


def child(tree, out_path):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    dt, BF = torch.bfloat16, _lib.BF16
    dev = "cuda"
    torch.manual_seed(0)
    res = {}

    def digest(*ts):
        h = hashlib.sha1()
        for t in ts:
            h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
        return h.hexdigest()[:16]

    def measure(name, go, fresh, outs, sums=None):
        """fresh(): restore the inputs; outs(): tensors to hash; sums(): (replica sums f64, sum |terms| f64) or None"""
        fresh()
        go()
        torch.cuda.synchronize()
        rec = {"hash": digest(*outs())}
        if sums:
            a, b, sumabs, links = sums()
            rec["sums"] = [a.flatten().tolist(), b.flatten().tolist()]
            rec["sumabs"] = [sumabs[0].flatten().tolist(), sumabs[1].flatten().tolist()]
            rec["links"] = links
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
        rec["us"] = min(ts)
        res[name] = rec

    for npix, C, G in SHAPES:
        tag = "%dx%d g%d" % (npix, C, G)
        count = float(npix // G)
        x0 = (torch.randn(npix, C, device=dev) * 1.3 + 0.2).to(dt)
        g0 = torch.randn(npix, C, device=dev).to(dt)
        x, gy, y = x0.clone(), g0.clone(), torch.empty_like(x0)
        xg = x0.float().reshape(G, -1, C)
        S1 = torch.stack([xg.sum(1), (xg * xg).sum(1)], 1).double()                       # [G][2][C]
        w = torch.rand(NREP, 1, 1, C, device=dev, dtype=torch.float64)
        S = (S1[None] * w / w.sum(0, keepdim=True)).contiguous()                         # spread over the replicas
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        rm0, rv0 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        rm, rv = rm0.clone(), rv0.clone()
        sc, sf, mu, inv = (torch.empty(G, C, device=dev) for _ in range(4))
        dsc, dsh = torch.zeros(NREP, G, C, device=dev), torch.zeros(NREP, G, C, device=dev)
        dS = (torch.randn(G, 2, C, device=dev, dtype=torch.float64) * 1e-3).contiguous()
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)

        def fresh():
            x.copy_(x0); gy.copy_(g0); rm.copy_(rm0); rv.copy_(rv0); dsc.zero_(); dsh.zero_()

        def fwd_bn():
            call("sdhip_affine_act_bn", ptr(x), C, ptr(y), C, None, 0, ptr(S), C, NREP, ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                 ptr(sc), ptr(sf), ptr(mu), ptr(inv), npix, C, G, count, 1e-5, 0.1, 1, BF, stream_ptr())
        measure("affine_act_bn " + tag, fwd_bn, fresh, lambda: (y, sc, sf, mu, inv, rm, rv))
        measure("affine_act " + tag, lambda: call("sdhip_affine_act", ptr(x), C, ptr(y), C, None, 0, ptr(sc), ptr(sf), npix, C, G, 1, BF, stream_ptr()),
                fresh, lambda: (y,))

        def red():
            call("sdhip_affine_act_bwd", ptr(gy), C, ptr(x), C, None, 0, ptr(sc), ptr(sf), ptr(dsc), ptr(dsh), NREP, npix, C, G, 1, 0, 1, BF, stream_ptr())

        def red_sums():
            z = x0.float() * sc.repeat_interleave(npix // G, 0) + sf.repeat_interleave(npix // G, 0)
            gm = (g0.float() * (z > 0)).double().reshape(G, -1, C)
            xa = x0.double().reshape(G, -1, C)
            units = C // 8
            tx = min(units, 64); ty = 256 // tx; gyb = -(-units // tx)
            gxb = max(1, min(-(-(npix // G) // ty), max(1024 // (gyb * G), 1)))
            links = -(-(npix // G) // (gxb * ty)) + ty + -(-gxb // NREP)
            return dsc.double().sum(0), dsh.double().sum(0), torch.stack([(gm * xa).abs().sum(1), gm.abs().sum(1)]), links
        measure("affine_act_bwd(sums) " + tag, red, fresh, lambda: (), red_sums)
        measure("bn_bwd_apply_fin " + tag,
                lambda: call("sdhip_bn_bwd_apply_fin", ptr(gy), C, ptr(x), C, ptr(y), C, ptr(sc), ptr(sf), ptr(dsc), ptr(dsh), NREP, ptr(gamma),
                             ptr(mu), ptr(inv), ptr(dg), ptr(db), 0, 1.0, npix, C, G, count, 1, BF, stream_ptr()),
                lambda: (fresh(), dsc.normal_(), dsh.normal_()), lambda: (y, dg, db))
        measure("bn_bwd_apply " + tag,
                lambda: call("sdhip_bn_bwd_apply", ptr(gy), C, ptr(x), C, ptr(y), C, ptr(sc), ptr(sf), ptr(dS), C, npix, C, G, 1, BF, stream_ptr()),
                fresh, lambda: (y,))
        measure("stats_fix(in place) " + tag,
                lambda: call("sdhip_stats_fix", ptr(gy), C, ptr(x), C, ptr(gy), C, ptr(dS), C, npix, C, G, BF, stream_ptr()), fresh, lambda: (gy,))
        measure("affine_act_bwd(gx+=) " + tag,
                lambda: call("sdhip_affine_act_bwd", ptr(gy), C, ptr(x), C, ptr(y), C, ptr(sc), ptr(sf), None, None, 1, npix, C, G, 1, 1, 0, BF, stream_ptr()),
                lambda: (fresh(), y.copy_(x0)), lambda: (y,))
        measure("act_out_bwd " + tag,
                lambda: call("sdhip_act_out_bwd", ptr(gy), C, ptr(x), C, ptr(y), C, ptr(sc), npix, C, G, 1, BF, stream_ptr()), fresh, lambda: (y,))
        del x0, g0, x, gy, y
    for npix, Ct, Cf, G in SLICES:
        tag = "%dx32 of %d, Cf %d g%d" % (npix, Ct, Cf, G)
        cs = Cf - 32
        slab0 = (torch.randn(npix, Ct, device=dev) * 1.3).to(dt)
        gs0 = torch.randn(npix, Ct, device=dev).to(dt)
        slab, gs, dy2 = slab0.clone(), gs0.clone(), torch.empty(npix, 32, device=dev, dtype=dt)
        dsc, dsh = torch.randn(NREP, G, Cf, device=dev), torch.randn(NREP, G, Cf, device=dev)
        gamma = torch.rand(Cf, device=dev) + 0.5
        mu, inv = torch.randn(G, Cf, device=dev), torch.rand(G, Cf, device=dev) + 0.5
        dS0 = (torch.randn(G, 2, Ct, device=dev, dtype=torch.float64) * 1e-3).contiguous()
        dS = dS0.clone()
        dg, db = torch.empty(Cf, device=dev), torch.empty(Cf, device=dev)
        sg, sx = gs[:, cs:], slab[:, cs:]
        measure("stats_fix_fin " + tag,
                lambda: call("sdhip_stats_fix_fin", ptr(sg), Ct, ptr(sx), Ct, ptr(dy2), 32, npix, ptr(dS), Ct, cs, ptr(dsc), ptr(dsh), NREP, ptr(gamma),
                             ptr(mu), ptr(inv), ptr(dg), ptr(db), 0, 1.0, Cf, G, float(npix // G), BF, stream_ptr()),
                lambda: dS.copy_(dS0), lambda: (dy2, dS, dg, db))
        del slab0, gs0, slab, gs
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
                out = os.path.join(tmp, "bn_stream_%s_%d.json" % (who, r))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, out], check=True, timeout=600)
                with open(out) as f:
                    runs[who].append(json.load(f))
    U32, table, ok = 2.0 ** -24, {}, True
    print("%-52s %9s %9s %7s  %s" % ("case", "other us", "this us", "ratio", "outputs"))
    for name in runs["this"][0]:
        a = statistics.median(r[name]["us"] for r in runs["other"])
        b = statistics.median(r[name]["us"] for r in runs["this"])
        ra, rb = runs["other"][0][name], runs["this"][0][name]
        same = ra["hash"] == rb["hash"]
        note = "same" if same else "DIFFERENT"
        if "sums" in rb:
            worst = 0.0
            for k in (0, 1):
                for va, vb, s in zip(ra["sums"][k], rb["sums"][k], rb["sumabs"][k]):
                    worst = max(worst, abs(va - vb) / (2 * (rb["links"] + 1) * U32 * s + 1e-300))
            note = "sums differ by %.3g of the bound" % worst
            same = worst <= 1.0
        ok = ok and same
        table[name] = {"other_us": a, "this_us": b, "outputs": note}
        print("%-52s %9.2f %9.2f %7.3f  %s" % (name, a, b, b / a, note), flush=True)
    if table_path:
        with open(table_path, "w") as f:
            json.dump(table, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
