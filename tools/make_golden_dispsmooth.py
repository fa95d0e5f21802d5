"""Fixture generator of the `smooth_grad` disparity regulariser: writes tests/golden/dispsmooth.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py) and calls the reference's
own smoothing_gradients (util/utilTorchLoss.py:41-101) on every case below.  Stored per case: the left image, the
disparity and the label map the one-hot target is built from (`.left`, `.disp`, `.lab`; the large case `big` holds none of
them: `inputs(case)` rebuilds them from the seed through oracle/detweights.py, and the tests make the same call), the value
(`.value`, f64 of the f32 result) and the gradient w.r.t. the disparity (`.grad`).  `city_nv` is `city` with channel 19
of the target dropped (label 19 becomes an all-zero row) and shares its inputs.

For every case the deviation of the reference's f32 run from the closed form of include/sdhip.h evaluated in f64 is stored
as `.dev` = (max |g32 - g64| / max |g64|, |l32 - l64| / |l64|); the reference itself cannot run in f64, its filter is cast
to f32.  The generator asserts that both stay below a tenth of the bar of tests/test_dispsmooth.py (1e-5); a case that
does not would get ten times its deviation written as `.bar`.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dispsmooth.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import make_golden as G  # noqa: E402
from oracle.detweights import rand_input  # noqa: E402

SEED = 71
BAR = 1e-5
# name -> (B, H, W, target channels, image channels, label block (rows, columns))
CASES = {"roses": (2, 37, 83, 2, 3, (9, 14)), "city": (1, 21, 40, 20, 4, (7, 8)), "plateau": (1, 17, 19, 2, 3, None),
         "one": (1, 3, 3, 3, 3, None), "none_a": (1, 2, 9, 2, 3, (2, 3)), "none_b": (1, 9, 2, 2, 3, (3, 2)),
         "big": (2, 70, 150, 9, 3, (12, 17))}
GATED = ("roses", "city", "big")       # at least 25 % of the pixels gated on, in at least two classes


def labels(case):
    """(B,H,W) int64 label map: piecewise constant (per-pixel random labels would gate almost every pixel off)."""
    B, H, W, Ct, _, blk = CASES[case]
    if case == "plateau":               # class 1 everywhere but one column of alternating labels: the gate is 0 in and beside it
        lab = torch.ones((B, H, W), dtype=torch.int64)
        lab[:, ::2, 9] = 0
        return lab
    if case == "one":
        return torch.full((B, H, W), 2, dtype=torch.int64)
    by, bx = blk
    gh, gw = (H + by - 1) // by, (W + bx - 1) // bx
    grid = (rand_input(SEED, case + ":lab", (B, gh, gw)) * Ct).long().clamp(0, Ct - 1)
    if case == "city":
        grid[0, 0, 0], grid[0, 1, 2] = 19, 19       # void regions: a class with the full one-hot, nothing with channel 19 dropped
    ys, xs = torch.arange(H) // by, torch.arange(W) // bx
    return grid[:, ys][:, :, xs]


def inputs(case):
    """(left, disp, lab, full one-hot target) of a case, from the seed."""
    B, H, W, Ct, Ci, _ = CASES[case]
    left = rand_input(SEED, case + ":left", (B, Ci, H, W))
    disp = rand_input(SEED, case + ":disp", (B, 1, H, W), 0.0, 8.0)
    if case == "plateau":               # a constant image (weight exactly e) and a disparity constant over 4 x 4 blocks (exact ties)
        left = torch.full((B, Ci, H, W), 0.5)
        coarse = rand_input(SEED, case + ":disp", (B, 1, (H + 3) // 4, (W + 3) // 4), 0.0, 8.0)
        disp = coarse[:, :, torch.arange(H) // 4][:, :, :, torch.arange(W) // 4].contiguous()
    lab = labels(case)
    return left, disp, lab, F.one_hot(lab, Ct).permute(0, 3, 1, 2).float().contiguous()


def gauss_table():
    """matlab_style_gauss2D((7, 7), 2) (util/utilTorchLoss.py:8-20; no entry falls under its epsilon cut), float64."""
    y, x = np.ogrid[-3:4, -3:4]
    h = np.exp(-(x * x + y * y) / 8.0)
    return h / h.sum()


def closed_form(left, disp, seg, weight=1.0, dtype=torch.float64):
    """(value, gradient w.r.t. disp, gate M) of the closed form of include/sdhip.h in `dtype`; the filter is rounded to f32 first."""
    left, d, seg = left.to(dtype), disp[:, 0].to(dtype), seg.to(dtype)
    B, H, W = d.shape
    Y = 0.2126 * left[:, 0] + 0.7152 * left[:, 1] + 0.0722 * left[:, 2]
    g = torch.from_numpy(gauss_table().astype(np.float32)).to(dtype)
    Ys = F.conv2d(F.pad(Y[:, None], (3, 3, 3, 3)), g[None, None])[:, 0]
    lab = torch.where(seg.sum(1) > 0, seg.argmax(1), torch.full((B, H, W), -1, dtype=torch.int64))
    M = torch.zeros((B, H, W), dtype=torch.bool)
    if H >= 3 and W >= 3:
        c = lab[:, 1:-1, 1:-1]
        m = c >= 0
        for dy in range(3):
            for dx in range(3):
                m = m & (lab[:, dy:H - 2 + dy, dx:W - 2 + dx] == c)
        M[:, 1:-1, 1:-1] = m
    zeros = torch.zeros((B, H, W), dtype=dtype)
    dv, dh, wv, wh = zeros.clone(), zeros.clone(), zeros.clone(), zeros.clone()
    dv[:, :-1] = d[:, :-1] - d[:, 1:]
    dh[:, :, :-1] = d[:, :, :-1] - d[:, :, 1:]
    wv[:, :-1] = torch.exp(1.0 - (Ys[:, :-1] - Ys[:, 1:]).abs())
    wh[:, :, :-1] = torch.exp(1.0 - (Ys[:, :, :-1] - Ys[:, :, 1:]).abs())
    wv, wh = wv * M, wh * M
    s = weight * 0.7 / (128.0 * B * H * W)
    value = s * (wv * dv.abs() + wh * dh.abs()).sum()
    gv, gh = wv * torch.sign(dv), wh * torch.sign(dh)
    grad = gv + gh
    grad[:, 1:] -= gv[:, :-1]
    grad[:, :, 1:] -= gh[:, :, :-1]
    return value, (s * grad)[:, None], M


def ref_loss(left, disp, seg):
    """smoothing_gradients(left, disp, seg) and its gradient w.r.t. the disparity."""
    from util.utilTorchLoss import smoothing_gradients
    d = disp.clone().requires_grad_(True)
    loss = smoothing_gradients(left.clone(), d, seg)
    if not loss.requires_grad:          # an image below 3 x 3: the mask zeroes every term
        return loss.detach(), torch.zeros_like(disp)
    loss.backward()
    return loss.detach(), d.grad.detach()


def main():
    G._install_stubs()
    arrays, worst = {}, [0.0, 0.0]

    def run(key, left, disp, lab, seg):
        loss, grad = ref_loss(left, disp, seg)
        l64, g64, M = closed_form(left, disp, seg)
        gmax, lmag = float(g64.abs().max()), abs(float(l64))
        dev = (float((grad.double() - g64).abs().max()) / gmax if gmax else float(grad.abs().max()),
               abs(float(loss) - float(l64)) / lmag if lmag else abs(float(loss)))
        arrays[key + ".value"] = np.float64(loss.item())
        arrays[key + ".grad"] = grad.numpy().copy()
        arrays[key + ".dev"] = np.array(dev, np.float64)
        bar = BAR
        if max(dev) > BAR / 10:
            bar = 10 * max(dev)
            arrays[key + ".bar"] = np.float64(bar)
            print("%s: deviation %s above a tenth of %g: the case's bar is %g" % (key, dev, BAR, bar))
        assert max(dev) <= bar / 10, (key, dev)
        worst[0], worst[1] = max(worst[0], dev[0]), max(worst[1], dev[1])
        gated = [int((M & (lab == c)).sum()) for c in range(seg.shape[1])]
        frac = float(M.float().mean())
        print("%-8s value %.6e  max|grad| %.3e  gated %.0f %% in %d classes  dev %.1e %.1e"
              % (key, float(loss), float(grad.abs().max()), 100 * frac, sum(1 for n in gated if n), dev[0], dev[1]))
        return frac, gated

    for case in CASES:
        left, disp, lab, seg = inputs(case)
        if case != "big":
            arrays[case + ".left"] = left.numpy().copy()
            arrays[case + ".disp"] = disp.numpy().copy()
            arrays[case + ".lab"] = lab.numpy().astype(np.int8)
        frac, gated = run(case, left, disp, lab, seg)
        if case in GATED:
            assert frac >= 0.25 and sum(1 for n in gated if n) >= 2, (case, frac, gated)
        if case == "one":
            assert sum(gated) == 1
        if case.startswith("none"):
            assert float(arrays[case + ".value"]) == 0.0 and not arrays[case + ".grad"].any()
        if case == "plateau":
            g = arrays[case + ".grad"][0, 0]
            assert (g[2:15, 1:7] == 0).sum() > 20 and (g != 0).any() and not g[:, 9:11].any()      # ties inside the blocks; the gated-off columns
        if case == "city":
            frac, gated = run("city_nv", left, disp, lab, seg[:, :19].contiguous())
            assert frac >= 0.25 and sum(1 for n in gated if n) >= 2, (frac, gated)
            assert float(arrays["city_nv.value"]) < float(arrays["city.value"])                    # the void regions no longer count
    arrays["cases"] = np.array(json.dumps(CASES, separators=(",", ":")))
    arrays["dev.worst"] = np.array(worst, np.float64)
    print("f32 reference vs the closed form in f64: worst grad %.2e (relative to max |grad|), worst value %.2e" % tuple(worst))
    G.save("dispsmooth", **arrays)


if __name__ == "__main__":
    main()
