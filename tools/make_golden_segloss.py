"""Fixture generator of the segmentation loss terms (`-loss`, `-segWeight`): writes tests/golden/segloss.npz (the four
small cases) and tests/golden/segloss_big.npz (the two large ones: no committed file may exceed 1 MiB).

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py) and calls the
reference's own lossSeg_fn (losses/multiLosses.py:8-128) for every case x list x segWeight below.  Stored per case: the
logits and the label map the one-hot target is built from (label = C marks a void pixel of the cityscapes cases, whose
target has C + 1 channels); per case x list x segWeight: the loss (`...loss`, f64 of the f32 result) and the gradient
w.r.t. the logits (`...grad`).  Arrays that are bit-identical to an earlier one (the never-weighted lists with segWeight
0 and 1, the roses table of ones, [dice_loss, diceEntropy] = [dice_loss]) are stored once; `aliases` (JSON) maps their
keys to the stored key.  The two large cases hold three lists only (BIG_LISTS) and not their logits: `inputs(case)`
rebuilds those from the seed, and the tests make the same call (oracle/detweights.py).

The class-weight tables are not copied from anywhere: a recording wrapper around the categoricalCrossEntropy that
lossSeg_fn calls notes the weight argument it is handed (`weights.<dataset>`).

For every list without the Lovasz term (which upstream cannot run in f64) the same call is repeated on f64 inputs and
the deviation of the f32 run stored as `...dev` = (max |g32 - g64| / max |g64|, |l32 - l64| / max(1, |l64|)): the generator asserts
that both stay below 1e-6, a tenth of the bars of tests/test_segloss.py.

Also stored for the `city` case: a second logit tensor with its weighted cross-entropy (the first head of a training
step) and a disparity pair with the masked L1 term of losses/multiLosses.py:134-141.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_segloss.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import make_golden as G  # noqa: E402
from oracle.detweights import rand_input, randn_input  # noqa: E402

SEED = 53
# name -> (dataset, C, target channels, B, H, W, logit sigma)
CASES = {"roses": ("roses", 2, 2, 2, 7, 13, 2.0), "roses_sat": ("roses", 2, 2, 1, 9, 17, 12.0),
         "garden": ("garden", 9, 9, 3, 5, 11, 2.0), "city": ("cityscapes", 19, 20, 2, 12, 21, 2.0),
         "roses_big": ("roses", 2, 2, 2, 64, 96, 2.0), "city_big": ("cityscapes", 19, 20, 1, 40, 56, 2.0)}
LISTS = (("dice_loss",), ("tversky_loss2",), ("diceEntropy",), ("cross_entropy", "lovasz_loss", "dice_loss"),
         ("cross_entropy", "tversky_loss2"), ("cross_entropy",), ("dice_loss", "diceEntropy"),
         ("lovasz_loss", "tversky_loss2", "diceEntropy"))
BIG_LISTS = (("dice_loss",), ("diceEntropy",), ("cross_entropy", "tversky_loss2"))


def tag(names):
    return "+".join(names)


def lists_of(case):
    return BIG_LISTS if case.endswith("_big") else LISTS


def labels(case):
    """(B,H,W) int64 label map; label = C is void (only where the target has C + 1 channels)."""
    ds, C, Ct, B, H, W, _ = CASES[case]
    if case == "garden":      # class 8 absent everywhere, class 7: one pixel (image 0), class 6: two pixels (image 1)
        lab = (rand_input(SEED, case + ":lab", (B, H, W)) * 6).long().clamp(0, 5)
        lab[0, 2, 3] = 7
        lab[1, 1, 4] = 6
        lab[1, 3, 7] = 6
        return lab
    return (rand_input(SEED, case + ":lab", (B, H, W)) * Ct).long().clamp(0, Ct - 1)


def inputs(case, name="z"):
    ds, C, Ct, B, H, W, sigma = CASES[case]
    z = randn_input(SEED, "%s:%s" % (case, name), (B, C, H, W), sigma)
    lab = labels(case)
    seg_full = F.one_hot(lab, Ct).permute(0, 3, 1, 2).float().contiguous()
    return z, lab, seg_full


def ref_loss(names, seg_full, z, dataset, seg_weight):
    """lossSeg_fn(...)[2] and its gradient w.r.t. the logits."""
    from losses.multiLosses import lossSeg_fn
    cfg = types.SimpleNamespace(datasetName=dataset, segWeight=seg_weight)
    x = z.clone().requires_grad_(True)
    loss = lossSeg_fn(list(names), seg_full, x, cfg, 0)[2]
    loss.backward()
    return loss.detach(), x.grad.detach()


def main():
    G._install_stubs()
    import losses.multiLosses as ML

    recorded = []
    inner = ML.categoricalCrossEntropy

    def recording_cce(y, gt, weight=[]):
        recorded.append(weight)
        return inner(y, gt, weight)
    ML.categoricalCrossEntropy = recording_cce

    small, big = ({}, {}, {}), ({}, {}, {})        # (arrays, aliases, first key of every stored content) per file

    def put(store, key, a):
        arrays, aliases, seen = store
        a = np.asarray(a)
        a = np.ascontiguousarray(a) if a.ndim else a          # (ascontiguousarray would turn a scalar into shape (1,))
        h = (a.dtype.str, a.shape, a.tobytes())
        if h in seen:
            aliases[key] = seen[h]
        else:
            seen[h] = key
            arrays[key] = a

    worst = [0.0, 0.0]
    for case, (ds, C, Ct, B, H, W, sigma) in CASES.items():
        z, lab, seg_full = inputs(case)
        store = big if case.endswith("_big") else small
        arrays = store[0]
        if store is small:
            arrays["%s.z" % case] = z.numpy().copy()
        arrays["%s.lab" % case] = lab.numpy().astype(np.int8)
        if case == "garden":
            counts = seg_full.sum((2, 3))
            assert counts[0, 7] == 1 and counts[1, 6] == 2 and counts[:, 8].sum() == 0, counts
        if "weights.%s" % ds not in small[0]:
            del recorded[:]
            ref_loss(("cross_entropy",), seg_full, z, ds, 1)
            assert len(recorded) == 1 and len(recorded[0]) != 0
            w = recorded[0].detach().numpy().reshape(-1).astype(np.float32)
            assert w.shape == (C,)
            small[0]["weights.%s" % ds] = w.copy()
        for names in lists_of(case):
            for sw in (0, 1):
                key = "%s.%s.sw%d" % (case, tag(names), sw)
                loss, grad = ref_loss(names, seg_full, z, ds, sw)
                put(store, key + ".loss", np.float64(loss.item()))
                put(store, key + ".grad", grad.numpy())
                if "lovasz_loss" not in names:
                    l64, g64 = ref_loss(names, seg_full.double(), z.double(), ds, sw)
                    dev = (float((grad.double() - g64).abs().max() / g64.abs().max()), abs(float(loss) - float(l64)) / max(1.0, abs(float(l64))))
                    assert dev[0] < 1e-6 and dev[1] < 1e-6, (key, dev)
                    worst = [max(worst[0], dev[0]), max(worst[1], dev[1])]
                    arrays[key + ".dev"] = np.array(dev, np.float64)
                print(key, "loss %.6f  max|grad| %.3e" % (float(loss), float(grad.abs().max())))
    # the first head and the disparity of a training step on `city`
    arrays = small[0]
    z1, _, seg_full = inputs("city", "z1")
    loss, grad = ref_loss(("cross_entropy",), seg_full, z1, "cityscapes", 1)
    arrays["city.z1"] = z1.numpy().copy()
    arrays["city.seg1.sw1.loss"] = np.float64(loss.item())
    arrays["city.seg1.sw1.grad"] = grad.numpy().copy()
    _, _, _, B, H, W, _ = CASES["city"]
    disp = rand_input(SEED, "city:disp", (B, 1, H, W), 0.0, 8.0).requires_grad_(True)
    disp_gt = rand_input(SEED, "city:disp_gt", (B, 1, H, W), -1.0, 8.0)          # some <= 0: invalid
    zeros = (disp_gt > 0) * 1.0
    l1 = torch.nn.L1Loss()(disp * zeros, disp_gt * zeros)                         # losses/multiLosses.py:139-141
    l1.backward()
    arrays["city.disp"] = disp.detach().numpy().copy()
    arrays["city.disp_gt"] = disp_gt.numpy().copy()
    arrays["city.l1.loss"] = np.float64(l1.item())
    arrays["city.l1.grad"] = disp.grad.numpy().copy()

    for arrays, aliases, _ in (small, big):
        arrays["aliases"] = np.array(json.dumps(aliases, separators=(",", ":"), sort_keys=True))
    small[0]["cases"] = np.array(json.dumps(CASES, separators=(",", ":")))
    small[0]["dev.worst"] = np.array(worst, np.float64)
    print("f32 vs f64 of the reference: worst grad %.2e (relative to max |grad|), worst loss %.2e" % tuple(worst))
    G.save("segloss", **small[0])
    G.save("segloss_big", **big[0])


if __name__ == "__main__":
    main()
