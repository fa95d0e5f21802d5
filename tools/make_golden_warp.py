"""Fixture generator of the disparity warp (`ops.apply_disparity`, `ops.warp_blend`): writes tests/golden/warp.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py) and imports the reference's
own `models.torch_dsnet.apply_disparity`; the only change is its `tensor_type` ARGUMENT ('torch.FloatTensor' instead of
the CUDA default), no arithmetic.  Stored:
  * operator cases: output, gradient w.r.t. the image and w.r.t. the offset of loss = sum(out * g), for odd sizes and
    offsets that are all zero, exact integers, fractional within +-3, larger than the row (every pixel clamped, both
    signs) and a per-pixel mix of those.  The offsets are stored; image and g are regenerated from seeds
    (oracle.detweights, seed 7, names "<case>:img" / "<case>:g").  Fractional offsets are drawn so that no j + offset lies
    within 1e-3 of an integer unless it is exactly one (the offset gradient jumps at integers, the value at W-1): the
    generator asserts that margin, so the reference alone decides every pixel;
  * blend cases: both = (1 - a) * l + a * apply_disparity(r, -d) with a one-channel gate a in (0, 1) and with
    a = softmax_c(raw scores); loss = sum(both * g1) + sum(warped * g2); both outputs and all four input gradients;
  * the networks minidsnetDivide / minidsnetDivideSoftmax (models/dsnet_t2_warp.py) at B=2 256x256, seed 31, whose
    `apply_disparity` is rebound to the same CPU partial: samples of all six outputs, the `ThreeOutPuts` loss with
    cross-entropy only (oracle.make_golden.train_loss over the first four outputs plus the cross-entropy of outs[4],
    torch_implementation.py:157-158,298), gradient norms per top-level module, the names of the parameters without a
    gradient, and the running statistics of the BatchNorms upstream updates twice per step (conv2d_ba0,
    segNet.Conv2DownUp1), of the discarded resnet_features.branch3_1 and of the tower's first BatchNorm.  The eval runs use
    trained-like running statistics: with the seed's random ones the eval network predicts disparities of thousands of
    pixels and the warp clamps 98 % of the image.  Every BatchNorm's momentum is set to 1 for ONE train-mode pass without
    gradients over the same input (the running statistics then are the batch statistics of the module's last call), the
    momentum is restored and the network evaluated; a test reproduces this with the same three steps, so no statistics
    are stored.  The eval runs are computed in float64 (as tools/make_golden_mobilenet.py), so that the expected values
    carry no f32 rounding of their own;
  * ordered state_dict keys / shapes and parameter names of every configuration the constructor tests build.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_warp.py
"""
import functools
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_golden as G  # noqa: E402
from oracle import ref_models as R  # noqa: E402
from oracle.detweights import _rs, fill_state_dict, rand_input, randn_input  # noqa: E402

SEED = 7
MARGIN = 1e-3
# (tag, B, C, H, W, offset kind)
OP_CASES = [("zero", 2, 2, 3, 13, "zero"), ("int", 1, 5, 4, 21, "int"), ("frac", 2, 19, 5, 27, "frac"),
            ("large", 2, 1, 3, 10, "large"), ("mix", 2, 19, 7, 37, "mix"), ("h1", 1, 2, 1, 9, "mix"),
            ("wide", 1, 5, 2, 1031, "mix")]
# (tag, B, C, H, W, softmax gate)
BLEND_CASES = [("sig2", 2, 2, 5, 19, False), ("sig19", 1, 19, 3, 27, False), ("smax5", 2, 5, 4, 21, True),
               ("smax19", 1, 19, 3, 33, True)]


def _x(off):
    """j + offset as the reference forms it (f32)."""
    W = off.shape[-1]
    return np.arange(W, dtype=np.float32) + off.astype(np.float32)


def _near_integer(off):
    x = _x(off).astype(np.float64)
    d = np.abs(x - np.round(x))
    return (d > 0) & (d < MARGIN)


def offsets(tag, kind, B, H, W):
    rs = _rs(SEED, "offset:" + tag)
    shape = (B, 1, H, W)

    def redraw(draw):
        o = draw(shape).astype(np.float32)
        for _ in range(100):
            bad = _near_integer(o)
            if not bad.any():
                break
            o[bad] = draw(int(bad.sum())).astype(np.float32)
        return o

    def frac():
        return redraw(lambda n: rs.uniform(-3.0, 3.0, size=n))

    def large():
        return redraw(lambda n: rs.choice([-1.0, 1.0], size=n) * (W + rs.uniform(1.0, 50.0, size=n)))

    kinds = {"zero": lambda: np.zeros(shape, np.float32), "int": lambda: rs.randint(-4, 5, size=shape).astype(np.float32),
             "frac": frac, "large": large}
    if kind != "mix":
        off = kinds[kind]()
    else:
        parts = [kinds[k]() for k in ("zero", "int", "frac", "large")]
        pick = rs.randint(0, 4, size=shape)
        off = np.choose(pick, parts).astype(np.float32)
    assert not _near_integer(off).any(), tag         # exactly an integer, or at least MARGIN away from one
    return off


def gen_ops(arrays, warp):
    for tag, B, C, H, W, kind in OP_CASES:
        img = randn_input(SEED, tag + ":img", (B, C, H, W)).requires_grad_(True)
        g = randn_input(SEED, tag + ":g", (B, C, H, W))
        off = torch.from_numpy(offsets(tag, kind, B, H, W)).requires_grad_(True)
        out = warp(img, off)
        (out * g).sum().backward()
        p = "op.%s" % tag
        arrays[p + ".offset"] = off.detach().numpy().copy()
        arrays[p + ".out"] = out.detach().numpy().copy()
        arrays[p + ".g_img"] = img.grad.numpy().copy()
        arrays[p + ".g_offset"] = off.grad.numpy().copy()
        x = _x(off.detach().numpy())
        print("op", tag, (B, C, H, W), "clamped left %d right %d of %d" % ((x < 0).sum(), (x > W - 1).sum(), x.size))


def gen_blend(arrays, warp):
    for tag, B, C, H, W, smax in BLEND_CASES:
        left = randn_input(SEED, tag + ":l", (B, C, H, W)).requires_grad_(True)
        right = randn_input(SEED, tag + ":r", (B, C, H, W)).requires_grad_(True)
        g1, g2 = randn_input(SEED, tag + ":g1", (B, C, H, W)), randn_input(SEED, tag + ":g2", (B, C, H, W))
        disp = torch.from_numpy(-offsets(tag, "mix", B, H, W)).requires_grad_(True)      # the networks warp with -disp
        if smax:
            gate = randn_input(SEED, tag + ":gate", (B, C, H, W)).requires_grad_(True)
            a = torch.softmax(gate, 1)
        else:
            gate = rand_input(SEED, tag + ":gate", (B, 1, H, W), 0.05, 0.95).requires_grad_(True)
            a = gate
        warped = warp(right, -disp)
        both = (1 - a) * left + a * warped
        ((both * g1).sum() + (warped * g2).sum()).backward()
        p = "blend.%s" % tag
        arrays[p + ".disp"] = disp.detach().numpy().copy()
        for k, v in (("both", both), ("warped", warped), ("g_left", left.grad), ("g_right", right.grad), ("g_disp", disp.grad),
                     ("g_gate", gate.grad)):
            arrays["%s.%s" % (p, k)] = v.detach().numpy().copy()
        if smax:
            arrays[p + ".prob"] = a.detach().numpy().copy()
        print("blend", tag, (B, C, H, W))


# (tag, class, CFG fields, patch type, backbone, labels, modes)
NETS = [("div_1d", "minidsnetDivide", dict(aspp=0), '1dcorr', 'densenet', 2, ("train", "eval")),
        ("div_2d", "minidsnetDivide", dict(aspp=0), '', 'densenet', 2, ("train",)),
        ("div_mb", "minidsnetDivide", dict(aspp=0), '1dcorr', 'mobilenet', 2, ("train",)),
        ("soft_1d", "minidsnetDivideSoftmax", dict(aspp=0), '1dcorr', 'densenet', 2, ("train", "eval")),
        ("div_l19", "minidsnetDivide", dict(aspp=0), '1dcorr', 'densenet', 19, ("eval",))]
# configurations whose keys alone are stored: (tag, class, CFG fields, patch type, backbone, labels, include_edges)
KEY_ONLY = [("div_a1_edges", "minidsnetDivide", dict(aspp=1), '', 'densenet', 8, True),
            ("div_mb_a1", "minidsnetDivide", dict(aspp=1), '1dcorr', 'mobilenet', 8, False),
            ("soft_a1_edges", "minidsnetDivideSoftmax", dict(aspp=1), '', 'densenet', 8, True),
            ("soft_mb", "minidsnetDivideSoftmax", dict(aspp=0), '1dcorr', 'mobilenet', 8, False)]
BN_KEYS = ("conv2d_ba0.0.layers.1", "resnet_features.branch3_1.1.layers.1", "segNet.Conv2DownUp1.c1.0.layers.1",
           "segNet.Conv2DownUp1.d5.0.layers.1")
OUT_NAMES = ("out0", "out1", "out2", "out3", "out4", "out5")


def ref_net(cls, kw, patch, backbone, labels, edges=False):
    from models import dsnet_t2_warp as D
    real = torch.load
    torch.load = lambda *a, **k: {}          # mobilenetv3_large() loads a weight file it never uses (tools/make_golden_mobilenet.py)
    try:
        return getattr(D, cls)(R.CFG(**kw), labels=labels, pretrained=False, patch_type=patch, include_edges=edges, backbone=backbone)
    finally:
        torch.load = real


def tower_bn(sd):
    return next(k[:-len(".running_mean")] for k in sd if k.startswith("resnet_features.resnet_features.") and k.endswith(".running_mean"))


def gen_nets(arrays):
    import torch.nn.functional as F
    for tag, cls, kw, patch, backbone, labels, modes in NETS:
        for tm in modes:
            ref = fill_state_dict(ref_net(cls, kw, patch, backbone, labels), 31)
            ref.train() if tm == "train" else ref.eval()
            a, b = rand_input(31, "left", (2, 3, 256, 256)), rand_input(31, "right", (2, 3, 256, 256))
            if labels == 2:
                lab = (rand_input(31, "seg", (2, 256, 256)) > 0.5).long()
            else:
                lab = (rand_input(31, "seg", (2, 256, 256)) * labels).long().clamp(0, labels - 1)
            seg = F.one_hot(lab, labels).permute(0, 3, 1, 2).float()
            disp = rand_input(31, "disp", (2, 1, 256, 256), 0.0, 8.0)
            if tm == "eval":     # float64, trained-like running statistics: see the module docstring
                ref, a, b, seg, disp = ref.double(), a.double(), b.double(), seg.double(), disp.double()
                bns = [m for m in ref.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
                for m in bns:
                    m.momentum = 1.0
                ref.train()
                with torch.no_grad():
                    ref(a, b)
                for m in bns:
                    m.momentum = 0.1
                ref.eval()
            outs = ref(a, b)
            loss = G.train_loss(outs[:4], seg, disp) + torch.mean(torch.sum(-seg * F.log_softmax(outs[4], 1), 1))
            p = "net.%s.%s" % (tag, tm)
            if tm == "train":
                loss.backward()
                for k, v in G.grad_norms(ref).items():
                    arrays["%s.gnorm.%s" % (p, k)] = v
                arrays["%s.nograd" % p] = np.array([k for k, prm in ref.named_parameters() if prm.grad is None])
                sd = ref.state_dict()
                for k in BN_KEYS + (tower_bn(sd),):
                    arrays["%s.rm.%s" % (p, k)] = sd[k + ".running_mean"].numpy().copy()
                    arrays["%s.rv.%s" % (p, k)] = sd[k + ".running_var"].numpy().copy()
            for name, o in zip(OUT_NAMES, outs):
                arrays.update(G.flat("%s.%s" % (p, name), G.sample(o, 16)))
            arrays["%s.loss" % p] = np.float64(loss.item())
            d = outs[1].detach()
            x = torch.arange(256, dtype=d.dtype) - d
            print("net", tag, tm, "loss %.6f" % loss.item(), "disp %.2f..%.2f" % (d.min(), d.max()),
                  "clamped left %.3f%% right %.3f%%" % (100 * (x < 0).double().mean(), 100 * (x > 255).double().mean()),
                  "max |seg| %.3g" % max(float(outs[i].abs().max()) for i in (0, 2, 4)),
                  "" if tm == "eval" else "no-grad %d of %d" % (len(arrays["%s.nograd" % p]), len(list(ref.parameters()))))


def keys():
    out = {}
    for tag, cls, kw, patch, backbone, labels, edges in [n[:6] + (False,) for n in NETS] + KEY_ONLY:
        m = ref_net(cls, kw, patch, backbone, labels, edges)
        out[tag] = {"cls": cls, "cfg": kw, "patch": patch, "backbone": backbone, "labels": labels, "edges": edges,
                    "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                    "parameters": [k for k, _ in m.named_parameters()]}
    return out


def main():
    G._install_stubs()
    from models import torch_dsnet as T
    from models import dsnet_t2_warp as D
    warp = functools.partial(T.apply_disparity, tensor_type='torch.FloatTensor')
    D.apply_disparity = warp          # an argument, no arithmetic: the default tensor type is the CUDA one
    arrays = {}
    gen_ops(arrays, warp)
    gen_blend(arrays, warp)
    gen_nets(arrays)
    arrays["keys"] = np.array(json.dumps(keys(), separators=(",", ":")))
    arrays["cases"] = np.array(json.dumps({"op": OP_CASES, "blend": BLEND_CASES, "seed": SEED}, separators=(",", ":")))
    G.save("warp", **arrays)


if __name__ == "__main__":
    main()
