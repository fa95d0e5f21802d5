"""Fixture generator of the `*_disp` warp networks (warp.minidsnetDivideDisp / minidsnetDivideDisp2) and of the operators under
them (ops.warp_image_masked, ops.photo_loss): writes tests/golden/warp_disp.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py) and imports the reference's
own networks; as in tools/make_golden_warp.py the only change is the `tensor_type` ARGUMENT of `apply_disparity`
('torch.FloatTensor' instead of the CUDA default), no arithmetic.  Stored (data only):
  * operator cases with the reference's own f32 result and its largest deviation from the same expression evaluated in f64:
      - masked warp `apply_disparity(img, -gt) * (gt > 0)` at the MASKED_CASES shapes; the ground truth `gt` is stored (a mix of
        exact zeros, negative values, integers, fractions and values beyond the row: the mask cuts, samples leave the image on
        both sides); the image is regenerated from its seed (oracle.detweights, seed 7, "<case>:img");
      - photometric MSE `nn.MSELoss()(w, l)` and its gradient w.r.t. w at the PHOTO_CASES shapes ("<case>:w", "<case>:l");
  * the networks at B=2, 256x256, labels=2, seed 31 (inputs by seed, as tools/make_golden_warp.py): samples of all six outputs,
    the step's loss with cross-entropy only - `ThreeOutPutsDisp`: CE(outs[0]) + CE(outs[2]) + CE(outs[4]) + L1(outs[1]);
    `ThreeOutPutsDispConsist`: the three cross-entropies + MSE(outs[5], left), upstream's 0 * L1 left out - gradient norms per
    top-level module, the names of the parameters without a gradient, the running statistics of the BN_KEYS probes and of the
    tower's first BatchNorm (three updates per step).  The input images are smooth (smooth_image below).  The eval runs are
    float64 on trained-like running statistics, formed as tools/make_golden_warp.py forms them but with momentum 0.5 over TWO
    train-mode passes without gradients: the tower and SmallsegNet are called several times per pass, momentum 1 would leave
    the statistics of the LAST call alone (the warped, in one network masked, image), and an eval network normalised with
    those predicts disparities of thousands of pixels on the left image; a mixture of the calls is what a trained checkpoint
    carries.  A test reproduces the same steps, so no statistics are stored;
  * the ground-truth disparity of the minidsnetDivideDisp cases is drawn from [-4, 12): a quarter of the pixels is cut by the
    mask and the first columns sample beyond the left edge;
  * for the minidsnetDivideDisp2 train cases the share of pixels whose sample position j - disp_out lies within 1e-3 of an
    integer (the warp's gradient jumps there; asserted <= 1 %) and a stride-4 sample of disp_out on which a test re-checks it;
  * ordered state_dict keys / shapes and parameter names of every configuration the constructor tests build.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_warp_disp.py
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
NEAR_CAP = 0.01
MAX_BYTES = 1 << 20
# (tag, B, C, H, W)
MASKED_CASES = [("m3", 2, 3, 5, 13), ("m4", 1, 4, 3, 27)]
PHOTO_CASES = [("p13", 2, 3, 5, 13), ("p9", 1, 3, 7, 9)]
# (tag, class, CFG fields, patch type, labels, modes)
NETS = [("disp_1d", "minidsnetDivideDisp", dict(aspp=0), '1dcorr', 2, ("train", "eval")),
        ("disp2_1d", "minidsnetDivideDisp2", dict(aspp=0), '1dcorr', 2, ("train", "eval")),
        ("disp2_2d", "minidsnetDivideDisp2", dict(aspp=0), '', 2, ("train",))]
# configurations whose keys alone are stored: (tag, class, CFG fields, patch type, labels, include_edges)
KEY_ONLY = [("disp_a1_edges", "minidsnetDivideDisp", dict(aspp=1), '', 8, True),
            ("disp2_a1_edges", "minidsnetDivideDisp2", dict(aspp=1), '', 8, True)]
BN_KEYS = ("conv2d_ba0.0.layers.1", "resnet_features.branch3_1.1.layers.1", "segNet.Conv2DownUp1.c1.0.layers.1",
           "segNet.Conv2DownUp1.d5.0.layers.1")
OUT_NAMES = ("out0", "out1", "out2", "out3", "out4", "out5")
GT_RANGE = (-4.0, 12.0)
STAT_MOMENTUM, STAT_PASSES = 0.5, 2


def near_integer_share(disp_out):
    """Share of pixels whose sample position j - disp_out (f32, as the warp forms it) is within MARGIN of an integer."""
    d = np.asarray(disp_out, dtype=np.float32)
    x = (np.arange(d.shape[-1], dtype=np.float32) - d).astype(np.float64)
    return float((np.abs(x - np.round(x)) < MARGIN).mean())


def masked_gt(tag, B, H, W):
    rs = _rs(SEED, "gt:" + tag)
    shape = (B, 1, H, W)
    parts = [np.zeros(shape), -rs.uniform(0.1, W + 5.0, size=shape), rs.randint(1, 5, size=shape).astype(np.float64),
             rs.uniform(0.05, 3.0, size=shape), W + rs.uniform(1.0, 20.0, size=shape)]
    gt = np.choose(rs.randint(0, len(parts), size=shape), parts).astype(np.float32)
    x = np.arange(W, dtype=np.float32) - gt
    assert (gt == 0).any() and (gt < 0).any() and ((gt > 0) & (x < 0)).any() and (x > W - 1).any() and ((gt > 0) & (x >= 0)).any(), tag
    return gt


def gen_ops(arrays, apply_disparity):
    for tag, B, C, H, W in MASKED_CASES:
        img = randn_input(SEED, tag + ":img", (B, C, H, W))
        gt = torch.from_numpy(masked_gt(tag, B, H, W))
        out = apply_disparity(img, -gt, tensor_type='torch.FloatTensor') * (gt > 0)
        out64 = apply_disparity(img.double(), -gt.double(), tensor_type='torch.DoubleTensor') * (gt > 0)
        p = "masked.%s" % tag
        arrays[p + ".gt"] = gt.numpy().copy()
        arrays[p + ".out"] = out.numpy().copy()
        arrays[p + ".dev64"] = np.float64((out.double() - out64).abs().max())
        print("masked", tag, (B, C, H, W), "cut %d of %d pixels, deviation from f64 %.2e" % ((gt <= 0).sum(), gt.numel(), arrays[p + ".dev64"]))
    for tag, B, C, H, W in PHOTO_CASES:
        l = rand_input(SEED, tag + ":l", (B, C, H, W))
        w = rand_input(SEED, tag + ":w", (B, C, H, W))
        res = []
        for dt in (torch.float32, torch.float64):
            wv = w.detach().clone().to(dt).requires_grad_(True)
            loss = torch.nn.MSELoss()(wv, l.to(dt))
            loss.backward()
            res.append((loss.detach(), wv.grad))
        p = "photo.%s" % tag
        arrays[p + ".loss"] = np.float32(res[0][0].item())
        arrays[p + ".grad"] = res[0][1].numpy().copy()
        arrays[p + ".loss64"] = np.float64(res[1][0].item())
        arrays[p + ".dev64"] = np.float64((res[0][1].double() - res[1][1]).abs().max())
        print("photo", tag, (B, C, H, W), "loss %.7f (f64 %.9f)" % (res[0][0].item(), res[1][0].item()))


def ref_net(cls, kw, patch, labels, edges=False):
    from models import dsnet_t2_warp as D
    return getattr(D, cls)(R.CFG(**kw), labels=labels, pretrained=False, patch_type=patch, include_edges=edges, backbone='densenet')


def tower_bn(sd):
    return next(k[:-len(".running_mean")] for k in sd if k.startswith("resnet_features.resnet_features.") and k.endswith(".running_mean"))


def smooth_image(name):
    """(2,3,256,256) in [0,1]: 32x32 uniform noise enlarged bilinearly by 8.  The third tower pass reads an image that moves with
    the predicted disparity, so the comparison is only as well conditioned as the image is smooth.  On the per-pixel noise of the
    other fixtures two f32 implementations of the same step were 4.6 % apart in the gradient norm of dispoutConv and 0.5 % in
    the outputs of the 2-D correlation case; ref_f64_distance prints how far the reference's f32 step is from its f64 step on
    these images (1-D: outputs 2e-5, gradient norms 6e-3 at most; 2-D: 4e-4 and 1.8e-2)."""
    import torch.nn.functional as F
    return F.interpolate(rand_input(31, name, (2, 3, 32, 32)), scale_factor=8, mode='bilinear', align_corners=False).contiguous()


def net_inputs():
    import torch.nn.functional as F
    a, b = smooth_image("left_lo"), smooth_image("right_lo")
    lab = (rand_input(31, "seg", (2, 256, 256)) > 0.5).long()
    seg = F.one_hot(lab, 2).permute(0, 3, 1, 2).float()
    return a, b, seg, rand_input(31, "disp_signed", (2, 1, 256, 256), *GT_RANGE)


def step_loss(cls, outs, a, seg, disp):
    import torch.nn.functional as F
    ce = lambda y: torch.mean(torch.sum(-seg * F.log_softmax(y, 1), 1))
    loss = ce(outs[0]) + ce(outs[2]) + ce(outs[4])
    if cls == "minidsnetDivideDisp2":
        return loss + torch.nn.MSELoss()(outs[5], a)         # torch_implementation.py:314-317 without the 0 * L1
    return loss + F.l1_loss(outs[1], disp)


def ref_f64_distance(tag, cls, kw, patch, labels, outs, gnorms):
    """Printed, not stored: how far the reference's f32 train step is from the same step in f64 (outputs relative to their largest
    value, gradient norms relatively) - the conditioning of the case the bars of the tests have to live with."""
    ref = fill_state_dict(ref_net(cls, kw, patch, labels), 31).double().train()
    a, b, seg, disp = (t.double() for t in net_inputs())
    o64 = ref(a, b)
    step_loss(cls, o64, a, seg, disp).backward()
    g64 = G.grad_norms(ref)
    print("  ", tag, "f32 against f64: outputs", ["%.1e" % float((o.detach().double() - q.detach()).abs().max() / max(1.0, float(q.abs().max())))
                                                 for o, q in zip(outs, o64)],
          "gradient norms", {k: "%.1e" % (abs(gnorms[k] - v) / max(v, 1e-3)) for k, v in g64.items()})


def gen_nets(arrays):
    for tag, cls, kw, patch, labels, modes in NETS:
        takes_disp = cls == "minidsnetDivideDisp"
        for tm in modes:
            ref = fill_state_dict(ref_net(cls, kw, patch, labels), 31)
            ref.train() if tm == "train" else ref.eval()
            a, b, seg, disp = net_inputs()
            if tm == "eval":     # float64, trained-like running statistics: see the module docstring
                ref, a, b, seg, disp = ref.double(), a.double(), b.double(), seg.double(), disp.double()
                bns = [m for m in ref.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
                for m in bns:
                    m.momentum = STAT_MOMENTUM
                ref.train()
                with torch.no_grad():
                    for _ in range(STAT_PASSES):
                        ref(a, b, disp) if takes_disp else ref(a, b)
                for m in bns:
                    m.momentum = 0.1
                ref.eval()
            outs = ref(a, b, disp) if takes_disp else ref(a, b)
            loss = step_loss(cls, outs, a, seg, disp)
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
            if tm == "train" and not takes_disp:
                ref_f64_distance(tag, cls, kw, patch, labels, outs, G.grad_norms(ref))
            d = outs[1].detach()
            note = ""
            if tm == "train" and not takes_disp:
                share = near_integer_share(d.numpy())
                assert share <= NEAR_CAP, (tag, share)
                arrays["%s.near_share" % p] = np.float64(share)
                arrays["%s.disp_q" % p] = d.numpy()[:, :, ::4, ::4].astype(np.float32).copy()
                note = "near-integer sample positions %.3f%%" % (100 * share)
            x = torch.arange(256, dtype=d.dtype) - d
            print("net", tag, tm, "loss %.6f" % loss.item(), "disp %.2f..%.2f" % (d.min(), d.max()),
                  "clamped left %.3f%% right %.3f%%" % (100 * (x < 0).double().mean(), 100 * (x > 255).double().mean()), note,
                  "" if tm == "eval" else "no-grad %d of %d" % (len(arrays["%s.nograd" % p]), len(list(ref.parameters()))))
    gt = net_inputs()[3].numpy()
    x = np.arange(256, dtype=np.float32) - gt
    assert (gt <= 0).mean() > 0.1 and ((gt > 0) & (x < 0)).any() and (x > 255).any()
    arrays["gt_range"] = np.array(GT_RANGE)


def keys():
    out = {}
    for tag, cls, kw, patch, labels, edges in [n[:5] + (False,) for n in NETS] + KEY_ONLY:
        m = ref_net(cls, kw, patch, labels, edges)
        out[tag] = {"cls": cls, "cfg": kw, "patch": patch, "backbone": "densenet", "labels": labels, "edges": edges,
                    "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                    "parameters": [k for k, _ in m.named_parameters()]}
    return out


def main():
    G._install_stubs()
    from models import torch_dsnet as T
    from models import dsnet_t2_warp as D
    D.apply_disparity = functools.partial(T.apply_disparity, tensor_type='torch.FloatTensor')   # an argument, no arithmetic
    arrays = {}
    gen_ops(arrays, T.apply_disparity)
    gen_nets(arrays)
    arrays["keys"] = np.array(json.dumps(keys(), separators=(",", ":")))
    arrays["cases"] = np.array(json.dumps({"masked": MASKED_CASES, "photo": PHOTO_CASES, "seed": SEED, "margin": MARGIN,
                                           "near_cap": NEAR_CAP}, separators=(",", ":")))
    G.save("warp_disp", **arrays)
    size = os.path.getsize(os.path.join(G.OUT, "warp_disp.npz"))
    assert size <= MAX_BYTES, "tests/golden/warp_disp.npz is %d bytes (limit %d)" % (size, MAX_BYTES)


if __name__ == "__main__":
    main()
