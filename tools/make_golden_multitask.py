"""Fixture generator of the multitask loss (`-multaskloss 1|2`): writes tests/golden/multitask.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py), whose helpers it
reuses unchanged: the reference's own multiTask_loss (util/utilTorchLoss.py:521-540) and minidsnetExt
(models/dsnet_t2.py) are imported at generation time and filled with the deterministic weights of oracle/detweights.py.
Stored: the loss alone on seeded tensors (maps, means, gradients), and minidsnetExt with multaskloss 1 and 2 at B=2,
256x256, seed 31 (output and loss-map samples, step loss, gradient norms per top-level module, exact log-variance
gradients, running statistics of a tower / pyramid / auxiliary BatchNorm), plus the ordered state_dict keys and
parameter names of the three configurations.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_multitask.py
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
from oracle import ref_models as R  # noqa: E402
from oracle.detweights import fill_state_dict, rand_input, randn_input  # noqa: E402

# (three_out, C, B, H, W, log-variances (disp, seg1, seg2)): both signs, label-19 pixels in every case
LOSS_CASES = {"t1_c2": (1, 2, 2, 12, 20, (0.3, -0.4, 0.25)), "t1_c19": (1, 19, 2, 12, 20, (-0.2, 0.5, -0.35)),
              "t2_c2": (2, 2, 2, 12, 20, (-0.3, 0.45, 0.0)), "t2_c19": (2, 19, 2, 12, 20, (0.15, -0.6, 0.0))}
# (tag, classes, modes, void pixels): void pixels come from a 20-channel one-hot (label 19 ignored by the loss)
NET_CASES = [("mt1", 1, 2, ("train", "eval"), False), ("mt1_l19", 1, 19, ("train",), True), ("mt2", 2, 2, ("train", "eval"), False)]
BN_KEYS = ("resnet_features.resnet_features.norm5", "resnet_features.branch0_0.1.layers.1", "conv2d_ba0.0.layers.1")


def loss_inputs(tag):
    """Seeded inputs of one loss case (the tests regenerate them with the same calls)."""
    three_out, C, B, H, W, lv = LOSS_CASES[tag]
    disp = rand_input(7, tag + ":disp", (B, 1, H, W), 0.0, 8.0)
    disp_gt = rand_input(7, tag + ":disp_gt", (B, 1, H, W), 0.0, 8.0)
    disp_gt.view(-1)[::37] = disp.view(-1)[::37]                  # a few exact ties: sign(0) = 0
    seg1 = randn_input(7, tag + ":seg1", (B, C, H, W), 2.0)
    seg2 = randn_input(7, tag + ":seg2", (B, C, H, W), 2.0)
    lab = (rand_input(7, tag + ":lab", (B, H, W)) * C).long().clamp(0, C - 1)
    lab[rand_input(7, tag + ":void", (B, H, W)) < 0.15] = 19
    return three_out, lv, disp, disp_gt, seg1, seg2, lab


def gen_loss(arrays):
    from util.utilTorchLoss import multiTask_loss
    for tag in LOSS_CASES:
        three_out, lv, disp, disp_gt, seg1, seg2, lab = loss_inputs(tag)
        m = multiTask_loss(three_out)
        with torch.no_grad():
            m.log_var_disp.fill_(lv[0]); m.log_var_seg1.fill_(lv[1])
            if three_out == 1:
                m.log_var_seg2.fill_(lv[2])
        xs = [t.clone().requires_grad_(True) for t in (disp, seg1, seg2)]
        ld, l1, l2 = m(xs[0], disp_gt, xs[1], xs[2], lab)
        loss = ld.mean() + l1.mean() + l2.mean()
        loss.backward()
        p = "loss.%s" % tag
        for name, t in (("ld", ld), ("l1", l1), ("l2", l2)):
            arrays["%s.%s" % (p, name)] = t.detach().numpy().copy()
            arrays["%s.%s.mean" % (p, name)] = np.float64(t.detach().double().mean())
        for name, t in zip(("disp", "seg1", "seg2"), xs):     # three_out == 2: seg2 is unused (no gradient)
            arrays["%s.grad.%s" % (p, name)] = t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32)
        for name, prm in m.named_parameters():
            arrays["%s.grad.%s" % (p, name)] = prm.grad.numpy().copy()
        print(tag, "loss", float(loss))


def net_inputs(classes, void):
    a, b = rand_input(31, "left", (2, 3, 256, 256)), rand_input(31, "right", (2, 3, 256, 256))
    disp = rand_input(31, "disp", (2, 1, 256, 256), 0.0, 8.0)
    if void:
        cls = (rand_input(31, "cls", (2, 256, 256)) * 20).long().clamp(0, 19)       # 19 = void
        seg = F.one_hot(cls, 20).permute(0, 3, 1, 2).float().contiguous()           # the FULL one-hot: argmax 19 is void
    else:
        seg = F.one_hot((rand_input(31, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float()
    return a, b, seg, disp


def ref_net(mode, classes):
    from models import dsnet_t2 as D
    return D.minidsnetExt(R.CFG(aspp=0, multaskloss=mode), labels=classes, pretrained=False, patch_type='1dcorr', backbone='densenet')


def gen_nets(arrays):
    for tag, mode, classes, modes, void in NET_CASES:
        for tm in modes:
            ref = fill_state_dict(ref_net(mode, classes), 31)
            ref.train() if tm == "train" else ref.eval()
            a, b, seg, disp = net_inputs(classes, void)
            outs = ref(a, b, None, disp, seg.argmax(1))
            loss = outs[4].mean() + outs[5].mean() + outs[6].mean()
            loss.backward()
            p = "%s.%s" % (tag, tm)
            for i, name in enumerate(("seg1", "disp", "seg2")):
                arrays.update(G.flat("%s.%s" % (p, name), G.sample(outs[i], 8)))
            for i, name in zip((4, 5, 6), ("ld", "l1", "l2")):
                arrays.update(G.flat("%s.%s" % (p, name), G.sample(outs[i].reshape(outs[i].shape[0], 1, *outs[i].shape[-2:])
                                                                  if outs[i].dim() == 3 else outs[i], 8)))
                arrays["%s.%s.mean" % (p, name)] = np.float64(outs[i].double().mean())
            arrays["%s.loss" % p] = np.float64(loss.item())
            for k, v in G.grad_norms(ref).items():
                arrays["%s.gnorm.%s" % (p, k)] = v
            for k, prm in ref.mtloss.named_parameters():
                arrays["%s.lvgrad.%s" % (p, k)] = prm.grad.numpy().copy()
            sd = ref.state_dict()
            for k in BN_KEYS:
                arrays["%s.rm.%s" % (p, k)] = sd[k + ".running_mean"].numpy().copy()
                arrays["%s.rv.%s" % (p, k)] = sd[k + ".running_var"].numpy().copy()
            arrays["%s.nograd" % p] = np.array([k for k, prm in ref.named_parameters() if prm.grad is None] or [""])
            print(tag, tm, "loss", loss.item())


def keys():
    out = {}
    for name, mode, classes in (("mini_mt1", 1, 2), ("mini_mt2", 2, 2), ("mini_mt1_l19", 1, 19)):
        m = ref_net(mode, classes)
        out[name] = {"state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                     "parameters": [k for k, _ in m.named_parameters()]}
    return out


def main():
    G._install_stubs()
    arrays = {}
    gen_loss(arrays)
    gen_nets(arrays)
    arrays["keys"] = np.array(json.dumps(keys(), separators=(",", ":")))
    arrays["meta.corr"] = np.array("assumed-semantics")
    G.save("multitask", **arrays)


if __name__ == "__main__":
    main()
