"""Fixture generator of the Ext_small edge networks (`-net sdnet_mini_ext_small*`, models/dsnet_t2_ext_small.py) and their
operators (`ops.grad_mag`, `ops.edge_loss`): writes tests/golden/ext_small.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py) and imports the reference's own
`util.utilTorchGate.compute_grad_mag`, `losses.multiLosses.lossEdge_fn` and `models.dsnet_t2_ext_small`; nothing of their
arithmetic is changed (the stubs of oracle.make_golden turn `.cuda()` into the identity).  Stored:
  * `compute_grad_mag(E, True, False)` cases: the reference's f32 output (every element: the largest case is 26 k values) for
    inputs regenerated from seeds (oracle.detweights.rand_input, seed 83, name "gm:<case>"), and the worst deviation of that f32
    run from the closed form of include/sdhip.h evaluated in f64, per case and overall (`gradmag.dev`);
  * `lossEdge_fn(edges, z)` cases: value, gradient w.r.t. z and the deviation of the reference's f32 run from the f64 closed form
    (value: relative; gradient: relative to its largest element; `edge.<case>.dev` is the larger of the two), for targets with
    about 10 % positives, a target holding values other than 0 / 1, no positives, all positives, and logits of +-80 (a
    single element, (1,1,1,1), is not among them: the reference's numpy indexing fails on it).  Logits are regenerated from the
    seed ("eb:<case>:z", standard deviation 3, or +-80), targets are stored;
  * the networks Ext_smallv0 / Ext_small / Ext_smallv2 at B=2 256x256, labels 2, densenet, `1dcorr`, and Ext_small with the
    2-D correlation, seed 31, train and eval with the sampling and the trained-like eval statistics of
    tools/make_golden_warp.py (eval in float64).  The edge models get compute_grad_mag(left, True, False) as third argument, as
    netForward gives it, and the `edgeOut` loss CE(outs[2]) + L1(outs[1]) + lossEdge_fn(edges, outs[0])
    (torch_implementation.py:170-171,279,304,320-325) with a seeded binary edge target made of 8 x 8 blocks ("edges", 15 % set);
    Ext_smallv0 gets the four-output loss of oracle.make_golden.train_loss.  Gradient norms per top-level module, the names of
    the parameters without a gradient, running statistics of four BatchNorms and of the tower's first, samples of all outputs;
  * ordered state_dict keys / shapes and parameter names of these and of three more configurations.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ext_small.py
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

SEED = 83
BAR = 1e-5           # tests/test_edge_kernels.py: the edge loss is held to this unless ten times a stored deviation is larger
# (tag, B, C, H, W)
GM_CASES = [("tiny", 1, 1, 2, 2), ("odd", 2, 3, 7, 9), ("four", 2, 4, 5, 8), ("big", 1, 3, 67, 131)]
# (tag, B, H, W, target kind, logit kind)
EB_CASES = [("small", 2, 7, 9, "p30", "randn"), ("p10", 2, 67, 131, "p10", "randn"), ("mixed", 2, 7, 9, "mixed", "randn"),
            ("nopos", 2, 7, 9, "zeros", "randn"), ("allpos", 2, 7, 9, "ones", "randn"), ("big80", 2, 67, 131, "p10", "pm80")]


def grad_mag_closed(E):
    """sqrt(Ox^2 + Oy^2 + 1e-6) of the zero-padded central differences, in the dtype of E."""
    P = F.pad(E, (1, 1, 1, 1))
    ox = 0.5 * (P[:, :, 1:-1, 2:] - P[:, :, 1:-1, :-2])
    oy = 0.5 * (P[:, :, 2:, 1:-1] - P[:, :, :-2, 1:-1])
    return torch.sqrt(ox * ox + oy * oy + 1e-6)


def edge_closed(z, t):
    """(value, gradient) of lossEdge_fn in f64; the two weights are f32 quotients, as the reference's are."""
    z, t = z.double(), t.double()
    pos, neg = int((t == 1).sum()), int((t == 0).sum())
    tot = pos + neg
    wp = float(np.float32(neg) / np.float32(tot)) if tot else 0.0
    wn = float(np.float32(pos) / np.float32(tot)) if tot else 0.0
    w = torch.where(t == 1, torch.full_like(t, wp), torch.where(t == 0, torch.full_like(t, wn), torch.zeros_like(t)))
    bce = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    n = z.numel()
    return float((w * bce).sum() / n), w * (torch.sigmoid(z) - t) / n


def edge_target(tag, kind, shape):
    r = rand_input(SEED, "eb:%s:t" % tag, shape)
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "ones":
        return torch.ones(shape)
    if kind == "mixed":      # a quarter each of 0, 1, 0.5 and 2: the last two carry no weight
        return torch.tensor([0.0, 1.0, 0.5, 2.0])[(r * 4).long().clamp(0, 3)]
    return (r > (0.7 if kind == "p30" else 0.9)).float()


def edge_logits(tag, kind, shape):
    if kind == "pm80":
        return torch.where(rand_input(SEED, "eb:%s:z" % tag, shape) > 0.5, torch.tensor(80.0), torch.tensor(-80.0))
    return randn_input(SEED, "eb:%s:z" % tag, shape, 3.0)


def gen_grad_mag(arrays):
    from util import utilTorchGate as U
    worst = 0.0
    for tag, B, C, H, W in GM_CASES:
        E = rand_input(SEED, "gm:" + tag, (B, C, H, W))
        out = U.compute_grad_mag(E, True, False)
        assert out.dtype == torch.float32 and out.shape == E.shape
        dev = float((out.double() - grad_mag_closed(E.double())).abs().max())
        arrays["gradmag.%s.out" % tag] = out.numpy().copy()
        arrays["gradmag.%s.dev" % tag] = np.float64(dev)
        worst = max(worst, dev)
        print("grad_mag", tag, (B, C, H, W), "dev %.3e, range %.4f..%.4f" % (dev, float(out.min()), float(out.max())))
    arrays["gradmag.dev"] = np.float64(worst)


def gen_edge_loss(arrays):
    from losses.multiLosses import lossEdge_fn
    for tag, B, H, W, tk, zk in EB_CASES:
        shape = (B, 1, H, W)
        t = edge_target(tag, tk, shape)
        z = edge_logits(tag, zk, shape).requires_grad_(True)
        loss = lossEdge_fn(t, z)
        loss.backward()
        loss = loss.detach()
        v64, g64 = edge_closed(z.detach(), t)
        gmax = float(g64.abs().max())
        dv = abs(float(loss) - v64) / abs(v64) if v64 else abs(float(loss))
        dg = float((z.grad.double() - g64).abs().max()) / gmax if gmax else float(z.grad.abs().max())
        assert max(dv, dg) <= BAR / 10, (tag, dv, dg)
        arrays["edge.%s.target" % tag] = t.numpy().copy()
        arrays["edge.%s.value" % tag] = np.float64(float(loss))
        arrays["edge.%s.grad" % tag] = z.grad.numpy().copy()
        arrays["edge.%s.dev" % tag] = np.float64(max(dv, dg))
        print("edge", tag, shape, "P %d N %d value %.8e dev value %.2e grad %.2e" % (int((t == 1).sum()), int((t == 0).sum()), float(loss), dv, dg))


# (tag, class, patch type, labels, include_edges, modes)
NETS = [("v0_1d", "Ext_smallv0", '1dcorr', 2, False, ("train", "eval")),
        ("es_1d", "Ext_small", '1dcorr', 2, False, ("train", "eval")),
        ("v2_1d", "Ext_smallv2", '1dcorr', 2, False, ("train", "eval")),
        ("es_2d", "Ext_small", '', 2, False, ("train", "eval"))]
KEY_ONLY = [("es_edges", "Ext_small", '', 8, True), ("v2_edges", "Ext_smallv2", '1dcorr', 8, True), ("v0_l8", "Ext_smallv0", '', 8, False)]
BN_KEYS = ("conv2d_ba0.0.layers.1", "conv2d_ba2.0.layers.1", "segNet.Conv2DownUp1.c1.0.layers.1", "Conv2DownUp10.c2.0.layers.1")
OUT_NAMES = ("out0", "out1", "out2", "out3")
EDGE_CLASSES = ("Ext_small", "Ext_smallv2")


def ref_net(cls, patch, labels, edges=False):
    from models import dsnet_t2_ext_small as D
    return getattr(D, cls)(R.CFG(aspp=0), labels=labels, pretrained=False, patch_type=patch, include_edges=edges, backbone='densenet')


def block_edges(B, H, W, blk=8, p=0.15):
    grid = (rand_input(31, "edges", (B, 1, (H + blk - 1) // blk, (W + blk - 1) // blk)) < p).float()
    return grid.repeat_interleave(blk, 2).repeat_interleave(blk, 3)[:, :, :H, :W].contiguous()


def tower_bn(sd):
    return next(k[:-len(".running_mean")] for k in sd if k.startswith("resnet_features.resnet_features.") and k.endswith(".running_mean"))


def gen_nets(arrays):
    from losses.multiLosses import lossEdge_fn
    from util import utilTorchGate as U
    for tag, cls, patch, labels, _, modes in NETS:
        for tm in modes:
            ref = fill_state_dict(ref_net(cls, patch, labels), 31)
            ref.train() if tm == "train" else ref.eval()
            a, b = rand_input(31, "left", (2, 3, 256, 256)), rand_input(31, "right", (2, 3, 256, 256))
            lab = (rand_input(31, "seg", (2, 256, 256)) > 0.5).long()
            seg = F.one_hot(lab, labels).permute(0, 3, 1, 2).float()
            disp = rand_input(31, "disp", (2, 1, 256, 256), 0.0, 8.0)
            edges = block_edges(2, 256, 256)
            extra = (U.compute_grad_mag(a, True, False),) if cls in EDGE_CLASSES else ()     # in f32: its filter taps are f32 tensors
            if tm == "eval":     # float64, trained-like running statistics: tools/make_golden_warp.py
                ref, a, b, seg, disp = ref.double(), a.double(), b.double(), seg.double(), disp.double()
                extra = tuple(e.double() for e in extra)
                bns = [m for m in ref.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
                for m in bns:
                    m.momentum = 1.0
                ref.train()
                with torch.no_grad():
                    ref(a, b, *extra)
                for m in bns:
                    m.momentum = 0.1
                ref.eval()
            outs = ref(a, b, *extra)
            assert len(outs) == 4
            if cls in EDGE_CLASSES:
                ce = torch.mean(torch.sum(-seg * F.log_softmax(outs[2], 1), 1))
                edge = lossEdge_fn(edges, outs[0].float())       # the weight tensor is f32: the eval run's logits are cast
                loss = ce + F.l1_loss(outs[1], disp) + edge
                arrays["net.%s.%s.edge_loss" % (tag, tm)] = np.float64(edge.item())
            else:
                loss = G.train_loss(outs, seg, disp)
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
            print("net", tag, tm, "loss %.6f" % loss.item(), [tuple(o.shape) for o in outs],
                  "params %.2f M" % (sum(q.numel() for q in ref.parameters()) / 1e6),
                  "" if tm == "eval" else "no-grad %d of %d" % (len(arrays["%s.nograd" % p]), len(list(ref.parameters()))))


def keys():
    out = {}
    for tag, cls, patch, labels, edges in [n[:5] for n in NETS] + KEY_ONLY:
        m = ref_net(cls, patch, labels, edges)
        out[tag] = {"cls": cls, "patch": patch, "labels": labels, "edges": edges,
                    "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                    "parameters": [k for k, _ in m.named_parameters()]}
    return out


def main():
    G._install_stubs()
    arrays = {}
    gen_grad_mag(arrays)
    gen_edge_loss(arrays)
    gen_nets(arrays)
    arrays["keys"] = np.array(json.dumps(keys(), separators=(",", ":")))
    arrays["cases"] = np.array(json.dumps({"gradmag": GM_CASES, "edge": EB_CASES, "seed": SEED}, separators=(",", ":")))
    G.save("ext_small", **arrays)
    assert os.path.getsize(os.path.join(G.OUT, "ext_small.npz")) < 1 << 20


if __name__ == "__main__":
    main()
