"""Fixture generator of the DeepLabV3+ / Xception-65 networks (`-net deeplab`, `-net deeplab_mod`): writes
tests/golden/deeplab.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py), whose helpers it reuses
unchanged; `spatial_correlation_sampler` is the oracle's restatement (fixtures through it: corr="assumed-semantics").
Every case is run twice, in float32 and in float64, from the same float32 weights and inputs.  The float64 result is the
expected value; next to it the generator stores `<key>.dev`, the deviation of the reference's own float32 result from it
in the metric the test applies to that key, so that a test can tell a bar the reference itself does not meet.
Stored:
  * ordered state_dict keys / shapes and parameter names of deeplab_mod (19 and 2 channels) and deeplab;
  * blocks (train mode, B=2, seed 7): SeparableConv2d (relu_first both ways x dilation 1 / 2 / 12), three XceptionBlocks,
    ASPP(32, 16, 8) on a 5x7 map, SPPDecoder with and without concat_prev: outputs, input gradients, parameter gradients
    (strided samples + norms) and running statistics;
  * networks (seed 41, encoder BatchNorm eps 1e-3 as getNetwork sets it, Dropout2d p = 0): deeplab_mod with 19 channels in
    train mode at B=2 32x48 and in eval mode at B=2 64x96 and B=1 40x72, deeplab in train and eval mode at B=2 32x48 — the
    heads, the outputs after the harness steps of netForward (torch_implementation.py:123-131,163-166), the loss
    CE(seg1) + CE(seg2) + L1(disp) on a 19-class one-hot target (deeplab: CE alone), gradient norms per top-level module and
    the running statistics of a few BatchNorm layers;
  * per head of the eval cases, the relative L2 deviation from the float64 result of a run whose Conv2d / BatchNorm2d
    weights, outputs and input images are rounded to bf16 storage (forward hooks): what bf16 storage alone costs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_deeplab.py
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
from oracle.detweights import fill_state_dict, rand_input, randn_input  # noqa: E402

MAX_FULL = 256      # parameter gradients up to this many elements are stored whole, larger ones as a strided sample
MAX_ACT = 4096      # the same for the outputs and input gradients of the block cases
SEED_BLK, SEED_NET = 7, 41
# (tag, relu_first, dilation): SeparableConv2d(12, 20) on 2 x 12 x 13 x 15
SEPS = [("sep_r%d_d%d" % (int(rf), d), rf, d) for rf in (True, False) for d in (1, 2, 12)]
# (tag, channel_list, stride, dilation, skip, relu_first, low_feat, H, W)
XBLOCKS = [("xb_conv_s2", [8, 16, 16, 16], 2, 1, 'conv', True, False, 9, 13),
           ("xb_sum_d2", [16, 16, 16, 16], 1, 2, 'sum', True, True, 7, 9),
           ("xb_none_d4", [16, 24, 24, 32], 1, 4, 'none', False, False, 7, 10)]
# (tag, concat_prev): SPPDecoder(12, 16, concat_prev) on x 2x16x3x4, low 2x12x7x9, other 2x24x7x9
DECODERS = [("dec_plain", False), ("dec_prev", 24)]
# (tag, net, mode, B, h, w)
NETS = [("mod.train", "deeplab_mod", "train", 2, 32, 48), ("mod.eval", "deeplab_mod", "eval", 2, 64, 96),
        ("mod.eval1", "deeplab_mod", "eval", 1, 40, 72), ("mono.train", "deeplab", "train", 2, 32, 48),
        ("mono.eval", "deeplab", "eval", 2, 32, 48)]
BN_KEYS = {"deeplab_mod": ("encoder.bn1", "encoder.block2.sep_conv3.block.bn_depth", "encoder.block8.sep_conv2.block.bn_point",
                           "encoder.block21.sep_conv3.block.bn_depth", "spp.aspp3.block.bn_depth", "spp.image_pooling.bn",
                           "decoder2.sep1.block.bn_depth", "decoder3.sep1.block.bn_point"),
           "deeplab": ("encoder.bn1", "encoder.block21.sep_conv3.block.bn_depth", "spp.aspp1.block.bn_depth", "decoder.sep1.block.bn_depth")}
HEAD_STRIDE = 8


def rel_max(a, b):
    """max |a - b| / max(1, max |b|): the metric of the sampled-tensor checks."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.float64(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else np.float64(0)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.float64(np.linalg.norm(a - b) / max(1e-12, np.linalg.norm(b)))


def flat_entry(out, key, t, max_full):
    """t flattened, whole up to max_full elements, else every step-th element (`<key>.step`)."""
    t = t.detach().reshape(-1)
    step = max(1, -(-t.numel() // max_full))
    out[key] = t[::step].double().numpy().copy()
    out[key + ".step"] = np.int64(step)


def grad_entry(out, key, g):
    flat_entry(out, key, g, MAX_FULL)
    out[key + ".l2"] = np.float64(g.detach().double().pow(2).sum().sqrt())


def rel_stat(a, b):
    """max |a - b| / (0.1 + |b|): the metric of the running-statistics checks (allclose with atol = rtol / 10)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.float64((np.abs(a - b) / (0.1 + np.abs(b))).max())


def is_stat(key):
    return ".buf." in key or ".rm." in key or ".rv." in key


def put(arrays, r32, r64):
    """Store the float64 results and, per key, the deviation of the float32 run in the test's metric."""
    for k, v in r64.items():
        if k.endswith(".step"):
            arrays[k] = v
            continue
        a = r32[k]
        if np.ndim(v) == 0:       # loss, norms, means: relative difference
            arrays[k] = np.float64(v)
            arrays[k + ".dev"] = np.float64(abs(float(a) - float(v)) / max(1e-3, abs(float(v))))
        else:
            arrays[k] = np.asarray(v, dtype=np.float32)
            arrays[k + ".dev"] = rel_stat(a, v) if is_stat(k) else rel_max(a, v)


def both(run):
    return run(torch.float32), run(torch.float64)


def block_results(p, mod, inputs, outs_of, dtype):
    """Train-mode forward + backward of `mod` on `inputs` (name -> f32 tensor) with the loss sum_i (out_i * w_i).sum()."""
    mod = mod.to(dtype).train()
    xs = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in inputs.items()}
    outs = outs_of(mod, xs)
    loss = 0
    res = {}
    for i, y in enumerate(outs):
        wy = randn_input(SEED_BLK, "%s:w%d" % (p, i), tuple(y.shape)).to(dtype)
        loss = loss + (y * wy).sum()
        flat_entry(res, "%s.y%d" % (p, i), y, MAX_ACT)
    loss.backward()
    for k, x in xs.items():
        flat_entry(res, "%s.g%s" % (p, k), x.grad, MAX_ACT)
    for n, prm in mod.named_parameters():
        grad_entry(res, "%s.grad.%s" % (p, n), prm.grad)
    for n, b in mod.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            res["%s.buf.%s" % (p, n)] = b.double().numpy().copy()
    return res


def block_cases():
    """(prefix, constructor(module namespace), inputs, outputs-of) of every block case; tests/test_deeplab.py builds the
    native modules from the same list (the tensors are regenerated from seeds)."""
    cases = []
    for tag, rf, d in SEPS:
        cases.append((tag, lambda M, rf=rf, d=d: M.SeparableConv2d(12, 20, dilation=d, relu_first=rf), {"x": (2, 12, 13, 15)},
                      lambda m, xs: [m(xs["x"])]))
    for tag, ch, s, d, skip, rf, low, H, W in XBLOCKS:
        cases.append((tag, lambda M, a=(ch, s, d, skip, rf, low): M.XceptionBlock(a[0], stride=a[1], dilation=a[2],
                                                                                   skip_connection_type=a[3], relu_first=a[4],
                                                                                   low_feat=a[5]),
                      {"x": (2, ch[0], H, W)}, lambda m, xs, low=low: list(m(xs["x"])) if low else [m(xs["x"])]))
    cases.append(("aspp", lambda M: _no_dropout(M.ASPP(32, 16, 8)), {"x": (2, 32, 5, 7)}, lambda m, xs: [m(xs["x"])]))
    for tag, prev in DECODERS:
        shapes = {"x": (2, 16, 3, 4), "low": (2, 12, 7, 9)}
        if prev:
            shapes["other"] = (2, prev, 7, 9)
        cases.append((tag, lambda M, prev=prev: M.SPPDecoder(12, 16, prev), shapes,
                      lambda m, xs, prev=prev: list(m(xs["x"], xs["low"], xs["other"]) if prev else m(xs["x"], xs["low"]))))
    return cases


def _no_dropout(m):
    m.dropout.p = 0.0
    return m


def gen_blocks(arrays):
    from models_deeplab_mod import common, spp, xception

    class M:
        SeparableConv2d, XceptionBlock, ASPP, SPPDecoder = common.SeparableConv2d, xception.XceptionBlock, spp.ASPP, spp.SPPDecoder

    for tag, make, shapes, outs_of in block_cases():
        p = "blk.%s" % tag
        inputs = {k: randn_input(SEED_BLK, "%s:%s" % (p, k), s) for k, s in shapes.items()}
        r32, r64 = both(lambda dt: block_results(p, fill_state_dict(make(M), SEED_BLK), inputs, outs_of, dt))
        put(arrays, r32, r64)
        print("block", tag, "max dev", max(float(arrays[k]) for k in arrays if k.startswith(p + ".") and k.endswith(".dev")))


def ref_net(name, channels=19):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):     # create_spp prints its dec_type
        if name == "deeplab_mod":
            from models_deeplab_mod.net import SPPNet
        else:
            from models_deeplab.net import SPPNet
        m = SPPNet(output_channels=channels)
    m.update_bn_eps()
    return m


def net_inputs(tag, B, h, w, channels=19):
    left, right = rand_input(SEED_NET, tag + ":left", (B, 3, h, w)), rand_input(SEED_NET, tag + ":right", (B, 3, h, w))
    labels = (rand_input(SEED_NET, tag + ":seg", (B, h, w)) * channels).long().clamp(max=channels - 1)
    seg = F.one_hot(labels, channels).permute(0, 3, 1, 2).float()
    disp = rand_input(SEED_NET, tag + ":disp", (B, 1, h, w), 0.0, 8.0)
    return left, right, seg, disp


def harness(model, name, left, right):
    """netForward of the reference for the two DeepLab output types (torch_implementation.py:123-131,159-166)."""
    left = left * 2 - 1
    h, w = left.shape[2:]
    left = F.pad(left, [0, 1, 0, 1])
    up = lambda y: F.interpolate(y, size=(h + 1, w + 1), mode='bilinear', align_corners=True)[..., :h, :w]
    if name == "deeplab_mod":
        heads = model(left, F.pad(right, [0, 1, 0, 1]))
        return list(heads), [up(heads[0]), up(heads[1]), up(heads[2])]
    heads = model(left)
    return [heads], [up(heads)]


def ce(y, seg):
    return torch.mean(torch.sum(-seg * F.log_softmax(y, 1), 1))


def net_loss(name, outs, seg, disp):
    if name == "deeplab_mod":
        return ce(outs[0], seg) + ce(outs[2], seg) + F.l1_loss(outs[1], disp)
    return ce(outs[0], seg)


HEADS = {"deeplab_mod": ("x", "disp", "seg"), "deeplab": ("x",)}
OUTS = {"deeplab_mod": ("seg1", "disp1", "seg2"), "deeplab": ("seg1",)}


def sampled(t):
    return G.sample(t.detach().double(), HEAD_STRIDE)["sample"].astype(np.float64)


def net_results(tag, name, mode, B, h, w, dtype, bf16_storage=False):
    m = fill_state_dict(ref_net(name), SEED_NET)
    m.spp.dropout.p = 0.0
    left, right, seg, disp = net_inputs(tag, B, h, w)
    if bf16_storage:
        rnd = lambda t: t.bfloat16().float()
        for mod in m.modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.BatchNorm2d)):
                for prm in mod.parameters(recurse=False):
                    prm.data = rnd(prm.data)
                mod.register_forward_hook(lambda mod, i, o: rnd(o))
        left, right = rnd(left), rnd(right)
    m = m.to(dtype)
    m.train() if mode == "train" else m.eval()
    left, right, seg, disp = (t.to(dtype) for t in (left, right, seg, disp))
    p = "net.%s" % tag
    res = {}
    with torch.set_grad_enabled(mode == "train"):
        heads, outs = harness(m, name, left, right)
        loss = net_loss(name, outs, seg, disp)
    for n, t in zip(HEADS[name], heads):
        res["%s.head.%s" % (p, n)] = sampled(t)
    for n, t in zip(OUTS[name], outs):
        res["%s.out.%s" % (p, n)] = sampled(t)
        res["%s.out.%s.mean" % (p, n)] = np.float64(t.detach().double().mean())
    res["%s.loss" % p] = np.float64(loss.item())
    if mode == "train":
        loss.backward()
        for k, v in G.grad_norms(m).items():
            res["%s.gnorm.%s" % (p, k)] = v
        sd = m.state_dict()
        for k in BN_KEYS[name]:
            res["%s.rm.%s" % (p, k)] = sd[k + ".running_mean"].double().numpy().copy()
            res["%s.rv.%s" % (p, k)] = sd[k + ".running_var"].double().numpy().copy()
    return res


def gen_nets(arrays):
    for tag, name, mode, B, h, w in NETS:
        r32, r64 = both(lambda dt: net_results(tag, name, mode, B, h, w, dt))
        put(arrays, r32, r64)
        p = "net.%s" % tag
        if mode == "eval":
            rb = net_results(tag, name, mode, B, h, w, torch.float32, bf16_storage=True)
            for n in OUTS[name]:
                arrays["%s.bf16dev.%s" % (p, n)] = rel_l2(rb["%s.out.%s" % (p, n)], r64["%s.out.%s" % (p, n)])
        print("net", tag, "loss", r64[p + ".loss"], "max dev", max(float(arrays[k]) for k in arrays if k.startswith(p + ".") and k.endswith(".dev")),
              {k: float(v) for k, v in arrays.items() if k.startswith(p + ".bf16dev")})


def keys():
    out = {}
    for tag, name, ch in (("deeplab_mod19", "deeplab_mod", 19), ("deeplab_mod2", "deeplab_mod", 2), ("deeplab19", "deeplab", 19)):
        m = ref_net(name, ch)
        out[tag] = {"state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()],
                    "parameters": [k for k, _ in m.named_parameters()]}
    return out


def main():
    G._install_stubs()
    arrays = {}
    gen_blocks(arrays)
    gen_nets(arrays)
    arrays["keys"] = np.frombuffer(json.dumps(keys(), separators=(",", ":")).encode(), dtype=np.uint8)
    arrays["meta.corr"] = np.array("assumed-semantics")
    G.save("deeplab", **arrays)


if __name__ == "__main__":
    main()
