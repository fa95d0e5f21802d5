"""Fixture generator of `-freeze_bn 1` (train.freeze_bn, TrainStep(freeze_bn=True)): writes tests/golden/freeze_bn.npz.

Runs on the CPU next to a checkout of the reference (SDHIP_REFERENCE, as oracle/make_golden.py), imports the reference's own
networks with the oracle stubs and applies the reference's own freeze loop (networkOutput, torch_implementation.py:235-241):
every nn.BatchNorm2d gets weight.requires_grad = bias.requires_grad = False and eval().  The network is otherwise in train
mode, every dropout has p = 0, B = 2, 256x256, float32.
Networks: minidsnetExt(aspp=0) on DenseNet ("dense"), minidsnetExt(backbone='mobilenet', aspp=2) ("mobile": depthwise, h-swish
and squeeze-excite nodes next to frozen norms) and dsnet ("dsnet": stride-2 transposed convolutions, log-softmax heads).

The state recipe (SEED, stored as `recipe`): oracle.detweights.fill_state_dict(model, SEED) draws gamma in [0.6, 1.4], beta and
every other parameter; then the running statistics are made trained-like as tools/make_golden_warp.py does - every
BatchNorm's momentum is set to 1 for ONE train-mode pass without gradients over the fixture's input (the running statistics
then are the batch statistics of the module's last call, far from 0 / 1: the frozen scale gamma / sqrt(var + eps) is nowhere
near 1, so a wrong or missing scale in a backward pass cannot pass), and the momentum is restored.  With the seed's random
running statistics the frozen network would blow up through its ~120 layers (oracle.make_golden.gen_cfg5).
These networks answer a relative change of 1e-6 in one statistic with up to 1e-3 in a head, so a test cannot re-derive the
statistics with its own kernels: they are rounded to bfloat16 (trained-like is all they have to be) and STORED, two bytes
each, in the order of model.modules() - `<net>.stats.rm` / `.rv` as uint16 bit patterns.
The expected values are those of the reference's own pass, float32 as upstream runs it.  A float64 pass of the same network is
run beside it only to print how far f32 is from it on this state: seg heads and first disparities 2e-5 .. 4e-4 of the head's
maximum, dsnet's second disparity 9e-4 - f32 passes agree with each other much better than with f64 there (their roundings
are correlated), so float64 values would ask of an f32 implementation what the f32 reference does not deliver.
Stored per network: those statistics, strided samples of the outputs, the loss, the gradient norm per top-level submodule,
the ordered names of the parameters without a gradient, the number of frozen norms.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_freeze_bn.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import make_golden as G  # noqa: E402
from oracle import ref_models as R  # noqa: E402
from oracle.detweights import fill_state_dict, rand_input  # noqa: E402

SEED = 47
NETS = ("dense", "mobile", "dsnet")
HEADS = {"dense": ("seg1", "disp", "seg2"), "mobile": ("seg1", "disp", "seg2"), "dsnet": ("seg1", "disp", "seg2", "disp2")}
RECIPE = {"seed": SEED, "batch": [2, 256, 256],
          "state": "fill_state_dict(model, seed); reset_running_stats and momentum = 1 on every BatchNorm; one train-mode "
                   "no-grad pass over (left, right) with every dropout at p = 0; momentum restored; running statistics "
                   "rounded to bfloat16 and stored (<net>.stats.rm / .rv, uint16 bits, model.modules() order)",
          "inputs": "rand_input(seed, 'left' | 'right' | 'seg' (> 0.5 -> one-hot of 2) | 'disp' (0..8))"}


def build(tag):
    from models import dsnet_t2 as D
    if tag == "dense":
        return D.minidsnetExt(R.CFG(aspp=0), labels=2, pretrained=False, patch_type='1dcorr', backbone='densenet')
    if tag == "mobile":
        real = torch.load
        torch.load = lambda *a, **k: {}      # mobilenetv3_large() loads a weight file it never uses (tools/make_golden_mobilenet.py)
        try:
            return D.minidsnetExt(R.CFG(aspp=2), labels=2, pretrained=False, patch_type='1dcorr', backbone='mobilenet')
        finally:
            torch.load = real
    return D.dsnet(R.CFG(), labels=2, pretrained=False)


def inputs():
    a, b = rand_input(SEED, "left", (2, 3, 256, 256)), rand_input(SEED, "right", (2, 3, 256, 256))
    seg = F.one_hot((rand_input(SEED, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float()
    disp = rand_input(SEED, "disp", (2, 1, 256, 256), 0.0, 8.0)
    return a, b, seg, disp


def loss_of(tag, outs, seg, disp):
    if tag == "dsnet":       # log-probability heads and two disparities, as oracle.make_golden.gen_dsnet
        return (torch.mean(torch.sum(-seg * outs[0], 1)) + torch.mean(torch.sum(-seg * outs[2], 1))
                + F.l1_loss(outs[1], disp) + F.l1_loss(outs[3], disp))
    return G.train_loss(outs[:4], seg, disp)


def prepare(model, a, b, seed):
    """The state recipe of the module docstring; returns the model in train mode."""
    fill_state_dict(model, seed)
    for m in model.modules():
        if isinstance(m, (nn.Dropout, nn.Dropout2d, nn.Dropout3d)):
            m.p = 0.0
    bns = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    keep = [m.momentum for m in bns]
    for m in bns:
        m.reset_running_stats()
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(a, b)
    for m, mom in zip(bns, keep):
        m.momentum = mom
        m.running_mean.copy_(m.running_mean.bfloat16().float())
        m.running_var.copy_(m.running_var.bfloat16().float())
    return model


def bf16_bits(ts):
    return torch.cat([t.reshape(-1) for t in ts]).bfloat16().view(torch.int16).numpy().view(np.uint16).copy()


def reference_freeze(model):
    """networkOutput's loop (torch_implementation.py:235-241), verbatim in effect."""
    n = 0
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.requires_grad = False
            m.bias.requires_grad = False
            m.eval()
            n += 1
    return n


def frozen_pass(tag, model, a, b, seg, disp):
    model.train()                       # the epoch loop's model.train() precedes networkOutput's freeze loop
    nfrozen = reference_freeze(model)
    outs = model(a, b)
    loss = loss_of(tag, outs, seg, disp)
    loss.backward()
    return nfrozen, outs, loss


def one(tag, a, b, seg, disp):
    """Fixture entries of one network."""
    arrays = {}
    model = prepare(build(tag), a, b, SEED)
    bns = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    arrays["%s.stats.rm" % tag] = bf16_bits([m.running_mean for m in bns])
    arrays["%s.stats.rv" % tag] = bf16_bits([m.running_var for m in bns])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    nfrozen, outs, loss = frozen_pass(tag, model, a, b, seg, disp)
    after = model.state_dict()
    for k, v in before.items():         # frozen: no running statistic moved (3-D norms: there are none in these networks)
        if "running_" in k or "num_batches" in k:
            assert torch.equal(v, after[k]), k
    for i, name in enumerate(HEADS[tag]):
        arrays.update(G.flat("%s.%s" % (tag, name), G.sample(outs[i], 16)))
    arrays["%s.loss" % tag] = np.float64(loss.item())
    for k, v in G.grad_norms(model).items():
        arrays["%s.gnorm.%s" % (tag, k)] = v
    arrays["%s.nograd" % tag] = np.array([k for k, p in model.named_parameters() if p.grad is None])
    arrays["%s.frozen" % tag] = np.int64(nfrozen)
    print("freeze_bn", tag, "frozen norms", nfrozen, "no-grad parameters", len(arrays["%s.nograd" % tag]), "loss", loss.item())
    outs = [o.detach() for o in outs]
    model.zero_grad(set_to_none=True)
    _, outs64, loss64 = frozen_pass(tag, model.double(), a.double(), b.double(), seg.double(), disp.double())
    for i, name in enumerate(HEADS[tag]):       # information only
        o64 = outs64[i].detach()
        dev = float((outs[i].double() - o64).abs().max()) / max(1.0, float(o64.abs().max()))
        print("  %s.%s: this f32 result is %.2e (max, relative to max(1, |max|)) from the f64 result" % (tag, name, dev))
    print("  loss in f64: %r" % loss64.item())
    return arrays


def main():
    G._install_stubs()
    arrays = {"recipe": np.array(json.dumps(RECIPE)), "nets": np.array(json.dumps(list(NETS))), "meta.corr": np.array("assumed-semantics")}
    a, b, seg, disp = inputs()
    for tag in NETS:
        arrays.update(one(tag, a, b, seg, disp))
    G.save("freeze_bn", **arrays)
    assert os.path.getsize(os.path.join(G.OUT, "freeze_bn.npz")) <= 1 << 20


if __name__ == "__main__":
    main()
