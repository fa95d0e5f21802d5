"""`-freeze_bn 1` (networkOutput, torch_implementation.py:235-241): train.freeze_bn and TrainStep(freeze_bn=True, fold_bn=...).

CPU: the public interface, the exported kernel, the fixture.
GPU: three networks (minidsnetExt on DenseNet, minidsnetExt on MobileNetV3 with ASPP 2, dsnet) against the reference fixture
tests/golden/freeze_bn.npz (tools/make_golden_freeze_bn.py) in four forms - captured step with folded packs, eager step with
folded packs, eager step on the scale / shift tables (fold_bn=False), and a model frozen by hand without a TrainStep - at the
suite's f32 bars (outputs and loss 1e-3, gradient norms per top-level module 2e-2, the parameters without gradient name for
name); the invariants of a frozen step under Adam and SGD; the captured step's node inventory; an EvalStep beside a frozen
TrainStep; bf16 against the f32 fixture.

The fixture's state: fill_state_dict(seed 47) plus trained-like running statistics (the reference's batch statistics of the
fixture's input, rounded to bfloat16), which the fixture stores - these networks amplify a 1e-6 change of one statistic up to
1e-3 in a head, so the statistics cannot be re-derived here.  The expected values are the reference's own float32 pass.

bf16 (test_bf16_*): relative L2 of the heads and of the gradient norms against the f32 fixture.  The folded form gets twice
what the fold_bn=False form reaches in the same run (independent roundings of the same size: weights rounded after scaling
as against the raw output rounded before scaling, the bound of tests/test_fold_kernel.py).  The fold_bn=False form IS the
arithmetic the bf16 path already runs for an eval-mode norm (convolution, raw output rounded to bf16, sdhip_affine_act with
scale / shift that the fold kernel writes bit-equal to sdhip_bn_finalize's): it is held to the heads of a hand-frozen model's
plain bf16 pass, to one bf16 rounding (relative L2 2^-8).  No per-head cap against f32 exists for it: tests/test_bf16_parity.py
has none for train mode, and its eval-mode caps (3 - 15 %) assume the random running statistics of its fixtures - with
trained-like statistics these networks are chaotic in bf16 (that file's docstring: 46 / 9 / 80 % on the cfg5 fixture), and a
frozen network on this fixture is that function.  Measured on one MI355X, relative L2 against the f32 fixture
(seg1, disp, seg2[, disp2]; gradient norms; loss against the f32 loss):
  dense   tables 0.49 / 0.21 / 0.89, 0.12, 6.570 (6.549)    folded 0.49 / 0.21 / 0.89, 0.05, 6.573
  mobile  tables 0.32 / 0.39 / 1.12, 2.66, 33.95 (24.02)    folded 0.33 / 0.23 / 0.37, 0.10, 26.87
  dsnet   tables 0.37 / 1.05 / 0.36 / 1.06, 0.03, 10.283 (10.258)    folded 0.37 / 1.05 / 0.36 / 1.07, 0.04, 10.278
(the folded form keeps the shift in an f32 bias instead of rounding the raw output, mean offset included, to bf16 first)."""
import functools
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_models as R
from oracle.detweights import fill_state_dict, rand_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "freeze_bn.npz")
SEED = 47
NETS = ("dense", "mobile", "dsnet")
HEADS = {"dense": ("seg1", "disp", "seg2"), "mobile": ("seg1", "disp", "seg2"), "dsnet": ("seg1", "disp", "seg2", "disp2")}
BF16_SAME_ARITHMETIC = 2.0 ** -8      # relative L2 between two bf16 runs of the same arithmetic: at most one output rounding


def _gold():
    return np.load(GOLD)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_freeze_bn_sets_exactly_the_reference_state():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import train
    tree = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.BatchNorm3d(5), nn.BatchNorm2d(6, affine=False)),
                         nn.Dropout(0.5), nn.Linear(4, 4)).train()
    before = {k: v.clone() for k, v in tree.state_dict().items()}
    mods = train.freeze_bn(tree)
    assert mods == [tree[1], tree[2][1]]
    for m in mods:
        assert not m.training
    assert not tree[1].weight.requires_grad and not tree[1].bias.requires_grad
    # everything else is as it was: the 3-D norm, the dropout and the containers train, every other parameter wants its gradient
    assert tree.training and tree[2].training and tree[2][0].training and tree[3].training and tree[0].training
    assert tree[2][0].weight.requires_grad and tree[2][0].bias.requires_grad
    assert all(p.requires_grad for p in list(tree[0].parameters()) + list(tree[4].parameters()))
    after = tree.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    tree.train()                    # what the reference's epoch loop does: it unfreezes the mode, so the step re-applies
    assert tree[1].training
    assert train.freeze_bn(tree) == mods and not tree[1].training


def test_bn_frozen_is_a_property_of_the_module():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    bn = nn.BatchNorm2d(4)
    assert not ops.bn_frozen(bn)
    bn.eval()
    assert not ops.bn_frozen(bn)            # eval mode alone: the parameters still want gradients
    bn.weight.requires_grad_(False)
    assert not ops.bn_frozen(bn)
    bn.bias.requires_grad_(False)
    assert ops.bn_frozen(bn)
    bn.train()
    assert not ops.bn_frozen(bn)


def test_header_exports_the_kernel():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    assert "int sdhip_act_out_bwd(const void* gy, int ldg, const void* y, int ldy, void* graw, int ldgr, const float* scale," in text
    assert "sdhip_act_out_bwd" in _lib.SIGNATURES


def test_trainstep_keywords_keep_their_order():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    sig = inspect.signature(TrainStep.__init__)
    names = list(sig.parameters)
    assert names[-2:] == ["loss", "class_weights"]
    assert names[-4:-2] == ["freeze_bn", "fold_bn"]
    assert sig.parameters["freeze_bn"].default is False and sig.parameters["fold_bn"].default is True


def test_dense_block_follows_its_norms():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, densenet, train
    blk = densenet._DenseBlock(2, 8, 2, 4).train()
    assert densenet.block_training(blk) is True
    assert densenet.block_training(blk.eval()) is False         # nothing frozen: the block's own flag, as before
    train.freeze_bn(blk.train())
    assert densenet.block_training(blk) is False                 # all frozen: running statistics although the block trains
    blk.denselayer2.norm1.train()
    with pytest.raises(_lib.SdhipError, match="features.1.*3 of its 4"):
        densenet.block_training(blk, "features.1")


def test_fixture_has_its_keys_and_is_small():
    assert os.path.getsize(GOLD) <= 1 << 20
    g = _gold()
    assert json.loads(str(g["nets"])) == list(NETS)
    recipe = json.loads(str(g["recipe"]))
    assert recipe["seed"] == SEED and recipe["batch"] == [2, 256, 256]
    for tag in NETS:
        for h in HEADS[tag]:
            for leaf in ("sample", "mean", "absmean", "l2"):
                assert "%s.%s.%s" % (tag, h, leaf) in g.files
        assert np.isfinite(float(g[tag + ".loss"]))
        nograd = [str(s) for s in g[tag + ".nograd"]]
        assert int(g[tag + ".frozen"]) > 100 and len(nograd) >= 2 * int(g[tag + ".frozen"])
        assert any(k.startswith(tag + ".gnorm.") for k in g.files)
        rm, rv = _bf16(g[tag + ".stats.rm"]), _bf16(g[tag + ".stats.rv"])
        assert g[tag + ".stats.rm"].dtype == np.uint16 and rm.shape == rv.shape and bool(torch.isfinite(rm).all()) and bool((rv > 0).all())
        assert float(((rv - 1).abs() > 0.1).float().mean()) > 0.8 and float((rm.abs() > 0.01).float().mean()) > 0.8   # trained-like
        sd = _state(tag)                # the native module tree takes them, norm by norm
        assert sum(v.numel() for k, v in sd.items() if k.endswith("running_var")) == rv.numel()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _build(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    if tag == "dense":
        return N.minidsnetExt(R.CFG(aspp=0), labels=2, patch_type='1dcorr')
    if tag == "mobile":
        return N.minidsnetExt(R.CFG(aspp=2), labels=2, patch_type='1dcorr', backbone='mobilenet')
    return N.dsnet(R.CFG(), labels=2)


@functools.lru_cache(maxsize=None)
def _inputs():
    a, b = rand_input(SEED, "left", (2, 3, 256, 256)), rand_input(SEED, "right", (2, 3, 256, 256))
    seg = F.one_hot((rand_input(SEED, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float()
    disp = rand_input(SEED, "disp", (2, 1, 256, 256), 0.0, 8.0)
    return tuple(t.cuda() for t in (a, b, seg, disp))


def _no_dropout(m):
    for x in m.modules():
        if isinstance(x, (nn.Dropout, nn.Dropout2d, nn.Dropout3d)):
            x.p = 0.0
    return m


def _bf16(bits):
    return torch.from_numpy(bits.astype(np.int16)).view(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _state(tag):
    """The fixture's state (on the CPU): seeded parameters, stored running statistics in the order of model.modules()."""
    g = _gold()
    m = fill_state_dict(_build(tag), SEED)
    rm, rv = _bf16(g[tag + ".stats.rm"]), _bf16(g[tag + ".stats.rv"])
    off = 0
    with torch.no_grad():
        for x in m.modules():
            if isinstance(x, nn.modules.batchnorm._BatchNorm):
                n = x.num_features
                x.running_mean.copy_(rm[off:off + n])
                x.running_var.copy_(rv[off:off + n])
                off += n
    assert off == rm.numel() == rv.numel()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _model(tag):
    m = _no_dropout(_build(tag))
    m.load_state_dict(_state(tag))
    return m.cuda().train()


def _loss(tag, outs, seg, disp):
    if tag == "dsnet":
        return (torch.mean(torch.sum(-seg * outs[0].float(), 1)) + torch.mean(torch.sum(-seg * outs[2].float(), 1))
                + F.l1_loss(outs[1].float(), disp) + F.l1_loss(outs[3].float(), disp))
    from test_nets import train_loss
    return train_loss([o for o in outs[:4]], seg, disp)


def _freeze_by_hand(m):
    for x in m.modules():
        if isinstance(x, nn.BatchNorm2d):
            x.weight.requires_grad = False
            x.bias.requires_grad = False
            x.eval()


def _bn_state(m):
    out = {}
    for n, x in m.named_modules():
        if isinstance(x, nn.BatchNorm2d):
            for leaf in ("running_mean", "running_var", "num_batches_tracked", "weight", "bias"):
                out["%s.%s" % (n, leaf)] = getattr(x, leaf).detach().clone()
    return out


def _assert_same(now, before):
    assert set(now) == set(before)
    for k, v in before.items():
        assert torch.equal(now[k], v), k


def _gnorms(named_grads):
    acc = {}
    for k, g in named_grads:
        top = k.split(".")[0]
        acc[top] = acc.get(top, 0.0) + float(g.double().pow(2).sum())
    return {k: float(np.sqrt(v)) for k, v in acc.items()}


def _check_net(gold, tag, outs, loss, gn, nograd):
    from test_nets import _check
    for i, name in enumerate(HEADS[tag]):
        _check(gold, "%s.%s" % (tag, name), outs[i], 1e-3, 16)
    want = float(gold[tag + ".loss"])
    print("freeze_bn %s loss %r (fixture %r)" % (tag, float(loss), want))
    assert abs(float(loss) - want) <= 1e-3 * max(1.0, abs(want)), (float(loss), want)
    wn = {k[len(tag + ".gnorm."):]: float(gold[k]) for k in gold.files if k.startswith(tag + ".gnorm.")}
    assert set(gn) == set(wn), set(gn) ^ set(wn)
    for k, w in wn.items():
        assert abs(gn[k] - w) <= 2e-2 * max(w, 1e-3), (tag, k, gn[k], w)
    assert list(nograd) == [str(s) for s in gold[tag + ".nograd"]]


def _run_step(tag, dtype, graph, fold):
    """One frozen TrainStep (lr 0: every pass sees the fixture's weights) -> (step, outputs, loss)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    m = _model(tag)
    keep = {}

    def loss_fn(outs, s, d):
        keep["outs"] = outs
        return _loss(tag, outs, s, d)
    ts = TrainStep(m, dtype=dtype, lr=0.0, use_graph=graph, freeze_bn=True, fold_bn=fold, loss_fn=loss_fn)
    loss = ts(a, b, seg, disp)
    torch.cuda.synchronize()
    assert (ts.graph is not None) == graph
    return ts, keep["outs"], loss


def _step_figures(ts):
    names = [k for k, _ in ts.model.named_parameters()]
    idle = set(ts.grad_free)
    gn = _gnorms((k, p.grad) for i, (k, p) in enumerate(ts.model.named_parameters()) if i not in idle)
    return gn, [names[i] for i in ts.grad_free]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["graph_folded", "eager_folded", "eager_tables"])
@pytest.mark.parametrize("tag", NETS)
def test_hip_frozen_step_matches_reference_fixture(tag, form):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    before = None
    try:
        ts, outs, loss = _run_step(tag, torch.float32, form == "graph_folded", form != "eager_tables")
        fold = ts.ctx.fold
        assert fold is not None and fold.train and not fold.live
        if form == "eager_tables":
            assert not fold.layers
        else:
            assert len(fold.layers) > 10 and all(r.ok for r in fold.layers.values())
        gn, nograd = _step_figures(ts)
        _check_net(_gold(), tag, outs, loss, gn, nograd)
        before = _state(tag)
        now = {k: v.cpu() for k, v in ts.model.state_dict().items()}
        for k, v in before.items():      # lr 0 and frozen norms: nothing moved at all
            assert torch.equal(now[k], v), k
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", NETS)
def test_hip_hand_frozen_model_matches_reference_fixture(tag):
    """No TrainStep, no keyword: the modules' own state decides.  The DenseNet tower used to follow block.training alone -
    batch statistics, and running statistics that moved."""
    a, b, seg, disp = _inputs()
    m = _model(tag)
    _freeze_by_hand(m)
    before = _bn_state(m)
    outs = m(a, b)
    loss = _loss(tag, outs, seg, disp)
    loss.backward()
    torch.cuda.synchronize()
    _assert_same(_bn_state(m), before)
    gn = _gnorms((k, p.grad) for k, p in m.named_parameters() if p.grad is not None)
    _check_net(_gold(), tag, outs, loss, gn, [k for k, p in m.named_parameters() if p.grad is None])


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_hip_frozen_norms_never_change(optimizer, tmp_path):
    """minidsnetExt: measuring pass, armed pass, capture and one replay with the default rate (SGD: the default weight decay
    too; a capture needs the two eager passes before it)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as ck, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    gold = _gold()
    a, b, seg, disp = _inputs()
    try:
        m = _model("dense")
        # (SGD: the fixture's gradient norm is ~700, the reference's rate of 0.005 leaves the f32 range within three steps)
        kw = dict(lr=1e-6) if optimizer == "sgd" else {}
        ts = TrainStep(m, dtype=torch.float32, use_graph=True, use_lovasz=False, optimizer=optimizer, freeze_bn=True, **kw)
        if optimizer == "sgd":
            assert ts.weight_decay == 1e-4
        norms0 = _bn_state(m)
        params0 = {k: p.detach().clone() for k, p in m.named_parameters()}
        ts.capture(a, b, seg, disp)                   # the measuring pass, one pass on the armed step, the capture
        loss = ts(a, b, seg, disp)                    # one replay
        torch.cuda.synchronize()
        assert ts.steps_done == 3 and ts.graph is not None and np.isfinite(float(loss))
        _assert_same(_bn_state(m), norms0)
        names = [k for k, _ in m.named_parameters()]
        nograd = [str(s) for s in gold["dense.nograd"]]
        assert [names[i] for i in ts.grad_free] == nograd
        for k, p in m.named_parameters():
            if k not in nograd:
                assert not torch.equal(p.detach(), params0[k]), k
            else:
                assert torch.equal(p.detach(), params0[k]), k
        frozen = {id(p) for x in m.modules() if isinstance(x, nn.BatchNorm2d) for p in (x.weight, x.bias)}
        assert len(frozen) == 2 * int(gold["dense.frozen"])
        for p in m.parameters():
            if id(p) in frozen:
                assert not bool(p.grad.any())         # its slice of the flat gradient buffer was never written
        assert float(ts.flat_g.abs().max()) > 0
        if optimizer == "sgd":
            assert ts.live is not None                # the rows weight decay may touch exclude the idle parameters
        # checkpoint: no optimizer state for the frozen parameters, and a bit-equal reload into a fresh frozen step
        state = ck.make_state(ts, 1)
        opt = state["optimizer"]
        idle = set(ts.grad_free)
        assert set(opt["state"]) == set(range(len(names))) - idle and opt["param_groups"][0]["params"] == list(range(len(names)))
        path = ck.save_checkpoint(state, 0.0, 0.0, 1.0, 1.0, filename=str(tmp_path / "frozen"))
        ops.set_step_context(None)
        m2 = _no_dropout(fill_state_dict(_build("dense"), 3)).cuda().train()
        ts2 = TrainStep(m2, dtype=torch.float32, use_graph=True, use_lovasz=False, optimizer=optimizer, freeze_bn=True, **kw)
        ck.load_checkpoint_and_params(path, ts2)
        sd1, sd2 = m.state_dict(), m2.state_dict()
        for k in sd1:
            assert torch.equal(sd1[k], sd2[k]), k
        if optimizer == "sgd":
            assert torch.equal(ts.momentum_buf, ts2.momentum_buf)
        else:
            assert torch.equal(ts.exp_avg, ts2.exp_avg) and torch.equal(ts.exp_avg_sq, ts2.exp_avg_sq) and ts2.steps_done == 3
        assert all(ops.bn_frozen(x) for x in m2.modules() if isinstance(x, nn.BatchNorm2d))
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
def test_hip_model_train_between_eager_steps_does_not_unfreeze():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    try:
        m = _model("dense")
        ts = TrainStep(m, dtype=torch.float32, use_graph=False, use_lovasz=False, freeze_bn=True)
        norms0 = _bn_state(m)
        ts(a, b, seg, disp)
        m.train()                                     # the reference's epoch loop
        assert any(x.training for x in m.modules() if isinstance(x, nn.BatchNorm2d))
        ts(a, b, seg, disp)
        torch.cuda.synchronize()
        assert all(ops.bn_frozen(x) for x in m.modules() if isinstance(x, nn.BatchNorm2d))
        _assert_same(_bn_state(m), norms0)
    finally:
        ops.set_step_context(None)


BN_WORK = ("sdhip_bn_finalize", "sdhip_bn_finalize_bwd", "sdhip_affine_act_bn", "sdhip_bn_bwd_apply", "sdhip_bn_bwd_apply_fin",
           "sdhip_bn_bwd_apply_fin_d", "sdhip_bn_fold_finalize", "sdhip_channel_stats", "sdhip_stats_replica_sum",
           "sdhip_stats_fix_fin", "sdhip_conv2d_fwd_bnpro", "sdhip_conv2d_fwd_bnbwd")


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [True, False], ids=["folded", "tables"])
def test_hip_armed_frozen_step_launches_no_batchnorm_work(fold, monkeypatch):
    """The launches of one armed eager step, by entry point: one batched fold launch at its head, none of the statistics /
    finalize / two-phase backward kernels, and sdhip_act_out_bwd exactly where layers are folded."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import densenet, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import train as T
    a, b, seg, disp = _inputs()
    names = []

    def spy(mod, attr):
        real = getattr(mod, attr)
        monkeypatch.setattr(mod, attr, lambda name, *args: (names.append(name), real(name, *args))[1])
    try:
        ts = T.TrainStep(_model("dense"), dtype=torch.float32, use_graph=False, use_lovasz=False, freeze_bn=True, fold_bn=fold)
        ts(a, b, seg, disp)                           # measuring pass: records layers and table slots
        for mod in (ops, densenet, T):
            spy(mod, "call")
        for mod in (ops, densenet):
            spy(mod, "try_call")
        ts(a, b, seg, disp)
        torch.cuda.synchronize()
        assert names[0] == "sdhip_conv_pack_fold_batch" and names.count("sdhip_conv_pack_fold_batch") == 1
        assert [n for n in names if n in BN_WORK] == []
        nfolded = names.count("sdhip_act_out_bwd")      # one per folded layer call the loss reaches
        assert (nfolded > 10 and len(ts.ctx.fold.layers) > 10) if fold else (nfolded == 0 and not ts.ctx.fold.layers)
        assert len(ts.ctx.fold.tables) > 100
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
def test_hip_half_frozen_dense_block_is_refused():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    try:
        m = _model("dense")
        _freeze_by_hand(m)
        name, blk = next((n, x) for n, x in m.named_modules() if type(x).__name__ == "_DenseBlock")
        blk.denselayer2.norm1.train()
        ts = TrainStep(m, dtype=torch.float32, use_graph=False, use_lovasz=False)
        before = _bn_state(m)
        with pytest.raises(_lib.SdhipError, match="dense block %s" % name.replace(".", r"\.")):
            ts(a, b, seg, disp)
        torch.cuda.synchronize()
        _assert_same(_bn_state(m), before)            # raised before any launch
        with pytest.raises(_lib.SdhipError, match="dense block"):     # and without a step, by the block itself
            m(a, b)
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
def test_hip_frozen_norms_exchange_no_statistics(monkeypatch):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, parallel
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    calls = []
    real = parallel.all_reduce_sum_
    monkeypatch.setattr(parallel, "all_reduce_sum_", lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    try:
        for frozen in (True, False):
            ts = TrainStep(_model("dense"), dtype=torch.float32, use_graph=False, use_lovasz=False, freeze_bn=frozen)
            del calls[:]
            ts.forward_backward(a, b, seg, disp)
            torch.cuda.synchronize()
            if frozen:
                assert calls == []                    # the gradient all-reduce (TrainStep.all_reduce) is the only collective left
            else:
                assert len(calls) > 100               # the counter does see the sync-BN call sites
            ops.set_step_context(None)
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
def test_hip_frozen_graph_has_fewer_kernel_nodes():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    nodes = {}
    try:
        for key, kw in (("unfrozen", {}), ("tables", dict(freeze_bn=True, fold_bn=False)), ("folded", dict(freeze_bn=True))):
            ts = TrainStep(_model("dense"), dtype=torch.bfloat16, use_graph=True, use_lovasz=False, **kw)
            ts.debug_graph = True
            ts.capture(a, b, seg, disp)
            nodes[key] = _lib.graph_node_counts(ts.graph)
            ops.set_step_context(None)
            del ts
        print("freeze_bn graph nodes %s" % nodes)
        for key in ("tables", "folded"):      # kernels only, but for the copy nodes every captured step of this model has
            n = nodes[key]
            assert n["memset"] == 0 and n["other"] == 0 and n["memcpy"] == nodes["unfrozen"]["memcpy"], (key, n)
            assert n["kernel"] + n["memcpy"] == n["total"], (key, n)
        assert nodes["folded"]["kernel"] < nodes["tables"]["kernel"] < nodes["unfrozen"]["kernel"], nodes
    finally:
        ops.set_step_context(None)


@pytest.mark.gpu
def test_hip_evalstep_beside_a_frozen_trainstep():
    """An armed frozen TrainStep and an EvalStep on the same model, replays interleaved: each has its own fold state and packs;
    the eval outputs equal an eager eval of a fresh model with the current weights (1e-3, the bar of
    test_hip_evalstep_beside_an_armed_trainstep)."""
    import copy
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _inputs()
    try:
        m = _model("dense")
        ts = TrainStep(m, dtype=torch.float32, use_graph=True, use_lovasz=False, lr=1e-4, freeze_bn=True)
        for _ in range(2):
            ts(a, b, seg, disp)
        graph = ts.graph
        assert graph is not None
        ev = None
        for _ in range(2):
            m.eval()
            torch.cuda.synchronize()
            sd = copy.deepcopy(m.state_dict())
            if ev is None:
                ev = EvalStep(m, dtype=torch.float32)
                assert ev.ctx.fold is not ts.ctx.fold
            got = [o.detach().float().clone() for o in ev(a, b)[:3]]
            fresh = _no_dropout(_build("dense"))
            fresh.load_state_dict(sd)
            fresh = fresh.cuda().eval()
            with torch.no_grad():
                want = [o.detach().float().clone() for o in fresh(a, b)[:3]]
            for g, w in zip(got, want):
                assert float((g - w).abs().max()) <= 1e-3 * max(1.0, float(w.abs().max()))
            m.train()
            loss = float(ts(a, b, seg, disp))           # the weights move between the two evaluations
            assert ts.graph is graph and np.isfinite(loss)
        assert ev.graph is not None
    finally:
        ops.set_step_context(None)
        torch.cuda.synchronize()


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(1e-12, np.linalg.norm(want)))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", NETS)
def test_bf16_frozen_step_against_the_f32_fixture(tag):
    from test_nets import _sample
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    gold = _gold()
    wn = {k[len(tag + ".gnorm."):]: float(gold[k]) for k in gold.files if k.startswith(tag + ".gnorm.")}
    tops = sorted(wn)
    errs = {}
    try:
        a, b, _, _ = _inputs()
        hand = _model(tag)
        _freeze_by_hand(hand)
        with torch.no_grad():
            plain = [_sample(o, 16) for o in hand(a.bfloat16(), b.bfloat16())[:len(HEADS[tag])]]
        del hand
        for fold in (False, True):
            ts, outs, loss = _run_step(tag, torch.bfloat16, False, fold)
            assert outs[0].dtype == torch.bfloat16
            gn, _ = _step_figures(ts)
            heads = [_rel(_sample(outs[i], 16), gold["%s.%s.sample" % (tag, h)]) for i, h in enumerate(HEADS[tag])]
            grads = _rel(np.array([gn[k] for k in tops]), np.array([wn[k] for k in tops]))
            errs[fold] = (heads, grads, float(loss))
            if not fold:
                same = [_rel(_sample(outs[i], 16), plain[i]) for i in range(len(HEADS[tag]))]
            ops.set_step_context(None)
            del ts
        want = float(gold[tag + ".loss"])
        print("freeze_bn bf16 rel L2 %s: tables heads %s grads %.4f loss %r; folded heads %s grads %.4f loss %r; f32 loss %r"
              % (tag, errs[False][0], errs[False][1], errs[False][2], errs[True][0], errs[True][1], errs[True][2], want))
        print("freeze_bn bf16 %s: fold_bn=False against the hand-frozen model's plain bf16 pass %s" % (tag, same))
        assert max(same) <= BF16_SAME_ARITHMETIC, (tag, "fold_bn=False is not the existing eval arithmetic", same)
        for ef, et, h in zip(errs[True][0], errs[False][0], HEADS[tag]):
            assert ef <= 2 * et, (tag, h, "folded", ef, et)
        assert errs[True][1] <= 2 * errs[False][1], (tag, "gradient norms", errs[True][1], errs[False][1])
    finally:
        ops.set_step_context(None)
