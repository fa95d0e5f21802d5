"""EvalStep: the captured forward of test_model (torch_implementation.py:450-582) with eval-mode BatchNorm folded into the packs.

CPU: the preconditions.  GPU, 256x256, B = 2 (the goldens' own size and the networks' minimum): f32 parity with the
reference-captured eval fixtures in the three forms of the step (folded + graph, unfolded + graph, folded + eager) at the
tolerance the existing eval tests use for those fixtures; bf16 within the per-head caps of tests/test_bf16_parity.py;
freshness (a replay sees weights and running statistics edited in place); life beside an armed TrainStep; node inventory.

Reference: models/dsnet_t2.py:1152-1299 (minidsnetExt), :120-330 (dsnet), models_psmnet/stackhourglass.py:86-155."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_models as R
from oracle.detweights import fill_state_dict, rand_input
from test_nets import _check, _net_inputs

GDIR = os.path.join(os.path.dirname(__file__), "golden")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_evalstep_refuses_a_cpu_model():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import SdhipError, nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    m = N.convbn(3, 8, 3, 1, 'same', 1).eval()
    with pytest.raises(SdhipError, match="GPU"):
        EvalStep(m)


def test_evalstep_refuses_a_training_mode_model():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import SdhipError, nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    m = N.convbn(3, 8, 3, 1, 'same', 1).train()
    with pytest.raises(SdhipError, match="training mode"):
        EvalStep(m)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _mini(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    aspp = {"mini_a0": 0, "mini_a1": 1, "mini_a2": 2}[tag]
    m = fill_state_dict(N.minidsnetExt(R.CFG(aspp=aspp), labels=2, patch_type='1dcorr'), 31).cuda().eval()
    a, b, seg, disp = (t.cuda() for t in _net_inputs())
    return m, a, b, seg, disp


def _dsnet():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    m = fill_state_dict(N.dsnet(R.CFG(), labels=2), 61).cuda().eval()
    a, b = rand_input(61, "left", (2, 3, 256, 256)).cuda(), rand_input(61, "right", (2, 3, 256, 256)).cuda()
    seg = F.one_hot((rand_input(61, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float().cuda()
    disp = rand_input(61, "disp", (2, 1, 256, 256), 0.0, 8.0).cuda()
    return m, a, b, seg, disp


def _psm64():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.psmnet import PSMNet
    from test_psmnet import _load_eval_stats
    gold = np.load(os.path.join(GDIR, "psmnet.npz"))
    m = _load_eval_stats(fill_state_dict(PSMNet(64), 41), gold).cuda().eval()
    a, b = rand_input(41, "left", (2, 3, 256, 256)).cuda(), rand_input(41, "right", (2, 3, 256, 256)).cuda()
    return m, a, b, gold


FORMS = {"folded_graph": dict(fold_bn=True, use_graph=True), "unfolded_graph": dict(fold_bn=False, use_graph=True),
         "folded_eager": dict(fold_bn=True, use_graph=False)}


def _done():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    torch.cuda.synchronize()
    assert ops._ctx[0] is None        # the context that was installed before the step (none) is back


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["mini_a0", "mini_a1", "mini_a2"])
def test_hip_evalstep_minidsnet_f32_matches_golden(tag, form):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    gold = np.load(os.path.join(GDIR, "nets.npz"))
    m, a, b, seg, disp = _mini(tag)
    ev = EvalStep(m, dtype=torch.float32, with_loss=True, loss_kwargs=dict(use_lovasz=False), **FORMS[form])
    for _ in range(2):            # the building call and a plain one (a replay, under a graph)
        outs = ev(a, b, seg, disp)
    for i, name in enumerate(("seg1", "disp", "seg2")):
        _check(gold, "%s.eval.%s" % (tag, name), outs[i], 1e-3)
    want = float(gold[tag + ".eval.loss"])
    assert abs(float(outs[-1]) - want) <= 1e-3 * max(1.0, abs(want)), (float(outs[-1]), want)
    assert (ev.graph is not None) == FORMS[form]["use_graph"]
    assert (ev.folded_calls > 0) == FORMS[form]["fold_bn"]
    _done()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_hip_evalstep_dsnet_f32_matches_golden(form):
    """dsnet's fixture loss (negative log-likelihood of its log-probability heads plus both disparity terms) is not the step's
    loss (ops.train_loss: two softmax cross-entropies and one L1): the outputs go against the fixture, the fixture's loss is
    recomputed from them, and the step's loss goes against its own three terms taken from the outputs by torch."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    gold = np.load(os.path.join(GDIR, "dsnet.npz"))
    m, a, b, seg, disp = _dsnet()
    ev = EvalStep(m, dtype=torch.float32, with_loss=True, loss_kwargs=dict(use_lovasz=False), **FORMS[form])
    for _ in range(2):
        outs = ev(a, b, seg, disp)
    for i, name in enumerate(("seg1", "disp", "seg2", "disp2")):
        _check(gold, "dsnet.eval.%s" % name, outs[i], 1e-3)
    ce = lambda y: torch.mean(torch.sum(-seg * F.log_softmax(y.float(), 1), 1))
    want = float(ce(outs[0]) + ce(outs[2]) + F.l1_loss(outs[1].float(), disp))
    assert abs(float(outs[-1]) - want) <= 1e-3 * max(1.0, abs(want)), (float(outs[-1]), want)
    full = float(torch.mean(torch.sum(-seg * outs[0].float(), 1)) + torch.mean(torch.sum(-seg * outs[2].float(), 1)) +
                 F.l1_loss(outs[1].float(), disp) + F.l1_loss(outs[3].float(), disp))
    assert abs(full - float(gold["dsnet.eval.loss"])) <= 1e-3 * max(1.0, float(gold["dsnet.eval.loss"]))
    _done()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("tag", ["a2_hanet_l19", "a0_hanet_l19"])
def test_hip_evalstep_cfg5_f32_matches_golden(tag, form):
    """19 classes + HANet (`pos` travels as the step's extra argument), trained-like running statistics, the cityscapes loss."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    from test_parity_r2 import _cfg5_case
    gold = np.load(os.path.join(GDIR, "cfg5.npz"))
    m, a, b, pos, seg, disp = _cfg5_case(gold, tag, N.minidsnetExt, "cuda")
    ev = EvalStep(m, dtype=torch.float32, with_loss=True, loss_kwargs=dict(use_lovasz=True, mask_invalid_disp=True, ignore_void=True),
                  **FORMS[form])
    for _ in range(2):
        outs = ev(a, b, seg, disp, pos)
    for i, name in enumerate(("seg1", "disp", "seg2")):
        _check(gold, "%s.eval.%s" % (tag, name), outs[i], 1e-3)
    want = float(gold[tag + ".eval.loss"])
    assert abs(float(outs[-1]) - want) <= 1e-3 * max(1.0, want), (float(outs[-1]), want)
    _done()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_hip_evalstep_psmnet_f32_matches_golden(form):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    m, a, b, gold = _psm64()
    ev = EvalStep(m, dtype=torch.float32, **FORMS[form])
    for _ in range(2):
        outs = ev(a, b)
    for i, o in enumerate(outs):
        want = gold["psm64.eval.pred%d.sample" % i]
        got = o.detach().cpu()[:, ::8, ::8].numpy()
        assert got.shape == want.shape
        err = np.abs(got - want)
        assert err.max() <= 1e-3 * max(1.0, np.abs(want).max()), (i, err.max())
    _done()


# ---- bf16: the per-head caps of tests/test_bf16_parity.py for the same fixtures (relative L2 of the strided samples)
def _rel_to_gold(gold, key, t):
    want = gold[key + ".sample"]
    from test_nets import _sample
    got = _sample(t)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    return float(np.linalg.norm(got - want) / max(1e-12, np.linalg.norm(want)))


BF16_MINI = {"mini_a0": (0.03, 0.035, 0.15), "mini_a1": (0.03, 0.035, 0.12), "mini_a2": (0.03, 0.035, 0.29)}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(BF16_MINI))
def test_hip_evalstep_minidsnet_bf16_within_caps(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    gold = np.load(os.path.join(GDIR, "nets.npz"))
    m, a, b, seg, disp = _mini(tag)
    ev = EvalStep(m, dtype=torch.bfloat16, with_loss=True, loss_kwargs=dict(use_lovasz=False))
    for _ in range(2):
        outs = ev(a, b, seg, disp)
    assert outs[0].dtype == torch.bfloat16 and ev.graph is not None and ev.folded_calls > 0
    for i, name in enumerate(("seg1", "disp", "seg2")):
        e = _rel_to_gold(gold, "%s.eval.%s" % (tag, name), outs[i])
        print("evalstep bf16 %s %s rel L2 %.4f (cap %.3f)" % (tag, name, e, BF16_MINI[tag][i]))
        assert e <= BF16_MINI[tag][i], (tag, name, e, BF16_MINI[tag][i])
    want = float(gold[tag + ".eval.loss"])
    assert abs(float(outs[-1]) - want) <= 1e-2 * max(1.0, abs(want)), (float(outs[-1]), want)
    _done()


@pytest.mark.gpu
def test_hip_evalstep_dsnet_bf16_within_caps():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    gold = np.load(os.path.join(GDIR, "dsnet.npz"))
    m, a, b, seg, disp = _dsnet()
    ev = EvalStep(m, dtype=torch.bfloat16)
    for _ in range(2):
        outs = ev(a, b)
    for i, (name, cap) in enumerate((("seg1", 0.03), ("disp", 0.015), ("seg2", 0.02), ("disp2", 0.04))):
        e = _rel_to_gold(gold, "dsnet.eval.%s" % name, outs[i])
        print("evalstep bf16 dsnet %s rel L2 %.4f (cap %.3f)" % (name, e, cap))
        assert e <= cap, (name, e, cap)
    loss = torch.mean(torch.sum(-seg * outs[0].float(), 1)) + torch.mean(torch.sum(-seg * outs[2].float(), 1)) + \
        F.l1_loss(outs[1].float(), disp) + F.l1_loss(outs[3].float(), disp)
    want = float(gold["dsnet.eval.loss"])
    assert abs(float(loss) - want) <= 5e-3 * want, (float(loss), want)
    _done()


@pytest.mark.gpu
def test_hip_evalstep_psmnet64_bf16_within_cap():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    m, a, b, gold = _psm64()
    ev = EvalStep(m, dtype=torch.bfloat16)
    for _ in range(2):
        outs = ev(a, b)
    want = gold["psm64.eval.pred0.sample"]
    got = outs[0].detach().float().cpu()[:, ::8, ::8].numpy()
    e = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print("evalstep bf16 psm64 rel L2 %.4f (cap 0.03)" % e)
    assert e <= 0.03, e
    _done()


# ---- freshness, life beside a TrainStep, node inventory
def _fresh_eager(ctor, sd, a, b):
    """An eager eval forward of a NEW model loaded from `sd` (public modules only, no step context)."""
    m = ctor()
    m.load_state_dict(sd)
    m = m.cuda().eval()
    with torch.no_grad():
        return [o.detach().float().clone() for o in m(a, b)[:3]]


def _close(got, want):
    err = float((got.float() - want).abs().max())
    return err, 1e-3 * max(1.0, float(want.abs().max()))


def _mini_ctor():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    return N.minidsnetExt(R.CFG(aspp=0), labels=2, patch_type='1dcorr')


@pytest.mark.gpu
def test_hip_evalstep_replay_sees_in_place_edits():
    """After the capture: a folded convolution weight, an unfolded DenseNet weight, and running_var / beta of one folded and one
    table BatchNorm are scaled in place.  The next replay equals an eager eval of a fresh model loaded from the same
    state_dict, and differs from the replay before."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    m, a, b, seg, disp = _mini("mini_a0")
    ev = EvalStep(m, dtype=torch.float32)
    ev(a, b)
    before = [o.detach().float().clone() for o in ev(a, b)[:3]]
    assert ev.graph is not None
    block = m.Conv2DownUp3
    conv, fbn = block.c2[0].layers[0].c2d, block.c2[0].layers[1]
    dense = m.resnet_features.resnet_features.denseblock[0].denselayer2
    fold = ev.ctx.fold
    assert (id(conv.weight), id(fbn), 'conv') in fold.layers and fold.layers[(id(conv.weight), id(fbn), 'conv')].ok
    assert not any(id(dense.conv1.weight) == k[0] for k in fold.layers) and any(k[0] == id(dense.norm1) for k in fold.tables)
    with torch.no_grad():
        conv.weight.mul_(1.5)
        dense.conv1.weight.mul_(1.5)
        for bn in (fbn, dense.norm1):
            bn.running_var.mul_(2.0)
            bn.bias.add_(0.25)
    sd = copy.deepcopy(m.state_dict())
    after = [o.detach().float().clone() for o in ev(a, b)[:3]]
    want = _fresh_eager(_mini_ctor, sd, a, b)
    moved = 0
    for got, w, old in zip(after, want, before):
        err, tol = _close(got, w)
        assert err <= tol, (err, tol)
        moved += int(float((got - old).abs().max()) > tol)
    assert moved >= 1
    _done()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_hip_evalstep_follows_hanet_conv1d_weights(graph):
    """HANet hands the kernels a cached (Cout, Cin, k, 1) VIEW of its Conv1d weights, whose pack is cached under the view, not
    under the parameter: the step's pack table must name it all the same.  After the step is built, every HANet Conv1d weight
    (and one BatchNorm1d's running statistics) is edited in place and reloaded by load_state_dict: the next call equals an eager
    eval of a fresh model with that state, and differs from the call before."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    from test_parity_r2 import _cfg5_case
    gold = np.load(os.path.join(GDIR, "cfg5.npz"))
    m, a, b, pos, seg, disp = _cfg5_case(gold, "a0_hanet_l19", N.minidsnetExt, "cuda")
    ev = EvalStep(m, dtype=torch.float32, use_graph=graph)
    ev(a, b, None, None, pos)
    before = [o.detach().float().clone() for o in ev(a, b, None, None, pos)[:3]]
    han = m.hanet_last
    convs = [c for c in han.modules() if isinstance(c, torch.nn.Conv1d)]
    assert len(convs) >= 2
    with torch.no_grad():
        for c in convs:
            c.weight.mul_(-1.5)
        han.attention_first[1].running_var.mul_(2.0)
    sd = copy.deepcopy(m.state_dict())
    m.load_state_dict(sd)                      # in place: the step must follow this as well
    after = [o.detach().float().clone() for o in ev(a, b, None, None, pos)[:3]]
    fresh = N.minidsnetExt(R.CFG(aspp=0, hanet=1), labels=19, patch_type='1dcorr')
    fresh.load_state_dict(sd)
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        want = [o.detach().float().clone() for o in fresh(a, b, pos)[:3]]
    for got, w in zip(after, want):
        err, tol = _close(got, w)
        assert err <= tol, (err, tol)
    err, tol = _close(after[2], before[2])     # the re-weighted head moved
    assert err > tol, (err, tol)
    _done()


@pytest.mark.gpu
def test_hip_fold_tables_are_16_byte_aligned():
    """Odd channel counts: every scale / shift table of FoldState starts on a 16-byte boundary (the convolution prologue reads
    them as f32x4), and holds what sdhip_bn_finalize gives."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    bns = [torch.nn.BatchNorm2d(c).cuda().eval() for c in (5, 7, 3)]
    with torch.no_grad():
        for bn in bns:
            bn.running_var.uniform_(0.5, 2.0); bn.running_mean.normal_(); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
    fold = ops.FoldState(torch.float32, torch.device("cuda"))
    for bn, g in zip(bns, (1, 3, 1)):
        assert fold.table(bn, g) is None
    fold.finish()
    fold._launch(fold.rows())
    for bn, g in zip(bns, (1, 3, 1)):
        sc, sh = fold.table(bn, g)
        assert sc.data_ptr() % 16 == 0 and sh.data_ptr() % 16 == 0 and sc.shape == (g, bn.num_features)
        want = [torch.empty((g, bn.num_features), device="cuda") for _ in range(2)]
        _lib.call("sdhip_bn_finalize", None, 0, 1, _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(bn.running_mean),
                  _lib.ptr(bn.running_var), _lib.ptr(want[0]), _lib.ptr(want[1]), None, None, bn.num_features, g, 1.0, float(bn.eps),
                  0.0, _lib.stream_ptr())
        assert torch.equal(sc, want[0]) and torch.equal(sh, want[1])


@pytest.mark.gpu
def test_hip_evalstep_beside_an_armed_trainstep():
    """TrainStep (graph, Adam, no Lovasz) takes 3 steps, EvalStep 2 calls, TrainStep 1 more.  The eval outputs equal an eager eval
    of a fresh model loaded from the state_dict taken just before them; the state_dict (num_batches_tracked included) and the
    dropout seed are bit-identical across the eval calls; the TrainStep keeps its graph and steps to a finite loss."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    m = fill_state_dict(_mini_ctor(), 31).cuda().train()
    a, b, seg, disp = (t.cuda() for t in _net_inputs())
    ts = TrainStep(m, dtype=torch.float32, use_graph=True, use_lovasz=False, lr=1e-4)
    for _ in range(3):
        ts(a, b, seg, disp)
    graph = ts.graph
    assert graph is not None
    m.eval()
    torch.cuda.synchronize()
    sd = copy.deepcopy(m.state_dict())
    seed = int(ts.ctx.seed.item())
    ev = EvalStep(m, dtype=torch.float32)
    outs = [[o.detach().float().clone() for o in ev(a, b)[:3]] for _ in range(2)]
    torch.cuda.synchronize()
    now = m.state_dict()
    assert set(now) == set(sd) and any(k.endswith("num_batches_tracked") for k in sd)
    for k, v in sd.items():
        assert torch.equal(now[k], v), k
    assert int(ts.ctx.seed.item()) == seed
    want = _fresh_eager(_mini_ctor, sd, a, b)
    for call_outs in outs:
        for got, w in zip(call_outs, want):
            err, tol = _close(got, w)
            assert err <= tol, (err, tol)
    m.train()
    loss = float(ts(a, b, seg, disp))
    assert ts.graph is graph and np.isfinite(loss)
    ops.set_step_context(None)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_hip_evalstep_scores_every_batch_once(graph):
    """metrics=StepMetrics: three calls (under a graph: measuring + capture + replay in the first, two replays) leave exactly the
    counters of three updates on the same outputs - the eager passes that build the step do not count."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.metrics import StepMetrics
    m, a, b, seg, disp = _mini("mini_a0")
    sm, want = StepMetrics(2, max_disp=8.0), StepMetrics(2, max_disp=8.0)
    ev = EvalStep(m, dtype=torch.float32, metrics=sm, use_graph=graph)
    for _ in range(3):
        outs = ev(a, b, seg, disp)
    for _ in range(3):
        want.update(outs[2], seg, outs[1], disp)
    torch.cuda.synchronize()
    (c, s), (wc, ws) = sm.totals(), want.totals()
    assert torch.equal(c, wc) and int(c[:4].sum()) == 3 * 2 * 256 * 256
    assert torch.allclose(s, ws, rtol=1e-12, atol=0)
    _done()


@pytest.mark.gpu
def test_hip_evalstep_failed_capture_is_closed():
    """An exception inside the capture: the capture is ended (sdhip_abort_capture), the previous context is back, torch's CUDA
    generator is usable, and the same step runs eagerly to the fixture's outputs."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    gold = np.load(os.path.join(GDIR, "nets.npz"))
    m, a, b, seg, disp = _mini("mini_a0")
    ev = EvalStep(m, dtype=torch.float32)

    def fault():
        raise RuntimeError("injected")
    ev._capture_fault = fault
    with pytest.raises(RuntimeError, match="injected"):
        ev(a, b)
    _done()
    assert ev.graph is None and not torch.cuda.is_current_stream_capturing()
    torch.randn(8, device="cuda")
    ev.use_graph = False
    outs = ev(a, b)
    for i, name in enumerate(("seg1", "disp", "seg2")):
        _check(gold, "mini_a0.eval.%s" % name, outs[i], 1e-3)
    _done()


@pytest.mark.gpu
def test_hip_evalstep_graph_inventory():
    """Kernel nodes only; every folded layer call saves at least one node against the unfolded captured step; the layers of all
    11 Conv2DownUp blocks of minidsnetExt fold."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, nn as N
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    nodes, evs = {}, {}
    for fold_bn in (True, False):
        m, a, b, seg, disp = _mini("mini_a0")
        ev = EvalStep(m, dtype=torch.bfloat16, fold_bn=fold_bn)
        ev.debug_graph = True
        ev(a, b)
        ev(a, b)
        nodes[fold_bn], evs[fold_bn] = _lib.graph_node_counts(ev.graph), ev
    print("evalstep nodes folded %s unfolded %s folded calls %d" % (nodes[True], nodes[False], evs[True].folded_calls))
    for n in nodes.values():
        assert n["memset"] == 0 and n["memcpy"] == 0, n
    assert evs[False].folded_calls == 0
    assert nodes[True]["kernel"] <= nodes[False]["kernel"] - evs[True].folded_calls, (nodes, evs[True].folded_calls)
    ev, m = evs[True], evs[True].model
    blocks = [mod for mod in m.modules() if isinstance(mod, N.Conv2DownUp)]
    assert len(blocks) == 11
    want = 0
    for blk in blocks:
        for seq in (blk.c1, blk.c2, blk.c3, blk.d3, blk.d4) + ((blk.d5,) if blk.lastLayer else ()):
            layers = seq[0].layers
            w = layers[0].c2d.weight if hasattr(layers[0], "c2d") else layers[0].ct2d.weight
            kind = 'conv' if hasattr(layers[0], "c2d") else 'deconv'
            rec = ev.ctx.fold.layers.get((id(w), id(layers[1]), kind))
            assert rec is not None and rec.ok, (kind, tuple(w.shape))
            want += 1
    assert ev.folded_calls >= want
    _done()
