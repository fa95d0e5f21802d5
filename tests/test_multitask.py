"""Uncertainty-weighted multitask loss (`-multaskloss 1|2`, util/utilTorchLoss.py:521-540) and minidsnetExt's multitask modes
(models/dsnet_t2.py:1126-1133,1162-1168,1295-1297): operators against an ATen restatement and the reference fixture
tests/golden/multitask.npz (tools/make_golden_multitask.py), networks, training step and checkpoints."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_models as R
from oracle.detweights import fill_state_dict, rand_input, randn_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("sdhip_mt_seg_fwd", "sdhip_mt_seg_bwd", "sdhip_mt_l1_fwd", "sdhip_mt_l1_bwd")


def _gold():
    return np.load(os.path.join(GDIR, "multitask.npz"))


def _native(mode, classes=2, hanet=0):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    return N.minidsnetExt(R.CFG(aspp=0, multaskloss=mode, hanet=hanet), labels=classes, patch_type='1dcorr')


# ------------------------------------------------------------------ CPU
def test_constructs_both_modes_and_rejects_others():
    for mode in (1, 2):
        m = _native(mode)
        assert m.multiTaskLoss == mode and hasattr(m, "mtloss")
        assert hasattr(m, "mt_convDisp") == (mode == 2) and hasattr(m, "mt_convSeg") == (mode == 2)
        names = [k for k, _ in m.mtloss.named_parameters()]
        assert names == (["log_var_disp", "log_var_seg1", "log_var_seg2"] if mode == 1 else ["log_var_disp", "log_var_seg1"])
    with pytest.raises(NotImplementedError):
        _native(3)


@pytest.mark.parametrize("name,mode,classes", [("mini_mt1", 1, 2), ("mini_mt2", 2, 2), ("mini_mt1_l19", 1, 19)])
def test_state_dict_keys_match_reference(name, mode, classes):
    want = json.loads(str(_gold()["keys"]))[name]
    m = _native(mode, classes)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want["state_dict"]
    assert [k for k, _ in m.named_parameters()] == want["parameters"]


def test_mode0_keys_unchanged():
    with open(os.path.join(GDIR, "keys.json")) as f:
        want = json.load(f)["mini_a0"]
    m = _native(0)
    assert not hasattr(m, "mtloss") and m.multiTaskLoss == 0
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want["state_dict"]
    assert [k for k, _ in m.named_parameters()] == want["parameters"]


def test_new_symbols_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_null_arguments_are_rejected_without_gpu_work():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    rc = _lib._lib.sdhip_mt_seg_fwd(None, 2, None, None, None, None, None, None, 16, 2, 19, 1.0, 0, None)
    assert rc == _lib.ERR_ARG
    rc = _lib._lib.sdhip_mt_l1_bwd(None, 1, None, None, None, 0, None, 1.0, None, 1, None, 16, 0, None)
    assert rc == _lib.ERR_ARG


# ------------------------------------------------------------------ GPU: operators
def _aten(disp, disp_gt, seg, lab, lvs):
    """The reference's multiTask_loss restated in ATen (f32), invalid labels mapped to the ignore index."""
    C = seg.shape[1]
    lab = torch.where((lab >= 0) & (lab < C), lab, torch.full_like(lab, 19))
    ld = torch.exp(-lvs[0]) * F.l1_loss(disp.float(), disp_gt, reduction='none') + lvs[0]
    ce = F.cross_entropy(seg.float(), lab, ignore_index=19, reduction='none')
    ls = torch.exp(-lvs[1]) * ce + lvs[1]
    return ld, ls


def _slab(x, C, k, ld):
    """x (B,C,H,W) as channels [k, k+C) of an NHWC slab with pixel stride ld; the rest of the slab holds a sentinel."""
    B, _, H, W = x.shape
    slab = torch.full((B, H, W, ld), 7.0, dtype=x.dtype, device=x.device)
    slab[..., k:k + C] = x.permute(0, 2, 3, 1)
    return slab, slab[..., k:k + C].permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 19])
@pytest.mark.parametrize("gmode", ["mean", "map", "sum"])
def test_operators_match_aten(dtype, C, gmode):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    B, H, W = 3, 13, 21                               # 819 pixels: not a multiple of the 256-pixel workgroup
    g = torch.Generator().manual_seed(C * 7 + len(gmode))
    logits = (torch.randn(B, C, H, W, generator=g) * 2).to(dtype).float()
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.15] = 19
    lab[0, 0, :3] = torch.tensor([-1, C + 3, 100])    # invalid labels: ignored, never used as an index
    lab[2] = 19                                       # an all-ignored image
    disp = (torch.rand(B, 1, H, W, generator=g) * 8).to(dtype).float()
    disp_gt = torch.rand(B, 1, H, W, generator=g) * 8
    disp_gt.view(-1)[::11] = disp.view(-1)[::11]      # ties: sign(0) = 0
    upstream = torch.rand(B, H, W, generator=g) + 0.5
    for lv_d, lv_s in ((0.3, -0.45), (-0.6, 0.2)):
        # ATen restatement on the bf16-rounded inputs, in f32
        lvs = [torch.tensor([lv_d], requires_grad=True), torch.tensor([lv_s], requires_grad=True)]
        xr = logits.clone().requires_grad_(True)
        dr = disp.clone().requires_grad_(True)
        ld_r, ls_r = _aten(dr, disp_gt, xr, lab, lvs)
        if gmode == "mean":
            (ld_r.mean() + ls_r.mean()).backward()
        elif gmode == "sum":
            (ld_r.sum() + ls_r.sum()).backward()
        else:
            (ld_r * upstream[:, None]).sum().backward()
            (ls_r * upstream).sum().backward()
        # native: logits as a channel slice (ld > C) of a slab, disparity as a dense map
        ld = 24 if C == 19 else 6
        slab, xv = _slab(logits.to(dtype).cuda(), C, 3, ld)
        xv.requires_grad_(True)
        dv = disp.to(dtype).cuda().requires_grad_(True)
        p_d = torch.nn.Parameter(torch.tensor([lv_d], device="cuda"))
        p_s = torch.nn.Parameter(torch.tensor([lv_s], device="cuda"))
        before = slab.clone()
        m_d = ops.multitask_l1_loss(dv, disp_gt.cuda(), p_d)
        m_s = ops.multitask_seg_loss(xv, lab.cuda(), p_s)
        if gmode == "mean":
            (ops.loss_map_mean(m_d) + ops.loss_map_mean(m_s)).backward()
        elif gmode == "sum":
            (m_d.sum() + m_s.sum()).backward()
        else:
            (m_d * upstream[:, None].cuda()).sum().backward()
            (m_s * upstream.cuda()).sum().backward()
        assert torch.equal(slab, before)              # the forward read the slice and wrote nothing into the slab
        rt = 1e-5 if dtype == torch.float32 else 1e-4
        for got, want in ((m_d, ld_r), (m_s, ls_r)):
            np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=rt, atol=rt)
        assert abs(float(ops.loss_map_mean(m_s)) - float(ls_r.mean())) <= rt * max(1.0, abs(float(ls_r.mean())))
        assert abs(float(ops.loss_map_mean(m_d)) - float(ld_r.mean())) <= rt * max(1.0, abs(float(ld_r.mean())))
        gt_x = 1e-5 if dtype == torch.float32 else 1e-2      # bf16 gradients: one bf16 rounding of the result
        np.testing.assert_allclose(xv.grad.float().cpu().numpy(), xr.grad.numpy(), rtol=gt_x, atol=gt_x * float(xr.grad.abs().max()))
        np.testing.assert_allclose(dv.grad.float().cpu().numpy(), dr.grad.numpy(), rtol=gt_x, atol=gt_x * float(dr.grad.abs().max()))
        assert (xv.grad.float()[2] == 0).all()           # the all-ignored image
        for p, r in ((p_d, lvs[0]), (p_s, lvs[1])):
            assert abs(float(p.grad) - float(r.grad)) <= 1e-4 * max(1.0, abs(float(r.grad))), (float(p.grad), float(r.grad))


@pytest.mark.gpu
def test_gradient_rows_touch_only_their_channels():
    """The backward pass writes the C logical channels of each gradient row and nothing else: a gradient handed back as a
    channel slice of a wider buffer is produced by autograd, but the kernel contract is checked directly here."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    B, C, H, W, ldx, k = 2, 19, 9, 31, 24, 2
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(B, H, W, C, device="cuda").to(dtype).contiguous()
        lab = torch.randint(0, C, (B, H, W), device="cuda")
        lv = torch.tensor([0.1], device="cuda")
        m = torch.empty(B, H, W, device="cuda"); lse = torch.empty_like(m)
        s = torch.zeros(1, dtype=torch.float64, device="cuda")
        call("sdhip_mt_seg_fwd", ptr(x), C, ptr(lab), ptr(lv), ptr(m), ptr(lse), ptr(s), None, B * H * W, C, 19, 1.0,
             _lib.dtype_code(x), stream_ptr())
        gslab = torch.full((B, H, W, ldx), 5.0, dtype=dtype, device="cuda")
        gv = gslab[..., k:k + C]
        call("sdhip_mt_seg_bwd", ptr(x), C, ptr(lab), ptr(lse), ptr(lv), None, 0, ptr(torch.ones((), device="cuda")), 1.0,
             ctypes.c_void_p(gv.data_ptr()), ldx, None, B * H * W, C, 19, _lib.dtype_code(x), stream_ptr())
        torch.cuda.synchronize()
        assert (gslab[..., :k] == 5).all() and (gslab[..., k + C:] == 5).all()
        want = torch.exp(-lv) * (torch.softmax(x.float(), -1) - F.one_hot(lab, C).float())
        assert float((gv.float() - want).abs().max()) < (1e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["t1_c2", "t1_c19", "t2_c2", "t2_c19"])
def test_module_matches_reference_fixture(tag):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden_multitask import loss_inputs      # the seeded inputs only (no reference code is imported)
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.multitask import multiTask_loss, step_loss
    gold = _gold()
    three_out, lvs, disp, disp_gt, seg1, seg2, lab = loss_inputs(tag)
    m = multiTask_loss(three_out).cuda()
    with torch.no_grad():
        for name, v in zip(("log_var_disp", "log_var_seg1", "log_var_seg2"), lvs):
            if hasattr(m, name):
                getattr(m, name).fill_(v)
    xs = [t.cuda().requires_grad_(True) for t in (disp, seg1, seg2)]
    ld, l1, l2 = m(xs[0], disp_gt.cuda(), xs[1], xs[2], lab.cuda())
    step_loss(ld, l1, l2).backward()
    p = "loss.%s" % tag
    for name, t in (("ld", ld), ("l1", l1), ("l2", l2)):
        np.testing.assert_allclose(t.detach().cpu().numpy(), gold["%s.%s" % (p, name)], rtol=1e-5, atol=1e-5)
    for name, t in zip(("disp", "seg1", "seg2"), xs):
        want = gold["%s.grad.%s" % (p, name)]
        got = t.grad.cpu().numpy() if t.grad is not None else np.zeros_like(want)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max() + 1e-30))
    for name, prm in m.named_parameters():
        assert abs(float(prm.grad) - float(gold["%s.grad.%s" % (p, name)][0])) <= 1e-4, name


# ------------------------------------------------------------------ GPU: networks
def _net_inputs(void):
    a, b = rand_input(31, "left", (2, 3, 256, 256)), rand_input(31, "right", (2, 3, 256, 256))
    disp = rand_input(31, "disp", (2, 1, 256, 256), 0.0, 8.0)
    if void:
        cls = (rand_input(31, "cls", (2, 256, 256)) * 20).long().clamp(0, 19)
        seg = F.one_hot(cls, 20).permute(0, 3, 1, 2).float().contiguous()
    else:
        seg = F.one_hot((rand_input(31, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float()
    return a.cuda(), b.cuda(), seg.cuda(), disp.cuda()


def _check(gold, key, t, tol):
    from test_nets import _check as chk
    chk(gold, key, t if t.dim() == 4 else t.reshape(t.shape[0], 1, *t.shape[-2:]), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,mode,classes,tm,void", [("mt1", 1, 2, "train", False), ("mt1", 1, 2, "eval", False),
                                                      ("mt1_l19", 1, 19, "train", True), ("mt2", 2, 2, "train", False),
                                                      ("mt2", 2, 2, "eval", False)])
def test_network_matches_reference_fixture(tag, mode, classes, tm, void):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.multitask import step_loss
    gold = _gold()
    a, b, seg, disp = _net_inputs(void)
    m = fill_state_dict(_native(mode, classes), 31).cuda()
    m.train() if tm == "train" else m.eval()
    outs = m(a, b, None, disp, seg.argmax(1))
    loss = step_loss(outs[4], outs[5], outs[6])
    assert len(outs) == 7
    loss.backward()
    p = "%s.%s" % (tag, tm)
    for i, name in enumerate(("seg1", "disp", "seg2")):
        _check(gold, "%s.%s" % (p, name), outs[i], 1e-3)
    for i, name in zip((4, 5), ("ld", "l1")) if mode == 2 else zip((4, 5, 6), ("ld", "l1", "l2")):
        _check(gold, "%s.%s" % (p, name), outs[i], 1e-3)
    want = float(gold[p + ".loss"])
    assert abs(float(loss) - want) <= 1e-3 * max(1.0, abs(want)), (float(loss), want)
    sd = m.state_dict()
    for k in ("resnet_features.resnet_features.norm5", "resnet_features.branch0_0.1.layers.1", "conv2d_ba0.0.layers.1"):
        for s, leaf in (("rm", "running_mean"), ("rv", "running_var")):
            np.testing.assert_allclose(sd["%s.%s" % (k, leaf)].cpu().numpy(), gold["%s.%s.%s" % (p, s, k)], rtol=1e-3, atol=1e-4)
    acc = {}
    for k, q in m.named_parameters():
        if q.grad is not None:
            top = k.split(".")[0]
            acc[top] = acc.get(top, 0.0) + float(q.grad.double().pow(2).sum())
    for top, v in acc.items():
        key = "%s.gnorm.%s" % (p, top)
        w = float(gold[key]) if key in gold.files else 0.0
        assert abs(np.sqrt(v) - w) <= 2e-2 * max(w, 1e-3), (key, np.sqrt(v), w)
    for k, prm in m.mtloss.named_parameters():
        want = float(gold["%s.lvgrad.%s" % (p, k)][0])
        assert abs(float(prm.grad) - want) <= 1e-4 * max(1.0, abs(want)), (k, float(prm.grad), want)
    nograd = set(str(x) for x in gold[p + ".nograd"]) - {""}
    for k, q in m.named_parameters():
        if k in nograd:   # reference: grad None; here the parameter gets exactly zero (or no) gradient
            assert q.grad is None or not bool(q.grad.any()), k
    if tag == "mt1":      # the network outputs are those of the plain network with the same weights
        nets = np.load(os.path.join(GDIR, "nets.npz"))
        for i, name in enumerate(("seg1", "disp", "seg2")):
            _check(nets, "mini_a0.%s.%s" % (tm, name), outs[i], 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("size_in,size_out", [((8, 8), (256, 256)), ((2, 4), (128, 256)), ((16, 8), (128, 64)), ((37, 23), (100, 60))])
def test_resize_backward_matches_aten(mode, size_in, size_out):
    """F.interpolate backward at large factors (mode 2's x32 heads, the x16-x64 pyramid branches): every destination that
    samples a source pixel contributes to its gradient (align_corners=False shifts the bilinear window by half a pixel)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *size_in, generator=g)
    gy = torch.randn(2, 3, *size_out, generator=g)
    xr = x.clone().requires_grad_(True)
    F.interpolate(xr, size=size_out, mode=mode).backward(gy)
    xv = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.interpolate(xv, size=size_out, mode=mode)
    np.testing.assert_allclose(y.detach().cpu().numpy(), F.interpolate(x, size=size_out, mode=mode).numpy(), rtol=1e-5, atol=1e-5)
    y.backward(gy.cuda())
    np.testing.assert_allclose(xv.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_mode1_with_hanet_runs():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.multitask import step_loss
    a, b, seg, disp = _net_inputs(True)
    m = fill_state_dict(_native(1, 19, hanet=1), 31).cuda().eval()
    outs = m(a, b, None, disp, seg.argmax(1))
    loss = step_loss(outs[4], outs[5], outs[6])
    loss.backward()
    assert len(outs) == 7 and bool(torch.isfinite(loss))
    assert any(p.grad is not None and bool(p.grad.any()) for p in m.hanet_last.parameters())
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.mtloss.parameters())


# ------------------------------------------------------------------ GPU: training
def _model(mode):
    torch.manual_seed(0)
    return fill_state_dict(_native(mode), 5).cuda().train()


def _batch():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch
    return synthetic_batch(2, 256, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_graph_replay_matches_eager(mode):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    losses = {}
    for graph in (False, True):
        ts = TrainStep(_model(mode), dtype=torch.float32, use_graph=graph, lr=1e-4)
        if graph:
            ts.capture(*batch, warmup=2)
            seq = [float(ts(*batch)) for _ in range(2)]
        else:
            seq = [float(ts(*batch)) for _ in range(5)][2:4]
        losses[graph] = seq
        ops.set_step_context(None)
    assert abs(losses[False][0] - losses[True][0]) <= 2e-3 * max(1.0, abs(losses[False][0])), losses
    assert abs(losses[False][1] - losses[True][1]) <= 2e-2 * max(1.0, abs(losses[False][1])), losses


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_replays_stay_finite_and_move_log_variances(mode):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    m = _model(mode)
    ts = TrainStep(m, dtype=torch.bfloat16, use_graph=True, lr=1e-3)
    ts.debug_graph = True
    float(ts(*batch))                                   # warm-up + capture + first replay
    names = [k for k, _ in m.named_parameters()]
    idle = [names[i] for i in ts.grad_free]
    # never reached by the loss, as in the reference (no gradient, no Adam state): conv2d_ba3 (computed, never used), the
    # 1/4-scale pyramid branches and the DenseNet classifier; in mode 2 the whole decoder.  The loss is always reached
    assert not any(k.startswith(("mtloss.", "mt_conv")) for k in idle), idle
    assert any(k.startswith("conv2d_ba3.") for k in idle) and (len(idle) > 100) == (mode == 2), idle
    params = dict(m.named_parameters())
    frozen = {k: params[k].detach().clone() for k in idle}
    lvs = dict(m.mtloss.named_parameters())
    off = {k: (p.data_ptr() - ts.flat_p.data_ptr()) // 4 for k, p in lvs.items()}
    lv0 = {k: float(p) for k, p in lvs.items()}
    losses = []
    for _ in range(20):
        before = {k: float(p) for k, p in lvs.items()}
        losses.append(float(ts(*batch)))
        for k, p in lvs.items():
            # every replay reads the log-variance Adam just wrote and moves it against its gradient's running mean
            # (Adam's first moment, which the replay's own gradient has just entered: the seg term's gradient changes sign
            # while the head learns, so the sign of one early gradient is not a bound on 20 steps)
            g, mom = float(p.grad), float(ts.exp_avg[off[k]])
            assert g != 0 and mom != 0 and (float(p) - before[k]) * mom < 0, (k, before[k], float(p), g, mom)
    ops.set_step_context(None)
    assert all(np.isfinite(losses)), losses
    assert ts.graph is not None and _lib.graph_node_counts(ts.graph)["memset"] == 0
    assert all(abs(float(p) - lv0[k]) > 1e-3 for k, p in lvs.items())
    for k in idle:
        assert torch.equal(params[k].detach(), frozen[k]), k


@pytest.mark.gpu
def test_gradient_accumulation_matches_reference_rule():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batches = [synthetic_batch(2, 256, 256, seed=100 + i) for i in range(2)]
    ref = TrainStep(_model(1), dtype=torch.float32, use_graph=False, lr=0.0)
    gsum = torch.zeros_like(ref.flat_g)
    for b in batches:
        ref(*b)
        gsum += ref.flat_g
    w0 = ref.flat_p.clone()
    ops.set_step_context(None)
    p = w0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-7)
    p.grad = gsum / 2
    opt.step()
    ts = TrainStep(_model(1), dtype=torch.float32, use_graph=False, lr=1e-3, accumulate=2)
    for b in batches:
        ts(*b)
    ops.set_step_context(None)
    assert ts.steps_done == 1
    d_want, d_got = (p.detach() - w0), (ts.flat_p - w0)
    assert float((d_got - d_want).norm() / d_want.norm()) < 2e-2
    assert float((ts.flat_g / 2 - gsum / 2).norm() / (gsum / 2).norm()) < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_checkpoint_round_trip_continues_the_run(mode, tmp_path):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, checkpoint as ck
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    a = TrainStep(_model(mode), dtype=torch.float32, use_graph=False, lr=1e-4)
    for _ in range(3):
        a(*batch)
    path = ck.save_checkpoint(ck.make_state(a, 1), 0.0, 0.0, 1.0, 1.0, filename=str(tmp_path / "mt"))
    state = torch.load(path, weights_only=False)
    n_params = len(list(a.model.parameters()))
    # torch keeps no Adam state for parameters that never had a gradient (mode 2: the whole decoder)
    assert len(state["optimizer"]["state"]) == n_params - len(a.grad_free) and a.grad_free
    assert any(k.startswith("module.mtloss.") for k in state["state_dict"])
    want = [float(a(*batch)) for _ in range(2)]
    ops.set_step_context(None)
    b = TrainStep(fill_state_dict(_native(mode), 77).cuda().train(), dtype=torch.float32, use_graph=False, lr=1e-4)
    ck.load_checkpoint_and_params(path, b)
    got = [float(b(*batch)) for _ in range(2)]
    ops.set_step_context(None)
    assert abs(got[0] - want[0]) <= 2e-3 * max(1.0, abs(want[0])), (got, want)
    assert abs(got[1] - want[1]) <= 2e-2 * max(1.0, abs(want[1])), (got, want)


@pytest.mark.gpu
def test_reference_shaped_mode2_optimizer_state_loads():
    """A reference-written mode-2 optimizer state: torch.optim.Adam over the reference's parameters after one step, with
    no state for the parameters that never had a gradient."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, checkpoint as ck
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    gold = _gold()
    nograd = set(str(x) for x in gold["mt2.train.nograd"]) - {""}
    m = _model(2)
    names = [k for k, _ in m.named_parameters()]
    params = [torch.zeros_like(p) for p in m.parameters()]
    for q, k in zip(params, names):
        q.grad = None if k in nograd else torch.full_like(q, 0.5)
    opt = torch.optim.Adam(params, lr=0.0015, eps=1e-7)
    opt.step()
    sd = opt.state_dict()
    assert len(sd["state"]) == len(names) - len(nograd)
    ts = TrainStep(m, dtype=torch.float32, use_graph=False, lr=1e-4)
    ck.load_optimizer_state(ts, sd)
    assert ts.steps_done == 1
    slices = ck._param_slices(m)
    for i, (k, p, off, n) in enumerate(slices):
        want = 0.0 if k in nograd else float(sd["state"][i]["exp_avg"].reshape(-1)[0])
        assert float(ts.exp_avg[off]) == pytest.approx(want), k
    loss = float(ts(*_batch()))
    ops.set_step_context(None)
    assert np.isfinite(loss)
