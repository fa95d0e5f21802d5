"""Segmentation loss terms of `-loss` / `-segWeight` (losses/multiLosses.py:8-128): dice_loss, diceEntropy, tversky_loss2 and
the class-weighted cross-entropy on the kernels of csrc/segloss.hip, against the reference's own lossSeg_fn
(tests/golden/segloss.npz and segloss_big.npz, tools/make_golden_segloss.py) in f32 and a torch restatement in bf16.

f32 bars: loss within 1e-5 * max(1, |want|); every gradient element within 1e-6 absolute AND 1e-5 * max |want| (the
reference's own f32 run deviates from its f64 run by at most 3.6e-7 * max |grad| and 9e-8 relative in the loss on these
shapes: `dev.worst` of the fixture).  bf16 bar: 2e-2 (tests/test_train.py)."""
import ctypes
import functools
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_models as R
from oracle.detweights import fill_state_dict, randn_input
from oracle.losses_ref import lovasz_softmax_onehot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("sdhip_seg_terms_workspace_bytes", "sdhip_seg_sums", "sdhip_seg_finish", "sdhip_seg_terms_bwd")
SEED = 53                 # tools/make_golden_segloss.py
LISTS = (("dice_loss",), ("tversky_loss2",), ("diceEntropy",), ("cross_entropy", "lovasz_loss", "dice_loss"),
         ("cross_entropy", "tversky_loss2"), ("cross_entropy",), ("dice_loss", "diceEntropy"),
         ("lovasz_loss", "tversky_loss2", "diceEntropy"))
BIG_LISTS = (("dice_loss",), ("diceEntropy",), ("cross_entropy", "tversky_loss2"))
SMALL, BIG = ("roses", "roses_sat", "garden", "city"), ("roses_big", "city_big")
ACCEPTED = ("cross_entropy", "lovasz_loss", "tversky_loss2", "dice_loss", "diceEntropy")
NOT_BUILT = ("tversky_loss", "area_ce", "area_hinge", "binary_ce", "categoricalNlll", "ohm_loss", "dual_edge_reg")
STEP_LIST = ("cross_entropy", "lovasz_loss", "dice_loss")
CASE_LISTS = [(c, l) for c in SMALL for l in LISTS] + [(c, l) for c in BIG for l in BIG_LISTS]


def _tag(names):
    return "+".join(names)


class _Gold:
    """Both fixture files behind one lookup that follows the `aliases` of bit-identical arrays."""

    def __init__(self):
        self.files = [np.load(os.path.join(GDIR, n)) for n in ("segloss.npz", "segloss_big.npz")]
        self.aliases = {}
        for f in self.files:
            self.aliases.update(json.loads(str(f["aliases"])))
        self.cases = json.loads(str(self.files[0]["cases"]))

    def __contains__(self, key):
        key = self.aliases.get(key, key)
        return any(key in f.files for f in self.files)

    def __getitem__(self, key):
        key = self.aliases.get(key, key)
        for f in self.files:
            if key in f.files:
                return f[key]
        raise KeyError(key)


@functools.lru_cache(None)
def _gold():
    return _Gold()


@functools.lru_cache(None)
def _inputs(case):
    """(logits, one-hot target of C channels with all-zero void rows, class weights, ignore_void) on the CPU, f32."""
    g = _gold()
    ds, C, Ct, B, H, W, sigma = g.cases[case]
    z = torch.from_numpy(g["%s.z" % case]) if case in SMALL else randn_input(SEED, "%s:z" % case, (B, C, H, W), sigma)
    lab = torch.from_numpy(g["%s.lab" % case].astype(np.int64))
    t = F.one_hot(lab, Ct).permute(0, 3, 1, 2).float()[:, :C].contiguous()
    return z, t, torch.from_numpy(g["weights.%s" % ds]), Ct != C


def _restate(z, t, names, w=None, ignore_void=False):
    """The table of lossSeg_fn's terms in plain torch (f32)."""
    z = z.float()
    B, C, H, W = z.shape
    lp, p = F.log_softmax(z, 1), torch.softmax(z, 1)
    wv = torch.ones(C) if w is None else w.float()
    ce = "cross_entropy" in names
    w1 = 0.5 if ce and len(names) > 2 else 1.0
    total = z.sum() * 0.0
    if ce:
        total = total + w1 * torch.mean(torch.sum(-t * lp * wv.view(1, C, 1, 1), 1))
    if "lovasz_loss" in names:
        total = total + w1 * lovasz_softmax_onehot(z, t, ignore_void)
    TP, P, G = (t * p).sum((2, 3)), p.sum((2, 3)), t.sum((2, 3))
    if "tversky_loss2" in names:
        tv = 1.0 - TP / (TP + (G - TP) + 0.3 * (P - TP) + 1e-6)
        total = total + 1.5 * (tv.mean(0) * wv).mean()
    dl = (G > 1).float() - 2.0 * TP / (P + G + 1.0)
    if "dice_loss" in names:
        total = total + dl.mean()
    elif "diceEntropy" in names:
        total = total + torch.mean(torch.sum(-t * lp * (10.0 * dl).view(B, C, 1, 1), 1))
    return total


def _restate_grad(z, t, names, w, ignore_void):
    x = z.clone().requires_grad_(True)
    loss = _restate(x, t, names, w, ignore_void)
    loss.backward()
    return float(loss.detach()), x.grad


def _run(z, t, names, w, ignore_void, dtype=torch.float32):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    x = z.cuda().to(dtype).requires_grad_(True)
    loss = ops.seg_loss(x, t.cuda(), names, None if w is None else w.cuda(), ignore_void)
    loss.backward()
    return loss.detach(), x.grad


def _check_f32(loss, grad, want_loss, want_grad, what):
    gerr, gmax = float((grad - want_grad).abs().max()), float(want_grad.abs().max())
    lerr = abs(float(loss) - float(want_loss))
    print("%s: loss %.8g want %.8g (err %.2e)  grad err %.2e  max|grad| %.3e" % (what, float(loss), float(want_loss), lerr, gerr, gmax))
    assert lerr <= 1e-5 * max(1.0, abs(float(want_loss))), what
    assert gerr <= 1e-6 and gerr <= 1e-5 * gmax, what


# ------------------------------------------------------------------ CPU
def test_fixture_keys_present():
    g = _gold()
    assert set(g.cases) == set(SMALL + BIG)
    for case, names in CASE_LISTS:
        ds, C, Ct, B, H, W, _ = g.cases[case]
        assert g["weights.%s" % ds].shape == (C,)
        assert g["%s.lab" % case].shape == (B, H, W)
        for sw in (0, 1):
            key = "%s.%s.sw%d" % (case, _tag(names), sw)
            assert g[key + ".grad"].shape == (B, C, H, W) and g[key + ".loss"].shape == (), key
            if "lovasz_loss" not in names:
                assert (g[key + ".dev"] < 1e-6).all(), key
    assert (g["dev.worst"] < 1e-6).all()
    assert not np.allclose(g["weights.cityscapes"], 1.0) and np.all(g["weights.roses"] == 1.0)
    _, t, _, _ = _inputs("garden")
    counts = t.sum((2, 3))
    assert counts[0, 7] == 1 and counts[1, 6] == 2 and counts[:, 8].sum() == 0       # G > 1 is false at 1, true at 2
    _, t, _, void = _inputs("city")
    assert void and (t.sum(1) == 0).any()                                           # void rows
    for k in ("city.z1", "city.seg1.sw1.loss", "city.seg1.sw1.grad", "city.disp", "city.disp_gt", "city.l1.loss", "city.l1.grad"):
        assert k in g, k
    for n in ("segloss.npz", "segloss_big.npz"):
        assert os.path.getsize(os.path.join(GDIR, n)) <= 1 << 20, n


def test_list_names():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    assert tuple(ops.SEG_LOSS_TERMS) == ACCEPTED and tuple(ops.SEG_LOSS_NOT_BUILT) == NOT_BUILT
    for n in ACCEPTED:
        ops.seg_loss_plan([n])
    for n in NOT_BUILT:
        with pytest.raises(NotImplementedError, match=n):
            ops.seg_loss_plan(["cross_entropy", n])
    for n in ("dice", "smooth_grad", "Cross_Entropy", ""):
        with pytest.raises(ValueError):
            ops.seg_loss_plan([n])
    T, D, E = _lib.SEG_TVERSKY, _lib.SEG_DICE, _lib.SEG_DICE_ENTROPY
    assert ops.seg_loss_plan(("cross_entropy",)) == (1.0, 0.0, 0)
    assert ops.seg_loss_plan(("cross_entropy", "lovasz_loss")) == (1.0, 1.0, 0)
    assert ops.seg_loss_plan(("cross_entropy", "lovasz_loss", "dice_loss")) == (0.5, 0.5, D)    # more than two entries
    assert ops.seg_loss_plan(("cross_entropy", "tversky_loss2")) == (1.0, 0.0, T)
    assert ops.seg_loss_plan(("cross_entropy", "tversky_loss2", "diceEntropy")) == (0.5, 0.0, T | E)
    assert ops.seg_loss_plan(("lovasz_loss", "tversky_loss2", "diceEntropy")) == (0.0, 1.0, T | E)   # Lovasz without CE
    assert ops.seg_loss_plan(("dice_loss", "diceEntropy")) == (0.0, 0.0, D)                     # if / elif upstream
    assert ops.seg_loss_plan("dice_loss") == (0.0, 0.0, D)


def test_argument_validation():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, SdhipError
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    z, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(SdhipError):                   # no CPU path
        ops.seg_loss(z, t, ("dice_loss",))
    with pytest.raises(SdhipError, match="3 entries"):
        ops.seg_loss(z, t, ("cross_entropy",), class_weights=[1.0, 2.0, 3.0])
    with pytest.raises(SdhipError, match="3 entries"):
        ops.seg_loss(z, t, ("cross_entropy",), class_weights=torch.ones(3))
    with pytest.raises(SdhipError):                   # a CPU weight table
        ops.seg_class_weights(torch.ones(2), 2)
    with pytest.raises(SdhipError, match="32"):
        ops.seg_loss(torch.zeros(1, 33, 4, 4), torch.zeros(1, 33, 4, 4), ("dice_loss",))
    with pytest.raises(SdhipError):
        ops.seg_loss(z, torch.zeros(1, 3, 4, 4), ("dice_loss",))
    with pytest.raises(ValueError):
        ops.seg_loss(z, t, ("dice_los",))
    with pytest.raises(SdhipError, match="3 entries"):
        ops.train_loss(z, z[:, :1], z, t, t[:, :1], class_weights=[1.0, 2.0, 3.0])
    with pytest.raises(NotImplementedError, match="area_ce"):
        ops.train_loss(z, z[:, :1], z, t, t[:, :1], loss=("cross_entropy", "area_ce"))
    # the new keywords come after the existing ones
    assert list(inspect.signature(ops.train_loss).parameters)[-2:] == ["loss", "class_weights"]
    assert list(inspect.signature(TrainStep.__init__).parameters)[-2:] == ["loss", "class_weights"]
    assert list(inspect.signature(ops.seg_loss).parameters) == ["logits", "seg_target", "loss", "class_weights", "ignore_void"]


def test_new_symbols_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_bad_arguments_are_rejected_without_gpu_work():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, SdhipError
    assert _lib._lib.sdhip_seg_sums(None, 2, None, 2, 1, 16, 2, None, 0, 0, None) == _lib.ERR_ARG
    assert _lib._lib.sdhip_seg_finish(None, 0, None, None, 1, 16, 2, 1.0, 0, None) == _lib.ERR_ARG
    assert _lib._lib.sdhip_seg_terms_bwd(None, 2, None, 2, None, 2, None, 0, 1, 16, 2, 0, None) == _lib.ERR_ARG
    assert _lib.seg_terms_workspace_bytes(2, 91, 2) >= 2 * 4 * 2 * 8 + 2 * 2 * 3 * 4
    # slots per image grow with the image and stay bounded
    assert _lib.seg_terms_workspace_bytes(1, 40 * 56, 19) > _lib.seg_terms_workspace_bytes(1, 256, 19)
    assert _lib.seg_terms_workspace_bytes(8, 1 << 24, 32) <= 1024 * 4 * 32 * 8 + 8 * 32 * 3 * 4 + 16
    with pytest.raises(SdhipError):
        _lib.seg_terms_workspace_bytes(1, 16, 33)


# ------------------------------------------------------------------ GPU: the operator
@pytest.mark.gpu
@pytest.mark.parametrize("case,names", CASE_LISTS, ids=["%s-%s" % (c, _tag(l)) for c, l in CASE_LISTS])
def test_f32_matches_reference(case, names):
    g = _gold()
    z, t, w, void = _inputs(case)
    for sw in (0, 1):
        key = "%s.%s.sw%d" % (case, _tag(names), sw)
        loss, grad = _run(z, t, names, w if sw else None, void)
        _check_f32(loss.cpu(), grad.cpu(), g[key + ".loss"], torch.from_numpy(g[key + ".grad"]), key)


@pytest.mark.gpu
@pytest.mark.parametrize("case,names", CASE_LISTS, ids=["%s-%s" % (c, _tag(l)) for c, l in CASE_LISTS])
def test_bf16_matches_restatement(case, names):
    z, t, w, void = _inputs(case)
    zb = z.bfloat16().float()
    for sw in (0, 1):
        want, wgrad = _restate_grad(zb, t, names, w if sw else None, void)
        loss, grad = _run(zb, t, names, w if sw else None, void, torch.bfloat16)
        gerr, gmax = float((grad.float().cpu() - wgrad).abs().max()), float(wgrad.abs().max())
        print("%s sw%d bf16: loss %.6g want %.6g  grad err %.2e  max|grad| %.3e" % (case, sw, float(loss), want, gerr, gmax))
        assert abs(float(loss) - want) <= 2e-2 * max(1.0, abs(want))
        assert gerr <= 2e-2 * gmax


def test_restatement_is_the_reference():
    """The torch restatement the bf16 and training-step tests lean on reproduces the fixture in f32 (CPU arithmetic only)."""
    g = _gold()
    for case in SMALL:
        z, t, w, void = _inputs(case)
        for names in LISTS:
            for sw in (0, 1):
                key = "%s.%s.sw%d" % (case, _tag(names), sw)
                want, wgrad = _restate_grad(z, t, names, w if sw else None, void)
                assert abs(want - float(g[key + ".loss"])) <= 1e-5 * max(1.0, abs(want)), key
                assert float((wgrad - torch.from_numpy(g[key + ".grad"])).abs().max()) <= 1e-5 * float(wgrad.abs().max()), key


@pytest.mark.gpu
@pytest.mark.parametrize("case,ld,off", [("roses", 8, 0), ("roses", 5, 3), ("city", 24, 0), ("city", 27, 5), ("city", 64, 0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_padded_pixel_stride(case, ld, off, dtype):
    """Logits as a channel slice of a wider NHWC buffer (ld > C), from channel 0 and from an odd channel (rows that are not
    16-byte aligned; in bf16 not even 4-byte aligned), and with a stride too wide for the LDS rows."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g = _gold()
    z, t, w, void = _inputs(case)
    B, C, H, W = z.shape
    if dtype == torch.bfloat16:
        z = z.bfloat16().float()
    for names in (("cross_entropy", "tversky_loss2"), ("diceEntropy",)):
        buf = torch.full((B, H, W, ld), 1e30, dtype=dtype, device="cuda")
        view = buf[..., off:off + C].permute(0, 3, 1, 2)
        view.copy_(z.cuda().to(dtype))
        x = view.detach().requires_grad_(True)
        assert ops.nhwc_view(x)[1] == ld
        loss = ops.seg_loss(x, t.cuda(), names, w.cuda(), void)
        loss.backward()
        key = "%s.%s.sw1" % (case, _tag(names))
        if dtype == torch.float32:
            _check_f32(loss.cpu(), x.grad.cpu(), g[key + ".loss"], torch.from_numpy(g[key + ".grad"]), key)
        else:
            want, wgrad = _restate_grad(z, t, names, w, void)
            assert abs(float(loss) - want) <= 2e-2 * max(1.0, abs(want))
            assert float((x.grad.float().cpu() - wgrad).abs().max()) <= 2e-2 * float(wgrad.abs().max())
        assert bool((buf[..., :off] == 1e30).all()) and bool((buf[..., off + C:] == 1e30).all())     # the slab around the slice


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_reproducible(dtype):
    z, t, w, void = _inputs("city_big")
    for names in BIG_LISTS:
        a = _run(z, t, names, w, void, dtype)
        b = _run(z, t, names, w, void, dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), names


@pytest.mark.gpu
def test_poisoned_workspace():
    """Every slot and coefficient is written before it is read: NaN in the workspace changes nothing."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    for case in ("city_big", "garden"):
        z, t, w, void = _inputs(case)
        for names in (("cross_entropy", "tversky_loss2"), ("diceEntropy",)):
            a = _run(z, t, names, w, void)
            assert any(k[0] == "seg" for k in ops._loss_ws)
            for ws in ops._loss_ws.values():
                ws.fill_(0xFF)                       # all-ones words: NaN as f32 and as f64
            b = _run(z, t, names, w, void)
            assert torch.isfinite(b[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (case, names)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_poisoned_slot_fold_workspaces(dtype):
    """photo_loss, edge_loss and disp_smooth_loss share one slot fold (csrc/loss_common.h): every slot is written before the
    fold reads it.  Shapes of more than one slot: 1500 pixels = 2 tiles of 1024, 4500 elements = 2 tiles of 4096, and a
    17 x 65 map = 2 x 2 stencil tiles of 16 x 64 (DS_TH x DS_TW)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: torch.rand(*s, generator=gen)
    left = r(1, 3, 5, 300).cuda()
    edges = (r(1, 1, 9, 500) < 0.3).float().cuda()
    img = r(1, 3, 17, 65).cuda()
    onehot = torch.zeros(1, 2, 17, 65)
    onehot[:, 0, :, :40] = 1
    onehot[:, 1, :, 40:] = 1
    onehot = onehot.cuda()
    terms = {"photo": (r(1, 3, 5, 300), lambda x: ops.photo_loss(x, left)),
             "edge": (r(1, 1, 9, 500) - 0.5, lambda x: ops.edge_loss(x, edges)),
             "disp_smooth": (8.0 * r(1, 1, 17, 65), lambda x: ops.disp_smooth_loss(img, x, onehot))}

    def run(x0, fn):
        x = x0.cuda().to(dtype).requires_grad_(True)
        loss = fn(x)
        loss.backward()
        return loss.detach().clone(), x.grad.clone()

    first = {k: run(*v) for k, v in terms.items()}
    assert set(terms) <= {k[0] for k in ops._loss_ws}
    for ws in ops._loss_ws.values():
        ws.fill_(0xFF)                               # all-ones words: NaN as f64, huge as u64
    for k, v in terms.items():
        loss, grad = run(*v)
        assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and float(loss) > 0, k
        assert torch.equal(loss, first[k][0]) and torch.equal(grad, first[k][1]), k


@pytest.mark.gpu
def test_upstream_gradient_scales():
    z, t, w, void = _inputs("roses")
    _, grad = _run(z, t, ("dice_loss",), None, void)
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    x = z.cuda().requires_grad_(True)
    (3.0 * ops.seg_loss(x, t.cuda(), ("dice_loss",))).backward()
    assert torch.allclose(x.grad, 3.0 * grad, rtol=1e-6, atol=0)


# ------------------------------------------------------------------ GPU: the step loss
@pytest.mark.gpu
def test_train_loss_with_list_and_weights():
    """seg1 carries the weighted cross-entropy, seg2 the list, the disparity the masked L1: the reference's parts, summed."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g = _gold()
    z2, t, w, void = _inputs("city")
    key = "city.%s.sw1" % _tag(STEP_LIST)
    xs = [torch.from_numpy(g[k]).cuda().requires_grad_(True) for k in ("city.z1", "city.disp")]
    x2 = z2.cuda().requires_grad_(True)
    total = ops.train_loss(xs[0], xs[1], x2, t.cuda(), torch.from_numpy(g["city.disp_gt"]).cuda(), True, mask_invalid_disp=True,
                           ignore_void=True, loss=STEP_LIST, class_weights=[float(v) for v in w])
    total.backward()
    want = float(g["city.seg1.sw1.loss"]) + float(g[key + ".loss"]) + float(g["city.l1.loss"])
    print("train_loss: got %.8g want %.8g" % (float(total), want))
    assert abs(float(total) - want) <= 1e-5 * max(1.0, abs(want))
    for x, k in ((xs[0], "city.seg1.sw1.grad"), (x2, key + ".grad"), (xs[1], "city.l1.grad")):
        wg = torch.from_numpy(g[k])
        err = float((x.grad.cpu() - wg).abs().max())
        print("  %s: grad err %.2e  max|grad| %.3e" % (k, err, float(wg.abs().max())))
        assert err <= 1e-6 and err <= 1e-5 * float(wg.abs().max()), k


def _model():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    torch.manual_seed(0)
    return fill_state_dict(N.minidsnetExt(R.CFG(), labels=2, patch_type='1dcorr'), 5).cuda().train()


STEP_WEIGHTS = (0.75, 2.5)


@pytest.mark.gpu
def test_step_loss_matches_restatement_on_its_own_outputs(monkeypatch):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    seen = []
    inner = ops.train_loss

    def recording(*a, **k):
        seen.append([t.detach().float().cpu() for t in a[:3]])
        return inner(*a, **k)
    monkeypatch.setattr(ops, "train_loss", recording)
    ts = TrainStep(_model(), dtype=torch.float32, use_graph=False, lr=1e-4, loss=STEP_LIST, class_weights=STEP_WEIGHTS)
    got = float(ts(*batch))
    ops.set_step_context(None)
    seg1, disp, seg2 = seen[0]
    seg, disp_t, w = batch[2].cpu(), batch[3].cpu(), torch.tensor(STEP_WEIGHTS)
    want = float(_restate(seg1, seg, ("cross_entropy",), w) + _restate(seg2, seg, STEP_LIST, w) + F.l1_loss(disp, disp_t))
    plain = float(_restate(seg1, seg, ("cross_entropy",)) + _restate(seg2, seg, ("cross_entropy", "lovasz_loss")) + F.l1_loss(disp, disp_t))
    print("step loss %.8g, restated %.8g (default loss on the same outputs: %.8g)" % (got, want, plain))
    assert abs(want - plain) > 1e-2            # the list and the weights matter on this batch
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want))


@pytest.mark.gpu
def test_step_with_list_captures_and_replays():
    """A replay of the captured step computes what an eager step computes FROM THE SAME STATE: the eager TrainStep takes
    over the captured one's parameters, Adam moments, running statistics and dropout seed bit for bit, then each runs
    its next step.  What is left between the two losses is the summation order of the network's f32 atomics (~1e-6).
    Two runs that train apart are no measure of the replay: Adam's first updates are +-lr whatever a gradient's size, so
    the ~1e-6 the atomics move a near-zero gradient flips whole updates: this model's loss, falling 4 % a step at lr 1e-4,
    was 5e-4 apart at the third step and 4e-3 at the fourth between an eager run and a captured one that trained apart —
    tests/test_train.py::test_graph_replay_matches_eager allows 2e-3 and 2e-2 there for the default loss."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    kw = dict(dtype=torch.float32, lr=1e-4, loss=STEP_LIST, class_weights=STEP_WEIGHTS)
    eager = TrainStep(_model(), use_graph=False, **kw)
    first = [float(eager(*batch)) for _ in range(2)]            # measuring step, armed step
    ops.set_step_context(None)
    ts = TrainStep(_model(), use_graph=True, **kw)
    ts.capture(*batch, warmup=2)
    assert ts.graph is not None                                 # captured, not fallen back to eager
    with torch.no_grad():
        for k in ("flat_p", "exp_avg", "exp_avg_sq", "beta_pow"):
            getattr(eager, k).copy_(getattr(ts, k))
        eager.ctx.seed.copy_(ts.ctx.seed)
        for dst, src in zip(eager.model.buffers(), ts.model.buffers()):
            dst.copy_(src)
    before = ts.flat_p.clone()
    want = float(eager(*batch))
    ops.set_step_context(None)
    got = [float(ts(*batch)) for _ in range(2)]
    print("eager steps 1-2 %s; step 3 from the captured step's state: eager %.8g, replays %s" % (first, want, got))
    assert abs(got[0] - want) <= 1e-3 * max(1.0, abs(want)), (got, want)
    # the replay holds the whole step, Adam included: the parameters move and the next replay scores the moved ones
    assert ts.steps_done == 4 and not torch.equal(ts.flat_p, before)
    assert math.isfinite(got[1]) and got[1] != got[0]


@pytest.mark.gpu
def test_default_step_keeps_its_launches():
    """loss=None, class_weights=None is the step as it was: the same kernel-node count as a TrainStep built without the keywords;
    the list adds the launches of the three heads' terms and nothing else."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    nodes = []
    for kw in ({}, dict(loss=None, class_weights=None), dict(loss=STEP_LIST, class_weights=STEP_WEIGHTS)):
        ts = TrainStep(_model(), dtype=torch.bfloat16, use_graph=True, lr=1e-4, **kw)
        ts.debug_graph = True
        ts(*batch)
        ops.set_step_context(None)
        assert ts.graph is not None
        nodes.append(_lib.graph_node_counts(ts.graph))
    print(nodes)
    assert nodes[0] == nodes[1]
    assert nodes[2]["memset"] == 0 and nodes[2]["kernel"] == nodes[0]["kernel"] + 2 * (3 - 1)    # two heads: 3 launches instead of 1
