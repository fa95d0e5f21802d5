"""The `*_disp` warp networks minidsnetDivideDisp / minidsnetDivideDisp2 (warp.py; `-net dsnet_warp_disp`, `dsnet_warp_disp_consist`),
their operators (ops.warp_image_masked, ops.gate_blend, ops.photo_loss on csrc/warp.hip), the image gradient of the DenseNet stem
(densenet._Stem) and the photometric step, against tests/golden/warp_disp.npz, which tools/make_golden_warp_disp.py computes with
the reference's own networks on the CPU."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.detweights import fill_state_dict, rand_input, randn_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("sdhip_warp_image_masked", "sdhip_gate_blend_fwd", "sdhip_gate_blend_bwd", "sdhip_photo_mse",
               "sdhip_photo_mse_workspace_bytes")
OP_TOL = 1e-5          # the bar of the package's other loss / warp kernels: relative to the largest expected magnitude
BF16_STEP = 2.0 ** -8  # one bf16 rounding of a value is within 2^-9 of it; two roundings (input and output side) within 2^-8
REPLAY_TOL = 1e-3      # tests/test_warp.py / tests/test_mobilenet.py: captured replay against eager steps
CONV_TOL = {torch.float32: 2e-4, torch.bfloat16: 4e-2}      # tests/test_conv.py::test_hip_conv_matches_oracle, data gradients
NET_TAGS = ["disp_1d", "disp2_1d", "disp2_2d"]
ALL_TAGS = NET_TAGS + ["disp_a1_edges", "disp2_a1_edges"]
OUT_NAMES = ("out0", "out1", "out2", "out3", "out4", "out5")


def _gold():
    return np.load(os.path.join(GDIR, "warp_disp.npz"))


def _cases():
    return json.loads(str(_gold()["cases"]))


def _keys():
    return json.loads(str(_gold()["keys"]))


def _native(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, warp
    k = _keys()[tag]
    return getattr(warp, k["cls"])(N.CFG(**k["cfg"]), labels=k["labels"], pretrained=False, patch_type=k["patch"],
                                   include_edges=k["edges"], backbone=k["backbone"])


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_constructs_with_the_reference_keys_and_parameter_order(tag):
    assert sorted(_keys()) == sorted(ALL_TAGS)
    k = _keys()[tag]
    m = _native(tag)
    assert [[n, list(v.shape)] for n, v in m.state_dict().items()] == k["state_dict"]
    assert [n for n, _ in m.named_parameters()] == k["parameters"]
    assert m.three_outputs
    disp2 = k["cls"] == "minidsnetDivideDisp2"
    assert getattr(m, "photo_outputs", False) == disp2 and getattr(m, "disp_input", False) == (not disp2)


@pytest.mark.parametrize("backbone", ["mobilenet", "resnet50", "resnet101"])
@pytest.mark.parametrize("cls", ["minidsnetDivideDisp", "minidsnetDivideDisp2"])
def test_other_backbones_are_refused_by_name(cls, backbone):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, warp
    with pytest.raises(NotImplementedError, match=backbone):
        getattr(warp, cls)(N.CFG(), labels=2, backbone=backbone)


def test_new_symbols_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert all(callable(getattr(ops, n)) for n in ("warp_image_masked", "gate_blend", "photo_loss"))
    assert _lib.photo_mse_workspace_bytes(1) == 8 and _lib.photo_mse_workspace_bytes(1025) == 16
    assert _lib.photo_mse_workspace_bytes(1 << 30) == 8 * 1024            # the slot count is capped
    for bad in (0, -3, (1 << 40) + 1):
        with pytest.raises(_lib.SdhipError):
            _lib.photo_mse_workspace_bytes(bad)


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _masked(L, img=16, bs=300, cs=1, ps=3, dti=0, gt=16, out=16, ldy=3, dto=0, B=1, H=2, W=9, C=3):
    return L.sdhip_warp_image_masked(_p(img), bs, cs, ps, dti, _p(gt), _p(out), ldy, dto, B, H, W, C, None)


def _blend_f(L, a=16, lda=5, b=16, ldb=5, g=16, ldg=1, y=16, ldy=5, npix=7, C=5, dt=0):
    return L.sdhip_gate_blend_fwd(_p(a), lda, _p(b), ldb, _p(g), ldg, _p(y), ldy, npix, C, dt, None)


def _blend_b(L, gy=16, ldgy=5, a=16, lda=5, b=16, ldb=5, g=16, ldg=1, ga=16, ldga=5, gb=16, ldgb=5, gg=16, ldgg=1, npix=7, C=5, dt=0):
    return L.sdhip_gate_blend_bwd(_p(gy), ldgy, _p(a), lda, _p(b), ldb, _p(g), ldg, _p(ga), ldga, _p(gb), ldgb, _p(gg), ldgg, npix, C,
                                  dt, None)


def _photo(L, w=16, ldw=3, dt=0, l=16, bs=300, cs=1, ps=3, grad=16, loss=16, weight=1.0, B=1, H=2, W=9, C=3, ws=16, wsb=64):
    return L.sdhip_photo_mse(_p(w), ldw, dt, _p(l), bs, cs, ps, _p(grad), _p(loss), weight, B, H, W, C, _p(ws), wsb, None)


def test_malformed_arguments_are_rejected_without_gpu_work():
    """Every call below would fault if a pointer were dereferenced or a kernel launched (the pointers are the address 16)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    L, E = _lib._lib, _lib.ERR_ARG
    assert _masked(L, img=None) == E and b"null" in L.sdhip_last_error()
    assert _masked(L, gt=None) == E and _masked(L, out=None) == E
    assert _masked(L, C=0) == E and _masked(L, C=5) == E and b"1 <= C <= 4" in L.sdhip_last_error()
    assert _masked(L, ldy=2) == E and b"pixel stride" in L.sdhip_last_error()
    assert _masked(L, W=0) == E and _masked(L, H=0) == E and _masked(L, B=0) == E
    assert _masked(L, ps=0) == E and _masked(L, cs=0) == E and _masked(L, bs=-1) == E
    assert _masked(L, dti=7) == E and _masked(L, dto=7) == E
    for fn in (_blend_f, _blend_b):
        assert fn(L, a=None) == E and fn(L, b=None) == E and fn(L, g=None) == E
        assert fn(L, lda=4) == E and fn(L, ldb=4) == E and fn(L, ldg=0) == E
        assert fn(L, npix=0) == E and fn(L, C=0) == E and fn(L, dt=7) == E
    assert _blend_f(L, y=None) == E and _blend_f(L, ldy=4) == E
    assert _blend_b(L, gy=None) == E and _blend_b(L, ga=None) == E and _blend_b(L, gb=None) == E and _blend_b(L, gg=None) == E
    assert _blend_b(L, ldgy=4) == E and _blend_b(L, ldga=4) == E and _blend_b(L, ldgb=4) == E and _blend_b(L, ldgg=0) == E
    assert _photo(L, w=None) == E and _photo(L, l=None) == E and _photo(L, grad=None) == E and _photo(L, loss=None) == E
    assert _photo(L, ws=None) == E
    assert _photo(L, wsb=4) == E and b"workspace" in L.sdhip_last_error()
    assert _photo(L, ws=20) == E                                          # not 8-byte aligned
    assert _photo(L, ldw=2) == E and _photo(L, C=5) == E and _photo(L, C=0) == E and _photo(L, dt=7) == E
    assert _photo(L, W=0) == E and _photo(L, cs=0) == E


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, SdhipError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    img, gt = z(1, 3, 4, 9), z(1, 1, 4, 9)
    with pytest.raises(SdhipError, match="no CPU path"):
        ops.warp_image_masked(img, gt)
    with pytest.raises(SdhipError, match="no CPU path"):
        ops.gate_blend(z(1, 5, 4, 9), z(1, 5, 4, 9), gt)
    with pytest.raises(SdhipError, match="no CPU path"):
        ops.photo_loss(img, img)
    for bad_gt in (z(1, 2, 4, 9), z(1, 1, 4, 8), z(1, 4, 9), z(1, 1, 4, 9, dt=torch.bfloat16), z(1, 1, 4, 18)[..., ::2]):
        with pytest.raises(SdhipError):
            ops.warp_image_masked(img, bad_gt)
    for bad_img in (z(1, 5, 4, 9), z(3, 4, 9), z(1, 3, 4, 9, dt=torch.float16), z(1, 3, 4, 9).requires_grad_(True)):
        with pytest.raises(SdhipError):
            ops.warp_image_masked(bad_img, gt)
    for bad_out in (z(1, 3, 4, 9), z(1, 4, 4, 9), z(1, 3, 4, 9, dt=torch.float16)):      # NCHW memory, wrong shape, wrong type
        with pytest.raises(SdhipError):
            ops.warp_image_masked(img, gt, out=bad_out)
    for a, b, g in ((z(1, 5, 4, 9), z(1, 4, 4, 9), gt), (z(1, 5, 4, 9), z(1, 5, 4, 9), z(1, 5, 4, 9)), (z(5, 4, 9), z(5, 4, 9), gt),
                    (z(1, 5, 4, 9), z(1, 5, 4, 9, dt=torch.bfloat16), gt), (z(0, 5, 4, 9), z(0, 5, 4, 9), z(0, 1, 4, 9))):
        with pytest.raises(SdhipError):
            ops.gate_blend(a, b, g)
    for w, l in ((img, z(1, 4, 4, 9)), (z(1, 5, 4, 9), z(1, 5, 4, 9)), (img, z(1, 3, 4, 9, dt=torch.bfloat16)), (z(3, 4, 9), z(3, 4, 9)),
                 (z(1, 3, 4, 9, dt=torch.float16), img)):
        with pytest.raises(SdhipError):
            ops.photo_loss(w, l)
    with pytest.raises(SdhipError):
        ops.apply_disparity(img, gt, sign=0.5)


def test_step_surface_refuses_what_upstream_cannot_run():
    """default_loss: a photo_outputs model needs the 3-channel left image; model_outputs: a disp_input model needs the target."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import step, SdhipError

    class Photo:
        photo_outputs = three_outputs = True

    class TakesDisp:
        disp_input = three_outputs = True

        def __call__(self, *a):
            raise AssertionError("the model must not be called")
    outs = [torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4)] * 2 + [torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 4, 4)]
    seg, disp = torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(SdhipError, match="left"):
        step.default_loss(Photo(), outs, seg, disp)
    with pytest.raises(SdhipError, match="3-channel"):
        step.default_loss(Photo(), outs, seg, disp, left=torch.zeros(1, 4, 4, 4))
    with pytest.raises(SdhipError, match="disparity target"):
        step.model_outputs(TakesDisp(), torch.float32, torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), seg, None)


def test_fixture_keeps_its_conditions():
    """What tools/make_golden_warp_disp.py asserts, re-checked on the stored data: sample positions of the Disp2 train cases stay
    off the integers (the warp's gradient jumps there), and the ground-truth disparities cut, clamp left and leave on the right."""
    gold, c = _gold(), _cases()
    for tag in ("disp2_1d", "disp2_2d"):
        assert float(gold["net.%s.train.near_share" % tag]) <= c["near_cap"]
        d = gold["net.%s.train.disp_q" % tag]
        assert d.shape == (2, 1, 64, 64) and d.dtype == np.float32
        x = (np.arange(0, 256, 4, dtype=np.float32) - d).astype(np.float64)
        assert float((np.abs(x - np.round(x)) < c["margin"]).mean()) <= c["near_cap"]
    for tag, B, C, H, W in c["masked"]:
        gt = gold["masked.%s.gt" % tag]
        x = np.arange(W, dtype=np.float32) - gt
        assert gt.shape == (B, 1, H, W) and (gt == 0).any() and (gt < 0).any()
        assert ((gt > 0) & (x < 0)).any() and (x > W - 1).any() and ((gt > 0) & (x >= 0) & (x < W - 1)).any()
    lo, hi = gold["gt_range"]
    gt = rand_input(31, "disp_signed", (2, 1, 256, 256), float(lo), float(hi)).numpy()
    x = np.arange(256, dtype=np.float32) - gt
    assert lo < 0 < hi and (gt <= 0).mean() > 0.1 and ((gt > 0) & (x < 0)).any() and (x > 255).any()
    assert os.path.getsize(os.path.join(GDIR, "warp_disp.npz")) <= 1 << 20


# ------------------------------------------------------------------ GPU: kernels alone
def _layout(t, how):
    """The same values in NCHW, channels-last, or as a channel slice of a wider channels-last buffer (padded pixel stride)."""
    t = t.detach()
    if how == "nchw":
        return t.clone(memory_format=torch.contiguous_format)
    if how == "cl":
        return t.clone(memory_format=torch.channels_last)
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, (C + 8) & ~7), float("nan"), dtype=t.dtype, device=t.device)
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return buf[..., :C].permute(0, 3, 1, 2)


def _close(got, want, tol, what):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("%s: max err %.3e, largest expected %.3e" % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("padded_out", [False, True])
@pytest.mark.parametrize("how", ["nchw", "cl", "slice"])
@pytest.mark.parametrize("tag", ["m3", "m4"])
def test_masked_warp_matches_the_reference(tag, how, padded_out):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    gold = _gold()
    B, C, H, W = next(c[1:] for c in _cases()["masked"] if c[0] == tag)
    img = randn_input(7, tag + ":img", (B, C, H, W)).cuda()
    gt = torch.from_numpy(gold["masked.%s.gt" % tag]).cuda()
    want = gold["masked.%s.out" % tag]
    assert float(gold["masked.%s.dev64" % tag]) <= OP_TOL * np.abs(want).max()        # the reference's own f32 error is below the bar

    def run(x, dtype):
        if padded_out:
            buf = torch.full((B, H, W, 8), 7.0, dtype=dtype, device="cuda")
            out = ops.warp_image_masked(x, gt, out=buf[..., :C].permute(0, 3, 1, 2))
            assert bool((buf[..., C:] == 7.0).all())                                   # pad lanes are not written
            return out
        out = ops.warp_image_masked(x, gt, out=ops.empty_nhwc(B, C, H, W, dtype, x.device))
        return out
    got = run(_layout(img, how), torch.float32)
    _close(got, want, OP_TOL, "masked %s %s f32" % (tag, how))
    cut = (gt <= 0).expand(B, C, H, W)
    edge = ((torch.arange(W, device="cuda", dtype=torch.float32) - gt) >= W - 1).expand(B, C, H, W)
    assert bool(cut.any()) and bool(edge.any())
    assert bool((got[cut] == 0).all()) and bool((got[edge] == 0).all())                # exact zeros: the mask and the right-edge rule
    default = ops.warp_image_masked(_layout(img, how), gt)                             # out=None: padded stride of the conv nodes
    assert torch.equal(default, got) and default.stride(3) == 8
    # bf16: the arithmetic is f32 on the rounded image, so the f32 result on the upcast image is the comparator; a bf16 output is
    # that result rounded once more
    imgb = img.bfloat16()
    ref32 = run(_layout(imgb.float(), how), torch.float32)
    assert torch.equal(run(_layout(imgb, how), torch.float32), ref32)                  # layout and storage type do not matter
    gotb = run(_layout(imgb, how), torch.bfloat16)
    assert gotb.dtype == torch.bfloat16
    _close(gotb, ref32.cpu().numpy(), BF16_STEP, "masked %s %s bf16" % (tag, how))
    assert bool((gotb[cut] == 0).all()) and bool((gotb[edge] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("how", ["cl", "slice"])
@pytest.mark.parametrize("shape", [(1, 2, 1, 37), (1, 19, 7, 43)])       # (npix, C) = (37, 2) and (301, 19)
def test_gate_blend_matches_aten(shape, how, dtype):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    B, C, H, W = shape
    g0 = torch.Generator().manual_seed(3)
    mk = lambda c, lo=None: (torch.randn(B, c, H, W, generator=g0) if lo is None else torch.rand(B, c, H, W, generator=g0)).cuda().to(dtype)
    a, b, g, gy = mk(C), mk(C), mk(1, 0), mk(C)
    ar, br, gr = (t.float().clone().requires_grad_(True) for t in (a, b, g))
    want = (1 - gr) * ar + gr * br
    want.backward(gy.float())
    pad = (lambda t: _layout(t, "slice")) if how == "slice" else (lambda t: _layout(t, "cl"))
    an, bn, gn = (pad(t).requires_grad_(True) for t in (a, b, g))
    got = ops.gate_blend(an, bn, gn)
    got.backward(pad(gy))
    tol = OP_TOL if dtype == torch.float32 else BF16_STEP     # f32: sums over <= 19 channels; bf16: one rounding of an f32 result
    for name, x, w in (("y", got, want), ("ga", an.grad, ar.grad), ("gb", bn.grad, br.grad), ("gg", gn.grad, gr.grad)):
        assert x.dtype == dtype and tuple(x.shape) == tuple(w.shape)
        _close(x, w.detach().cpu().numpy(), tol, "gate_blend %s %s %s %s" % (shape, how, dtype, name))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["p13", "p9"])
def test_photo_loss_matches_the_reference_and_repeats_bit_for_bit(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    gold = _gold()
    B, C, H, W = next(c[1:] for c in _cases()["photo"] if c[0] == tag)
    l = rand_input(7, tag + ":l", (B, C, H, W)).cuda()
    w = rand_input(7, tag + ":w", (B, C, H, W)).cuda()
    want, want_g = float(gold["photo.%s.loss" % tag]), gold["photo.%s.grad" % tag]
    assert abs(want - float(gold["photo.%s.loss64" % tag])) <= OP_TOL * want and float(gold["photo.%s.dev64" % tag]) <= OP_TOL * np.abs(want_g).max()
    for dtype in (torch.float32, torch.bfloat16):
        wd = w.to(dtype)
        if dtype == torch.float32:
            ref, ref_g, tol_g = want, want_g, OP_TOL
        else:       # the closed form in f64 on the rounded input; the gradient is stored in bf16
            d = wd.double() - l.double()
            ref, ref_g, tol_g = float((d * d).mean()), (2 * d / d.numel()).cpu().numpy(), BF16_STEP
        runs = []
        for wh, lh in (("cl", "nchw"), ("cl", "nchw"), ("slice", "cl"), ("nchw", "slice")):
            x = _layout(wd, wh).requires_grad_(True)
            loss = ops.photo_loss(x, _layout(l, lh))
            loss.backward()
            assert loss.dtype == torch.float32 and x.grad.dtype == dtype
            runs.append((loss.detach().clone(), x.grad.contiguous().clone()))
        print("photo %s %s: loss %.8f (reference %.8f)" % (tag, dtype, float(runs[0][0]), ref))
        assert abs(float(runs[0][0]) - ref) <= OP_TOL * ref
        _close(runs[0][1], ref_g, tol_g, "photo %s %s grad" % (tag, dtype))
        for v, g in runs[1:]:           # a second run, a padded pixel stride, other image layouts: the same bits
            assert torch.equal(v, runs[0][0]) and torch.equal(g, runs[0][1])
        x = wd.detach().clone().requires_grad_(True)
        ops.photo_loss(x, l, weight=0.25).backward()
        _close(x.grad, 0.25 * np.asarray(ref_g), tol_g, "photo %s %s weighted grad" % (tag, dtype))


@pytest.mark.gpu
def test_photo_loss_folds_many_workgroups():
    """More than one slot and a tail: 3 x 41 x 53 pixels = 7 workgroups of 1024 pixels, the last one partly filled."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g0 = torch.Generator().manual_seed(11)
    w, l = torch.rand(3, 3, 41, 53, generator=g0), torch.rand(3, 3, 41, 53, generator=g0)
    x = w.cuda().requires_grad_(True)
    loss = ops.photo_loss(x, l.cuda())
    loss.backward()
    d = w.double() - l.double()
    assert abs(float(loss) - float((d * d).mean())) <= OP_TOL * float((d * d).mean())
    _close(x.grad, (2 * d / d.numel()).numpy(), OP_TOL, "photo many workgroups grad")


# ------------------------------------------------------------------ GPU: the stem's image gradient
class _Spy:
    """Stands in for the ctypes library and records the names of the entry points that are called."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("sdhip_"):
            return fn

        def wrapped(*a):
            self._log.append(name)
            return fn(*a)
        return wrapped


def _stem_run(x, w, bn, g0):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import densenet as D
    if w.shape[-1] == 4:
        x = D._SpaceToDepth2.apply(x) if x.requires_grad else D._space_to_depth2(x)
    c0, _ = D._Stem.apply(x, w, bn.weight, bn.bias, bn, 1)
    c0.backward(g0)
    return c0


@pytest.mark.gpu
@pytest.mark.parametrize("size,s2d", [((16, 24), True), ((15, 23), False)])
def test_stem_image_gradient_matches_f64_autograd(size, s2d, monkeypatch):
    """conv0's data gradient through tap 0, the raw convolution output: the 7x7 / stride 2 form and the space-to-depth 4x4 form
    (mapped back to the image), f32 against F.conv2d's f64 autograd on the CPU, bf16 against the f32 result; an image that requires
    no gradient adds no launch."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib, densenet as D
    g = torch.Generator().manual_seed(17)
    H, W = size
    x = torch.randn(2, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    g0 = torch.randn(2, 64, (H + 1) // 2, (W + 1) // 2, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, stride=2, padding=3).backward(g0.double())
    bn = torch.nn.BatchNorm2d(64).cuda().train()
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        xn = x.cuda().to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wn = w.cuda().requires_grad_(True)
        c0 = _stem_run(xn, D._stem_s2d_weight(wn) if s2d else wn, bn, g0.cuda().to(dtype))
        assert xn.grad is not None and xn.grad.dtype == dtype and tuple(xn.grad.shape) == (2, 3, H, W)
        res[dtype] = xn.grad.float().cpu()
        if dtype == torch.float32:
            _close(c0, F.conv2d(x.double(), w.double(), stride=2, padding=3).numpy(), CONV_TOL[dtype], "stem %s y" % (size,))
            _close(xn.grad, xr.grad.numpy(), CONV_TOL[dtype], "stem %s gx f32" % (size,))
            _close(wn.grad, wr.grad.numpy(), CONV_TOL[dtype], "stem %s gw f32" % (size,))
    _close(res[torch.bfloat16], res[torch.float32].numpy(), CONV_TOL[torch.bfloat16], "stem %s gx bf16 against f32" % (size,))
    logs = {}
    for need in (False, True):
        logs[need] = []
        monkeypatch.setattr(_lib, "_lib", _Spy(_lib._lib, logs[need]))
        xn = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(need)
        wn = w.cuda().requires_grad_(True)
        _stem_run(xn, D._stem_s2d_weight(wn) if s2d else wn, bn, g0.cuda())
        monkeypatch.undo()
        assert (xn.grad is not None) == need
    extra = list(logs[True])
    for n in logs[False]:
        extra.remove(n)                                     # every launch of the plain backward is part of the other one
    print("launches without an image gradient %d, added by it: %s" % (len(logs[False]), extra))
    assert logs[False].count("sdhip_conv2d_fwd") == 1 and "sdhip_stuff" not in logs[False]      # the forward convolution alone
    assert "sdhip_conv2d_fwd" in extra and set(extra) <= {"sdhip_conv2d_fwd", "sdhip_stuff", "sdhip_conv_pack_weights", "sdhip_conv_packed_elems"}


# ------------------------------------------------------------------ GPU: networks
def _smooth_image(name):
    """The generator's smooth_image: 32x32 uniform noise enlarged bilinearly by 8.  The third tower pass reads an image that moves
    with the predicted disparity, so the comparison is only as well conditioned as the image is smooth (the generator prints how far
    the reference's own f32 step is from its f64 step)."""
    return F.interpolate(rand_input(31, name, (2, 3, 32, 32)), scale_factor=8, mode="bilinear", align_corners=False).contiguous()


def _net_inputs():
    a, b = _smooth_image("left_lo"), _smooth_image("right_lo")
    seg = F.one_hot((rand_input(31, "seg", (2, 256, 256)) > 0.5).long(), 2).permute(0, 3, 1, 2).float()
    lo, hi = _gold()["gt_range"]
    disp = rand_input(31, "disp_signed", (2, 1, 256, 256), float(lo), float(hi))
    return a.cuda(), b.cuda(), seg.cuda(), disp.cuda()


def _call(m, a, b, disp):
    return m(a, b, disp) if getattr(m, "disp_input", False) else m(a, b)


def _step_loss(m, outs, a, seg, disp):
    """The step's sum with cross-entropy only, as the generator forms it (ATen, test side)."""
    ce = lambda y: torch.mean(torch.sum(-seg * F.log_softmax(y.float(), 1), 1))
    loss = ce(outs[0]) + ce(outs[2]) + ce(outs[4])
    if getattr(m, "photo_outputs", False):
        return loss + F.mse_loss(outs[5].float(), a)
    return loss + F.l1_loss(outs[1].float(), disp)


def _trained_like_statistics(m, a, b, disp):
    """The generator's steps: momentum 0.5, two train-mode passes without gradients, momentum restored (a mixture of the
    statistics of a module's several calls; momentum 1 would keep those of the last call, the warped image, alone)."""
    bns = [x for x in m.modules() if isinstance(x, torch.nn.modules.batchnorm._BatchNorm)]
    for x in bns:
        x.momentum = 0.5
    m.train()
    with torch.no_grad():
        for _ in range(2):
            _call(m, a, b, disp)
    for x in bns:
        x.momentum = 0.1
    return m.eval()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,tm", [("disp_1d", "train"), ("disp_1d", "eval"), ("disp2_1d", "train"), ("disp2_1d", "eval"),
                                    ("disp2_2d", "train")])
def test_network_matches_reference_fixture(tag, tm):
    from test_nets import _check
    gold = _gold()
    a, b, seg, disp = _net_inputs()
    m = fill_state_dict(_native(tag), 31).cuda()
    if tm == "train":
        m.train()
        outs = _call(m, a, b, disp)
    else:       # float64 reference with trained-like running statistics: see the generator
        _trained_like_statistics(m, a, b, disp)
        with torch.no_grad():
            outs = _call(m, a, b, disp)
    assert len(outs) == 6 and [tuple(o.shape)[1] for o in outs] == [2, 1, 2, 1, 2, 3 if m.__class__.__name__.endswith("2") else 1]
    loss = _step_loss(m, outs, a, seg, disp)
    p = "net.%s.%s" % (tag, tm)
    for name, o in zip(OUT_NAMES, outs):
        _check(gold, "%s.%s" % (p, name), o, 1e-3, 16)
    want = float(gold[p + ".loss"])
    got = float(loss.detach())
    print("%s loss %.6f (reference %.6f)" % (p, got, want))
    assert abs(got - want) <= 1e-3 * max(1.0, abs(want)), (got, want)
    if tm != "train":
        return
    loss.backward()
    sd = m.state_dict()
    bn_keys = [k[len(p) + 4:] for k in gold.files if k.startswith(p + ".rm.")]
    assert len(bn_keys) == 5
    for k in bn_keys:
        for s, leaf in (("rm", "running_mean"), ("rv", "running_var")):
            np.testing.assert_allclose(sd["%s.%s" % (k, leaf)].cpu().numpy(), gold["%s.%s.%s" % (p, s, k)], rtol=1e-3, atol=1e-4)
    assert {k for k, q in m.named_parameters() if q.grad is None} == set(gold[p + ".nograd"].tolist())
    acc = {}
    for k, q in m.named_parameters():
        if q.grad is not None:
            top = k.split(".")[0]
            acc[top] = acc.get(top, 0.0) + float(q.grad.double().pow(2).sum())
    want_n = {k[len(p) + 7:]: float(gold[k]) for k in gold.files if k.startswith(p + ".gnorm.")}
    assert set(acc) == set(want_n), set(acc) ^ set(want_n)
    for top, v in want_n.items():
        print("%s gnorm %s: %.6e (reference %.6e)" % (p, top, np.sqrt(acc[top]), v))
        assert abs(np.sqrt(acc[top]) - v) <= 2e-2 * max(v, 1e-3), (top, np.sqrt(acc[top]), v)


@pytest.mark.gpu
def test_disp2_trains_its_disparity_head_without_disparity_labels():
    """The step's default loss with an all-zero disparity target: dispoutConv still receives a gradient, through the warped image
    (the photometric term and the segmentation loss of the third tower pass)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import step
    a, b, seg, disp = _net_inputs()
    m = fill_state_dict(_native("disp2_1d"), 31).cuda().train()
    outs = step.model_outputs(m, torch.float32, a, b, seg, torch.zeros_like(disp))
    loss = step.default_loss(m, outs, seg, torch.zeros_like(disp), left=a, use_lovasz=False)
    want = float(_step_loss(m, outs, a, seg, disp).detach())
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want), (float(loss.detach()), want)         # no L1 term in it
    loss.backward()
    n = float(torch.cat([q.grad.flatten() for q in m.dispoutConv.parameters()]).double().norm())
    print("dispoutConv gradient norm with a zero disparity target: %.4e" % n)
    assert math.isfinite(n) and n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["disp_a1_edges", "disp2_a1_edges"])
def test_edge_and_aspp_variants_train_finite(tag):
    """include_edges (the tower reads three channels, the auxiliary convolutions four) and CFG.aspp = 1 (built, never called)."""
    a, b, _, disp = _net_inputs()
    a = torch.cat([a, rand_input(31, "edge_l", (2, 1, 256, 256)).cuda()], 1)
    b = torch.cat([b, rand_input(31, "edge_r", (2, 1, 256, 256)).cuda()], 1)
    seg = F.one_hot((rand_input(31, "seg", (2, 256, 256)) * 8).long().clamp(0, 7), 8).permute(0, 3, 1, 2).float().cuda()
    m = fill_state_dict(_native(tag), 31).cuda().train()
    outs = _call(m, a, b, disp)
    last = 3 if tag.startswith("disp2") else 1
    assert [tuple(o.shape) for o in outs] == [(2, c, 256, 256) for c in (8, 1, 8, 1, 8, last)]
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    _step_loss(m, outs, a[:, :3], seg, disp).backward()
    assert not any(n.startswith("aspp.") and q.grad is not None for n, q in m.named_parameters())
    assert all(bool(torch.isfinite(q.grad).all()) for _, q in m.named_parameters() if q.grad is not None)


# bf16 eval against the float64 reference, relative L2 of the strided samples per head (both / disp / seg_left / seg_right / gate for
# minidsnetDivideDisp; both / disp / seg_left / seg_right / warped_right for minidsnetDivideDisp2).  MEASURED on one MI355X, caps
# twice that (the convention of tests/test_warp.py and tests/test_bf16_parity.py):
BF16_HEADS = (0, 1, 2, 4, 5)
#   disp_1d   4.50 / 2.55 / 5.16 / 4.15 / 2.05 %
#   disp2_1d  7.39 / 9.12 / 7.57 / 11.51 / 0.51 %
# (a wrong tile or lane order gives errors near 100 %; the warped image of disp2_1d is one interpolation away from its input)
BF16_MEASURED = {"disp_1d": (0.0450, 0.0255, 0.0516, 0.0415, 0.0205), "disp2_1d": (0.0739, 0.0912, 0.0757, 0.1151, 0.0051)}
BF16_CAPS = {k: tuple(2 * e for e in v) for k, v in BF16_MEASURED.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(BF16_CAPS))
def test_bf16_eval_per_head_matches_reference(tag):
    from test_nets import _sample
    gold = _gold()
    a, b, _, disp = _net_inputs()
    m = fill_state_dict(_native(tag), 31).cuda()
    _trained_like_statistics(m, a, b, disp)           # statistics collected in f32, as a trained checkpoint carries them
    with torch.no_grad():
        outs = _call(m, a.bfloat16(), b.bfloat16(), disp)
    assert all(o.dtype == torch.bfloat16 for o in outs)
    errs = []
    for i in BF16_HEADS:
        want = gold["net.%s.eval.%s.sample" % (tag, OUT_NAMES[i])]
        got = _sample(outs[i], 16)
        errs.append(float(np.linalg.norm(got - want) / max(1e-12, np.linalg.norm(want))))
    print("bf16 eval rel L2 %s: %s" % (tag, ["%.4f" % e for e in errs]))
    assert BF16_CAPS[tag] is not None, "no measured caps for %s" % tag
    for e, cap, i in zip(errs, BF16_CAPS[tag], BF16_HEADS):
        assert e <= cap, (tag, OUT_NAMES[i], errs, BF16_CAPS[tag])


# ------------------------------------------------------------------ GPU: steps
def _model(tag, seed=5):
    torch.manual_seed(0)
    return fill_state_dict(_native(tag), seed).cuda().train()


def _batch():
    """train.synthetic_batch with the fixture's smooth images in place of its per-pixel noise (see _smooth_image)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch
    _, _, seg, disp = synthetic_batch(2, 256, 256)
    return [_smooth_image("left_lo").cuda(), _smooth_image("right_lo").cuda(), seg, disp]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["disp_1d", "disp2_1d"])
def test_graph_replay_matches_eager_and_keeps_unreached_parameters(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    gold = _gold()
    batch = _batch()
    losses = {}
    for graph in (False, True):
        ts = TrainStep(_model(tag), dtype=torch.float32, use_graph=graph, lr=1e-4)
        before = {k: v.detach().clone() for k, v in ts.model.named_parameters()}
        if graph:
            ts.capture(*batch, warmup=2)
            assert ts.graph is not None                                   # captured, not fallen back to eager
            seq = [float(ts(*batch)) for _ in range(3)]
        else:
            seq = [float(ts(*batch)) for _ in range(5)][2:5]
        losses[graph] = seq
        assert all(math.isfinite(v) for v in seq), seq
        names = [k for k, _ in ts.model.named_parameters()]
        idle = {names[i] for i in ts.grad_free}
        assert idle == set(gold["net.%s.train.nograd" % tag].tolist())     # the reference's list of parameters without a gradient
        for k, v in ts.model.named_parameters():
            if k in idle:
                assert torch.equal(v.detach(), before[k]), k
        assert not torch.equal(ts.model.dispoutConv.ct2d.weight.detach(), before["dispoutConv.ct2d.weight"])
        ops.set_step_context(None)
    print("%s eager %s, replayed %s" % (tag, losses[False], losses[True]))
    for i in range(3):
        assert abs(losses[False][i] - losses[True][i]) <= REPLAY_TOL * max(1.0, abs(losses[False][i])), losses


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["disp_1d", "disp2_1d"])
def test_loss_falls_on_a_fixed_batch(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    ts = TrainStep(_model(tag), dtype=torch.float32, use_graph=False, lr=1e-4)
    seq = [float(ts(*batch)) for _ in range(8)]
    ops.set_step_context(None)
    print(tag, "losses", seq)
    assert all(math.isfinite(v) for v in seq) and seq[-1] < seq[0], seq


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["disp_1d", "disp2_1d"])
def test_eval_step_with_loss_equals_the_eager_forward(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, step, SdhipError
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.evalstep import EvalStep
    a, b, seg, disp = _batch()
    m = _trained_like_statistics(fill_state_dict(_native(tag), 5).cuda(), a, b, disp)
    with torch.no_grad():
        outs = step.model_outputs(m, torch.float32, a, b, seg, disp)
        want = float(step.default_loss(m, outs, seg, disp, left=a) if tag.startswith("disp2") else step.default_loss(m, outs, seg, disp))
    ev = EvalStep(m, dtype=torch.float32, with_loss=True)
    res = ev(a, b, seg, disp)
    got = float(res[-1])
    ops.set_step_context(None)
    print("%s EvalStep loss %.6f, eager %.6f" % (tag, got, want))
    assert len(res) == 7 and abs(got - want) <= 1e-3 * max(1.0, abs(want)), (got, want)
    if tag == "disp_1d":
        with pytest.raises(SdhipError):
            EvalStep(m, dtype=torch.float32, use_graph=False)(a, b)         # a disp_input model cannot run without the target
