"""DeepLabV3+ / Xception-65 (`-net deeplab`, `-net deeplab_mod`; models_deeplab*/): the dilated depthwise kernels against a
float64 reference, blocks and networks against the reference fixture tests/golden/deeplab.npz
(tools/make_golden_deeplab.py), the harness steps, graph replay and checkpoints.

Bars.  Kernel: 1e-5 (f32) / 1e-2 (bf16) of max|want| for y and gx, 1e-5 for gw — those of the existing depthwise test
(tests/test_mobilenet.py).  Fixtures: blocks y 1e-4, gradients 1e-3; heads and loss 1e-3; gradient norms 2e-2; running
statistics rtol 1e-3 (atol rtol/10).  The fixture stores, per quantity, the deviation of the reference's own float32 run
from its float64 run in the same metric; where that exceeds a tenth of the bar, the bar is ten times the deviation
(`_bar`).  That applies to the gradient of bn_depth.bias in the relu_first SeparableConv2d (analytically zero: bn_point
removes a per-channel constant, so both runs hold rounding noise only), to the gradient norms of `encoder` and `spp` in
the train-mode networks, and to the first head of train-mode deeplab_mod (`x` and seg1: 1.6e-4 and 1.4e-4, bars 1.6e-3 and
1.4e-3).
"""
import ctypes
import copy
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.detweights import fill_state_dict, randn_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_deeplab as MG  # noqa: E402  (case lists and input generators shared with the fixture generator)

NEW_SYMBOLS = ("sdhip_dw_dil_conv_fwd", "sdhip_dw_dil_conv_dgrad", "sdhip_dw_dil_conv_wgrad", "sdhip_dw_dil_wgrad_parts")
PKG = "pmt_learning_for_semantic_segmentation_and_disparity_amd"


def _gold():
    return np.load(os.path.join(GDIR, "deeplab.npz"))


def _bar(gold, key, base):
    dev = float(gold[key + ".dev"])
    return base if dev <= base / 10 else 10 * dev


def _mods():
    import importlib
    return importlib.import_module(PKG + ".deeplab_mod"), importlib.import_module(PKG + ".deeplab")


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag,which,ch", [("deeplab_mod19", 0, 19), ("deeplab_mod2", 0, 2), ("deeplab19", 1, 19)])
def test_state_dict_keys_and_parameter_order_match_reference(tag, which, ch):
    want = json.loads(_gold()["keys"].tobytes().decode())[tag]
    m = _mods()[which].SPPNet(output_channels=ch)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want["state_dict"]
    assert [k for k, _ in m.named_parameters()] == want["parameters"]
    n = sum(p.numel() for p in m.parameters())
    assert (41.0e6 < n < 41.1e6) if which else (41.8e6 < n < 41.9e6), n
    assert sum(isinstance(x, torch.nn.BatchNorm2d) for x in m.modules()) == (146 if which else 156)
    assert sum(isinstance(x, torch.nn.Conv2d) and x.groups > 1 for x in m.modules()) == (68 if which else 72)


def test_unsupported_options_raise():
    DM, D = _mods()
    for mod in (DM, D):
        with pytest.raises(NotImplementedError):
            mod.SPPNet(enc_type='mobilenetv2')
        for dec in ('oc_base', 'oc_asp', 'spp', 'maspp'):
            with pytest.raises(NotImplementedError):
                mod.SPPNet(dec_type=dec)
        m = mod.SPPNet(output_channels=2)
        x = torch.zeros(1, 3, 8, 8)
        for call in (lambda: m.tta(x), lambda: m.pred_resize(x, (8, 8)), lambda: m.hflip(x), lambda: m.vflip(x), lambda: m.trans(x)):
            with pytest.raises(NotImplementedError):
                call()
    with pytest.raises(NotImplementedError):
        DM.Xception65(output_stride=32)
    with pytest.raises(NotImplementedError):
        DM.getNetwork('sdnet')
    with pytest.raises(TypeError):
        DM.SPPNet(19, 'xception65', 'aspp', 8, True)          # harness is keyword-only
    assert DM.Xception65(output_stride=16).block3.sep_conv3.block.depthwise.stride == (2, 2)
    net = DM.getNetwork('deeplab_mod')
    assert net.output_channels == 19 and net.encoder.bn1.eps == 1e-3 and not net.harness


def test_new_symbols_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def test_null_and_unsupported_arguments_are_rejected_without_gpu_work():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    L, P = _lib._lib, ctypes.c_void_p(16)
    assert L.sdhip_dw_dil_conv_fwd(None, 8, None, None, 8, None, 8, 1, 2, 9, 9, 8, 1, 2, 0, 1, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_dgrad(None, 8, None, None, 8, None, 8, 2, 9, 9, 8, 1, 2, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_wgrad(None, 8, None, 8, None, None, 1, 2, 9, 9, 8, 1, 2, 0, 0, None) == _lib.ERR_ARG
    # stride 3, dilation 0, a pixel stride below C, groups that do not divide B, an unknown dtype: refused before any launch
    assert L.sdhip_dw_dil_conv_fwd(P, 8, P, P, 8, None, 8, 1, 2, 9, 9, 8, 3, 2, 0, 1, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_fwd(P, 8, P, P, 8, None, 8, 1, 2, 9, 9, 8, 1, 0, 0, 1, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_fwd(P, 4, P, P, 8, None, 8, 1, 2, 9, 9, 8, 1, 2, 0, 1, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_fwd(P, 8, P, P, 8, None, 8, 1, 3, 9, 9, 8, 1, 2, 0, 2, 0, None) == _lib.ERR_ARG
    assert L.sdhip_dw_dil_conv_dgrad(P, 8, P, None, 0, P, 8, 2, 9, 9, 8, 1, 2, 7, None) == _lib.ERR_ARG
    # a workspace sized for another shape is refused
    assert L.sdhip_dw_dil_wgrad_parts(2, 9, 9, 8, 1) == 1 and L.sdhip_dw_dil_wgrad_parts(2, 9, 9, 8, 3) < 0
    assert L.sdhip_dw_dil_conv_wgrad(P, 8, P, 8, P, P, 5, 2, 9, 9, 8, 1, 2, 0, 0, None) == _lib.ERR_ARG
    assert 1 < L.sdhip_dw_dil_wgrad_parts(8, 33, 65, 2048, 1) <= 256


def test_update_bn_eps_touches_the_encoder_only():
    DM, _ = _mods()
    m = DM.SPPNet(output_channels=2)
    m.update_bn_eps()
    enc = {id(x) for x in m.encoder.modules()}
    bns = [x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)]
    assert all(x.eps == (1e-3 if id(x) in enc else 1e-5) for x in bns)
    assert sum(id(x) in enc for x in bns) == 132 and len(bns) == 156
    assert [id(p) for p in m.get_1x_lr_params()] == [id(p) for p in m.encoder.parameters()]
    ten = [id(p) for p in m.get_10x_lr_params()]
    assert ten == [id(p) for mod in (m.spp, m.logits, m.decoder) for p in mod.parameters()]
    m.train()
    m.freeze_bn()
    assert m.training and not any(x.training for x in bns)


def dwdil_ref(x, w, gy, stride, d, relu):
    """float64 numpy reference of the dilated depthwise 3x3 (forward, data gradient, weight gradient; input ReLU)."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((B, C, H + 2 * d, W + 2 * d))
    xp[:, :, d:d + H, d:d + W] = np.maximum(x, 0) if relu else x
    gxp = np.zeros_like(xp)
    y = np.zeros((B, C, Ho, Wo))
    gw = np.zeros((C, 1, 3, 3))
    for kh in range(3):
        for kw in range(3):
            sl = (slice(None), slice(None), slice(kh * d, kh * d + (Ho - 1) * stride + 1, stride),
                  slice(kw * d, kw * d + (Wo - 1) * stride + 1, stride))
            wk = w[None, :, 0, kh, kw, None, None]
            y += wk * xp[sl]
            gw[:, 0, kh, kw] = (gy * xp[sl]).sum((0, 2, 3))
            gxp[sl] += wk * gy
    gx = gxp[:, :, d:d + H, d:d + W]
    return y, gx * (x > 0) if relu else gx, gw


@pytest.mark.parametrize("C,H,W,d,stride", [(3, 5, 7, 2, 1), (4, 9, 6, 4, 1), (2, 7, 8, 1, 2), (3, 6, 5, 12, 1), (2, 8, 9, 3, 2)])
@pytest.mark.parametrize("relu", [False, True])
def test_numpy_reference_equals_aten_in_f64(C, H, W, d, stride, relu):
    x = randn_input(3, "ref:x:%d%d%d" % (C, H, d), (2, C, H, W)).double()
    w = randn_input(3, "ref:w:%d" % C, (C, 1, 3, 3), 0.3).double()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gy = randn_input(3, "ref:g:%d%d" % (C, Ho), (2, C, Ho, Wo)).double()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(F.relu(xr) if relu else xr, wr, None, stride, d, d, C)
    assert tuple(yr.shape) == (2, C, Ho, Wo)
    yr.backward(gy)
    y, gx, gw = dwdil_ref(x.numpy(), w.numpy(), gy.numpy(), stride, d, relu)
    for got, want in ((y, yr.detach()), (gx, xr.grad), (gw, wr.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)


def test_fixture_is_small_and_carries_the_deviations():
    path = os.path.join(GDIR, "deeplab.npz")
    assert os.path.getsize(path) <= 1 << 20
    gold = _gold()
    data = [k for k in gold.files if not k.endswith((".dev", ".step")) and k not in ("keys", "meta.corr") and ".bf16dev." not in k]
    assert len(data) > 300 and all(k + ".dev" in gold.files and float(gold[k + ".dev"]) >= 0 for k in data)
    for tag, name, mode, _, _, _ in MG.NETS:
        if mode == "eval":
            for n in MG.OUTS[name]:
                assert 0 < float(gold["net.%s.bf16dev.%s" % (tag, n)]) < 0.2
    # the quantities whose bar comes from the reference's own deviation (module docstring)
    wide = sorted(k for k in data if _bar(gold, k, _base(k)) != _base(k))
    ok = re.compile(r"blk\.\w+\.grad\.[\w.]*bn_depth\.bias\.l2$|net\.\w+\.train\.gnorm\.(encoder|spp)$|net\.mod\.train\.(head\.x|out\.seg1)$")
    assert wide and all(ok.match(k) for k in wide), wide


def _base(key):
    if key.startswith("blk."):
        return 1e-4 if re.match(r"blk\.\w+\.y\d$", key) else 1e-3
    return 2e-2 if ".gnorm." in key else 1e-3


# ------------------------------------------------------------------ GPU: the kernels against the float64 reference
SHAPES = [(8, 5, 7, 2, 1), (20, 9, 13, 4, 1), (412, 6, 5, 1, 1), (64, 33, 65, 12, 1), (24, 13, 12, 12, 1), (16, 33, 65, 36, 1),
          (2048, 5, 7, 24, 1), (5, 1, 1, 2, 1),
          (728, 64, 65, 2, 1),                        # enough workgroups that a thread walks 2 (bf16) / 3 (f32) pixels, the last partly
          (128, 9, 13, 1, 2), (20, 8, 7, 2, 2)]       # stride 2: the entry-flow sep_conv3 (upstream only with dilation 1)
# (input ReLU, statistics groups, slab), fully crossed.  slab: None = a tensor of its own (pixel stride C rounded up to 8),
# 'aligned' = channels [8, 8+C) of a wider slab with 16-byte aligned pixels, 'odd' = channels [3, 3+C) of a slab with an odd
# pixel stride (the element-wise path)
VARIANTS = [(relu, groups, slab) for relu in (False, True) for groups in (1, 2) for slab in (None, 'aligned', 'odd')]


def _slab_geometry(C, slab):
    if slab is None:
        return 0, (C + 7) & ~7
    if slab == 'aligned':
        return 8, (8 + C + 8 + 7) & ~7
    return 3, (3 + C + 5) | 1


def _nan_slab(shape, off, ld, dtype, fill=None):
    """Channels [off, off+C) of a NaN-filled NHWC slab with pixel stride ld, holding `fill` (B,C,H,W) if given: (view, slab)."""
    B, C, H, W = shape
    slab = torch.full((B, H, W, ld), float('nan'), dtype=dtype, device="cuda")
    if fill is not None:
        slab[..., off:off + C] = fill.cuda().permute(0, 2, 3, 1)
    return slab[..., off:off + C].permute(0, 3, 1, 2), slab


def _pads_untouched(slab, off, C):
    bits = slab.view(torch.int16 if slab.dtype == torch.bfloat16 else torch.int32)
    nan = torch.full((1,), float('nan'), dtype=slab.dtype, device=slab.device).view(bits.dtype)
    return bool((bits[..., :off] == nan).all()) and bool((bits[..., off + C:] == nan).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,H,W,d,stride", SHAPES)
def test_dilated_depthwise_matches_f64_reference(dtype, C, H, W, d, stride):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    B = 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = randn_input(13, "dwd:x:%d:%d:%d" % (C, H, W), (B, C, H, W)).to(dtype)
    w = randn_input(13, "dwd:w:%d" % C, (C, 1, 3, 3), 0.3)
    gy = randn_input(13, "dwd:gy:%d:%d:%d" % (C, Ho, Wo), (B, C, Ho, Wo)).to(dtype)
    refs = {r: dwdil_ref(x.double().numpy(), w.double().numpy(), gy.double().numpy(), stride, d, r) for r in (False, True)}
    dt = _lib.F32 if dtype == torch.float32 else _lib.BF16
    wd = w.cuda()
    nparts = _lib._lib.sdhip_dw_dil_wgrad_parts(B, H, W, C, stride)
    assert nparts >= 1
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for relu, groups, slab in VARIANTS:
        off, ld = _slab_geometry(C, slab)
        xv, xs = _nan_slab((B, C, H, W), off, ld, dtype, x)
        gv, gs = _nan_slab((B, C, Ho, Wo), off, ld, dtype, gy)
        yv, ys = _nan_slab((B, C, Ho, Wo), off, ld, dtype)
        gxv, gxs = _nan_slab((B, C, H, W), off, ld, dtype)
        runs = []
        for _ in range(2):
            stats = torch.zeros((3, groups, 2, C + 2), dtype=torch.float64, device="cuda")
            call("sdhip_dw_dil_conv_fwd", ptr(xv), ld, ptr(wd), ptr(yv), ld, ptr(stats), C + 2, 3, B, H, W, C, stride, d, int(relu), groups,
                 dt, stream_ptr())
            call("sdhip_dw_dil_conv_dgrad", ptr(gv), ld, ptr(wd), ptr(xv) if relu else None, ld, ptr(gxv), ld, B, H, W, C, stride, d, dt,
                 stream_ptr())
            gw = torch.zeros_like(wd)
            part = torch.full((nparts * 9 * C,), float('nan'), device="cuda")     # every slot must be written before it is read
            call("sdhip_dw_dil_conv_wgrad", ptr(xv), ld, ptr(gv), ld, ptr(gw), ptr(part), nparts, B, H, W, C, stride, d, int(relu), dt,
                 stream_ptr())
            torch.cuda.synchronize()
            runs.append((stats, gw))
        what = (C, H, W, d, stride, relu, groups, slab)
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what     # bit-equal over two launches
        for s_, o_ in ((xs, off), (gs, off), (ys, off), (gxs, off)):
            assert _pads_untouched(s_, o_, C), what
        y_ref, gx_ref, gw_ref = refs[relu]
        for name, got, want, t in (("y", yv, y_ref, tol), ("gx", gxv, gx_ref, tol), ("gw", gw, gw_ref, 1e-5)):
            got = got.double().cpu().numpy()
            assert np.isfinite(got).all(), (name, what)
            scale = float(np.abs(want).max()) + 1e-30
            err = float(np.abs(got - want).max()) / scale
            print("dwdil", what, name, "err/scale %.3e (bar %.0e)" % (err, t))
            assert err <= t, (name, what, err, t)
        # statistics: (sum, sum of squares) of the STORED output per group, replicas added.  At these shapes a workgroup
        # adds at most 256 values per channel in f32 before the f64 atomics: (n - 1) * 2^-24 <= 1.6e-5 of sum |y| at worst
        ysto = yv.double().cpu().numpy().reshape(groups, B // groups, C, Ho * Wo)
        st = stats.sum(0).cpu().numpy()
        assert not st[:, :, C:].any(), what
        for g in range(groups):
            s1, s2 = ysto[g].sum((0, 2)), (ysto[g] ** 2).sum((0, 2))
            assert np.abs(st[g, 0, :C] - s1).max() <= 2e-5 * np.abs(ysto[g]).sum((0, 2)).max() + 1e-30, what
            assert np.abs(st[g, 1, :C] - s2).max() <= 2e-5 * s2.max() + 1e-30, what


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,H,W", [(412, 6, 5), (1536, 5, 7), (2048, 5, 7)])
def test_existing_depthwise_kernels_accept_the_deeplab_channel_counts(dtype, stride, C, H, W):
    """sdhip_dw_conv_* (k 3, dilation 1) at the channel counts of the DeepLab networks, against the same float64 reference:
    412 is no multiple of the bf16 chunk, 1536 / 2048 exceed MobileNetV3's widest layer.  The DeepLab modules do not call
    these kernels (they have no input ReLU); this records that they take the shapes as they are."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.ops import alloc_nhwc, nhwc_view
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    B = 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = randn_input(17, "dw1:x:%d" % C, (B, C, H, W)).to(dtype)
    w = randn_input(17, "dw1:w:%d" % C, (C, 1, 3, 3), 0.3)
    gy = randn_input(17, "dw1:gy:%d:%d" % (C, stride), (B, C, Ho, Wo)).to(dtype)
    refs = dwdil_ref(x.double().numpy(), w.double().numpy(), gy.double().numpy(), stride, 1, False)
    xv, ldx = nhwc_view(x.cuda().contiguous(memory_format=torch.channels_last))
    gv, ldg = nhwc_view(gy.cuda().contiguous(memory_format=torch.channels_last))
    wd = w.cuda()
    dt = _lib.dtype_code(xv)
    y, ldy = alloc_nhwc(B, C, Ho, Wo, dtype, "cuda")
    gx, ldgx = alloc_nhwc(B, C, H, W, dtype, "cuda")
    call("sdhip_dw_conv_fwd", ptr(xv), ldx, ptr(wd), ptr(y), ldy, None, C, 1, None, 0, B, H, W, C, 3, stride, 1, dt, stream_ptr())
    call("sdhip_dw_conv_dgrad", ptr(gv), ldg, ptr(wd), ptr(gx), ldgx, B, H, W, C, 3, stride, dt, stream_ptr())
    gw = torch.zeros_like(wd)
    nparts = _lib.dw_wgrad_parts(B, H, W, C, 3, stride)
    part = torch.full((nparts * 9 * C,), float('nan'), device="cuda")
    call("sdhip_dw_conv_wgrad", ptr(xv), ldx, ptr(gv), ldg, ptr(gw), ptr(part), nparts, B, H, W, C, 3, stride, dt, stream_ptr())
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for name, got, want, t in (("y", y, refs[0], tol), ("gx", gx, refs[1], tol), ("gw", gw, refs[2], 1e-5)):
        got = got.double().cpu().numpy()
        assert np.isfinite(got).all(), name
        err = float(np.abs(got - want).max()) / (float(np.abs(want).max()) + 1e-30)
        assert err <= t, (name, err, t)


# ------------------------------------------------------------------ GPU: blocks and networks against the reference fixture
def _flat_close(gold, key, t, base, what):
    want = gold[key]
    got = t.detach().float().reshape(-1)[::int(gold[key + ".step"])].cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bar = _bar(gold, key, base)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    assert err <= bar, (what, err, bar)


def _stat_close(gold, key, t, what):
    want = gold[key]
    bar = _bar(gold, key, 1e-3)
    err = float((np.abs(t.detach().float().cpu().numpy() - want) / (0.1 + np.abs(want))).max())
    assert err <= bar, (what, err, bar)


BLOCK_CASES = MG.block_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_block_matches_reference_fixture(case):
    DM, _ = _mods()
    gold = _gold()
    tag, make, shapes, outs_of = case
    p = "blk.%s" % tag
    m = fill_state_dict(make(DM), MG.SEED_BLK).cuda().train()
    xs = {k: randn_input(MG.SEED_BLK, "%s:%s" % (p, k), s).cuda().requires_grad_(True) for k, s in shapes.items()}
    outs = outs_of(m, xs)
    loss = 0
    for i, y in enumerate(outs):
        loss = loss + (y * randn_input(MG.SEED_BLK, "%s:w%d" % (p, i), tuple(y.shape)).cuda()).sum()
        _flat_close(gold, "%s.y%d" % (p, i), y, 1e-4, "y%d" % i)
    loss.backward()
    for k, x in xs.items():
        _flat_close(gold, "%s.g%s" % (p, k), x.grad, 1e-3, "g" + k)
    for n, prm in m.named_parameters():
        key = "%s.grad.%s" % (p, n)
        _flat_close(gold, key, prm.grad, 1e-3, n)
        l2, want = float(prm.grad.double().pow(2).sum().sqrt()), float(gold[key + ".l2"])
        assert abs(l2 - want) <= _bar(gold, key + ".l2", 1e-3) * max(1e-3, want), (n, l2, want)
    for n, b in m.named_buffers():
        if n.endswith(("running_mean", "running_var")):
            _stat_close(gold, "%s.buf.%s" % (p, n), b, n)


def _native_net(name, channels=19, seed=MG.SEED_NET):
    DM, D = _mods()
    m = (DM if name == "deeplab_mod" else D).SPPNet(output_channels=channels, harness=True)
    m.update_bn_eps()
    m = fill_state_dict(m, seed).cuda()
    m.spp.dropout.p = 0.0        # as the fixture: deterministic
    return m


def _sampled(t):
    from test_nets import _sample
    return _sample(t, MG.HEAD_STRIDE)


def _run(m, name, left, right):
    return m(left, right)[:3] if name == "deeplab_mod" else (m(left),)


def _heads(m, name, left, right):
    """The network's own outputs (1/4 resolution) on the inputs the harness prepares."""
    m.harness = False
    try:
        pad = lambda t: F.pad(t, [0, 1, 0, 1])
        return _run(m, name, pad(left * 2 - 1), pad(right))
    finally:
        m.harness = True


@pytest.mark.gpu
@pytest.mark.parametrize("tag,name,mode,B,h,w", MG.NETS, ids=[n[0] for n in MG.NETS])
def test_network_matches_reference_fixture(tag, name, mode, B, h, w):
    gold = _gold()
    p = "net.%s" % tag
    left, right, seg, disp = (t.cuda() for t in MG.net_inputs(tag, B, h, w))
    m = _native_net(name)
    m.train() if mode == "train" else m.eval()
    with torch.no_grad():
        heads = _heads(copy.deepcopy(m) if mode == "train" else m, name, left, right)     # train: the running statistics move once
    for n, t in zip(MG.HEADS[name], heads):
        assert tuple(t.shape[2:]) == ((h + 1 + 3) // 4, (w + 1 + 3) // 4)
        _close_sample(gold, "%s.head.%s" % (p, n), t)
    with torch.set_grad_enabled(mode == "train"):
        outs = _run(m, name, left, right)
        loss = MG.net_loss(name, [o.float() for o in outs], seg, disp)
    for n, t in zip(MG.OUTS[name], outs):
        assert tuple(t.shape[2:]) == (h, w)
        _close_sample(gold, "%s.out.%s" % (p, n), t)
        key = "%s.out.%s.mean" % (p, n)
        assert abs(float(t.detach().double().mean()) - float(gold[key])) <= _bar(gold, key, 1e-3) * max(1.0, abs(float(gold[key]))), key
    want = float(gold[p + ".loss"])
    assert abs(float(loss) - want) <= _bar(gold, p + ".loss", 1e-3) * max(1.0, abs(want)), (float(loss), want)
    if name == "deeplab_mod":
        # the same value from the step's own loss kernels (ops.train_loss, what TrainStep calls; the fixture has no Lovasz
        # term); in train mode the backward below starts from it
        from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
        with torch.set_grad_enabled(mode == "train"):
            loss = ops.train_loss(outs[0], outs[1], outs[2], seg, disp, False)
        assert abs(float(loss) - want) <= _bar(gold, p + ".loss", 1e-3) * max(1.0, abs(want)), ("ops.train_loss", float(loss), want)
    if mode != "train":
        return
    loss.backward()
    acc = {}
    for k, q in m.named_parameters():
        if q.grad is not None:
            top = k.split(".")[0]
            acc[top] = acc.get(top, 0.0) + float(q.grad.double().pow(2).sum())
    wanted = {k[len(p + ".gnorm."):]: float(gold[k]) for k in gold.files if k.startswith(p + ".gnorm.") and not k.endswith(".dev")}
    assert set(acc) == set(wanted), set(acc) ^ set(wanted)
    for top, v in wanted.items():
        bar = _bar(gold, "%s.gnorm.%s" % (p, top), 2e-2)
        assert abs(math.sqrt(acc[top]) - v) <= bar * max(v, 1e-3), (top, math.sqrt(acc[top]), v, bar)
    sd = m.state_dict()
    for k in MG.BN_KEYS[name]:
        _stat_close(gold, "%s.rm.%s" % (p, k), sd[k + ".running_mean"], k)
        _stat_close(gold, "%s.rv.%s" % (p, k), sd[k + ".running_var"], k)


def _close_sample(gold, key, t):
    want, got = gold[key], _sampled(t)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    bar = _bar(gold, key, 1e-3)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    assert err <= bar, (key, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,name,mode,B,h,w", [n for n in MG.NETS if n[2] == "eval"], ids=[n[0] for n in MG.NETS if n[2] == "eval"])
def test_bf16_eval_per_head_within_twice_the_storage_deviation(tag, name, mode, B, h, w):
    """bf16 eval against the float64 reference, relative L2 of the sampled outputs per head.  The cap is twice what bf16
    STORAGE alone costs the reference (fixture: Conv2d / BatchNorm2d weights and outputs rounded by hooks) — twice, because
    the accumulation order and the fused roundings differ; it is not a number taken from the HIP path."""
    gold = _gold()
    left, right, _, _ = (t.cuda() for t in MG.net_inputs(tag, B, h, w))
    m = _native_net(name).eval()
    with torch.no_grad():
        outs = _run(m, name, left.bfloat16(), right.bfloat16())
    assert outs[0].dtype == torch.bfloat16
    errs = {}
    for n, t in zip(MG.OUTS[name], outs):
        want = gold["net.%s.out.%s" % (tag, n)]
        errs[n] = (float(MG.rel_l2(_sampled(t), want)), 2 * float(gold["net.%s.bf16dev.%s" % (tag, n)]))
    print("bf16 eval rel L2 (got, cap) %s: %s" % (tag, errs))
    for n, (e, cap) in errs.items():
        assert e <= cap, (tag, n, errs)


# ------------------------------------------------------------------ GPU: harness
@pytest.mark.gpu
def test_harness_steps():
    tag, name, _, B, h, w = MG.NETS[2]
    assert (B, h, w) == (1, 40, 72)
    left, right, _, _ = (t.cuda() for t in MG.net_inputs(tag, B, h, w))
    m = _native_net(name).eval()
    with torch.no_grad():
        outs = m(left, right)
        assert len(outs) == 4 and outs[3] is outs[1] and all(tuple(o.shape[2:]) == (h, w) for o in outs)
        assert outs[0].shape[1] == 19 and outs[1].shape[1] == 1 and outs[2].shape[1] == 19
        # the same steps by hand (ATen), the right image NOT rescaled: equal; with the right image rescaled too: different
        up = lambda y: F.interpolate(y.float(), size=(h + 1, w + 1), mode='bilinear', align_corners=True)[..., :h, :w]
        by_hand = [up(t) for t in _heads(m, name, left, right)]
        rescaled = [up(t) for t in _heads(m, name, left, right * 2 - 1)]
    # seg1 never sees the right image; in disp1 and seg2 a rescaled right image must show two orders of magnitude above what
    # separates the resize kernel from ATen's
    for n, o, a, b in zip(("seg1", "disp1", "seg2"), outs[:3], by_hand, rescaled):
        scale = float(a.abs().max())
        same, other = float((o - a).abs().max()) / scale, float((o - b).abs().max()) / scale
        print("harness %s: by hand %.3e, right image rescaled %.3e (of max|out|)" % (n, same, other))
        assert same <= 1e-4, (n, same)
        assert other <= 1e-4 if n == "seg1" else other > 100 * max(same, 1e-6), (n, same, other)
    # gradients reach both images through the stem
    m.train()
    l, r = left.clone().requires_grad_(True), right.clone().requires_grad_(True)
    outs = m(l, r)
    (outs[0].float().mean() + outs[1].float().mean() + outs[2].float().mean()).backward()
    for g in (l.grad, r.grad):
        assert g is not None and tuple(g.shape) == (B, 3, h, w) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float(m.encoder.conv1.weight.grad.abs().max()) > 0


# ------------------------------------------------------------------ GPU: training step
REPLAY_TOL = 1e-3     # as tests/test_mobilenet.py: the depthwise weight gradients are order-fixed; the remaining f32 atomics move ~1e-6


def _step_model(seed=5):
    return _native_net("deeplab_mod", channels=2, seed=seed).train()


def _batch():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch
    return synthetic_batch(2, 32, 48)


def _step_state(ts):
    st = [ts.flat_p, ts.exp_avg, ts.exp_avg_sq, ts.beta_pow, ts.ctx.seed]
    return st + [b for _, b in sorted(ts.model.named_buffers())]


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.gpu
def test_graph_replay_matches_eager():
    """Two replays of the captured step against two eager steps FROM THE SAME STATE: parameters, Adam moments, running
    statistics and dropout seed of the eager run after its two warm-up steps are copied into the captured step's buffers,
    then both sides step twice.  Compared within REPLAY_TOL: the loss of both steps (the second is computed from the
    parameters the first step's backward and Adam update produced), and after the first step the whole flat gradient buffer
    (the captured backward, the depthwise weight gradients that add into it included) and both Adam moments (the captured
    update), as relative L2 over the buffer.  The parameters themselves are not compared element-wise: a parameter whose true
    gradient is zero (bn_depth.bias of the relu_first blocks) holds rounding noise in its gradient, and Adam turns that into a
    step of size ~lr with a sign that differs from run to run; the output does not depend on it.

    Independent runs, the pattern of tests/test_mobilenet.py, were measured on this step instead of assumed (losses at steps
    3 / 4, bar 1e-3 * loss = 5.4e-3): eager vs eager differed by 1.1e-3 / 2.7e-3; graph vs eager by 4.6e-4 / 3.2e-3 in one
    pair of runs and by 6.5e-3 / 3.4e-2 in another — SGD and Adam at lr 5e-6 scatter alike.  At B=2 the 32x48 crop leaves 5x7
    maps, the image-pooling BatchNorm sees two values per channel, and the rounding noise of one step (3e-7 at step 2) grows
    by orders of magnitude per step: that comparison passes or fails by the draw, whatever the capture does."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    eager = TrainStep(_step_model(), dtype=torch.float32, use_graph=False, lr=1e-4)
    for _ in range(2):
        eager(*batch)
    ops.set_step_context(None)
    graph = TrainStep(_step_model(), dtype=torch.float32, use_graph=True, lr=1e-4)
    graph.capture(*batch, warmup=2)
    ops.set_step_context(None)
    with torch.no_grad():
        for dst, src in zip(_step_state(graph), _step_state(eager)):
            assert dst.shape == src.shape and dst.dtype == src.dtype
            dst.copy_(src)
    before = graph.flat_p.clone()
    got, want = [], []
    for step in range(2):
        got.append(float(graph(*batch)))
        want.append(float(eager(*batch)))
        ops.set_step_context(None)
        if step == 0:
            assert float(eager.flat_g.abs().max()) > 0 and not torch.equal(graph.flat_p, before)
            errs = {n: _rel_l2(getattr(graph, n), getattr(eager, n)) for n in ("flat_g", "exp_avg", "exp_avg_sq")}
            print("replay vs eager after one step, relative L2: %r" % errs)
            for n, e in errs.items():
                assert e <= REPLAY_TOL, (n, errs)
    print("replay %r, eager %r" % (got, want))
    for g, w in zip(got, want):
        assert math.isfinite(g) and abs(g - w) <= REPLAY_TOL * max(1.0, abs(w)), (got, want)
    assert want[1] < want[0]


@pytest.mark.gpu
def test_checkpoint_round_trip_keeps_the_reference_keys(tmp_path):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, checkpoint as ck
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    a = TrainStep(_step_model(), dtype=torch.float32, use_graph=False, lr=1e-4)
    for _ in range(2):
        a(*batch)
    path = ck.save_checkpoint(ck.make_state(a, 1), 0.0, 0.0, 1.0, 1.0, filename=str(tmp_path / "dl"))
    want = float(a(*batch))
    ops.set_step_context(None)
    saved = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    ref_keys = json.loads(_gold()["keys"].tobytes().decode())["deeplab_mod2"]["state_dict"]
    assert [[k, list(v.shape)] for k, v in saved.items()] == [["module." + k, s] for k, s in ref_keys]
    b = TrainStep(_step_model(77), dtype=torch.float32, use_graph=False, lr=1e-4)
    ck.load_checkpoint_and_params(path, b)
    got = float(b(*batch))
    ops.set_step_context(None)
    assert abs(got - want) <= 2e-3 * max(1.0, abs(want)), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_poisoned_allocations_do_not_reach_the_outputs(dtype, monkeypatch):
    """Every fresh allocation of the forward / backward filled with NaN first: an output or gradient that read memory
    nobody wrote would turn NaN."""
    import pmt_learning_for_semantic_segmentation_and_disparity_amd.ops as O
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float('nan'))
        return t
    monkeypatch.setattr(O.torch, "empty", poisoned)
    tag, name, _, B, h, w = MG.NETS[0]
    left, right, seg, disp = (t.cuda() for t in MG.net_inputs(tag, B, h, w))
    m = _native_net(name).train()
    outs = m(left.to(dtype), right.to(dtype))
    loss = MG.net_loss(name, [o.float() for o in outs[:3]], seg, disp)
    loss.backward()
    assert math.isfinite(float(loss))
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
