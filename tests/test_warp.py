"""The disparity warp (ops.apply_disparity / ops.warp_blend, csrc/warp.hip) and the warp networks minidsnetDivide /
minidsnetDivideSoftmax (warp.py) against tests/golden/warp.npz, which tools/make_golden_warp.py computes with the reference's
own apply_disparity and networks on the CPU."""
import ctypes
import inspect
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
NEW_SYMBOLS = ("sdhip_warp_blend_fwd", "sdhip_warp_blend_bwd")
SEED = 7
OP_TOL = 1e-5          # relative to the largest expected magnitude: bit-equal weights, one fused multiply-add, sums over <= 19 channels
REPLAY_TOL = 1e-3      # tests/test_mobilenet.py's convention: captured replay against eager steps (f32 atomics move ~1e-6)


def _gold():
    return np.load(os.path.join(GDIR, "warp.npz"))


def _cases():
    return json.loads(str(_gold()["cases"]))


def _keys():
    return json.loads(str(_gold()["keys"]))


def _native(tag):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, warp
    k = _keys()[tag]
    return getattr(warp, k["cls"])(N.CFG(**k["cfg"]), labels=k["labels"], pretrained=False, patch_type=k["patch"],
                                   include_edges=k["edges"], backbone=k["backbone"])


ALL_TAGS = ["div_1d", "div_2d", "div_mb", "soft_1d", "div_l19", "div_a1_edges", "div_mb_a1", "soft_a1_edges", "soft_mb"]


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_constructs_with_the_reference_keys_and_parameter_order(tag):
    """1-D / 2-D correlation, include_edges, aspp 0 / 1, both backbones, 2 / 8 / 19 labels."""
    assert sorted(_keys()) == sorted(ALL_TAGS)
    k = _keys()[tag]
    m = _native(tag)
    assert [[n, list(v.shape)] for n, v in m.state_dict().items()] == k["state_dict"]
    assert [n for n, _ in m.named_parameters()] == k["parameters"]
    assert m.three_outputs


def test_softmax_network_ignores_its_backbone_argument():
    a, b = _keys()["soft_mb"], _keys()["soft_1d"]
    assert a["backbone"] == "mobilenet" and [n for n, _ in a["state_dict"]] == [n for n, _ in b["state_dict"]]


@pytest.mark.parametrize("backbone", ["resnet50", "resnet101"])
def test_unsupported_backbones_raise(backbone):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, warp
    with pytest.raises(NotImplementedError):
        warp.minidsnetDivide(N.CFG(), labels=2, backbone=backbone)
    with pytest.raises(NotImplementedError):
        warp.piramidNet2Warp(backbone=backbone)


def test_new_symbols_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n


def _fwd(L, left=16, ldl=8, right=16, ldr=8, disp=16, ldd=1, sign=1.0, gate=16, ldgt=1, gch=1, smax=0, warped=16, ldw=8, both=16,
         ldb=8, prob=None, ldp=0, B=1, H=2, W=9, C=5, dt=0):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return L.sdhip_warp_blend_fwd(p(left), ldl, p(right), ldr, p(disp), ldd, sign, p(gate), ldgt, gch, smax, p(warped), ldw, p(both),
                                  ldb, p(prob), ldp, B, H, W, C, dt, None)


def _bwd(L, g_both=16, ldgb=8, g_warped=16, ldgw=8, left=16, ldl=8, right=16, ldr=8, disp=16, ldd=1, sign=-1.0, gate=16, ldgt=1,
         gch=1, smax=0, g_left=16, ldgl=8, g_right=16, ldgr=8, g_disp=16, ldgd=1, g_gate=16, ldgg=1, B=1, H=2, W=9, C=5, dt=0):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return L.sdhip_warp_blend_bwd(p(g_both), ldgb, p(g_warped), ldgw, p(left), ldl, p(right), ldr, p(disp), ldd, sign, p(gate), ldgt,
                                  gch, smax, p(g_left), ldgl, p(g_right), ldgr, p(g_disp), ldgd, p(g_gate), ldgg, B, H, W, C, dt, None)


def test_malformed_arguments_are_rejected_without_gpu_work():
    """Every call below would fault if a pointer were dereferenced or a kernel launched (the pointers are the address 16)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    L, E = _lib._lib, _lib.ERR_ARG
    for fn in (_fwd, _bwd):
        assert fn(L, right=None) == E and b"null" in L.sdhip_last_error()
        assert fn(L, disp=None) == E
        assert fn(L, gch=3) == E and b"must be 1 or C" in L.sdhip_last_error()            # gate channels neither 1 nor C
        assert fn(L, gch=1, smax=1) == E                                                   # softmax gate with one channel
        assert fn(L, ldd=0) == E and b"ONE channel" in L.sdhip_last_error()                # disp is one channel, stride >= 1
        assert fn(L, ldr=4) == E                                                           # pixel stride below the channel count
        assert fn(L, left=None) == E                                                       # a gate without seg_left
        assert fn(L, W=0) == E and fn(L, C=0) == E and fn(L, dt=7) == E
        assert fn(L, sign=0.5) == E
        assert fn(L, gate=None, gch=1) == E                                                # gate shape without a gate
    assert _fwd(L, warped=None) == E
    assert _fwd(L, both=None) == E                                                         # a gate without `both`
    assert _fwd(L, gate=None, gch=0, left=None, both=16) == E                              # `both` without a gate
    assert _fwd(L, gch=5, ldgt=8, smax=1, prob=None) == E                                  # softmax gate without `prob`
    assert _bwd(L, g_both=None, g_warped=None) == E
    assert _bwd(L, gate=None, gch=0, left=None, g_left=None, g_gate=None) == E             # g_both without a gate
    assert _bwd(L, W=30000) == E and b"LDS" in L.sdhip_last_error()                        # row longer than the LDS accumulator
    assert _bwd(L, ldgg=0) == E


def test_ops_refuse_cpu_tensors():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, SdhipError
    x, d = torch.zeros(1, 2, 3, 5), torch.zeros(1, 1, 3, 5)
    with pytest.raises(SdhipError):
        ops.apply_disparity(x, d)
    with pytest.raises(SdhipError):
        ops.warp_blend(x, x, d, d)
    with pytest.raises(SdhipError):
        ops.warp_blend(x, x, d, None)


def test_train_loss_third_term_is_opt_in():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    assert inspect.signature(ops.train_loss).parameters["seg3"].default is None


def test_fixture_offsets_keep_their_margin():
    """No j + offset of the fixture lies within 1e-3 of an integer unless it is exactly one, so the reference alone decides
    every pixel of every operator case (none is left out of the comparisons below)."""
    gold = _gold()
    for tag, B, C, H, W, _ in _cases()["op"]:
        off = gold["op.%s.offset" % tag]
        x = (np.arange(W, dtype=np.float32) + off).astype(np.float64)
        d = np.abs(x - np.round(x))
        assert not ((d > 0) & (d < 1e-3)).any(), tag


# ------------------------------------------------------------------ GPU: operator
def _slab(x, C, k, ld):
    """x (B,C,H,W) as channels [k, k+C) of an NHWC slab with pixel stride ld; the rest of the slab holds NaN."""
    B, _, H, W = x.shape
    slab = torch.full((B, H, W, ld), float('nan'), dtype=x.dtype, device=x.device)
    slab[..., k:k + C] = x.permute(0, 2, 3, 1)
    return slab[..., k:k + C].permute(0, 3, 1, 2)


def _close(got, want, what):
    want = np.asarray(want)
    got = got.detach().float().cpu().numpy()
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("%s: max err %.3e, largest expected %.3e" % (what, err, scale))
    assert err <= OP_TOL * max(scale, 1e-30), "%s: max err %.3e > %.0e * %.3e" % (what, err, OP_TOL, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("case", _cases()["op"] if os.path.exists(os.path.join(GDIR, "warp.npz")) else [], ids=lambda c: c[0])
def test_apply_disparity_matches_reference_fixture(case, slab):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    tag, B, C, H, W, _ = case
    gold = _gold()
    img0 = randn_input(SEED, tag + ":img", (B, C, H, W)).cuda()
    g = randn_input(SEED, tag + ":g", (B, C, H, W)).cuda()
    off0 = torch.from_numpy(gold["op.%s.offset" % tag]).cuda()
    if slab:     # channel slices of NaN-filled slabs with padded pixel strides
        img = _slab(img0, C, 3, ((C + 3 + 7) & ~7) + 8).requires_grad_(True)
        off = _slab(off0, 1, 2, 8).requires_grad_(True)
        g = _slab(g, C, 1, C + 3)
    else:
        img = img0.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        off = off0.clone().requires_grad_(True)
    out = ops.apply_disparity(img, off)
    out.backward(g)
    _close(out, gold["op.%s.out" % tag], tag + ".out")
    _close(img.grad, gold["op.%s.g_img" % tag], tag + ".g_img")
    _close(off.grad, gold["op.%s.g_offset" % tag], tag + ".g_offset")
    # the three edge rules, exactly
    x = torch.arange(W, dtype=torch.float32, device="cuda") + off0            # (B,1,H,W), the reference's f32 sum
    right = (x >= W - 1).expand(B, C, H, W)
    left = (x <= 0).expand(B, C, H, W)
    assert bool((out.detach()[right] == 0).all())                                                    # right edge: zero, not the edge pixel
    assert torch.equal(out.detach()[left], img0[..., :1].expand(B, C, H, W)[left])                   # left edge: column 0
    assert bool((off.grad[(x < 0) | (x > W - 1)] == 0).all())                                        # no offset gradient under the clamp
    if tag == "zero":    # identity except in the last column, which is zero
        assert torch.equal(out.detach()[..., :W - 1], img0[..., :W - 1]) and bool((out.detach()[..., W - 1] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("case", _cases()["blend"] if os.path.exists(os.path.join(GDIR, "warp.npz")) else [], ids=lambda c: c[0])
def test_warp_blend_matches_reference_fixture(case, slab):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    tag, B, C, H, W, smax = case
    gold = _gold()
    mk = lambda n: randn_input(SEED, tag + ":" + n, (B, C, H, W)).cuda()
    left, right, g1, g2 = mk("l"), mk("r"), mk("g1"), mk("g2")
    gate = (randn_input(SEED, tag + ":gate", (B, C, H, W)) if smax else rand_input(SEED, tag + ":gate", (B, 1, H, W), 0.05, 0.95)).cuda()
    disp = torch.from_numpy(gold["blend.%s.disp" % tag]).cuda()
    if slab:
        ld = ((C + 2 + 7) & ~7) + 8
        left, right = _slab(left, C, 2, ld), _slab(right, C, 1, ld)
        gate = _slab(gate, gate.shape[1], 3, gate.shape[1] + 5)
        disp = _slab(disp, 1, 5, 8)
    else:
        left, right = (t.contiguous(memory_format=torch.channels_last) for t in (left, right))
    left, right, gate, disp = (t.requires_grad_(True) for t in (left, right, gate, disp))
    outs = ops.warp_blend(left, right, disp, gate, softmax_gate=smax)
    assert len(outs) == (3 if smax else 2)
    (outs[0] * g1 + outs[1] * g2).sum().backward()
    p = "blend.%s." % tag
    _close(outs[0], gold[p + "both"], p + "both")
    _close(outs[1], gold[p + "warped"], p + "warped")
    if smax:
        assert not outs[2].requires_grad
        _close(outs[2], gold[p + "prob"], p + "prob")
    for name, t in (("g_left", left), ("g_right", right), ("g_disp", disp), ("g_gate", gate)):
        _close(t.grad, gold[p + name], p + name)


def _fractional_offsets(shape, gen):
    """An integer in [-6, 5] plus k/8, k = 1..7: never an integer, and exact in bf16 too (|offset| < 8: three integer bits and
    three fraction bits)."""
    whole = torch.randint(-6, 6, shape, generator=gen).float()
    frac = torch.randint(1, 8, shape, generator=gen).float() / 8.0
    return whole + frac


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_warp_properties_at_cityscapes_size(dtype):
    """B=4, C=19, 512x1024: integer offsets are a column shift, bit for bit; <warp(x), g> == <x, warp^T(g)>; every gradient
    is finite; two runs agree (bit-equal except g_img, whose LDS float adds have no fixed order: DESIGN.md section 2)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    B, C, H, W = 4, 19, 512, 1024
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((B, H, W, C), generator=gen).to(dtype).cuda().permute(0, 3, 1, 2)
    g = torch.randn((B, H, W, C), generator=gen).to(dtype).cuda().permute(0, 3, 1, 2)
    # integer offsets: out[..., j] = x[..., j + off] for j + off <= W-2 (clamped on the left to column 0), 0 from W-1 on
    off = torch.randint(-5, 6, (B, 1, H, W), generator=gen).to(dtype).cuda()
    out = ops.apply_disparity(x, off)
    src = torch.arange(W, device="cuda").view(1, 1, 1, W) + off.long()
    want = torch.gather(x, 3, src.clamp(0, W - 1).expand(B, C, H, W))
    want = torch.where((src >= W - 1).expand(B, C, H, W), torch.zeros_like(want), want)
    assert torch.equal(out, want)
    del out, want, src
    # fractional offsets: adjoint identity in float64 on the host, from the op's outputs
    off = _fractional_offsets((B, 1, H, W), gen).to(dtype).cuda()
    runs = []
    for _ in range(2):
        xr, o = x.detach().requires_grad_(True), off.detach().requires_grad_(True)
        out = ops.apply_disparity(xr, o)
        out.backward(g)
        runs.append((out.detach(), xr.grad, o.grad))
    out, gx, go = runs[0]
    assert all(bool(torch.isfinite(t).all()) for t in (out, gx, go))
    lhs_terms = out.cpu().double() * g.cpu().double()
    rhs_terms = x.cpu().double() * gx.cpu().double()
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    if dtype == torch.float32:
        bound = 1e-5 * max(abs(lhs), abs(rhs))
    else:   # every stored element of `out` and `gx` is rounded once to bf16: at most 2^-9 of each term
        bound = 2.0 ** -9 * (float(lhs_terms.abs().sum()) + float(rhs_terms.abs().sum()))
    print("adjoint %s: <warp(x), g> = %.9e, <x, warp^T(g)> = %.9e, bound %.3e" % (dtype, lhs, rhs, bound))
    assert abs(lhs - rhs) <= bound
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    d = float((runs[0][1].float() - runs[1][1].float()).abs().max())
    # f32: a handful of adds per source pixel in another order; bf16: the f32 sum is rounded once, so at most one bf16 ulp
    tol = (1e-5 if dtype == torch.float32 else 2.0 ** -7) * float(gx.float().abs().max())
    print("g_img between two runs %s: max diff %.3e (tolerance %.3e)" % (dtype, d, tol))
    assert d <= tol


def _reference_blend(left, right, disp, gate):
    """The issue's formulas on the CPU: coordinates and weights in f32 in the reference's order, everything after them in
    float64 (inputs are float64 leaves).  gate: (B,C,H,W) blend weights."""
    B, C, H, W = right.shape
    x = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W) + (-disp.detach().float())
    inside = ((x >= 0) & (x <= W - 1)).double()
    x = torch.clamp(x, 0.0, W - 1)
    x0 = torch.floor(x)
    x1 = (x0 + 1).clamp(max=W - 1)
    i0, i1 = x0.long().expand(B, C, H, W), x1.long().expand(B, C, H, W)
    r0, r1 = right.gather(3, i0), right.gather(3, i1)
    # d(warped)/d(disp) = -(r1 - r0) where the clamp is inactive: carried by a term that is 0 in value
    frac = (x - x0).double() - inside * (disp - disp.detach())
    warped = (x1 - x).double() * r0 + (x - x0).double() * r1 + (frac - (x - x0).double()) * (r1 - r0).detach()
    return (1 - gate) * left + gate * warped, warped


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_wider_than_the_lds_accumulator_split_into_channel_groups(dtype):
    """W * C = 1100 * 19 > 20480 accumulator floats: the row scatter runs as two channel groups (18 + 1 channels: a second
    grid row, a tail group narrower than the first, per-pixel strided stores), here with a per-channel gate, which that launch
    reads at the group's channel offset.  Comparator: the issue's formulas in float64 on the CPU (_reference_blend) on the same
    (for bf16: the rounded) inputs.  f32 at the operator bar 1e-5; bf16 within 2^-7 of the largest expected magnitude (outputs
    and gradients are rounded once, 2^-9 relative, and `both` / the gate gradient use the warped map as stored: one more rounding)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    B, C, H, W = 2, 19, 3, 1100
    gen = torch.Generator().manual_seed(13)
    mk = lambda c: torch.randn((B, c, H, W), generator=gen).to(dtype)
    left, right, g1, g2 = mk(C), mk(C), mk(C), mk(C)
    gate = torch.rand((B, C, H, W), generator=gen).to(dtype)
    disp = (-_fractional_offsets((B, 1, H, W), gen)).to(dtype)
    disp[:, :, :, :40] += 64.0          # some pixels beyond the left edge ...
    disp[:, :, :, -40:] -= 64.0         # ... and some beyond the right edge; both sides compute j - disp in f32 from the same stored values
    ref_in = [t.double().requires_grad_(True) for t in (left, right, disp, gate)]
    rb, rw = _reference_blend(*ref_in)
    ((rb * g1.double()).sum() + (rw * g2.double()).sum()).backward()
    dev_in = [t.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in (left, right, disp, gate)]
    both, warped = ops.warp_blend(*dev_in)
    torch.autograd.backward([both, warped], [g1.cuda(), g2.cuda()])
    tol = OP_TOL if dtype == torch.float32 else 2.0 ** -7
    for name, got, want in [("both", both, rb), ("warped", warped, rw)] + \
            [(n, d.grad, r.grad) for n, d, r in zip(("g_left", "g_right", "g_disp", "g_gate"), dev_in, ref_in)]:
        want = want.detach().numpy()
        err = float(np.abs(got.detach().float().cpu().numpy() - want).max())
        scale = float(np.abs(want).max())
        print("%s %s: max err %.3e, largest expected %.3e" % (dtype, name, err, scale))
        assert err <= tol * scale, (name, err, scale)


@pytest.mark.gpu
def test_ops_refuse_mismatched_shapes_and_types():
    """The Python-level checks of ops._warp_check, behind the device check: GPU tensors of the wrong shape or type."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, SdhipError
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    x, d = z(1, 5, 3, 7), z(1, 1, 3, 7)
    for bad_disp in (z(1, 2, 3, 7), z(1, 1, 3, 8), z(2, 1, 3, 7), z(1, 3, 7), z(1, 1, 3, 7, dt=torch.bfloat16)):
        with pytest.raises(SdhipError):
            ops.apply_disparity(x, bad_disp)
    for bad_gate in (z(1, 3, 3, 7), z(1, 1, 3, 8), z(1, 1, 3, 7, dt=torch.bfloat16)):
        with pytest.raises(SdhipError):
            ops.warp_blend(x, x, d, bad_gate)
    with pytest.raises(SdhipError):
        ops.warp_blend(x, x, d, z(1, 1, 3, 7), softmax_gate=True)          # a softmax gate has C channels
    with pytest.raises(SdhipError):
        ops.warp_blend(z(1, 4, 3, 7), x, d, d)                              # seg_left and seg_right differ
    with pytest.raises(SdhipError):
        ops.warp_blend(x, x, d, None)
    assert len(ops.warp_blend(x, x, d, z(1, 5, 3, 7), softmax_gate=True)) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("size_in,size_out", [((32, 32), (16, 16)), ((32, 64), (16, 32)), ((37, 23), (18, 11)), ((33, 31), (16, 15))])
def test_bilinear_downscale_matches_aten(size_in, size_out):
    """The x1/2 bilinear resize of the 1/8 pyramid branch to the 1/16 size (piramidNet2Warp): 32 channels, even and odd sizes;
    ATen on the CPU as comparator, the tolerances of tests/test_multitask.py::test_resize_backward_matches_aten."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, *size_in, generator=g)
    gy = torch.randn(2, 32, *size_out, generator=g)
    xr = x.clone().requires_grad_(True)
    F.interpolate(xr, size=size_out, mode="bilinear").backward(gy)
    xv = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.interpolate(xv, size=size_out, mode="bilinear")
    np.testing.assert_allclose(y.detach().cpu().numpy(), F.interpolate(x, size=size_out, mode="bilinear").numpy(), rtol=1e-5, atol=1e-5)
    y.backward(gy.cuda())
    np.testing.assert_allclose(xv.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ GPU: networks
OUT_NAMES = ("out0", "out1", "out2", "out3", "out4", "out5")


def _net_inputs(labels=2):
    a, b = rand_input(31, "left", (2, 3, 256, 256)), rand_input(31, "right", (2, 3, 256, 256))
    if labels == 2:
        lab = (rand_input(31, "seg", (2, 256, 256)) > 0.5).long()
    else:
        lab = (rand_input(31, "seg", (2, 256, 256)) * labels).long().clamp(0, labels - 1)
    seg = F.one_hot(lab, labels).permute(0, 3, 1, 2).float()
    disp = rand_input(31, "disp", (2, 1, 256, 256), 0.0, 8.0)
    return a.cuda(), b.cuda(), seg.cuda(), disp.cuda()


def _three_loss(outs, seg, disp):
    """The `ThreeOutPuts` sum with cross-entropy only, as the generator forms it (ATen, test side)."""
    from test_nets import train_loss
    return train_loss([o.float() for o in outs[:4]], seg, disp) + torch.mean(torch.sum(-seg * F.log_softmax(outs[4].float(), 1), 1))


def _trained_like_statistics(m, a, b):
    """The generator's three steps: momentum 1, one train-mode pass without gradients, momentum restored."""
    bns = [x for x in m.modules() if isinstance(x, torch.nn.modules.batchnorm._BatchNorm)]
    for x in bns:
        x.momentum = 1.0
    m.train()
    with torch.no_grad():
        m(a, b)
    for x in bns:
        x.momentum = 0.1
    return m.eval()


def _check(gold, key, t, tol, stride=16):
    from test_nets import _check as chk
    chk(gold, key, t, tol, stride)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,tm", [("div_1d", "train"), ("div_1d", "eval"), ("div_2d", "train"), ("div_mb", "train"),
                                    ("soft_1d", "train"), ("soft_1d", "eval"), ("div_l19", "eval")])
def test_network_matches_reference_fixture(tag, tm):
    gold = _gold()
    labels = _keys()[tag]["labels"]
    a, b, seg, disp = _net_inputs(labels)
    m = fill_state_dict(_native(tag), 31).cuda()
    if tm == "train":
        m.train()
        outs = m(a, b)
    else:       # float64 reference with trained-like running statistics: see the generator
        _trained_like_statistics(m, a, b)
        with torch.no_grad():
            outs = m(a, b)
    assert len(outs) == 6
    loss = _three_loss(outs, seg, disp)
    p = "net.%s.%s" % (tag, tm)
    for name, o in zip(OUT_NAMES, outs):
        _check(gold, "%s.%s" % (p, name), o, 1e-3)
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
@pytest.mark.parametrize("tag", ["div_a1_edges", "soft_a1_edges", "div_mb_a1"])
def test_edge_and_aspp_variants_train_finite(tag):
    """include_edges (4-channel inputs: the towers read three channels, the auxiliary convolutions four), CFG.aspp = 1 (an ASPP
    head that is built for its keys and never called), 2-D correlation, 8 labels, both backbones: one train-mode forward and
    backward with finite outputs and gradients, and the reference's output shapes."""
    k = _keys()[tag]
    a, b, _, disp = _net_inputs()
    if k["edges"]:
        a = torch.cat([a, rand_input(31, "edge_l", (2, 1, 256, 256)).cuda()], 1)
        b = torch.cat([b, rand_input(31, "edge_r", (2, 1, 256, 256)).cuda()], 1)
    lab = (rand_input(31, "seg", (2, 256, 256)) * 8).long().clamp(0, 7)
    seg = F.one_hot(lab, 8).permute(0, 3, 1, 2).float().cuda()
    m = fill_state_dict(_native(tag), 31).cuda().train()
    outs = m(a, b)
    gate_ch = 8 if k["cls"] == "minidsnetDivideSoftmax" else 1
    assert [tuple(o.shape) for o in outs] == [(2, c, 256, 256) for c in (8, 1, 8, 1, 8, gate_ch)]
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    _three_loss(outs, seg, disp).backward()
    assert not any(n.startswith("aspp.") and q.grad is not None for n, q in m.named_parameters())
    for n, q in m.named_parameters():
        if q.grad is not None:
            assert bool(torch.isfinite(q.grad).all()), n


# bf16 eval against the float64 reference, relative L2 of the strided samples per output (both / disp / seg_left / warped / gate
# for minidsnetDivide; seg_left / disp / both / warped / gate for minidsnetDivideSoftmax).  Measured on one MI355X:
#   div_1d  12.3 / 27.5 / 12.7 / 18.4 / 13.0 %
#   soft_1d 25.6 / 27.5 / 22.7 / 23.9 / 14.4 %
# (random weights leave the eval network far from a trained one's conditioning: tests/test_mobilenet.py measures 5-17 % on
# minidsnetExt the same way; the disparity head, 27.5 %, is the same tensor in both networks; a wrong tile or lane order gives
# errors near 100 %).  The caps are twice that (the convention of tests/test_bf16_parity.py).
BF16_HEADS = (0, 1, 2, 4, 5)
BF16_CAPS = {"div_1d": (0.25, 0.55, 0.26, 0.37, 0.27), "soft_1d": (0.52, 0.55, 0.46, 0.48, 0.29)}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(BF16_CAPS))
def test_bf16_eval_per_head_matches_reference(tag):
    from test_nets import _sample
    gold = _gold()
    a, b, _, _ = _net_inputs()
    m = fill_state_dict(_native(tag), 31).cuda()
    _trained_like_statistics(m, a, b)           # statistics collected in f32, as a trained checkpoint carries them
    with torch.no_grad():
        outs = m(a.bfloat16(), b.bfloat16())
    assert all(o.dtype == torch.bfloat16 for o in outs)
    errs = []
    for i in BF16_HEADS:
        want = gold["net.%s.eval.%s.sample" % (tag, OUT_NAMES[i])]
        got = _sample(outs[i], 16)
        errs.append(float(np.linalg.norm(got - want) / max(1e-12, np.linalg.norm(want))))
    print("bf16 eval rel L2 %s: %s" % (tag, ["%.4f" % e for e in errs]))
    for e, cap, i in zip(errs, BF16_CAPS[tag], BF16_HEADS):
        assert e <= cap, (tag, OUT_NAMES[i], errs, BF16_CAPS[tag])


# ------------------------------------------------------------------ GPU: training step
def _model(seed=5):
    torch.manual_seed(0)
    return fill_state_dict(_native("div_1d"), seed).cuda().train()


def _batch():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch
    return synthetic_batch(2, 256, 256)


@pytest.mark.gpu
def test_graph_replay_matches_eager_and_keeps_unreached_parameters():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    gold = _gold()
    batch = _batch()
    losses = {}
    for graph in (False, True):
        ts = TrainStep(_model(), dtype=torch.float32, use_graph=graph, lr=1e-4)
        before = {k: v.detach().clone() for k, v in ts.model.named_parameters()}
        rm = ts.model.resnet_features.branch3_1[1].layers[1].running_mean.clone()
        if graph:
            ts.capture(*batch, warmup=2)
            seq = [float(ts(*batch)) for _ in range(3)]
        else:
            seq = [float(ts(*batch)) for _ in range(5)][2:5]
        losses[graph] = seq
        assert all(math.isfinite(v) for v in seq), seq
        names = [k for k, _ in ts.model.named_parameters()]
        idle = {names[i] for i in ts.grad_free}
        assert idle == set(gold["net.div_1d.train.nograd"].tolist())          # the reference's list of parameters without a gradient
        for k, v in ts.model.named_parameters():
            if k in idle:
                assert torch.equal(v.detach(), before[k]), k                  # never reached: bit-identical
        assert not torch.equal(ts.model.segNet.conv1d_1[0].c2d.weight.detach(), before["segNet.conv1d_1.0.c2d.weight"])
        assert not torch.equal(ts.model.resnet_features.branch3_1[1].layers[1].running_mean, rm)    # discarded branch: statistics still move
        ops.set_step_context(None)
    print("eager %s, replayed %s" % (losses[False], losses[True]))
    for i in range(3):
        assert abs(losses[False][i] - losses[True][i]) <= REPLAY_TOL * max(1.0, abs(losses[False][i])), losses


@pytest.mark.gpu
def test_loss_falls_on_a_fixed_batch():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    ts = TrainStep(_model(), dtype=torch.float32, use_graph=False, lr=1e-4)
    seq = [float(ts(*batch)) for _ in range(20)]
    ops.set_step_context(None)
    print("losses", seq)
    assert all(math.isfinite(v) for v in seq) and seq[-1] < seq[0], seq


@pytest.mark.gpu
def test_train_loss_with_a_third_output_matches_aten():
    """ops.train_loss with seg3 (the loss kernels, a third cross-entropy call) equals the ATen sum over the same outputs, and the
    gradients autograd assembles for the blended map's two inputs equal those of the ATen loss."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    a, b, seg, disp = _net_inputs()
    grads = []
    for native in (True, False):
        m = fill_state_dict(_native("div_1d"), 31).cuda().train()
        outs = m(a, b)
        loss = ops.train_loss(outs[0], outs[1], outs[2], seg, disp, use_lovasz=False, seg3=outs[4]) if native else _three_loss(outs, seg, disp)
        loss.backward()
        grads.append((float(loss.detach()), {k: q.grad.double().norm().item() for k, q in m.named_parameters() if q.grad is not None}))
    assert abs(grads[0][0] - grads[1][0]) <= 1e-5 * abs(grads[1][0]), (grads[0][0], grads[1][0])
    assert set(grads[0][1]) == set(grads[1][1])
    for k, v in grads[1][1].items():
        assert abs(grads[0][1][k] - v) <= 1e-3 * max(v, 1e-6), (k, grads[0][1][k], v)


@pytest.mark.gpu
def test_train_step_trains_on_the_three_output_loss():
    """TrainStep itself: the loss its first eager step returns (f32, no Lovasz term) is the ATen `ThreeOutPuts` sum of the same
    model on the same batch - CE(outs[0]) + CE(outs[2]) + CE(outs[4]) + L1(outs[1]) - and the fixture's loss on the fixture's
    batch.  1e-5: the same f32 forward twice (bit-reproducible) and two summation orders of the loss terms."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    a, b, seg, disp = _net_inputs()
    m = fill_state_dict(_native("div_1d"), 31).cuda().train()
    with torch.no_grad():
        want = float(_three_loss(m(a, b), seg, disp))
    m = fill_state_dict(_native("div_1d"), 31).cuda().train()       # fresh running statistics, as the model above had
    ts = TrainStep(m, dtype=torch.float32, use_graph=False, use_lovasz=False, lr=1e-4)
    got = float(ts(a, b, seg, disp))
    ops.set_step_context(None)
    print("TrainStep %.7f, ATen %.7f, fixture %.7f" % (got, want, float(_gold()["net.div_1d.train.loss"])))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert abs(got - float(_gold()["net.div_1d.train.loss"])) <= 1e-3 * abs(want)


@pytest.mark.gpu
def test_checkpoint_round_trip_continues_the_run(tmp_path):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, checkpoint as ck
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    batch = _batch()
    a = TrainStep(_model(), dtype=torch.float32, use_graph=False, lr=1e-4)
    for _ in range(3):
        a(*batch)
    state = ck.make_state(a, 1)
    assert [k for k in state["state_dict"]] == ["module." + k for k, _ in _keys()["div_1d"]["state_dict"]]
    assert len(state["optimizer"]["state"]) == len(_keys()["div_1d"]["parameters"]) - len(a.grad_free)     # as torch.optim.Adam: none for idle parameters
    path = ck.save_checkpoint(state, 0.0, 0.0, 1.0, 1.0, filename=str(tmp_path / "warp"))
    want = [float(a(*batch)) for _ in range(2)]
    ops.set_step_context(None)
    b = TrainStep(_model(77), dtype=torch.float32, use_graph=False, lr=1e-4)
    ck.load_checkpoint_and_params(path, b)
    got = [float(b(*batch)) for _ in range(2)]
    ops.set_step_context(None)
    print("continued %s, uninterrupted %s" % (got, want))
    assert abs(got[0] - want[0]) <= 2e-3 * max(1.0, abs(want[0])), (got, want)
    # the second continued step runs on weights the restored Adam moments produced (the first is a forward on loaded weights)
    assert abs(got[1] - want[1]) <= 2e-2 * max(1.0, abs(want[1])), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag", ["div_1d", "soft_1d"])
def test_poisoned_allocations_do_not_reach_the_outputs(tag, dtype, monkeypatch):
    """Every fresh allocation of the forward/backward filled with NaN first (tests/diag/gpu_poison.py's rule): an output or
    gradient that read memory nobody wrote would turn NaN."""
    import pmt_learning_for_semantic_segmentation_and_disparity_amd.ops as O
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.is_cuda and t.is_floating_point():
            t.fill_(float('nan'))
        return t
    monkeypatch.setattr(O.torch, "empty", poisoned)
    a, b, seg, disp = _net_inputs()
    m = fill_state_dict(_native(tag), 31).cuda().train()
    outs = m(a.to(dtype), b.to(dtype))
    for name, o in zip(OUT_NAMES, outs):
        assert bool(torch.isfinite(o).all()), name
    loss = _three_loss(outs, seg, disp)
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k


# ------------------------------------------------------------------ GPU: data parallel
def _dp_step(m, a, b, seg, disp):
    outs = m(a, b)
    loss = _three_loss(outs, seg, disp)
    loss.backward()
    torch.cuda.synchronize()
    return ([o.detach().cpu().numpy() for o in outs], float(loss.detach()),
            {k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None},
            {k: v.cpu().numpy() for k, v in m.named_buffers() if "running" in k and k.startswith(("segNet.", "conv2d_ba0."))})


def _dp_rank_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import parallel
    parallel.configure(dist.group.WORLD, world)
    m = fill_state_dict(_native("div_1d"), 31).cuda().train()
    res = _dp_step(m, *_net_inputs())
    top = {}
    for k, g in res[2].items():
        top[k.split(".")[0]] = top.get(k.split(".")[0], 0.0) + float((g.astype(np.float64) ** 2).sum())
    q.put((rank, [o[:, :, ::16, ::16] for o in res[0]], res[1], top, res[3]))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_on_the_duplicated_batch_equal_one_rank():
    """minidsnetDivide, 2 gloo ranks that both hold the same batch: the sync-BN statistics of the joint batch equal those of
    the batch itself, so outputs, loss, per-rank gradients and the twice-updated running statistics of the shared SmallsegNet
    and of conv2d_ba0 equal the 1-rank step.  Bars: 1e-4 of the largest value for outputs (the same f32 kernels, statistics
    summed in another order), the suite's 1e-3 / 1e-4 for running statistics, 1e-3 for gradient norms per top-level module."""
    from test_parallel import _spawn2
    res = _spawn2(_dp_rank_worker, 29500 + (os.getpid() % 400))
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import parallel
    parallel.configure(None, 1)
    m = fill_state_dict(_native("div_1d"), 31).cuda().train()
    outs, loss, grads, bufs = _dp_step(m, *_net_inputs())
    top = {}
    for k, g in grads.items():
        top[k.split(".")[0]] = top.get(k.split(".")[0], 0.0) + float((g.astype(np.float64) ** 2).sum())
    for r in res:
        for o, w in zip(r[1], outs):
            w = w[:, :, ::16, ::16]
            assert np.abs(o - w).max() <= 1e-4 * max(1.0, np.abs(w).max())
        assert abs(r[2] - loss) <= 1e-4 * abs(loss)
        assert set(r[3]) == set(top)
        for k, v in top.items():
            assert abs(math.sqrt(r[3][k]) - math.sqrt(v)) <= 1e-3 * max(math.sqrt(v), 1e-6), (k, r[3][k], v)
        assert set(r[4]) == set(bufs) and len(bufs) >= 20
        for k, v in bufs.items():
            np.testing.assert_allclose(r[4][k], v, rtol=1e-3, atol=1e-4)
