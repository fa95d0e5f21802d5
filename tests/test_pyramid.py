"""The pyramid entry points of pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/pyramid.hip — sdhip_pyramid_upcat_fwd / _bwd — against the float64
references of tests/rowops_ref.py, composed per branch, and against the single-tensor launches they replace (bit for bit where
the arithmetic is the same).

Bounds: those of tests/test_resample.py (b_resize, b_resize_bwd, b_avgpool_bwd), composed:
  slab         x-part: a copy, bound 0 (equality); branch j: b_resize of map j.
  map grads    b_resize_bwd of the slab gradient's slice j.
  tap grad     avgpool_bwd of the pooled map's gradient (b_avgpool_bwd) plus the x-part of the slab's gradient: one f32
               addition (u |sum|) and the store.
Without a GPU: the composed references reject the plausible mistakes at these bounds.  With a GPU (marker `gpu`): the C ABI
directly, every tensor a channel slice of a NaN-filled slab; then nn._pyramid and one minidsnetExt training step, fused
against composed (SDHIP_DIAG_NO_PYRAMID_FUSE=1), each in a fresh child process (the switches are read once, at import).
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from rowops_ref import U32, Rows, check, quant  # noqa: E402
from test_resample import b_avgpool_bwd, b_resize, b_resize_bwd, code, img, st  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
CAP = 4096 * 256
CHANNELS = [pytest.param(64, 32, id="C64_Cb32"), pytest.param(16, 8, id="C16_Cb8")]


# =========================================================================== composed references and bounds
def upcat_ref(x, maps, H, W, mode=1, x_off=0):
    """x_off: wrong reference, the branches start x_off channels early (over the end of x)."""
    C = x.shape[-1]
    y = np.concatenate([np.asarray(x, np.float64)] + [R.resize(m, H, W, mode) for m in maps], -1)
    if x_off:
        y[..., C - x_off:-x_off] = y[..., C:].copy()
    return y


def b_upcat(x, maps, H, W, dtype):
    shape = x.shape[:3] + (maps[0].shape[-1],)
    return np.concatenate([np.zeros(x.shape)] + [np.broadcast_to(b_resize(m, H, W, 1, dtype), shape) for m in maps], -1)


def upcat_bwd_ref(g, C, Cb, sizes, shifted_window=True):
    return [R.resize_bwd(g[..., C + j * Cb:C + (j + 1) * Cb], h, w, 1, shifted_window=shifted_window) for j, (h, w) in enumerate(sizes)]


def tap_grad_ref(G0, addend, k, dtype, quarter=1.0):
    """(avgpool_bwd_k(G0) + addend, its bound); quarter: wrong reference, the pool's 1 / k^2 applied with another factor."""
    H, W = k * G0.shape[1], k * G0.shape[2]
    up = R.avgpool_bwd(G0, H, W, k)
    e = b_avgpool_bwd(G0, H, W, k, dtype)
    s = up * quarter + np.asarray(addend, np.float64)
    e = e + U32 * (np.abs(s) + e)
    return s, e + st(s, dtype, e) + 1e-300


def lanes(n_in, n_out):
    """bwd_lanes of csrc/resample_common.h."""
    span = 2.0 / float(np.float32(n_in) / np.float32(n_out)) + 5.0
    return 16 if span >= 32 else 4 if span >= 12 else 1


# =========================================================================== CPU
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_comparator_rejects_wrong_pyramids(dtype):
    rng = np.random.default_rng(3)
    B, H, W, C, Cb = 1, 32, 64, 16, 8
    sizes = [(1, 2), (2, 4), (4, 8)]
    x = quant(rng.standard_normal((B, H, W, C)), dtype)
    maps = [quant(rng.standard_normal((B, h, w, Cb)), dtype) for h, w in sizes]
    good, bound = upcat_ref(x, maps, H, W), b_upcat(x, maps, H, W, dtype)
    assert R.worst_ratio(good, good, bound) == 0.0
    assert R.worst_ratio(upcat_ref(x, maps[::-1], H, W)[..., C:], good[..., C:], b_upcat(x, maps[::-1], H, W, dtype)[..., C:]) > 1   # branch order
    assert R.worst_ratio(upcat_ref(x, maps, H, W, mode=2), good, bound) > 1                                   # align_corners flipped
    assert R.worst_ratio(upcat_ref(x, maps, H, W, x_off=8), good, bound) > 1                                  # x-part off by a unit
    g = quant(rng.standard_normal(good.shape), dtype)
    want = upcat_bwd_ref(g, C, Cb, sizes)
    for j, (h, w) in enumerate(sizes):
        e = b_resize_bwd(g[..., C + j * Cb:C + (j + 1) * Cb], h, w, 1, dtype)
        assert R.worst_ratio(upcat_bwd_ref(g, C, Cb, sizes, shifted_window=False)[j], want[j], e) > 1         # unshifted window
        if j != len(sizes) - 1 - j:                                                                             # branch order
            assert R.worst_ratio(upcat_bwd_ref(g, C, Cb, sizes[::-1])[len(sizes) - 1 - j], want[j], e) > 1
    # the tap gradient with the pool's 1 / k^2 applied twice
    G0, add = quant(rng.standard_normal((B, 4, 8, C)), dtype), quant(rng.standard_normal((B, 32, 64, C)), dtype)
    want, e = tap_grad_ref(G0, add, 8, dtype)
    assert R.worst_ratio(want, want, e) == 0.0 and R.worst_ratio(tap_grad_ref(G0, add, 8, dtype, quarter=1 / 64)[0], want, e) > 1


def test_pyr_map_matches_the_typedef():
    """_lib.PyrMap is written by hand: member names, order and kinds are those of SdhipPyrMap in include/sdhip.h."""
    import re
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    with open(os.path.join(ROOT, "include", "sdhip.h")) as f:
        body = re.search(r"typedef\s+struct\s+SdhipPyrMap\s*\{(.*?)\}\s*SdhipPyrMap\s*;", f.read(), flags=re.S).group(1)
    want = []
    for decl in body.split(";"):
        if decl.strip():
            kind = ctypes.c_void_p if "*" in decl else ctypes.c_int
            want += [(n.strip(), kind) for n in decl.replace("void*", "").replace("int ", "").split(",")]
    assert [(n, t) for n, t in _lib.PyrMap._fields_] == want


# =========================================================================== GPU: the C ABI
SLICE = lambda C: (8, C + 16)        # channels [8, 8 + C) of a slab: 16-byte aligned in both dtypes, pads on both sides


def run(name, *args):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()


def table(rows_hw):
    """HOST table of [(Rows or None, h, w)]"""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    t = (_lib.PyrMap * len(rows_hw))()
    for e, (r, h, w) in zip(t, rows_hw):
        e.p, e.h, e.w, e.ld = (r.v.data_ptr() if r is not None else None), h, w, (r.ld if r is not None else 0)
    return t


def tptr(t):
    return ctypes.cast(t, ctypes.c_void_p)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _intact(*rows):
    for r in rows:
        assert r.pads_intact(), "an element outside the slice changed"


def copy_into(src, dst, off, C, dtype):
    """sdhip_affine_act as the copy _ConcatFn makes: src rows -> channels [off, off + C) of dst."""
    n = src.v.shape[0]
    run("sdhip_affine_act", src.p, src.ld, ctypes.c_void_p(dst.v[:, off:].data_ptr()), dst.ld, None, 0, None, None, n, C, 1, 0, code(dtype))


def _upcat_case(label, dtype, B, H, W, C, Cb, sizes, seed, composed=True, splits=None):
    rng = np.random.default_rng([H, W, C, Cb, len(sizes), seed])
    n, Ct = len(sizes), C + len(sizes) * Cb
    x = quant(rng.standard_normal((B, H, W, C)), dtype)
    maps = [quant(rng.standard_normal((B, h, w, Cb)), dtype) for h, w in sizes]
    xd = Rows(B * H * W, C, dtype, SLICE(C), x)
    md = [Rows(B * h * w, Cb, dtype, SLICE(Cb), m) for m, (h, w) in zip(maps, sizes)]
    yd = Rows(B * H * W, Ct, dtype, SLICE(Ct))
    t = table([(r, h, w) for r, (h, w) in zip(md, sizes)])
    run("sdhip_pyramid_upcat_fwd", xd.p, xd.ld, tptr(t), n, yd.p, yd.ld, B, H, W, C, Cb, code(dtype))
    _intact(xd, yd, *md)
    check(label + " fwd", img(yd.np(), B, H, W), upcat_ref(x, maps, H, W), b_upcat(x, maps, H, W, dtype))
    if composed:      # the launches of interpolate + concat
        y2 = Rows(B * H * W, Ct, dtype, SLICE(Ct))
        copy_into(xd, y2, 0, C, dtype)
        for j, (h, w) in enumerate(sizes):
            up = Rows(B * H * W, Cb, dtype)
            run("sdhip_resize_fwd", md[j].p, md[j].ld, up.p, up.ld, B, h, w, Cb, H, W, 1, 0.0, 0.0, code(dtype))
            copy_into(up, y2, C + j * Cb, Cb, dtype)
        _intact(y2)
        assert torch.equal(bits(yd.v), bits(y2.v)), label + ": the slab differs from resize_fwd + copies"
    # backward: the slab gradient read in place
    g = quant(rng.standard_normal((B, H, W, Ct)), dtype)
    gd = Rows(B * H * W, Ct, dtype, SLICE(Ct), g)
    gm = [Rows(B * h * w, Cb, dtype, SLICE(Cb)) for h, w in sizes]
    tmp = torch.full((B * H * Cb * sum(w for _, w in sizes),), float('nan'), device="cuda")
    tg = table([(r, h, w) for r, (h, w) in zip(gm, sizes)])
    run("sdhip_pyramid_upcat_bwd", gd.p, gd.ld, tptr(tg), n, tmp.data_ptr(), B, H, W, C, Cb, code(dtype))
    _intact(gd, *gm)
    assert bool(torch.isfinite(tmp).all())
    want = upcat_bwd_ref(g, C, Cb, sizes)
    for j, (h, w) in enumerate(sizes):
        gj = g[..., C + j * Cb:C + (j + 1) * Cb]
        e = b_resize_bwd(gj, h, w, 1, dtype)
        got = img(gm[j].np(), B, h, w)
        check("%s bwd map %d" % (label, j), got, want[j], e)
        check("%s bwd map %d mass" % (label, j), got.sum((1, 2)), gj.sum((1, 2)), e.sum((1, 2)))
        if splits is not None:
            splits.update((lanes(h, H), lanes(w, W)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Cb", CHANNELS)
def test_upcat(dtype, C, Cb):
    """Maps 1x2, 2x4, 4x8 under a 32x64 tap (x32 .. x8: 16 and 4 lanes per item in the backward); then 16x32 (x2: one lane)
    beside 3x5 (a ratio that is no integer).  The slab has the bits of resize_fwd + copies; the three lane splits occur."""
    splits = set()
    _upcat_case("upcat pyramid", dtype, 2, 32, 64, C, Cb, [(1, 2), (2, 4), (4, 8)], 1, splits=splits)
    _upcat_case("upcat x2 + odd", dtype, 2, 32, 64, C, Cb, [(16, 32), (3, 5)], 2, splits=splits)
    assert splits == {1, 4, 16}, splits


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_upcat_capped_grid(dtype):
    """C = 16, Cb = 8, one 3x5 map: 3 (bf16) / 6 (f32) units per pixel.  419 x 835 (bf16) / 296 x 591 (f32) pixels are the
    smallest such images with more than CAP = 4096 x 256 items: one trip and a ragged second."""
    H, W = (419, 835) if dtype == BF16 else (296, 591)
    units = 24 // (8 if dtype == BF16 else 4)
    assert CAP < H * W * units < CAP + 2048
    _upcat_case("upcat capped", dtype, 1, H, W, 16, 8, [(3, 5)], 3, composed=False)


@pytest.mark.gpu
def test_upcat_declines_what_it_cannot_vectorise():
    """A slice that starts one element in is no whole number of 16-byte units: SDHIP_ERR_UNSUPPORTED, nothing written."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    B, H, W, C, Cb = 1, 4, 8, 16, 8
    xd = Rows(B * H * W, C, BF16, "misal", np.ones((B * H * W, C)))
    md = Rows(B * 2 * 4, Cb, BF16, SLICE(Cb), np.ones((B * 2 * 4, Cb)))
    yd = Rows(B * H * W, C + Cb, BF16, SLICE(C + Cb))
    t = table([(md, 2, 4)])
    rc = _lib._lib.sdhip_pyramid_upcat_fwd(xd.p, xd.ld, tptr(t), 1, yd.p, yd.ld, B, H, W, C, Cb, 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and bool(torch.isnan(yd.slab).all())
    rc = _lib._lib.sdhip_pyramid_upcat_fwd(xd.p, xd.ld, tptr(t), 9, yd.p, yd.ld, B, H, W, C, Cb, 1, _lib.stream_ptr())      # > 8 maps
    assert rc == _lib.ERR_ARG and _lib._lib.sdhip_last_error().decode()


# =========================================================================== GPU: modules, fused against composed
_CHILD = r"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
from oracle.detweights import fill_state_dict, rand_input
from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, ops

out = sys.argv[1]
if sys.argv[2] == "pyramids":
    m = fill_state_dict(N.piramidNet2(False, 'densenet'), 22).cuda().train()      # f32 parameters, bf16 activations
    pooled, avgpool = [], ops.avgpool
    def recording(x, k):                      # the first pool of a pyramid (k = 8, of the tap): its total gradient is wanted
        y = avgpool(x, k)
        if k == 8 and y.requires_grad:
            y.retain_grad()
            pooled.append(y)
        return y
    ops.avgpool = recording
    res = {}
    shapes = [(64, 128, 128, 5), (128, 64, 64, 4), (256, 32, 32, 3)]          # the taps of a 256 x 256 image, 2 x 2 groups
    for i, (C, H, W, n) in enumerate(shapes):
        x = rand_input(40 + i, "tap", (4, C, H, W)).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = N._pyramid([getattr(m, 'branch%%d_%%d' %% (i, j)) for j in range(n)], x, 2)
        wgt = rand_input(50 + i, "w", tuple(y.shape)).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        y.backward(wgt)
        torch.cuda.synchronize()
        res["slab%%d" %% i] = y.detach().float().cpu().numpy()
        res["gtap%%d" %% i] = x.grad.float().permute(0, 2, 3, 1).cpu().numpy()
        res["wx%%d" %% i] = wgt[:, :C].float().permute(0, 2, 3, 1).cpu().numpy()
        res["gpool%%d" %% i] = pooled[i].grad.float().permute(0, 2, 3, 1).cpu().numpy()
    np.savez(out, **res)
else:
    m = fill_state_dict(N.minidsnetExt(N.CFG(dropout=0.0, aspp=0, use_att=1), labels=2, pretrained=False, patch_type='1dcorr', backbone='densenet'), 31).cuda().train()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("resnet_features.branch0_")}
    a = rand_input(31, "left", (2, 3, 256, 256)).cuda().to(torch.bfloat16)
    b = rand_input(31, "right", (2, 3, 256, 256)).cuda().to(torch.bfloat16)
    outs = m(a, b)
    loss = sum(o.float().square().mean() for o in outs[:3])
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": np.float64(loss.item())}
    for i in range(3):
        res["out%%d" %% i] = outs[i].detach().float().cpu().numpy()
    for k, v in m.state_dict().items():
        if k.startswith("resnet_features.branch0_") and ("running" in k or "num_batches" in k):
            res["bn." + k] = v.detach().double().cpu().numpy()
            res["bn0." + k] = before[k].double().cpu().numpy()
    gr = {k: (None if p.grad is None else float(p.grad.abs().max())) for k, p in m.named_parameters() if k.startswith("resnet_features.branch0_")}
    res["branch0_grads"] = np.array(json.dumps(gr))
    np.savez(out, **res)
"""


def _child(tmp, what, tag, **env):
    path = os.path.join(tmp, "%s_%s.npz" % (what, tag))
    script = os.path.join(tmp, "child.py")
    with open(script, "w") as f:
        f.write(_CHILD % {"root": ROOT})
    e = dict(os.environ)
    e.pop("SDHIP_DIAG_NO_PYRAMID_FUSE", None)
    e.update(env)
    r = subprocess.run([sys.executable, script, path, what], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(path)


@pytest.mark.gpu
def test_pyramids_fused_against_composed():
    """nn._pyramid on the three taps of a 256 x 256 image (the smallest the 128-pixel pool accepts), B = 2 x 2 groups, bf16:
    the slabs of the fused path have the bits of the composed one; on either path the tap gradient lies within the bound of
    the f64 composition of that path's own inputs (avgpool_bwd of the pooled map's total gradient + the x-part of the slab
    gradient), and the two paths agree within the sum of their bounds."""
    with tempfile.TemporaryDirectory() as tmp:
        fused = _child(tmp, "pyramids", "fused")
        comp = _child(tmp, "pyramids", "composed", SDHIP_DIAG_NO_PYRAMID_FUSE="1")
        for i in range(3):
            assert np.array_equal(fused["slab%d" % i], comp["slab%d" % i]), "slab %d" % i
            bounds = []
            for tag, res in (("fused", fused), ("composed", comp)):
                want, e = tap_grad_ref(res["gpool%d" % i], res["wx%d" % i], 8, BF16)
                check("tap %d gradient, %s" % (i, tag), res["gtap%d" % i], want, e)
                bounds.append(e)
            check("tap %d gradient, composed against fused" % i, comp["gtap%d" % i], fused["gtap%d" % i], bounds[0] + bounds[1])


def _ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


@pytest.mark.gpu
def test_minidsnet_step_without_the_unread_slab():
    """minidsnetExt in the benchmark's configuration at 256 x 256 (the smallest size tests/test_nets.py uses), bf16, one forward
    + backward: outputs and loss of the fused path (no b0 slab) equal the composed path's within twice what two runs of the
    composed path differ by (the step has unordered float atomics); the branch0_* running statistics moved and agree within
    4 f32 ulps (f64 atomic sums, one f32 rounding can flip, two more f32 operations follow in the update); the branch0_*
    parameter gradients are absent or zero on both paths."""
    with tempfile.TemporaryDirectory() as tmp:
        c1 = _child(tmp, "step", "composed1", SDHIP_DIAG_NO_PYRAMID_FUSE="1")
        c2 = _child(tmp, "step", "composed2", SDHIP_DIAG_NO_PYRAMID_FUSE="1")
        fu = _child(tmp, "step", "fused")
        for key in ["loss"] + ["out%d" % i for i in range(3)]:
            noise = float(np.abs(c1[key] - c2[key]).max())
            diff = float(np.abs(fu[key] - c1[key]).max())
            print("%s: composed twice %.3g, fused against composed %.3g" % (key, noise, diff))
            assert diff <= 2 * noise, (key, diff, noise)
        moved = 0
        for key in [k for k in fu.files if k.startswith("bn.")]:
            if "num_batches" in key:
                assert fu[key] == c1[key] and fu[key] > fu["bn0." + key[3:]], key      # one count per tower
                continue
            assert _ulps32(fu[key], c1[key]).max() <= 4, (key, _ulps32(fu[key], c1[key]).max())
            moved += int((fu[key] != fu["bn0." + key[3:]]).any())
        assert moved == 10, moved        # running_mean and running_var of the five branches
        for res in (fu, c1):
            gr = json.loads(str(res["branch0_grads"]))
            assert gr and all(v is None or v == 0.0 for v in gr.values()), gr
