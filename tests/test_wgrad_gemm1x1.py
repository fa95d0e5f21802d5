"""The pixel-contraction GEMM kernel of the 1x1 weight gradient (csrc/conv_wgrad_gemm1x1.h): bf16, 1x1 / stride 1 / unpadded,
BatchNorm(+ReLU) prologue on X, Cout a multiple of 128, Cin >= 96 — the DenseNet bottlenecks (models/densenet.py:25-93) and
transitions.  dW[m][k] = sum over pixels of dY[pix][m] * Xhat[pix][k].

Reference: Xhat is formed as the kernel forms it — fma(x, scale_g, shift_g) rounded once to f32, ReLU, rounded to bf16 — and
contracted with dY in float64 (tests/convops_ref.py).  Bound: the per-element bound tests/test_conv_kernels.py applies to its
bf16 prologue cases (wg_ref: npix u sum |dy Xhat| for the f32 accumulation in any order and any split over workgroups, plus
sum |dy| e_z for the prologue's two roundings).  Every case checks the packed buffer (pad rows / channel tails exactly zero,
nothing written past it), the unpacked gradient and the untouched padding of X and dY (gpu_wgrad of test_conv_kernels.py: the
operands are channel slices of NaN-filled slabs, the channels [Cin, ldx) of every pixel hold NaN), and the same inputs under
SDHIP_WGRAD_NO_GEMM=1 (the kernels this one replaces).

Shapes are the smallest that reach each way the kernel can go wrong: channel tails inside a 64-channel chunk and inside the
256-channel workgroup tile, several tile groups, several 128-output blocks, slabs of 64 pixels that end inside an image
(3x5: 15 of 64 rows real, 5x13: 64 + 1), two statistics groups with different coefficients (negative scales, shifts of
either sign and |shift| >= 0.25: relu(shift) on a masked row would show), one and many slab shares per workgroup.

Without a GPU: the library's own dispatch, asked in dry mode (test_conv_kernels.chosen: sdhip_dispatch_dry / sdhip_last_path),
names "gemm1x1" for every case, another kernel in f32, under SDHIP_WGRAD_NO_GEMM and under each switch the branch stands
aside for, and for each single violation of its predicate (wg_fast of csrc/conv_wgrad.hip, wgrad_gemm1x1_ok).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convops_ref as CR  # noqa: E402
import test_conv_kernels as K  # noqa: E402
import test_wgrad_group as G  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
NO_GEMM = {"SDHIP_WGRAD_NO_GEMM": "1"}
STAND_ASIDE = ("SDHIP_WGRAD_GENERIC", "SDHIP_WGRAD_FORCE_PACK", "SDHIP_WGRAD_NO_PACK")


def mk(name, B, H, W, Cin, Cout=128, ldx=None, groups=2, pro="relu", **kw):
    return K.mk(name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, kh=1, kw=1, pro=pro, groups=groups, lx=(0, ldx or Cin), ly="dense", **kw)


CASES = [mk("cin%d" % ci, 4, 16, 32, ci, ldx=1024) for ci in (96, 128, 160, 256, 288, 1024)]          # channel tails and widths
CASES += [mk("tiny3x5", 2, 3, 5, 160, ldx=192), mk("ragged5x13", 6, 5, 13, 128), mk("map8x16", 2, 8, 16, 512)]   # partial and tiny slabs
CASES += [mk("lin5x13", 4, 5, 13, 160, ldx=192, pro="lin")]                                              # no ReLU: masked rows would hold the shift
CASES += [mk("cout256", 2, 8, 16, 512, Cout=256), mk("cout512", 2, 4, 8, 1024, Cout=512)]             # several output blocks
SPLIT = mk("split64x128", 4, 64, 128, 96)                                                                # many slab shares
BY = {c.name: c for c in CASES + [SPLIT]}


def on_gemm1x1(c, dtype, env=None):
    """Does the dispatch of sdhip_conv2d_wgrad (csrc/conv_wgrad.hip: the GEMM branch of wg_fast) run the case on conv_wgrad_gemm1x1.h?"""
    return K.chosen(c, dtype, env, entry="wgrad") == "gemm1x1"


def test_gemm1x1_predicate():
    for c in CASES + [SPLIT]:
        assert on_gemm1x1(c, BF16), c.name
        assert not on_gemm1x1(c, F32), c.name
        assert not on_gemm1x1(c, BF16, NO_GEMM), c.name
        for sw in STAND_ASIDE:
            assert not on_gemm1x1(c, BF16, {sw: "1"}), (c.name, sw)
    base = dict(B=4, H=16, W=32, Cin=128, Cout=128, kh=1, kw=1, pro="relu", groups=2)
    assert on_gemm1x1(K.mk("ok", **base), BF16)
    for name, kw in (("cout64", dict(Cout=64)), ("cin64", dict(Cin=64)), ("t9", dict(kh=3, kw=3)), ("s2", dict(stride=2)),
                     ("nopro", dict(pro=None)), ("dbias", dict(dbias=1)), ("ldodd", dict(lx="ldodd")), ("cout136", dict(Cout=136))):
        assert not on_gemm1x1(K.mk(name, **dict(base, **kw)), BF16), name
    for c in K.WG + K.WGPACK:      # the tables of test_conv_kernels.py stay on the kernels they were written for
        assert not on_gemm1x1(c, BF16), c.name


_REFS = {}


def refs(c):
    """(draw, (dW, None, bound, None)) of a case, computed once."""
    if c.name not in _REFS:
        d = K.draw(c, BF16)
        g = CR.group_of(c.B, c.groups)
        sc, sh = (np.asarray(t, np.float64)[g][:, None, None, None, :] for t in (d.sc, d.sh))
        z = (CR._x5(d.x) * sc + sh).astype(np.float32).astype(np.float64)       # fmaf: the exact product, one f32 rounding
        xhat = K.quant(np.maximum(z, 0.0) if c.pro == "relu" else z, BF16)
        dW, _ = CR.wgrad(xhat, d.dy, 1, 1, 1)
        _, _, bW, _ = K.wg_ref(c, BF16, d)
        _REFS[c.name] = (d, (dW, None, bW, None))
    return _REFS[c.name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_gemm1x1_wgrad(name):
    c = BY[name]
    d, r = refs(c)
    new = K.gpu_wgrad(c, BF16, d)
    assert K.last_path() == "gemm1x1", (name, K.last_path())
    K.check_wgrad("gemm1x1 %s" % name, c, BF16, d, new, r)
    old = K.gpu_wgrad(c, BF16, d, NO_GEMM)
    assert K.family(K.last_path()) == "fast", (name, K.last_path())
    K.check_wgrad("gemm1x1 %s NO_GEMM" % name, c, BF16, d, old, r)
    K.check("gemm1x1 %s new vs old" % name, new[1], old[1], r[2])


def _as_layer(c, d):
    """The case as a layer of test_wgrad_group.py's helpers (NaN in the slab channels [Cin, ldx))."""
    dev = torch.device("cuda:0")
    Cin, ldx = d.Cin, c.lx[1]
    x = torch.full((c.B, c.H, c.W, ldx), float("nan"), dtype=BF16, device=dev)
    x[..., :Cin] = torch.from_numpy(d.x[:, 0]).to(BF16).to(dev)
    dy = torch.from_numpy(d.dy[:, 0]).to(BF16).to(dev).contiguous()
    sc, sh = (torch.from_numpy(np.ascontiguousarray(t)).float().to(dev) for t in (d.sc, d.sh))
    geo = (c.B, c.H, c.W, Cin, ldx, c.Ho, c.Wo, c.Cout, c.Cout, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1 if c.pro == "relu" else 0, c.groups)
    return dict(x=x, dy=dy, sc=sc, sh=sh, per=CR.packed_elems(c.Cout, Cin, 1, True), bias=False, geo=geo)


@pytest.mark.gpu
def test_pixel_split_alone_and_grouped():
    """64x128 maps, Cin = 96: many slab shares per (output block, chunk group), launched alone, as a group of one, and as a group
    of one limited to 96 workgroups: all within the bound of the reference, and equal up to the order of the f32 atomics."""
    c = SPLIT
    d, r = refs(c)
    K.check_wgrad("gemm1x1 split", c, BF16, d, K.gpu_wgrad(c, BF16, d), r)
    assert K.last_path() == "gemm1x1", K.last_path()
    K.check_wgrad("gemm1x1 split NO_GEMM", c, BF16, d, K.gpu_wgrad(c, BF16, d, NO_GEMM), r)
    assert K.family(K.last_path()) == "fast", K.last_path()
    L = _as_layer(c, d)
    dev = L["x"].device
    got = [G._run_single(L, dev)[0], G._run_group([L], dev, 0)[0][0], G._run_group([L], dev, 96)[0][0]]
    torch.cuda.synchronize()
    want, bound = CR.pack_conv(r[0], True)[0], CR.pack_conv(r[2], True)[0]
    for i, a in enumerate(got):
        K.check("gemm1x1 split launch %d packed" % i, a.double().cpu().numpy().reshape(want.shape), want, bound)
    n = float(got[0].norm())
    for a in got[1:]:
        assert float((a - got[0]).norm()) <= 2e-5 * n


@pytest.mark.gpu
def test_mixed_group_equals_per_layer_launches():
    """Eight bottlenecks of growing Cin on ONE slab and a transition over the whole slab, mixed with 3x3 layers, in one grouped
    call (max_workgroups 0 and 96): equal to the per-layer launches up to the order of the f32 atomics."""
    dev = torch.device("cuda:0")
    layers = []
    for i in range(8):
        layers.append(G._layer(dev, 4, 16, 32, 96 + 32 * i, 128, 1, ldx=512, pro=True, groups=2, seed=i))
        layers.append(G._layer(dev, 4, 16, 32, 128, 32, 3, pro=True, groups=2, seed=100 + i))
    layers.append(G._layer(dev, 4, 16, 32, 512, 256, 1, ldx=512, pro=True, groups=2, seed=50))
    slab = layers[-1]["x"]
    for L in layers:
        if L["geo"][9] == 1:
            L["x"] = slab
    want = [G._run_single(L, dev)[0] for L in layers]
    for max_wg in (0, 96):
        got = G._run_group(layers, dev, max_wg)
        torch.cuda.synchronize()
        for i, (w, (g, _)) in enumerate(zip(want, got)):
            n = float(w.norm())
            assert n > 0, i
            assert float((g - w).norm()) <= 2e-5 * n, (i, max_wg, layers[i]["geo"])
