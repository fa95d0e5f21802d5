"""The four correlation kernels of pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/corr.hip (wave-per-pixel forward and
backward, tiled MFMA forward and backward), on every dispatch path, against the float64 references of tests/corrops_ref.py.

Without a GPU: the reference agrees with the plain-C oracle, with torch autograd and with a hand-checkable vector; a Python
mirror of the dispatch predicates (corr_tiled_ok, corr_tile_plan, sdhip_vec_ok, the NKS split of the backward) names the
forward and the backward kernel of every case of the table below, and a test asserts that the table brings every layout and
every channel count to every kernel in each dtype the kernel exists in; the comparator rejects a list of plausible wrong
references on the table's own inputs at the very bounds the GPU tests use; malformed arguments are refused before any GPU work.
With a GPU (marker `gpu`): both entry points are called through the C ABI on inputs rounded to the dtype under test, every
tensor a channel slice of a NaN-filled slab and every output NaN before the call (a NaN in a result is a lane beside the
tensor that was read, or an element that was not written), and compared with the reference; after each call every slab,
the inputs' too, has the bits it had outside the tensor.  No element is excluded from any comparison.

Rounding model (u = 2^-24):
  forward    C u A + half an ulp of the stored bf16 value, A = sum_c |in1| |in2| over the terms of the element: an f32
             accumulation of C terms in any order (per-lane fma chains and a wave reduction, or MFMA blocks over the
             64-channel chunks).  bf16 x bf16 products are exact in f32 and an fma rounds an f32 product only with the sum, so
             the accumulation term is the same on the MFMA and the wave paths; in bf16 the only other rounding is the store.
  backward   P u sum_p |gout| |in| + half an ulp of the stored bf16 value: P = PH * PW terms per gradient element.
  zero       where the reference is exactly 0 because no term exists (displacements that leave the image) the bound is 0:
             the kernel must store 0.
  exact      inputs and gout in {-1, 0, 1} with every result an integer of magnitude <= 256 (which bf16 holds): the result
             must equal the reference bit for bit — the sharp test of indexing (halo offsets, the mirrored displacement of the
             tiled backward's second pass, the LDS gather of the tiled forward).

Worst |error| / bound per kernel, from one `pytest -s` run on an MI355X (documentation, not thresholds; a ratio near 1 in
bf16 is a value that rounded at a tie of its half-ulp bound):
  forward   tile<3> 0.998   tile<4> 1.0   tile<9> 1.0        wave_vec bf16 1.0 / f32 0.278   wave_scalar bf16 1.0 / f32 0.49
  backward  tile<6> 0.999   tile<7> 0.999   tile<18> 0.996   wave_vec bf16 1.0 / f32 0.997   wave_scalar bf16 1.0 / f32 0.989
  module    bf16: out 0.995, gin1 0.999, gin2 0.999          f32: out 0.0139, gin1 0.22, gin2 0.229
(the f32 backward's 0.99 is the (1, 1) patch: one product per element, whose single rounding is the whole bound).  A kernel
trace of every case of the table, taken once with the profiler, named the kernels the mirror names, 284 launches of 284.

No kernel or glue defect showed: every case passed on corr.hip and ops._CorrFn as they were.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corrops_ref as KR  # noqa: E402
import rowops_ref as R  # noqa: E402
from rowops_ref import U32, Rows, check, diag_switches, half_ulp_bf16, quant, worst_ratio  # noqa: E402

from oracle.detweights import randn_input  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
NOTILED = {"SDHIP_CORR_NO_TILED": "1"}
B = 2                       # every case: a wrong image offset shows


def isbf(dtype):
    return dtype == BF16


def code(dtype):
    return 1 if isbf(dtype) else 0


def dname(dtype):
    return "bf16" if isbf(dtype) else "f32"


# =========================================================================== the case table
class Case(dict):
    """One correlation.  patch (PH, PW), dil, hw (H, W), C, lay: the layout of in1 / in2 / gin1 / gin2 (rowops_ref.layout;
    the ABI shares one ld_in), gap: ld_out = P + 3 instead of P, env: diagnostic switches, only: the dtype the case is for."""
    __getattr__ = dict.__getitem__


def mk(patch, C, hw=(9, 13), lay="dense", gap=0, dil=1, env=None, only=None):
    c = Case(patch=patch, PH=patch[0], PW=patch[1], P=patch[0] * patch[1], C=C, H=hw[0], W=hw[1], lay=lay, gap=gap, dil=dil,
             env=env or {}, only=only)
    c["name"] = "p%dx%d_c%d_%dx%d_%s%s%s%s" % (patch[0], patch[1], C, hw[0], hw[1], lay, "_gap" if gap else "", "_d%d" % dil if dil > 1 else "",
                                               "_notiled" if env else "")
    return c


M913, M816, M330, M11 = (9, 13), (8, 16), (3, 30), (1, 1)    # 2x2 ragged tiles / aligned row stores / one tile row, four columns / one pixel


def cases():
    cs = []
    # shipped configurations and the non-square patches on the same tile plans: NT 3 / NKS 6, 4 / 7, 9 / 18
    cs += [mk((1, 17), 8), mk((1, 17), 64, M816, "slab8"), mk((5, 9), 72, M913, "slab8"), mk((5, 9), 136, M330), mk((1, 17), 8, M11),
           mk((5, 9), 64, M816), mk((1, 17), 136, M913, "slab8"), mk((5, 9), 8, M330, "slab8"), mk((1, 17), 72, M330)]
    cs += [mk((1, 21), 72), mk((1, 21), 136, M816, "slab8"), mk((3, 13), 8, M330, "slab8"), mk((3, 13), 64), mk((3, 13), 8, M11),
           mk((1, 21), 64, M330, "slab8"), mk((3, 13), 72, M816, "slab8"), mk((3, 13), 136, M913), mk((1, 21), 8, M816)]
    cs += [mk((17, 17), 8, M913, "slab8"), mk((17, 17), 136, M816), mk((13, 21), 72), mk((13, 21), 64, M330, "slab8"), mk((17, 17), 64, M11),
           mk((13, 21), 8, M816), mk((17, 17), 72, M330, "slab8"), mk((13, 21), 136, M913, "slab8"), mk((17, 17), 64)]
    # tiled forward (NT 4), wave backward (NKS 8 has no instantiation)
    cs += [mk((9, 9), 72), mk((9, 9), 8, M816, "slab8"), mk((1, 23), 136, M330), mk((1, 23), 64, M913, "slab8"), mk((9, 9), 64, M11),
           mk((9, 9), 136, M330, "slab8"), mk((1, 23), 8), mk((1, 23), 72, M816)]
    # patches with a tile plan that must fall back: ld_out > P, rows that are no 16-byte chunks, ragged channels
    cs += [mk((5, 9), 64, gap=1), mk((13, 21), 8, M816, "slab8", gap=1), mk((1, 17), 136, M330, gap=1), mk((9, 9), 72, M913, "slab8", gap=1),
           mk((17, 17), 8, lay="ldodd"), mk((1, 17), 72, lay="misal"), mk((3, 13), 64, M816, "ldodd", gap=1), mk((1, 21), 136, M330, "misal"),
           mk((1, 21), 12), mk((17, 17), 5, M330), mk((5, 9), 12, M816, "slab8"), mk((1, 17), 5, M913, "slab8", gap=1)]
    # no tile plan: the vector wave kernels in bf16 too
    cs += [mk((3, 3), 8), mk((3, 3), 136, M816, "slab8"), mk((3, 3), 72, lay="ldodd"), mk((3, 3), 5, M330), mk((3, 3), 64, lay="misal"),
           mk((3, 3), 520), mk((3, 3), 64, M11, "slab8", gap=1),
           mk((1, 9), 64, M330), mk((1, 9), 72, M913, "slab8", gap=1), mk((1, 9), 12, M913, "slab8"), mk((1, 9), 136, M11, "ldodd", gap=1),
           mk((1, 9), 8, M816, "misal"),
           mk((1, 1), 8), mk((1, 1), 5, M11, "ldodd"), mk((1, 1), 136, M816, "slab8", gap=1), mk((1, 1), 72, M330, "misal")]
    # dilation: wave kernels in both dtypes
    cs += [mk((3, 5), 8, dil=2), mk((3, 5), 72, M816, "slab8", dil=2), mk((3, 5), 5, lay="misal", dil=2), mk((3, 5), 12, M330, "ldodd", dil=2),
           mk((3, 5), 64, gap=1, dil=2), mk((3, 5), 136, M330, dil=2)]
    # the bf16 wave kernels on tiled shapes
    cs += [mk((17, 17), 64, env=NOTILED, only="bf16"), mk((1, 17), 136, M816, "slab8", env=NOTILED, only="bf16"),
           mk((1, 17), 8, M330, "slab8", env=NOTILED, only="bf16"), mk((17, 17), 72, M816, env=NOTILED, only="bf16")]
    return cs


CASES = cases()
BYNAME = {c.name: c for c in CASES}
assert len(BYNAME) == len(CASES)


def params(cs=None):
    """(case name, dtype) of every case in every dtype it is for."""
    return [pytest.param(c.name, dt, id="%s-%s" % (c.name, dname(dt))) for c in (CASES if cs is None else cs) for dt in (F32, BF16)
            if c.only in (None, dname(dt))]


# =========================================================================== mirror of the dispatch predicates
def cdiv(a, b):
    return -(-a // b)


def tile_plan(PH, PW):
    """corr_tile_plan: (tiles per wave quartet of the forward or 0, 32-pixel k-steps of the backward)."""
    nh = (8 + PH - 1) * (8 + PW - 1)
    nt = cdiv(cdiv(nh, 16), 4)
    return (nt if nt in (3, 4, 9) else 0), cdiv(nh, 32)


def vec_ok(c, dtype):
    """sdhip_vec_ok for the maps of the case: C and ld whole 16-byte chunks, the slices 16-byte aligned (torch allocations
    are)."""
    n, es = (8, 2) if isbf(dtype) else (4, 4)
    k, ld = R.layout(c.lay, c.C)
    return c.C % n == 0 and ld % n == 0 and (k * es) % 16 == 0


def out_layout(c):
    """(first element, pixel stride) of out / gout inside their slab."""
    return (1, c.P + 3) if c.gap else (0, c.P)


def paths(c, dtype):
    """(forward kernel, backward kernel) sdhip_corr_fwd / sdhip_corr_bwd launch for the case."""
    nt, nks = tile_plan(c.PH, c.PW)
    tiled = (isbf(dtype) and c.dil == 1 and vec_ok(c, dtype) and out_layout(c)[1] == c.P and c.P >= 9 and nt != 0 and
             "SDHIP_CORR_NO_TILED" not in c.env)
    wave = "wave_vec" if vec_ok(c, dtype) else "wave_scalar"
    return ("tile%d" % nt if tiled else wave), ("tile%d" % nks if tiled and nks in (6, 7, 18) else wave)


FWD_KERNELS = {"f32": ["wave_vec", "wave_scalar"], "bf16": ["tile3", "tile4", "tile9", "wave_vec", "wave_scalar"]}
BWD_KERNELS = {"f32": ["wave_vec", "wave_scalar"], "bf16": ["tile6", "tile7", "tile18", "wave_vec", "wave_scalar"]}

# one case per kernel for the exact-input and the determinism tests (the mirror test asserts that they reach every kernel)
PICKS = ["p5x9_c72_9x13_slab8", "p3x13_c136_9x13_dense", "p13x21_c72_9x13_dense", "p9x9_c72_9x13_dense", "p3x3_c72_9x13_ldodd",
         "p3x5_c72_8x16_slab8_d2", "p17x17_c72_8x16_dense_notiled", "p5x9_c64_9x13_dense_gap", "p1x21_c12_9x13_dense", "p1x23_c64_9x13_slab8"]


def test_mirror_reaches_every_kernel():
    """Every forward and backward kernel of corr.hip is reached in each dtype it exists in: the tiled kernels by both
    vector layouts and all four channel counts, by a square / one-row and a non-square patch, by every map; the wave kernels
    by their layouts, both ld_out and their channel counts; the pairing tiled forward + wave backward; the bf16 vector wave
    kernels under SDHIP_CORR_NO_TILED and on patches without a plan; the one-per-kernel picks cover every kernel too."""
    assert [tile_plan(*p) for p in ((1, 17), (5, 9), (1, 21), (3, 13), (17, 17), (13, 21), (9, 9), (1, 23), (3, 3), (1, 9))] == \
        [(3, 6), (3, 6), (4, 7), (4, 7), (9, 18), (9, 18), (4, 8), (4, 8), (0, 4), (0, 4)]
    for dt in (F32, BF16):
        seen = {}
        for c in CASES:
            if c.only not in (None, dname(dt)):
                continue
            f, b = paths(c, dt)
            for side, k in (("fwd", f), ("bwd", b)):
                s = seen.setdefault((side, k), dict(lay=set(), C=set(), hw=set(), gap=set(), patch=set(), env=set(), pair=set()))
                s["lay"].add(c.lay); s["C"].add(c.C); s["hw"].add((c.H, c.W)); s["gap"].add(c.gap); s["patch"].add(c.patch)
                s["env"].add(bool(c.env)); s["pair"].add((f, b))
        assert sorted(k for s, k in seen if s == "fwd") == sorted(FWD_KERNELS[dname(dt)])
        assert sorted(k for s, k in seen if s == "bwd") == sorted(BWD_KERNELS[dname(dt)])
        for (side, k), s in seen.items():
            if k.startswith("tile"):
                assert s["lay"] == {"dense", "slab8"} and s["C"] >= {8, 64, 72, 136} and s["hw"] == {M913, M816, M330, M11}, (side, k, s)
                assert any(p[0] == 1 or p[0] == p[1] for p in s["patch"]) and any(1 < p[0] != p[1] for p in s["patch"]), (side, k, s)
            elif k == "wave_vec":
                assert s["lay"] == {"dense", "slab8"} and s["C"] >= {8, 64, 72, 136, 520} and s["gap"] == {0, 1}, (side, k, s)
                assert s["hw"] == {M913, M816, M330, M11}, (side, k, s)
            else:
                assert s["lay"] >= {"ldodd", "misal", "dense"} and s["C"] >= {5, 8, 64, 72, 136} | ({12} if isbf(dt) else set()), (side, k, s)
                assert s["gap"] == {0, 1}, (side, k, s)
        if isbf(dt):
            assert ("tile4", "wave_vec") in seen[("fwd", "tile4")]["pair"]                       # tiled forward, wave backward
            assert seen[("fwd", "wave_vec")]["env"] == {False, True} and seen[("bwd", "wave_vec")]["env"] == {False, True}
            assert {(1, 1), (3, 3), (1, 9), (3, 5)} <= seen[("fwd", "wave_vec")]["patch"]
            assert all(paths(c, dt) == ("wave_vec", "wave_vec") for c in CASES if c.env)
            assert all(paths(c, dt)[0].startswith("wave") for c in CASES if c.gap)               # ld_out > P falls back
        assert {paths(BYNAME[n], dt)[0] for n in PICKS if BYNAME[n].only in (None, dname(dt))} == set(FWD_KERNELS[dname(dt)])
        assert {paths(BYNAME[n], dt)[1] for n in PICKS if BYNAME[n].only in (None, dname(dt))} == set(BWD_KERNELS[dname(dt)])


# =========================================================================== inputs, references and bounds
def fwd_bound(c, dtype, out, A):
    return c.C * U32 * A + (half_ulp_bf16(np.abs(out)) if isbf(dtype) else 0.0)


def bwd_bound(c, dtype, gin, Ag):
    return c.P * U32 * Ag + (half_ulp_bf16(np.abs(gin)) if isbf(dtype) else 0.0)


@functools.lru_cache(maxsize=None)
def _draw(name, bf, exact):
    c, dtype = BYNAME[name], BF16 if bf else F32
    shape, oshape = (B, c.H, c.W, c.C), (B, c.H, c.W, c.P)
    if exact:
        rng = np.random.default_rng([c.PH, c.PW, c.C, c.H, c.W, bf])
        a, b = (rng.integers(-1, 2, shape).astype(np.float64) for _ in range(2))
        g = rng.integers(-1, 2, oshape) * (rng.random(oshape) < min(1.0, 48.0 / c.P))    # sparse: |gin| <= sum_p |gout| stays small
        g = g.astype(np.float64)
    else:
        a, b = (quant(randn_input(1, n, shape).numpy(), dtype) for n in "ab")
        g = quant(randn_input(2, "g", oshape).numpy(), dtype)
        tiny = np.finfo(np.float32).tiny
        assert all((np.abs(v[v != 0]) >= tiny).all() for v in (a, b, g))                 # no denormal values
    d = Case(a=a, b=b, g=g)
    d["out"], d["A"] = KR.corr_fwd(a, b, c.PH, c.PW, c.dil), KR.corr_fwd_abs(a, b, c.PH, c.PW, c.dil)
    d["g1"], d["g2"] = KR.corr_bwd(a, b, g, c.PH, c.PW, c.dil)
    d["A1"], d["A2"] = KR.corr_bwd_abs(a, b, g, c.PH, c.PW, c.dil)
    d["bout"], d["b1"], d["b2"] = fwd_bound(c, dtype, d.out, d.A), bwd_bound(c, dtype, d.g1, d.A1), bwd_bound(c, dtype, d.g2, d.A2)
    for v in d.values():
        v.setflags(write=False)
    return d


def draw(c, dtype, exact=False):
    """Inputs of the case rounded to the dtype (exact: values in {-1, 0, 1}), the f64 results, their |.| sums and the
    bounds; computed once per (case, dtype) and read-only."""
    return _draw(c.name, isbf(dtype), exact)


# =========================================================================== CPU: the reference checks out three ways
ORACLE_CASES = [  # the cases of tests/test_corr.py: B, C, H, W, patch, dil
    (2, 16, 6, 9, (1, 17), 1), (1, 352, 8, 16, (1, 17), 1), (2, 24, 7, 10, (17, 17), 1), (1, 5, 4, 6, (3, 5), 2), (1, 8, 1, 1, (1, 17), 1)]


def nhwc(x):
    return np.ascontiguousarray(np.moveaxis(np.asarray(x), 1, -1))


@pytest.mark.parametrize("Bn,C,H,W,patch,dil", ORACLE_CASES)
def test_reference_matches_c_oracle(oracle_clib, Bn, C, H, W, patch, dil):
    """Within the f32 oracle's own accumulation error: C u A forward (C products and adds per element), P u sum |g||in|
    backward; exactly where no term exists."""
    from oracle import cbuild
    PH, PW = patch
    a, b = randn_input(1, "a", (Bn, C, H, W)).numpy(), randn_input(1, "b", (Bn, C, H, W)).numpy()
    yc = cbuild.corr_forward(oracle_clib, a, b, patch, dil)                       # (B, PH, PW, H, W)
    g = randn_input(2, "g", yc.shape).numpy()
    g1c, g2c = cbuild.corr_backward(oracle_clib, a, b, g, patch, dil)
    an, bn, gn = nhwc(a), nhwc(b), nhwc(g.reshape(Bn, PH * PW, H, W))
    out, A = KR.corr_fwd(an, bn, PH, PW, dil), KR.corr_fwd_abs(an, bn, PH, PW, dil)
    check("oracle fwd", nhwc(yc.reshape(Bn, PH * PW, H, W)), out, C * U32 * A)
    (g1, g2), (A1, A2) = KR.corr_bwd(an, bn, gn, PH, PW, dil), KR.corr_bwd_abs(an, bn, gn, PH, PW, dil)
    check("oracle gin1", nhwc(g1c), g1, PH * PW * U32 * A1)
    check("oracle gin2", nhwc(g2c), g2, PH * PW * U32 * A2)


def torch_corr(a, b, PH, PW, dil):
    """The forward restated with torch f64 ops (pad, slice, multiply, sum) for autograd."""
    _, H, W, _ = a.shape
    rh, rw = PH // 2 * dil, PW // 2 * dil
    bp = torch.nn.functional.pad(b, (0, 0, rw, rw, rh, rh))
    return torch.stack([(a * bp[:, ph * dil:ph * dil + H, pw * dil:pw * dil + W]).sum(-1) for ph in range(PH) for pw in range(PW)], -1)


@pytest.mark.parametrize("name", ["p5x9_c8_3x30_slab8", "p3x5_c5_9x13_misal_d2", "p17x17_c8_9x13_slab8", "p1x17_c8_1x1_dense", "p3x3_c8_9x13_dense"])
def test_reference_backward_is_autograd(name):
    c = BYNAME[name]
    d = draw(c, F32)
    a, b = (torch.from_numpy(np.array(v)).requires_grad_(True) for v in (d.a, d.b))
    y = torch_corr(a, b, c.PH, c.PW, c.dil)
    assert np.abs(y.detach().numpy() - d.out).max() <= 1e-12 * max(1.0, np.abs(d.out).max())
    g1, g2 = torch.autograd.grad(y, (a, b), torch.from_numpy(np.array(d.g)))
    for got, want in ((d.g1, g1.numpy()), (d.g2, g2.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_reference_known_answer():
    """The hand-checkable vector of tests/test_corr.py: displacement index j pairs in1[w] with in2[w + j - PW//2]."""
    a = np.array([1., 2, 3, 4]).reshape(1, 1, 4, 1)
    b = np.array([10., 20, 30, 40]).reshape(1, 1, 4, 1)
    y = KR.corr_fwd(a, b, 1, 3)[0, 0]                                               # (W, PW)
    assert y[:, 0].tolist() == [0, 2 * 10, 3 * 20, 4 * 30]
    assert y[:, 1].tolist() == [10, 40, 90, 160]
    assert y[:, 2].tolist() == [1 * 20, 2 * 30, 3 * 40, 0]
    g = np.zeros((1, 1, 4, 3)); g[0, 0, 1, 2] = 1.0                                 # only out[w=1, j=2] = in1[1] * in2[2] matters
    g1, g2 = KR.corr_bwd(a, b, g, 1, 3)
    assert g1.ravel().tolist() == [0, 30, 0, 0] and g2.ravel().tolist() == [0, 0, 2, 0]


# =========================================================================== CPU: the comparator rejects wrong references
def _rej(label, wrong, ref, bound):
    r = worst_ratio(wrong, ref, bound)
    print("reject %-52s %.3g" % (label, r))
    assert r > 1.0, label


def rbf(x):
    return quant(x, BF16)


WRONG = [  # (what, keywords of the wrong reference, cases, which results: f = out, b = gin1 / gin2)
    ("PH/PW swapped", dict(swap=True), ["p5x9_c72_9x13_slab8", "p3x13_c64_9x13_dense", "p13x21_c72_9x13_dense", "p3x5_c8_9x13_dense_d2"], "fb"),
    ("displacement sign flipped", dict(sign=-1), ["p1x17_c8_9x13_dense", "p5x9_c72_9x13_slab8", "p17x17_c8_9x13_slab8", "p3x3_c8_9x13_dense",
                                                  "p3x5_c8_9x13_dense_d2"], "fb"),
    ("radius off by one", dict(radius=1), ["p1x21_c72_9x13_dense", "p13x21_c72_9x13_dense", "p9x9_c72_9x13_dense", "p3x3_c8_9x13_dense"], "fb"),
    ("border clamped", dict(clamp=True), ["p1x17_c8_9x13_dense", "p3x13_c64_9x13_dense", "p17x17_c8_9x13_slab8", "p1x9_c64_3x30_dense",
                                          "p3x5_c8_9x13_dense_d2"], "fb"),
    ("last 8-channel chunk dropped", dict(drop_chunk=True), ["p1x17_c136_9x13_slab8", "p3x13_c136_9x13_dense", "p13x21_c72_9x13_dense", "p3x3_c8_9x13_dense",
                                                             "p3x3_c520_9x13_dense"], "fb"),
    ("gin1/gin2 exchanged", dict(exchange=True), ["p1x17_c8_9x13_dense", "p5x9_c72_9x13_slab8", "p17x17_c8_9x13_slab8", "p1x1_c8_9x13_dense"], "b"),
    ("accumulation rounded to bf16 per term", dict(term_round=rbf), ["p1x17_c64_8x16_slab8", "p3x3_c72_9x13_ldodd", "p5x9_c8_3x30_slab8"], "fb"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", [w[0] for w in WRONG])
def test_comparator_rejects_wrong_references(what, dtype):
    """Each plausible mistake, fed to the comparator as the kernel's output on the table's own inputs and bounds, fails."""
    _, kw, names, which = next(w for w in WRONG if w[0] == what)
    for name in names:
        c = BYNAME[name]
        d = draw(c, dtype)
        if "f" in which:
            _rej("%s: out %s" % (what, name), KR.corr_fwd(d.a, d.b, c.PH, c.PW, c.dil, **kw), d.out, d.bout)
        w1, w2 = KR.corr_bwd(d.a, d.b, d.g, c.PH, c.PW, c.dil, **kw)
        _rej("%s: gin1 %s" % (what, name), w1, d.g1, d.b1)
        _rej("%s: gin2 %s" % (what, name), w2, d.g2, d.b2)


# =========================================================================== CPU: arguments, exact-input precondition
def test_malformed_arguments_are_rejected_without_gpu_work():
    """Each call below would fault if a pointer were dereferenced or a kernel launched (the pointers are the address 16)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    L, E, p = _lib._lib, _lib.ERR_ARG, ctypes.c_void_p(16)

    def fwd(Bn=1, H=4, W=6, C=8, ld_in=8, PH=1, PW=17, dil=1, ld_out=17, dt=0):
        return L.sdhip_corr_fwd(p, p, p, Bn, H, W, C, ld_in, PH, PW, dil, ld_out, dt, None)

    def bwd(Bn=1, H=4, W=6, C=8, ld_in=8, PH=1, PW=17, dil=1, ld_out=17, dt=0):
        return L.sdhip_corr_bwd(p, p, p, p, p, Bn, H, W, C, ld_in, PH, PW, dil, ld_out, dt, None)

    for f in (fwd, bwd):
        assert f(PW=16, ld_out=16) == E and b"odd" in L.sdhip_last_error()        # an even patch
        assert f(PH=2, ld_out=34) == E
        assert f(dil=0) == E and b"dilation" in L.sdhip_last_error()
        assert f(ld_in=7) == E and b"stride" in L.sdhip_last_error()             # ld_in < C
        assert f(ld_out=16) == E                                                  # ld_out < PH * PW
        assert f(dt=7) == E and b"dtype" in L.sdhip_last_error()
        assert f(Bn=0) == E and b"empty" in L.sdhip_last_error()


@pytest.mark.parametrize("name,dtype", params([BYNAME[n] for n in PICKS]))
def test_exact_inputs_have_exact_results(name, dtype):
    """Precondition of the exact-input GPU test: every expected value is an integer of magnitude <= 256, which bf16 (8
    significant bits) and f32 hold, and every partial sum of an f32 accumulation of integers that small is exact."""
    d = draw(BYNAME[name], dtype, exact=True)
    for v in (d.out, d.g1, d.g2):
        assert np.abs(v).max() <= 256 and np.array_equal(v, np.round(v))
    for A in (d.A, d.A1, d.A2):
        assert A.max() < 2 ** 24


# =========================================================================== GPU plumbing
def run(name, *args):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(rows, ref, dtype):
    """Do the logical values of a Rows hold exactly the bits of `ref` rounded to dtype (a -0 of numpy's taken as 0)?"""
    want = torch.from_numpy(np.asarray(ref, np.float64).reshape(-1, rows.C) + 0.0).to(dtype)
    return bool(torch.equal(bits(rows.v), bits(want)))


def gpu_fwd(c, dtype, d):
    n = B * c.H * c.W
    with diag_switches(**c.env):
        a, b = Rows(n, c.C, dtype, c.lay, np.array(d.a)), Rows(n, c.C, dtype, c.lay, np.array(d.b))       # (copies: d is read-only)
        out = Rows(n, c.P, dtype, out_layout(c))
        assert (a.vec(8 if isbf(dtype) else 4) and b.vec(8 if isbf(dtype) else 4)) == vec_ok(c, dtype)      # the mirror's premise
        run("sdhip_corr_fwd", a.p, b.p, out.p, B, c.H, c.W, c.C, a.ld, c.PH, c.PW, c.dil, out.ld, code(dtype))
    return a, b, out


def gpu_bwd(c, dtype, d):
    n = B * c.H * c.W
    with diag_switches(**c.env):
        a, b = Rows(n, c.C, dtype, c.lay, np.array(d.a)), Rows(n, c.C, dtype, c.lay, np.array(d.b))
        g = Rows(n, c.P, dtype, out_layout(c), np.array(d.g))
        g1, g2 = Rows(n, c.C, dtype, c.lay), Rows(n, c.C, dtype, c.lay)
        run("sdhip_corr_bwd", a.p, b.p, g.p, g1.p, g2.p, B, c.H, c.W, c.C, a.ld, c.PH, c.PW, c.dil, g.ld, code(dtype))
    return a, b, g, g1, g2


def intact(label, *rows):
    for i, r in enumerate(rows):
        assert r.pads_intact(), "%s: the slab of tensor %d changed beside the tensor" % (label, i)


def resh(rows, c):
    return rows.np().reshape(B, c.H, c.W, rows.C)


# =========================================================================== GPU: the two entry points on every case
@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", params())
def test_corr_fwd(name, dtype):
    """sdhip_corr_fwd on the kernel the mirror names: every element of out within the bound (0 where no term exists), the
    NaN lanes beside in1 / in2 not read, the NaN beside out (the ld_out gap too) and the inputs untouched."""
    c = BYNAME[name]
    d = draw(c, dtype)
    a, b, out = gpu_fwd(c, dtype, d)
    check("fwd %-11s %-4s %s" % (paths(c, dtype)[0], dname(dtype), name), resh(out, c), d.out, d.bout)
    intact(name, a, b, out)
    assert same_bits(a, d.a, dtype) and same_bits(b, d.b, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", params())
def test_corr_bwd(name, dtype):
    """sdhip_corr_bwd likewise: every element of gin1 and gin2, NaN before the call, within the bound."""
    c = BYNAME[name]
    d = draw(c, dtype)
    a, b, g, g1, g2 = gpu_bwd(c, dtype, d)
    k = paths(c, dtype)[1]
    check("bwd %-11s %-4s gin1 %s" % (k, dname(dtype), name), resh(g1, c), d.g1, d.b1)
    check("bwd %-11s %-4s gin2 %s" % (k, dname(dtype), name), resh(g2, c), d.g2, d.b2)
    intact(name, a, b, g, g1, g2)
    assert same_bits(a, d.a, dtype) and same_bits(b, d.b, dtype) and same_bits(g, d.g, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", params([BYNAME[n] for n in PICKS]))
def test_exact_inputs_bitwise(name, dtype):
    """Inputs and gout in {-1, 0, 1}: no rounding anywhere (test_exact_inputs_have_exact_results), so out, gin1 and gin2 are
    the reference bit for bit on every kernel."""
    c = BYNAME[name]
    d = draw(c, dtype, exact=True)
    a, b, out = gpu_fwd(c, dtype, d)
    assert same_bits(out, d.out, dtype), "out differs from the reference"
    intact(name, a, b, out)
    a, b, g, g1, g2 = gpu_bwd(c, dtype, d)
    assert same_bits(g1, d.g1, dtype), "gin1 differs from the reference"
    assert same_bits(g2, d.g2, dtype), "gin2 differs from the reference"
    intact(name, a, b, g, g1, g2)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", params([BYNAME[n] for n in PICKS]))
def test_deterministic(name, dtype):
    """No atomics in corr.hip: two calls on the same inputs give the same bits."""
    c = BYNAME[name]
    d = draw(c, dtype)
    o1, o2 = gpu_fwd(c, dtype, d)[2], gpu_fwd(c, dtype, d)[2]
    assert torch.equal(bits(o1.v), bits(o2.v))
    r1, r2 = gpu_bwd(c, dtype, d), gpu_bwd(c, dtype, d)
    assert torch.equal(bits(r1[3].v), bits(r2[3].v)) and torch.equal(bits(r1[4].v), bits(r2[4].v))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p1x17_c64_8x16_slab8", "p3x13_c72_8x16_slab8", "p17x17_c136_8x16_dense"])
def test_tiled_out_two_byte_aligned(name):
    """The tiled kernels ask 16-byte alignment of the maps only: out and gout one element into a dense NaN buffer (ld_out
    = P) stay on them, every row store of the W % 8 == 0 map on the element-wise path, and write nothing before or after."""
    c, n = BYNAME[name], B * BYNAME[name].H * BYNAME[name].W
    assert paths(c, BF16) == ("tile%d" % tile_plan(c.PH, c.PW)[0], "tile%d" % tile_plan(c.PH, c.PW)[1])
    d = draw(c, BF16)
    flat = torch.full((n * c.P + 16,), float('nan'), dtype=BF16, device="cuda")
    gflat = flat.clone()
    gflat[1:1 + n * c.P] = torch.from_numpy(np.array(d.g)).to(BF16).cuda().reshape(-1)
    gbefore = bits(gflat)
    a, b = Rows(n, c.C, BF16, c.lay, np.array(d.a)), Rows(n, c.C, BF16, c.lay, np.array(d.b))
    g1, g2 = Rows(n, c.C, BF16, c.lay), Rows(n, c.C, BF16, c.lay)
    run("sdhip_corr_fwd", a.p, b.p, ctypes.c_void_p(flat.data_ptr() + 2), B, c.H, c.W, c.C, a.ld, c.PH, c.PW, 1, c.P, 1)
    run("sdhip_corr_bwd", a.p, b.p, ctypes.c_void_p(gflat.data_ptr() + 2), g1.p, g2.p, B, c.H, c.W, c.C, a.ld, c.PH, c.PW, 1, c.P, 1)
    check("fwd %-11s bf16 %s_offset" % (paths(c, BF16)[0], name), flat[1:1 + n * c.P].double().cpu().numpy().reshape(d.out.shape), d.out, d.bout)
    assert bool(torch.isnan(flat[:1]).all() and torch.isnan(flat[1 + n * c.P:]).all())
    check("bwd %-11s bf16 gin1 %s_offset" % (paths(c, BF16)[1], name), resh(g1, c), d.g1, d.b1)
    check("bwd %-11s bf16 gin2 %s_offset" % (paths(c, BF16)[1], name), resh(g2, c), d.g2, d.b2)
    intact(name, a, b, g1, g2)
    assert torch.equal(bits(gflat), gbefore)


# =========================================================================== GPU: through nn.SpatialCorrelationSampler
def slab_views(d, C, dtype, same):
    """in1 / in2 as NCHW views of channel slices of NaN-filled NHWC slabs.  same: two slices of ONE slab (equal pixel
    strides, 16-byte aligned: the slab stride reaches the kernel); else two slabs of different strides."""
    shp = d.a.shape[:3]
    if same:
        s = torch.full(shp + (2 * C + 16,), float('nan'), dtype=dtype, device="cuda")
        slabs, va, vb = [s], s[..., 8:8 + C], s[..., 8 + C:8 + 2 * C]
    else:
        sa = torch.full(shp + (C + 8,), float('nan'), dtype=dtype, device="cuda")
        sb = torch.full(shp + (C + 16,), float('nan'), dtype=dtype, device="cuda")
        slabs, va, vb = [sa, sb], sa[..., :C], sb[..., 8:8 + C]
    va.copy_(torch.from_numpy(np.array(d.a)).to(dtype))
    vb.copy_(torch.from_numpy(np.array(d.b)).to(dtype))
    return slabs, va.permute(0, 3, 1, 2).requires_grad_(True), vb.permute(0, 3, 1, 2).requires_grad_(True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("same", [1, 0], ids=["one_slab", "two_strides"])
@pytest.mark.parametrize("name", ["p1x17_c72_3x30_dense", "p17x17_c72_3x30_slab8"])
def test_module_on_slab_slices(name, same, dtype, monkeypatch):
    """nn.SpatialCorrelationSampler forward and backward on channel slices of NaN slabs, within the same bounds: equal strides
    hand the slab stride to the forward kernel (and the backward, which wants dense maps, copies); different strides take the
    lda != ldb copy.  The slabs keep their bits."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.nn import SpatialCorrelationSampler
    c = BYNAME[name]
    d = draw(c, dtype)
    slabs, a, b = slab_views(d, c.C, dtype, same)
    before = [bits(s) for s in slabs]
    seen, real = [], ops.call

    def spy(fn, *args, **kw):
        seen.append((fn, args))
        return real(fn, *args, **kw)
    monkeypatch.setattr(ops, "call", spy)
    y = SpatialCorrelationSampler(1, c.patch, 1, 0, 1, c.dil)(a, b)
    assert tuple(y.shape) == (B, c.PH, c.PW, c.H, c.W)
    g = torch.from_numpy(np.array(d.g)).to(dtype).cuda().view(B, c.H, c.W, c.PH, c.PW).permute(0, 3, 4, 1, 2)
    y.backward(g)
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == ["sdhip_corr_fwd", "sdhip_corr_bwd"]
    assert seen[0][1][7] == (2 * c.C + 16 if same else c.C) and seen[1][1][9] == c.C          # ld_in of the two launches
    tag = "module %s %s %s" % ("one_slab" if same else "two_strides", dname(dtype), name)
    nh = lambda t: t.detach().permute(0, 2, 3, 1).double().cpu().numpy()
    check(tag + " out", y.detach().permute(0, 3, 4, 1, 2).reshape(B, c.H, c.W, c.P).double().cpu().numpy(), d.out, d.bout)
    check(tag + " gin1", nh(a.grad), d.g1, d.b1)
    check(tag + " gin2", nh(b.grad), d.g2, d.b2)
    for s, was in zip(slabs, before):
        assert torch.equal(bits(s), was)
