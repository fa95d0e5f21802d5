"""The pooling, resize and broadcast entry points of pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/resample.hip against the float64 references of tests/rowops_ref.py.

Without a GPU: the references are F.max_pool2d(3, 2, 1, return_indices=True), F.avg_pool2d and F.interpolate (size= and
scale_factor=; nearest, bilinear, bilinear align_corners=True) and their gradients on the CPU in float64, and the
comparator rejects the plausible mistakes at the bounds the GPU tests use.  With a GPU (marker `gpu`): the C ABI directly, inputs
rounded to the dtype under test, tensors as channel slices of NaN-filled slabs.

Branches: vector kernels for C = 8, 12 (f32), 32, 64, 72 on `dense` / `slab8`; scalar ones for C = 3, 65, 12 (bf16) and for the
layouts `ldodd` / `misal` at any C; the resize backward with 1, 4 and 16 lanes per item (test_resize_lane_splits).
Capped grid: every kernel of the file launches through grid_for(), which stops at 4096 workgroups of 256 threads and lets the
item loop go round; test_pools_capped_grid, test_resize_capped_grid and test_mul_bcast_capped_grid give each entry point more
than 1,048,576 threads' worth of items, with a ragged last trip.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from rowops_ref import U32, UBF, Rows, check, quant  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
LAYOUTS = ("dense", "slab8", "ldodd", "misal")
CAP = 4096 * 256      # grid_for(): at most 4096 workgroups x 256 threads walk the items; beyond that the item loop takes another trip
MODES = {0: dict(mode="nearest"), 1: dict(mode="bilinear", align_corners=False), 2: dict(mode="bilinear", align_corners=True)}


def st(ref, dtype, e=0.0):
    """Rounding of the stored output: half an ulp of the bf16 value that is rounded, which lies within e of ref."""
    return R.half_ulp_bf16(np.abs(ref) + e) if dtype == BF16 else 0.0


def code(dtype):
    return 0 if dtype == F32 else 1


def run(name, *args):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()


def nchw(a):
    """NHWC numpy -> NCHW torch f64."""
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def img(rows, B, H, W):
    return rows.reshape(B, H, W, -1)


# =========================================================================== bounds
def b_maxpool_bwd(gy, tap, H, W, dtype):
    """An input pixel sums the gradients of at most 4 windows in f32: 3 u sum|terms|; then the store."""
    e = 3 * U32 * R.maxpool3s2_bwd(np.abs(gy), tap, H, W)
    return e + st(R.maxpool3s2_bwd(gy, tap, H, W), dtype, e) + 1e-300


def b_avgpool(x, k, dtype):
    """k^2 sequential f32 adds (each rounds a partial sum <= sum|x|) and the product with fl(1 / k^2): (k^2 + 1) u mean|x|."""
    e = (k * k + 1) * U32 * R.avgpool(np.abs(x), k)
    return e + st(R.avgpool(x, k), dtype, e) + 1e-300


def b_avgpool_bwd(gy, H, W, k, dtype):
    """gy * fl(1 / k^2): two roundings; the leftover rows and columns are exact zeros (bound 0: equality is required)."""
    ref = R.avgpool_bwd(gy, H, W, k)
    return 2 * U32 * np.abs(ref) + st(ref, dtype, 2 * U32 * np.abs(ref))


def axis_err(n_in, n_out, mode):
    """Error of an interpolation weight of one axis: the source coordinate is formed in f32 — fl(in / out), one product, for
    align_corners=False the +0.5 / -0.5 as well — so it is off by at most 4 u (coordinate + 1) <= 4 u (in + 1); nearest has no
    weight (the f32 index arithmetic is ATen's own and the reference repeats it)."""
    return 0.0 if mode == 0 else 4 * U32 * (n_in + 1)


def b_resize(x, Ho, Wo, mode, dtype, sh=0.0, sw=0.0):
    """Nearest copies: exact.  Bilinear: 8 f32 operations on four taps, 8 u max|tap|, plus the weight errors of both axes
    times the tap differences (<= 2 max|tap| each); max|tap| is taken as the maximum of the (b, c) map."""
    ref = R.resize(x, Ho, Wo, mode, sh, sw)
    if mode == 0:
        return np.zeros_like(ref)
    M = np.abs(x).max((1, 2), keepdims=True)
    e = (8 * U32 + 2 * axis_err(x.shape[1], Ho, mode) + 2 * axis_err(x.shape[2], Wo, mode)) * M
    return e + st(ref, dtype, e) + 1e-300


def _pattern(n_in, n_out, mode, s):
    """0/1 matrix of the destinations that may reach a source: the reference's, widened by one source either way (a
    coordinate within rounding of an integer may hand a weight of ~u to the neighbour)."""
    P = (R.resize_matrix(n_in, n_out, mode, s) > 0).astype(np.float64)
    if mode == 0:
        return P
    Q = P.copy()
    Q[:, 1:] += P[:, :-1]
    Q[:, :-1] += P[:, 1:]
    return (Q > 0).astype(np.float64)


def b_resize_bwd(gy, H, W, mode, dtype, sh=0.0, sw=0.0):
    """Two separable passes, each a sum of n candidates with fma in f32: (n_h + n_w + 4) u sum(w |gy|) with n the largest
    number of destinations of one source; the weight errors of both axes times sum|gy| over the destinations in reach; the
    intermediate stays f32, the output is stored once."""
    Ho, Wo = gy.shape[1], gy.shape[2]
    Mh, Mw = R.resize_matrix(H, Ho, mode, sh), R.resize_matrix(W, Wo, mode, sw)
    nh, nw = int((Mh > 0).sum(0).max()), int((Mw > 0).sum(0).max())
    A = np.einsum('oh,bopc,pw->bhwc', Mh, np.abs(gy), Mw, optimize=True)
    reach = np.einsum('oh,bopc,pw->bhwc', _pattern(H, Ho, mode, sh), np.abs(gy), _pattern(W, Wo, mode, sw), optimize=True)
    ref = R.resize_bwd(gy, H, W, mode, sh, sw)
    e = (nh + nw + 4) * U32 * A + (axis_err(H, Ho, mode) + axis_err(W, Wo, mode)) * reach
    return e + st(ref, dtype, e) + 1e-300


# =========================================================================== CPU: the references are the ATen operations
def _aten_tap(index, H, W):
    """ATen's flat input index of the maximum -> the tap kh * 3 + kw inside the window of its output pixel."""
    B, C, Ho, Wo = index.shape
    h, w = index // W, index % W
    oh, ow = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return ((h - (2 * oh - 1)) * 3 + (w - (2 * ow - 1))).permute(0, 2, 3, 1).numpy()


def _maps(rng, B, H, W, C, kind):
    n = H * W
    if kind == "const":
        return np.full((B, H, W, C), -3.0)
    x = np.stack([np.stack([rng.permutation(n) for _ in range(C)], -1) for _ in range(B)]).reshape(B, H, W, C).astype(np.float64)
    if kind == "perm":
        return x - n // 2                                # consecutive integers that straddle zero
    if kind == "negative":
        return x - n                                     # all negative: the padding must never win
    return np.floor(x / 5) - n // 10                     # ties: every value five times


@pytest.mark.parametrize("H,W", [(8, 10), (9, 13), (5, 7), (1, 1), (2, 3)])
@pytest.mark.parametrize("kind", ["perm", "negative", "ties", "const"])
def test_maxpool_reference_is_aten(H, W, kind):
    rng = np.random.default_rng(H * 31 + W)
    x = _maps(rng, 2, H, W, 3, kind)
    xt = nchw(x).clone().requires_grad_(True)
    yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    gy = rng.standard_normal(nhwc(yt).shape)
    yt.backward(nchw(gy))
    y, tap = R.maxpool3s2(x)
    assert np.array_equal(y, nhwc(yt)) and np.array_equal(tap, _aten_tap(it, H, W))
    assert np.allclose(R.maxpool3s2_bwd(gy, tap, H, W), nhwc(xt.grad), rtol=1e-14, atol=0)


def test_maxpool_reference_propagates_nan_like_aten():
    rng = np.random.default_rng(5)
    x = _maps(rng, 1, 9, 13, 2, "perm")
    x[0, 5, 7, 0] = np.nan
    yt, it = F.max_pool2d(nchw(x), 3, 2, 1, return_indices=True)
    y, tap = R.maxpool3s2(x)
    assert np.array_equal(y, nhwc(yt), equal_nan=True) and np.isnan(y).sum() == 4 and np.array_equal(tap, _aten_tap(it, 9, 13))


@pytest.mark.parametrize("k,H,W", [(2, 9, 13), (3, 9, 13), (4, 9, 13), (8, 17, 19), (2, 8, 8)])
def test_avgpool_reference_is_aten(k, H, W):
    rng = np.random.default_rng(k)
    x = rng.standard_normal((2, H, W, 3))
    xt = nchw(x).clone().requires_grad_(True)
    yt = F.avg_pool2d(xt, k)
    gy = rng.standard_normal(nhwc(yt).shape)
    yt.backward(nchw(gy))
    assert np.allclose(R.avgpool(x, k), nhwc(yt), rtol=1e-13, atol=1e-15)
    assert np.allclose(R.avgpool_bwd(gy, H, W, k), nhwc(xt.grad), rtol=1e-13, atol=0)


RESIZES = [((5, 7), dict(size=(9, 13))), ((9, 13), dict(size=(5, 7))), ((1, 1), dict(size=(9, 13))), ((9, 13), dict(size=(1, 1))),
           ((8, 8), dict(size=(256, 256))), ((3, 5), dict(size=(42, 70))), ((5, 7), dict(scale_factor=2)), ((5, 7), dict(scale_factor=8)),
           ((9, 13), dict(scale_factor=0.5)), ((7, 5), dict(scale_factor=0.5)), ((5, 7), dict(size=(5, 7)))]


def _resize_args(hw, how):
    """(Ho, Wo, scale_h, scale_w) as ops.interpolate hands them to the kernel."""
    if "size" in how:
        return how["size"][0], how["size"][1], 0.0, 0.0
    f = how["scale_factor"]
    return int(hw[0] * f), int(hw[1] * f), 1.0 / f, 1.0 / f


@pytest.mark.parametrize("hw,how", RESIZES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resize_reference_is_aten(hw, how, mode):
    rng = np.random.default_rng(mode)
    x = rng.standard_normal((2, hw[0], hw[1], 3))
    xt = nchw(x).clone().requires_grad_(True)
    yt = F.interpolate(xt, **how, **MODES[mode])
    gy = rng.standard_normal(nhwc(yt).shape)
    yt.backward(nchw(gy))
    Ho, Wo, sh, sw = _resize_args(hw, how)
    if mode == 2:
        sh = sw = 0.0                      # align_corners=True ignores the scale factor
    assert (Ho, Wo) == tuple(yt.shape[2:])
    assert np.allclose(R.resize(x, Ho, Wo, mode, sh, sw), nhwc(yt), rtol=1e-12, atol=1e-13)
    assert np.allclose(R.resize_bwd(gy, hw[0], hw[1], mode, sh, sw), nhwc(xt.grad), rtol=1e-12, atol=1e-13)


def test_comparator_rejects_wrong_pool_and_resize_references():
    rng = np.random.default_rng(11)
    for dtype in (F32, BF16):
        # the max-pool tie going to the last maximum; zero padding instead of -inf padding
        x = _maps(rng, 2, 9, 13, 3, "ties")
        y, tap = R.maxpool3s2(x)
        gy = quant(rng.standard_normal(y.shape), dtype)
        _, tap_last = R.maxpool3s2(x, last_wins=True)
        assert (tap != tap_last).any()
        b = b_maxpool_bwd(gy, tap, 9, 13, dtype)
        assert R.worst_ratio(R.maxpool3s2_bwd(gy, tap_last, 9, 13), R.maxpool3s2_bwd(gy, tap, 9, 13), b) > 1
        xn = _maps(rng, 2, 9, 13, 3, "negative")
        y0, _ = R.maxpool3s2(xn, pad=0.0)
        assert R.worst_ratio(y0, R.maxpool3s2(xn)[0], 0.0) == np.inf and R.worst_ratio(R.maxpool3s2(xn)[0], R.maxpool3s2(xn)[0], 0.0) == 0.0
        # the average-pool backward filling the floor-mode leftover rows
        g = quant(rng.standard_normal((2, 4, 6, 3)), dtype)
        assert R.worst_ratio(R.avgpool_bwd(g, 9, 13, 2, fill_leftover=True), R.avgpool_bwd(g, 9, 13, 2), b_avgpool_bwd(g, 9, 13, 2, dtype)) == np.inf
        # the resize backward window of align_corners=False without its half-pixel shift: at x32 it loses part of the gradient
        g = quant(rng.standard_normal((1, 256, 256, 3)), dtype)
        good = R.resize_bwd(g, 8, 8, 1)
        bad = R.resize_bwd(g, 8, 8, 1, shifted_window=False)
        lost = 1.0 - R.resize_bwd(np.ones_like(g), 8, 8, 1, shifted_window=False).sum() / g.size
        assert 0.03 < lost < 0.2, lost
        assert R.worst_ratio(bad, good, b_resize_bwd(g, 8, 8, 1, dtype)) > 1
        # ... and a gradient that drops 7 % of its mass fails the conservation check
        e = b_resize_bwd(g, 8, 8, 1, dtype)
        assert R.worst_ratio((0.93 * good).sum((1, 2)), g.sum((1, 2)), e.sum((1, 2))) > 1
        assert R.worst_ratio(good.sum((1, 2)), g.sum((1, 2)), e.sum((1, 2))) < 1e-6


# =========================================================================== GPU
def _intact(*rows):
    for r in rows:
        assert r.pads_intact(), "a pad element changed"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [3, 8, 12, 72])
def test_maxpool(dtype, C):
    """Values and tap indices exactly (the maps are small integers, exact in bf16); the backward against ATen's on the CPU."""
    shapes = [(2, 8, 10), (2, 9, 13), (3, 5, 7), (1, 16, 16)]
    for ci, (lay, kind) in enumerate([(l, k) for l in LAYOUTS for k in ("perm", "negative", "ties", "const", "nan")]):
        if kind == "nan" and (dtype != F32 or lay != "dense"):
            continue
        B, H, W = shapes[ci % 4]
        rng = np.random.default_rng([C, ci, 20])
        x = _maps(rng, B, H, W, C, "perm" if kind == "nan" else kind)
        if kind == "nan":
            x[0, H // 2, W // 2, 0] = np.nan
        assert np.array_equal(quant(x, dtype), x, equal_nan=True)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        xd, yd = Rows(B * H * W, C, dtype, lay, x), Rows(B * Ho * Wo, C, dtype, lay)
        idx = torch.full((B * Ho * Wo, C), 255, dtype=torch.uint8, device="cuda")
        run("sdhip_maxpool3s2_fwd", xd.p, xd.ld, yd.p, yd.ld, idx.data_ptr(), B, H, W, C, code(dtype))
        y, tap = R.maxpool3s2(x)
        _intact(xd, yd)
        assert np.array_equal(img(yd.np(), B, Ho, Wo), y, equal_nan=True), (lay, kind)
        assert np.array_equal(idx.cpu().numpy().reshape(B, Ho, Wo, C), tap), (lay, kind)
        if kind == "nan":
            continue
        gy = quant(rng.standard_normal(y.shape), dtype)
        xt = nchw(x).clone().requires_grad_(True)
        F.max_pool2d(xt, 3, 2, 1).backward(nchw(gy))
        gd, gxd = Rows(B * Ho * Wo, C, dtype, lay, gy), Rows(B * H * W, C, dtype, lay)
        run("sdhip_maxpool3s2_bwd", gd.p, gd.ld, idx.data_ptr(), gxd.p, gxd.ld, B, H, W, C, code(dtype))
        _intact(gd, gxd)
        check("maxpool3s2_bwd", img(gxd.np(), B, H, W), nhwc(xt.grad), b_maxpool_bwd(gy, tap, H, W, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,H,W", [(2, 9, 13), (3, 9, 13), (4, 9, 13), (8, 17, 19)])
def test_avgpool(dtype, k, H, W):
    for ci, (lay, C) in enumerate([(l, c) for l in LAYOUTS for c in (3, 8, 12, 72)]):
        B = 2
        rng = np.random.default_rng([k, ci, 21])
        x = quant(rng.standard_normal((B, H, W, C)) + 0.5, dtype)
        Ho, Wo = H // k, W // k
        gy = quant(rng.standard_normal((B, Ho, Wo, C)), dtype)
        xd, yd = Rows(B * H * W, C, dtype, lay, x), Rows(B * Ho * Wo, C, dtype, lay)
        gd, gxd = Rows(B * Ho * Wo, C, dtype, lay, gy), Rows(B * H * W, C, dtype, lay)
        run("sdhip_avgpool_fwd", xd.p, xd.ld, yd.p, yd.ld, B, H, W, C, k, code(dtype))
        run("sdhip_avgpool_bwd", gd.p, gd.ld, gxd.p, gxd.ld, B, H, W, C, k, code(dtype))
        _intact(xd, yd, gd, gxd)
        check("avgpool_fwd k%d" % k, img(yd.np(), B, Ho, Wo), R.avgpool(x, k), b_avgpool(x, k, dtype))
        got = img(gxd.np(), B, H, W)
        assert not got[:, Ho * k:].any() and not got[:, :, Wo * k:].any() and np.isfinite(got).all(), "leftover rows / columns must be written as zeros"
        check("avgpool_bwd k%d" % k, got, R.avgpool_bwd(gy, H, W, k), b_avgpool_bwd(gy, H, W, k, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [16, 32])
def test_avgpool_chain_matches_aten(dtype, k):
    """ops.avgpool(x, 16) = 8 then 2, (x, 32) = 8 then 4: two stages, each with b_avgpool's f32 terms (65 u and <= 17 u) and, in
    bf16, a store (<= 2^-8 relative): 2 (65 u + 2^-8) of the window's mean |x| (resp. of |gx| for the backward, two products and two stores)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    rng = np.random.default_rng([k, 22])
    B, C, H, W = 2, 8, 2 * k + 3, 3 * k + 1
    x = quant(rng.standard_normal((B, H, W, C)) + 0.5, dtype)
    gy = quant(rng.standard_normal((B, H // k, W // k, C)), dtype)
    xt = nchw(x).clone().requires_grad_(True)
    yt = F.avg_pool2d(xt, k)
    yt.backward(nchw(gy))
    xg = nchw(x).to(dtype).cuda().requires_grad_(True)
    y = ops.avgpool(xg, k)
    y.backward(nchw(gy).to(dtype).cuda())
    torch.cuda.synchronize()
    ub = UBF if dtype == BF16 else 0.0
    check("ops.avgpool(%d)" % k, nhwc(y.double().cpu()), nhwc(yt), 2 * (65 * U32 + ub) * R.avgpool(np.abs(x), k) + 1e-300)
    check("ops.avgpool(%d) bwd" % k, nhwc(xg.grad.double().cpu()), nhwc(xt.grad), 2 * (2 * U32 + ub) * np.abs(nhwc(xt.grad)))


def _mul_bcast_case(label, dtype, C, n, lay, m_lay, gm_lay, seed):
    """y = a m: one product.  ga = g m: one product.  gm = sum_c g a: C fused multiply-adds in one thread, C u sum|g a|."""
    rng = np.random.default_rng([C, seed, 23])
    a, g = quant(rng.standard_normal((n, C)), dtype), quant(rng.standard_normal((n, C)), dtype)
    m = quant(rng.uniform(0.1, 1.0, (n, 1)), dtype)
    ad, gd, yd, gad = Rows(n, C, dtype, lay, a), Rows(n, C, dtype, lay, g), Rows(n, C, dtype, lay), Rows(n, C, dtype, lay)
    md, gmd = Rows(n, 1, dtype, m_lay, m), Rows(n, 1, dtype, gm_lay)
    run("sdhip_mul_bcast_fwd", ad.p, ad.ld, md.p, md.ld, yd.p, yd.ld, n, C, code(dtype))
    run("sdhip_mul_bcast_bwd", gd.p, gd.ld, ad.p, ad.ld, md.p, md.ld, gad.p, gad.ld, gmd.p, gmd.ld, n, C, code(dtype))
    _intact(ad, gd, yd, gad, md, gmd)
    y = R.mul_bcast(a, m[:, 0])
    gar, gmr = R.mul_bcast_bwd(g, a, m[:, 0])
    e_gm = C * U32 * np.abs(g * a).sum(-1)
    check(label + "_fwd", yd.np(), y, U32 * np.abs(y) + st(y, dtype, U32 * np.abs(y)) + 1e-300)
    check(label + "_bwd ga", gad.np(), gar, U32 * np.abs(gar) + st(gar, dtype, U32 * np.abs(gar)) + 1e-300)
    check(label + "_bwd gm", gmd.np()[:, 0], gmr, e_gm + st(gmr, dtype, e_gm) + 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 64, 65])
def test_mul_bcast(dtype, C):
    for ci, lay in enumerate(LAYOUTS):
        _mul_bcast_case("mul_bcast", dtype, C, (70, 468)[ci % 2], lay, (3, 6), (2, 5), ci)      # m, gm: one channel of a wider slab


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mul_bcast_capped_grid(dtype):
    """mul_bcast_bwd has one thread per pixel: CAP + 333 pixels are one trip and a ragged second.  With C = 3 (scalar items)
    mul_bcast_fwd has 3 (CAP + 333) items: three trips and 999 items of a fourth.  12.6 MB per tensor in f32."""
    n = CAP + 333
    assert n > CAP and 3 * n > 3 * CAP and (3 * n) % CAP == 999
    _mul_bcast_case("mul_bcast capped", dtype, 3, n, "dense", "dense", "dense", 99)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_pools_capped_grid(dtype):
    """C = 3 (scalar: one item per element), one 1190 x 1191 image (17 MB in f32).  Forward items: max pool 595 x 596 x 3 =
    1,063,860 and average pool (k = 2) 595 x 595 x 3 = 1,062,075, one trip of CAP = 1,048,576 and a ragged second.  Backward items:
    the 4,251,870 input elements, four trips and a ragged fifth.  W is odd, so the average pool leaves a column over."""
    B, H, W, C = 1, 1190, 1191, 3
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert CAP < B * Ho * Wo * C < 2 * CAP and CAP < B * (H // 2) * (W // 2) * C < 2 * CAP and 4 * CAP < B * H * W * C < 5 * CAP
    rng = np.random.default_rng(26)
    x = quant(rng.standard_normal((B, H, W, C)), dtype)
    xd, yd = Rows(B * H * W, C, dtype, "dense", x), Rows(B * Ho * Wo, C, dtype)
    idx = torch.full((B * Ho * Wo, C), 255, dtype=torch.uint8, device="cuda")
    run("sdhip_maxpool3s2_fwd", xd.p, C, yd.p, C, idx.data_ptr(), B, H, W, C, code(dtype))
    y, tap = R.maxpool3s2(x)
    assert np.array_equal(img(yd.np(), B, Ho, Wo), y) and np.array_equal(idx.cpu().numpy().reshape(B, Ho, Wo, C), tap)
    gy = quant(rng.standard_normal(y.shape), dtype)
    gd, gxd = Rows(B * Ho * Wo, C, dtype, "dense", gy), Rows(B * H * W, C, dtype)
    run("sdhip_maxpool3s2_bwd", gd.p, C, idx.data_ptr(), gxd.p, C, B, H, W, C, code(dtype))
    check("maxpool3s2_bwd capped", img(gxd.np(), B, H, W), R.maxpool3s2_bwd(gy, tap, H, W), b_maxpool_bwd(gy, tap, H, W, dtype))
    k, Ha, Wa = 2, H // 2, W // 2
    gy = quant(rng.standard_normal((B, Ha, Wa, C)), dtype)
    yd, gd, gxd = Rows(B * Ha * Wa, C, dtype), Rows(B * Ha * Wa, C, dtype, "dense", gy), Rows(B * H * W, C, dtype)
    run("sdhip_avgpool_fwd", xd.p, C, yd.p, C, B, H, W, C, k, code(dtype))
    run("sdhip_avgpool_bwd", gd.p, C, gxd.p, C, B, H, W, C, k, code(dtype))
    check("avgpool_fwd capped", img(yd.np(), B, Ha, Wa), R.avgpool(x, k), b_avgpool(x, k, dtype))
    got = img(gxd.np(), B, H, W)
    assert not got[:, :, Wa * k:].any() and np.isfinite(got).all()
    check("avgpool_bwd capped", got, R.avgpool_bwd(gy, H, W, k), b_avgpool_bwd(gy, H, W, k, dtype))


def _resize_case(label, dtype, B, H, W, C, Ho, Wo, mode, lay, lay_g, seed, sh=0.0, sw=0.0):
    rng = np.random.default_rng([H, W, Ho, Wo, mode, C, seed])
    x = quant(rng.standard_normal((B, H, W, C)), dtype)
    gy = quant(rng.standard_normal((B, Ho, Wo, C)), dtype)
    xd, yd = Rows(B * H * W, C, dtype, lay, x), Rows(B * Ho * Wo, C, dtype, lay)
    gd, gxd = Rows(B * Ho * Wo, C, dtype, lay_g, gy), Rows(B * H * W, C, dtype, lay)
    tmp = torch.full((B * Ho * W * C,), float('nan'), device="cuda")
    run("sdhip_resize_fwd", xd.p, xd.ld, yd.p, yd.ld, B, H, W, C, Ho, Wo, mode, sh, sw, code(dtype))
    run("sdhip_resize_bwd", gd.p, gd.ld, gxd.p, gxd.ld, tmp.data_ptr(), B, H, W, C, Ho, Wo, mode, sh, sw, code(dtype))
    _intact(xd, yd, gd, gxd)
    assert bool(torch.isfinite(tmp).all())
    check(label + " fwd", img(yd.np(), B, Ho, Wo), R.resize(x, Ho, Wo, mode, sh, sw), b_resize(x, Ho, Wo, mode, dtype, sh, sw))
    got, e = img(gxd.np(), B, H, W), b_resize_bwd(gy, H, W, mode, dtype, sh, sw)
    check(label + " bwd", got, R.resize_bwd(gy, H, W, mode, sh, sw), e)
    # every row of the interpolation matrices sums to 1: the gradient's mass per (b, c) is conserved, to the summed bound
    check(label + " bwd mass", got.sum((1, 2)), gy.sum((1, 2)), e.sum((1, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 12, 32])
def test_resize(dtype, mode, C):
    """Up and down, in == 1 and out == 1, every layout; gy in a slab (`ldodd`) that forces the scalar first pass while gx stays
    vectorisable."""
    sizes = [((5, 7), (9, 13)), ((9, 13), (5, 7)), ((1, 1), (9, 13)), ((9, 13), (1, 1)), ((5, 7), (5, 7)), ((4, 6), (8, 12))]
    for ci, (hw, out) in enumerate(sizes):
        lay = LAYOUTS[ci % 4]
        _resize_case("resize m%d" % mode, dtype, 2, hw[0], hw[1], C, out[0], out[1], mode, lay, lay, ci)
    _resize_case("resize m%d slab gy" % mode, dtype, 2, 5, 7, C, 9, 13, mode, "dense", "ldodd", 9)
    _resize_case("resize m%d slab gy" % mode, dtype, 2, 5, 7, C, 9, 13, mode, "slab8", "misal", 10)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resize_lane_splits(dtype, mode):
    """lanes() gives an item 1, 4 or 16 lanes for a candidate span 2 / scale + 5 below 12, below 32, or above: factors 3 | 4
    (spans 11 | 13) and 13 | 14 (31 | 33) sit on both sides of each threshold; (8, 8) -> (256, 256) is the x32 of the pyramid."""
    for f in (3, 4, 13, 14):
        _resize_case("resize m%d x%d" % (mode, f), dtype, 1, 3, 5, 12, 3 * f, 5 * f, mode, "dense", "dense", f)
    _resize_case("resize m%d x32" % mode, dtype, 1, 8, 8, 3, 256, 256, mode, "dense", "dense", 32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_resize_capped_grid(dtype, mode):
    """C = 3 (scalar items).  (150, 150) -> (600, 600): the forward has 600 x 600 x 3 = 1,080,000 items, one trip of CAP and a
    ragged second.  Its backward runs the W pass with 4 lanes per item (span 2 / 0.25 + 5 = 13), so a trip holds CAP / 4 =
    262,144 of the 600 x 150 x 3 = 270,000 items: the shuffle reduction runs again on a second, ragged trip, in which whole
    waves and parts of the last one have already left the loop.  (40, 40) -> (600, 600): 16 lanes (span 35), a trip holds
    CAP / 16 = 65,536 of the 600 x 40 x 3 = 72,000 items."""
    assert CAP < 600 * 600 * 3 < 2 * CAP and CAP // 4 < 600 * 150 * 3 < 2 * (CAP // 4) and CAP // 16 < 600 * 40 * 3 < 2 * (CAP // 16)
    _resize_case("resize m%d capped x4" % mode, dtype, 1, 150, 150, 3, 600, 600, mode, "dense", "dense", 41)
    _resize_case("resize m%d capped x15" % mode, dtype, 1, 40, 40, 3, 600, 600, mode, "dense", "dense", 42)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hw,f", [((5, 7), 2), ((5, 7), 8), ((9, 13), 0.5), ((7, 5), 0.5)])
def test_interpolate_scale_factor_matches_aten(dtype, mode, hw, f):
    """ops.interpolate(scale_factor=f) hands the kernel 1 / f as ATen does; forward and backward against F.interpolate on the
    CPU in f64 (which the reference is shown to equal without a GPU)."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    rng = np.random.default_rng([hw[0], mode, int(f * 10), 24])
    B, C = 2, 12
    x = quant(rng.standard_normal((B, hw[0], hw[1], C)), dtype)
    xt = nchw(x).clone().requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=f, **MODES[mode])
    gy = quant(rng.standard_normal(nhwc(yt).shape), dtype)
    yt.backward(nchw(gy))
    xg = nchw(x).to(dtype).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.interpolate(xg, scale_factor=f, **MODES[mode])
    y.backward(nchw(gy).to(dtype).cuda())
    torch.cuda.synchronize()
    Ho, Wo, sh, sw = _resize_args(hw, dict(scale_factor=f))
    if mode == 2:
        sh = sw = 0.0
    assert tuple(y.shape[2:]) == tuple(yt.shape[2:]) == (Ho, Wo)
    check("interpolate m%d f%g" % (mode, f), nhwc(y.double().cpu()), nhwc(yt), b_resize(x, Ho, Wo, mode, dtype, sh, sw))
    e = b_resize_bwd(gy, hw[0], hw[1], mode, dtype, sh, sw)
    got = nhwc(xg.grad.double().cpu())
    check("interpolate m%d f%g bwd" % (mode, f), got, nhwc(xt.grad), e)
    check("interpolate m%d f%g bwd mass" % (mode, f), got.sum((1, 2)), gy.sum((1, 2)), e.sum((1, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_into_a_slab(dtype):
    """The out= path of _ResizeFn: the result lands in channels [8, 20) of a 40-channel slab and nothing else of it changes."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    rng = np.random.default_rng(25)
    B, H, W, C, Ho, Wo = 2, 5, 7, 12, 9, 13
    x = quant(rng.standard_normal((B, H, W, C)), dtype)
    od = Rows(B * Ho * Wo, C, dtype, (8, 40))
    out = od.slab.view(B, Ho, Wo, 40)[..., 8:20].permute(0, 3, 1, 2)
    xg = nchw(x).to(dtype).cuda().contiguous(memory_format=torch.channels_last)
    y = ops._ResizeFn.apply(xg, Ho, Wo, 1, 0.0, 0.0, out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and od.pads_intact()
    check("resize out= slab", img(od.np(), B, Ho, Wo), R.resize(x, Ho, Wo, 1), b_resize(x, Ho, Wo, 1, dtype))


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    lib, sp = _lib._lib, _lib.stream_ptr()
    x, y = Rows(70, 8, F32, "dense", np.ones((70, 8))), Rows(70, 8, F32)
    idx = torch.zeros(70 * 8, dtype=torch.uint8, device="cuda")
    bad = [("sdhip_maxpool3s2_fwd", (x.p, 7, y.p, 8, idx.data_ptr(), 2, 5, 7, 8, 0, sp)),            # ld < C
           ("sdhip_avgpool_fwd", (x.p, 8, y.p, 8, 2, 5, 7, 8, 6, 0, sp)),                            # k > H
           ("sdhip_avgpool_bwd", (x.p, 8, y.p, 8, 2, 5, 7, 8, 2, 9, sp)),                            # unknown dtype
           ("sdhip_resize_fwd", (x.p, 8, y.p, 8, 2, 5, 7, 8, 5, 7, 3, 0.0, 0.0, 0, sp)),              # unknown mode
           ("sdhip_resize_bwd", (x.p, 8, y.p, 8, None, 2, 5, 7, 8, 5, 7, 1, 0.0, 0.0, 0, sp)),        # no workspace
           ("sdhip_mul_bcast_fwd", (x.p, 7, x.p, 1, y.p, 8, 70, 8, 0, sp))]                          # lda < C
    for name, args in bad:
        rc = getattr(lib, name)(*args)
        assert rc < 0 and lib.sdhip_last_error().decode(), name
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.slab).all())
