"""The BatchNorm-backward epilogue of the persistent whole-CU convolution (conv_band_bx_kernel of csrc/conv_band.h, reached
through sdhip_conv2d_fwd_bnbwd mode 0) at the smallest shapes that still take that path (>= 192 tiles of 16 x 32) and still
have every hazard of its operand loads, which are issued in the layout of the 16-byte stores — a stage ahead of the epilogue at
32 output channels, in one batch at its head at 64:

  ragged     2 images of 100 x 440 = 7 x 14 tiles each, 196 in all: the last tile row has 4 rows, the last tile column 24
             pixels; 5x5 64 -> 64 (two channel halves, streamed weights) and 3x3 32 -> 32 (resident weights in registers)
  groups     4 images of 100 x 416 in 4 statistics groups: 91 tiles per image, two per workgroup, so workgroup 45 holds
             tiles 90 and 91 — an epilogue, a flush of the sums and a change of scale / shift in the middle of a workgroup
  tail       24 output channels at pixel stride 32: every tile takes the guarded (non-interior) path
  3x3 wide   3x3 32 -> 64 on the ragged map: the 64-channel 3x3 forms (weights in LDS, u and the addend at the epilogue's head)

Each with and without an addend.  Checked per case:
  y     without an addend bit-identical to the plain launch of the same convolution; with one, bit-identical to
        sdhip_conv2d_fwd_add at the same shape (f32 sum, rounded once).  The addend cases use small-integer x and w, so that
        every accumulator is an integer of at most 256 — exact in bf16 — and round(y0 + addend) IS the single rounding: y0 is
        checked against an exact transposed convolution, y against that rounding.
  sums  against an f64 computation from the stored y, u, scale and shift, within 2e-4 of the largest wanted sum
  stray stores   y stands between guard pixels of a sentinel and carries the sentinel in its channel lanes beyond Cout
  stray loads    u and the addend carry NaN beyond their channels up to the pixel stride (a NaN fails every comparison)
  route          by kernel name (sdhip_last_path after every launch: "band(5x5, bx)" / "band(3x3, bx)", and "fast(...)" for
                 the one form that is not built — 5x5, 64 outputs, addend — and under SDHIP_CONV_NO_BAND_BX=1) and by result:
                 with the switch the same call gives the same sums within the bound and the same y bits.  Two kernels add the
                 taps up in different orders, so the y bits are compared on the integer-valued inputs, where every order gives
                 the same f32 accumulator.

ops._conv_backward fuses shapes beyond its small-map rule only where this kernel runs, and asks the library which those are
(ops._bnbwd_band_form: a dry call).  Without a GPU the answer is held against the forms written out below; with one,
against the kernel every real launch of this file ran on."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rowops_ref import diag_switches  # noqa: E402

GUARD = 48          # guard pixels in front of and behind y
SENT = 1.5          # sentinel (exact in bf16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _guarded(npix, ld, dev):
    whole = torch.full((npix + 2 * GUARD, ld), SENT, dtype=torch.bfloat16, device=dev)
    return whole, whole[GUARD:GUARD + npix]


def _check_guards(whole, npix, C):
    sent = _bits(torch.full((1,), SENT, dtype=torch.bfloat16, device=whole.device))[0]
    assert bool((_bits(whole[:GUARD]) == sent).all()), "guard pixels in front of y were written"
    assert bool((_bits(whole[GUARD + npix:]) == sent).all()), "guard pixels behind y were written"
    assert bool((_bits(whole[GUARD:GUARD + npix, C:]) == sent).all()), "channel lanes beyond Cout were written"


def _with_nan_tail(t, C, ld):
    """[npix][C] -> [npix][ld] with NaN in the lanes beyond C"""
    out = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    out[:, :C] = t
    return out


def _check_sums(sums, y, u, sc, sh, groups, C):
    # the sums over the STORED values, f64.  fmaf(u, scale, shift) > 0 exactly when the exact u * scale + shift > 0, and the
    # f64 product of a bf16 and an f32 value is exact
    yv = y[:, :C].double().reshape(groups, -1, C)
    uv = u[:, :C].double().reshape(groups, -1, C)
    gm = yv * ((uv * sc.double()[:, None] + sh.double()[:, None]) > 0)
    want = torch.stack([(gm * uv).sum(1), gm.sum(1)], 1)        # [groups][2][C]
    err, bound = (want - sums.sum(0)).abs().max().item(), 2e-4 * want.abs().max().item()
    print("sums: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound


def _form_built(k, C, with_add):      # every form of the epilogue is built but 5x5 with more than 32 outputs and an addend
    return not (k == 5 and C > 32 and with_add)


SHAPES = {"ragged_5x5_64": (2, 100, 440, 5, 64, 64, 72, 1), "ragged_3x3_32": (2, 100, 440, 3, 32, 32, 40, 1),
          "groups_5x5_64": (4, 100, 416, 5, 64, 64, 72, 4), "tail_5x5_24_of_32": (2, 100, 440, 5, 32, 24, 32, 1),
          "ragged_3x3_64_outputs": (2, 100, 440, 3, 32, 64, 72, 1)}        # B H W k K C ld groups


def _made_up_args(B, H, W, k, K, C, ld, groups, with_add=False, ldx=None, add_off=0):
    """The arguments of fused() below with made-up 256-byte-aligned operand addresses (a dry call reads none of them)."""
    P = ctypes.c_void_p
    return (P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), C, 32, P(5 << 20), ld, P(6 << 20), P(7 << 20), P((8 << 20) + add_off) if with_add else None,
            ld if with_add else 0, B, H, W, K, ldx or K, H, W, C, ld, k, k, 1, k // 2, k // 2, groups, 0, 1, None)


def test_band_form_is_the_librarys_answer():
    """ops._bnbwd_band_form, which decides for ops._conv_backward: the form of every shape of this file; the smallest map with
    192 tiles of 16 x 32 and one tile fewer; a gradient at a pixel stride that is no multiple of 8, an addend 8 bytes off a
    16-byte boundary and an addend at such a stride (the library declines all three: the earlier Python copy of the predicate
    knew only the first); the switches that send the call past the kernel."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    assert ops.BAND_BX_FORMS == ("5x5", "3x3") or os.environ.get("SDHIP_TUNE_BAND_BX_FORMS") is not None
    for name, shp in SHAPES.items():
        k, C = shp[3], shp[5]
        for with_add in (False, True):
            want = ("%dx%d" % (k, k)) if _form_built(k, C, with_add) else None
            assert ops._bnbwd_band_form(_made_up_args(*shp, with_add=with_add)) == want, (name, with_add)
    assert ops._bnbwd_band_form(_made_up_args(1, 177, 481, 5, 32, 32, 32, 1)) == "5x5"          # 12 x 16 tiles
    assert ops._bnbwd_band_form(_made_up_args(1, 177, 481, 3, 32, 32, 32, 1)) == "3x3"
    assert ops._bnbwd_band_form(_made_up_args(1, 176, 481, 5, 32, 32, 32, 1)) is None           # 11 x 16
    assert ops._bnbwd_band_form(_made_up_args(1, 177, 480, 3, 32, 32, 32, 1)) is None           # 12 x 15
    shp = SHAPES["ragged_3x3_32"]
    for kw in (dict(ldx=36), dict(with_add=True, add_off=8), dict(ld=36, with_add=True)):        # (ld: u and the addend at stride 36)
        assert ops._bnbwd_band_form(_made_up_args(*shp[:6], **dict(dict(ld=40, groups=1), **kw))) is None, kw
    for kw in (dict(C=6, ld=8), dict(C=3, ld=8), dict(ld=34, with_add=True)):      # the entry point refuses these (SDHIP_ERR_ARG): no kernel, no exception
        assert ops._bnbwd_band_form(_made_up_args(2, 100, 440, 5, 32, **dict(dict(C=32, groups=1), **kw))) is None, kw
    for sw in ("SDHIP_CONV_NO_BAND_BX", "SDHIP_CONV_NO_BAND", "SDHIP_CONV_GENERIC", "SDHIP_CONV_NO_BAND3"):
        with diag_switches(**{sw: "1"}):
            assert ops._bnbwd_band_form(_made_up_args(*shp)) is None, sw
            assert ops._bnbwd_band_form(_made_up_args(*SHAPES["ragged_5x5_64"])) == (None if sw != "SDHIP_CONV_NO_BAND3" else "5x5"), sw


def _run(B, H, W, k, K, C, ld, groups, with_add):
    """The data gradient of a k x k convolution C -> K: x has K channels, y and u have C channels at pixel stride ld."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr, dtype_code, last_path
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W + C + k)
    npix, pad = B * H * W, k // 2
    assert -(-H // 16) * -(-W // 32) * B >= 192                 # the persistent kernel's smallest grid
    # integer-valued inputs: accumulators are sums of k*k*K products of {-2..2} x {-1, 0, 1}, a share `dens` of the weights
    # non-zero -> variance 2 * dens * k*k*K = 160, the largest of ~6e6 accumulators far below 256 (asserted)
    dens = 80.0 / (k * k * K)
    xi = torch.randint(-2, 3, (npix, K), generator=g).float().to(dev).to(bf)
    wi = (torch.randint(-1, 2, (K, C, k, k), generator=g) * (torch.rand(K, C, k, k, generator=g) < dens)).float().to(dev)
    if with_add:
        x, w = xi, wi
    else:
        x = torch.randn(npix, K, generator=g).to(dev).to(bf)
        w = (torch.randn(K, C, k, k, generator=g) * 0.1).to(dev)
    u = _with_nan_tail((torch.randn(npix, C, generator=g) * 1.3).to(dev).to(bf), C, ld)
    a = _with_nan_tail(torch.randn(npix, C, generator=g).to(dev).to(bf), C, ld) if with_add else None
    sc = (torch.rand(groups, C, generator=g) + 0.5).to(dev)
    sh = (torch.randn(groups, C, generator=g) * 0.3).to(dev)
    dt = dtype_code(x)

    def plain(xv, wd):
        y = torch.empty(npix, ld, dtype=bf, device=dev)
        ops._conv_launch(xv, K, wd, y, ld, None, None, None, None, B, H, W, K, H, W, C, k, k, 1, 1, pad, pad, False, 1, 0, False)
        return y

    def fused(xv, wd, av, band=True):
        whole, y = _guarded(npix, ld, dev)
        sums = torch.zeros(ops.NREP, groups, 2, C, dtype=torch.float64, device=dev)
        args = (ptr(xv), ptr(wd), ptr(y), ptr(sums), C, ops.NREP, ptr(u), ld, ptr(sc), ptr(sh),
                ptr(av), ld if av is not None else 0, B, H, W, K, K, H, W, C, ld, k, k, 1, pad, pad, groups, 0, dt, stream_ptr())
        call("sdhip_conv2d_fwd_bnbwd", *args)
        ran = last_path()
        want = "band(%dx%d, bx)" % (k, k) if band and _form_built(k, C, av is not None) else "fast("      # else: the halo-tile kernel
        assert ran.startswith(want), (ran, want)
        assert ops._bnbwd_band_form(args) == ops._BAND_BX_NAMES.get(ran), ran          # what _conv_backward is told = what ran
        torch.cuda.synchronize()
        _check_guards(whole, npix, C)
        return y, sums

    wd = ops.packed_weight(w, 'conv', 'dgrad', bf)
    y0 = plain(x, wd)
    y1, sums = fused(x, wd, a)
    if with_add:
        exact = F.conv_transpose2d(x.float().reshape(B, H, W, K).permute(0, 3, 1, 2), w, padding=pad)
        exact = exact.permute(0, 2, 3, 1).reshape(npix, C)
        assert exact.abs().max().item() <= 256 and torch.equal(y0[:, :C].float(), exact)   # y0 holds the accumulators themselves
        assert torch.equal(_bits(y1[:, :C]), _bits((y0[:, :C].float() + a[:, :C].float()).to(bf)))
        y2 = torch.empty(npix, ld, dtype=bf, device=dev)
        call("sdhip_conv2d_fwd_add", ptr(x), ptr(wd), ptr(y2), ptr(a), ld, B, H, W, K, K, H, W, C, ld, k, k, pad, pad, dt, stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1[:, :C]), _bits(y2[:, :C]))
    else:
        assert torch.equal(_bits(y1[:, :C]), _bits(y0[:, :C]))
    _check_sums(sums, y1, u, sc, sh, groups, C)

    # the route: the same call past the persistent kernel
    with diag_switches(SDHIP_CONV_NO_BAND_BX="1"):
        y3, sums3 = fused(x, wd, a, band=False)
    _check_sums(sums3, y3, u, sc, sh, groups, C)
    ref = sums3.sum(0)
    assert (sums.sum(0) - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()
    if with_add:
        assert torch.equal(_bits(y1[:, :C]), _bits(y3[:, :C]))
    else:   # random inputs: the two kernels round differently; the integer-valued ones give the same bits
        wdi = ops.packed_weight(wi, 'conv', 'dgrad', bf)
        yi, _ = fused(xi, wdi, None)
        with diag_switches(SDHIP_CONV_NO_BAND_BX="1"):
            yo, _ = fused(xi, wdi, None, band=False)
        assert torch.equal(_bits(yi[:, :C]), _bits(yo[:, :C]))


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_ragged_5x5_64(with_add):
    _run(*SHAPES["ragged_5x5_64"], with_add)


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_ragged_3x3_32(with_add):
    _run(*SHAPES["ragged_3x3_32"], with_add)


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_two_tiles_across_groups_5x5_64(with_add):
    _run(*SHAPES["groups_5x5_64"], with_add)


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_channel_tail_5x5_24_of_32(with_add):
    _run(*SHAPES["tail_5x5_24_of_32"], with_add)


@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_ragged_3x3_64_outputs(with_add):
    _run(*SHAPES["ragged_3x3_64_outputs"], with_add)


@pytest.mark.gpu
@pytest.mark.parametrize("case,fuses", [("5x5", True), ("3x3", True), ("ldg", False), ("addend", False), ("tiles", False)])
def test_conv_backward_fuses_where_the_kernel_runs(case, fuses, monkeypatch):
    """ops._conv_backward beyond its small-map rule (switched off here for the 3x3 shapes, which are below it): the
    BatchNorm-backward sums ride on the data gradient exactly where that launch runs on the persistent kernel — the 5x5 and
    3x3 shapes of this file — and not where the library declines it: a gradient at pixel stride 36, a parked gradient at
    pixel stride 36, 176 tiles.  There the data gradient is a plain launch and the slot stays empty."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import last_path
    monkeypatch.setattr(ops, "BN_SLOT_MAX_BYTES", 0)
    dev, bf = "cuda", torch.bfloat16
    k, C = (5, 64) if case == "5x5" else (5, 32) if case == "tiles" else (3, 32)
    B, H, W = (1, 176, 481) if case == "tiles" else (2, 100, 440)

    def nhwc(ld):
        return torch.randn(B, H, W, ld, device=dev).to(bf)[..., :C].permute(0, 3, 1, 2)
    x, g, u = nhwc(C), nhwc(36 if case == "ldg" else C), nhwc(C)
    addend = nhwc(36) if case == "addend" else None
    w = torch.randn(C, C, k, k, device=dev) * 0.1
    slot = ops.BNSlot()
    slot.u, slot.ldu, slot.groups, slot.C = u, C, 1, C
    slot.scale, slot.shift = torch.rand(1, C, device=dev) + 0.5, torch.randn(1, C, device=dev) * 0.3
    spec = ops.ConvSpec('conv', k, k, 1, 1, k // 2, k // 2, H, W)
    gpost, _, _ = ops._conv_backward(spec, x, C, w, g, 36 if case == "ldg" else C, None, None, False, 1, True, False, addend=addend, bn_slot=slot)
    ran = last_path()
    torch.cuda.synchronize()
    assert (slot.sums is not None) == fuses == (ran in ops._BAND_BX_NAMES), (case, ran, slot.sums is not None)
    assert bool(torch.isfinite(gpost.float()).all())
