"""The BatchNorm-backward epilogue of the halo-tile convolution (conv_fast_kernel<.., DMA, BX>, sdhip_conv2d_fwd_bnbwd) at the
smallest shapes where its batched, clamped operand loads can go wrong: ragged tiles in both directions, a channel group past
Cout, every output-channel width of both k-step forms, the 8 x 32 tile with its pipelined batches, and a map of one row.

Mode 0: y must equal, bit for bit, the plain launch of the same convolution (plus the addend, summed in f32 and rounded once);
the two sums are checked against an f64 computation from the stored y, u, scale and shift.  The cases with an addend use
small-integer x and w, so that every accumulator is an integer of at most 256 — exact in bf16: the plain launch then holds
the accumulators themselves (checked against an f64 transposed convolution), and round(y0 + addend) IS the single rounding.
Mode 1: against the two-launch route (convolution, then sdhip_affine_act_bwd with accumulate), with the bounds of
tests/test_conv.py::test_hip_1x1_dgrad_apply_mode.
In every case y stands between guard pixels of a sentinel and carries the sentinel in its channel lanes beyond Cout: a store
that lost its predicate shows.  u and the addend carry NaN beyond Cout up to their pixel stride: a clamped load that reads
the wrong lane shows in the sums (a NaN fails every comparison)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rowops_ref import diag_switches  # noqa: E402

GUARD = 48          # guard pixels in front of and behind y
SENT = 1.5          # sentinel (exact in bf16)
SMALL = {}                                                  # conv_plan's own choice: 4 x 16 tile, width split down to 32
WIDE = {"SDHIP_TUNE_SPLIT": "0"}                            # 4 x 16 tile, the unsplit width: BN = 32 / 64 / 128 by Cout
BIG = {"SDHIP_CONV_BIG": "1", "SDHIP_TUNE_SPLIT": "0"}      # 8 x 32 tile (four pixel tiles per wave: pipelined batches)


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


def _run_mode0(B, H, W, Cin, Cout, groups, with_add, env):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr, dtype_code, last_path
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(B * 1000 + H * 37 + W + Cout)
    npix, ld = B * H * W, Cout + 8
    if with_add:   # integer accumulators of at most 3*3*Cin*2 * (share of non-zero weights) -> far below 256 (asserted)
        x = torch.randint(-2, 3, (npix, Cin), generator=g).float()
        w = (torch.randint(-1, 2, (Cin, Cout, 3, 3), generator=g) * (torch.rand(Cin, Cout, 3, 3, generator=g) < 0.25)).float()
    else:
        x = torch.randn(npix, Cin, generator=g)
        w = torch.randn(Cin, Cout, 3, 3, generator=g) * 0.1
    x, w = x.to(dev).to(bf), w.to(dev)
    u = _with_nan_tail((torch.randn(npix, Cout, generator=g) * 1.3).to(dev).to(bf), Cout, ld)
    a = _with_nan_tail(torch.randn(npix, Cout, generator=g).to(dev).to(bf), Cout, ld) if with_add else None
    sc = (torch.rand(groups, Cout, generator=g) + 0.5).to(dev)
    sh = (torch.randn(groups, Cout, generator=g) * 0.3).to(dev)
    wd = ops.packed_weight(w, 'conv', 'dgrad', bf)
    dt = dtype_code(x)
    y0 = torch.empty(npix, Cout, dtype=bf, device=dev)
    whole, y1 = _guarded(npix, ld, dev)
    sums = torch.zeros(ops.NREP, groups, 2, Cout, dtype=torch.float64, device=dev)
    with diag_switches(**env):
        ops._conv_launch(x, Cin, wd, y0, Cout, None, None, None, None, B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, False, 1, 0, False)
        call("sdhip_conv2d_fwd_bnbwd", ptr(x), ptr(wd), ptr(y1), ptr(sums), Cout, ops.NREP, ptr(u), ld, ptr(sc), ptr(sh),
             ptr(a), ld if with_add else 0, B, H, W, Cin, Cin, H, W, Cout, ld, 3, 3, 1, 1, 1, groups, 0, dt, stream_ptr())
        assert last_path().startswith("fast(8x32" if "SDHIP_CONV_BIG" in env else "fast(4x16"), (last_path(), env)     # the kernel under test ran
        torch.cuda.synchronize()
    ref = y0
    if with_add:
        exact = F.conv_transpose2d(x.double().reshape(B, H, W, Cin).permute(0, 3, 1, 2), w.double(), padding=1)
        exact = exact.permute(0, 2, 3, 1).reshape(npix, Cout)
        assert exact.abs().max().item() <= 256 and torch.equal(y0.double(), exact)     # y0 holds the accumulators themselves
        ref = (y0.float() + a[:, :Cout].float()).to(bf)
    assert torch.equal(_bits(y1[:, :Cout]), _bits(ref))
    _check_guards(whole, npix, Cout)
    # the sums over the STORED values, f64.  fmaf(u, scale, shift) > 0 exactly when the exact u * scale + shift > 0, and the
    # f64 product of a bf16 and an f32 value is exact
    yv = y1[:, :Cout].double().reshape(groups, -1, Cout)
    uv = u[:, :Cout].double().reshape(groups, -1, Cout)
    gm = yv * ((uv * sc.double()[:, None] + sh.double()[:, None]) > 0)
    want = torch.stack([(gm * uv).sum(1), gm.sum(1)], 1)        # [groups][2][Cout]
    got = sums.sum(0)
    err, bound = (want - got).abs().max().item(), 2e-4 * want.abs().max().item()
    print("mode 0 sums: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound


def _run_mode1(B, H, W, K, C, Ct, groups, env):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr, dtype_code, last_path
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator().manual_seed(C * 100 + H * 7 + W)
    npix = B * H * W
    x = torch.randn(npix, K, generator=g).to(dev).to(bf)                       # gradient of the 1x1 convolution's output
    u0 = torch.randn(npix, C, generator=g).to(dev).to(bf)                      # features: the first C channels of the slab
    gs0 = torch.randn(npix, C, generator=g).to(dev).to(bf)                     # slab gradient so far
    w = (torch.randn(K, C, 1, 1, generator=g) * 0.1).to(dev)
    sc = (torch.rand(groups, C, generator=g) + 0.5).to(dev)
    sh = (torch.randn(groups, C, generator=g) * 0.3).to(dev)
    wd = ops.packed_weight(w, 'conv', 'dgrad', bf)
    dt = dtype_code(x)
    slab = _with_nan_tail(u0, C, Ct)
    whole, gs = _guarded(npix, Ct, dev)
    gs[:, :C] = gs0
    both = torch.zeros(2, ops.NREP, groups, C, dtype=torch.float32, device=dev)
    # the two-launch route, on clean copies
    gp = torch.empty(npix, C, dtype=bf, device=dev)
    gs_ref = gs0.clone()
    both0 = torch.zeros_like(both)
    with diag_switches(**env):
        ops._conv_launch(x, K, wd, gp, C, None, None, None, None, B, H, W, K, H, W, C, 1, 1, 1, 1, 0, 0, False, 1, 0, False)
        call("sdhip_affine_act_bwd", ptr(gp), C, ptr(u0), C, ptr(gs_ref), C, ptr(sc), ptr(sh), ptr(both0[0]), ptr(both0[1]), ops.NREP,
             npix, C, groups, 1, 1, 0, dt, stream_ptr())
        call("sdhip_conv2d_fwd_bnbwd", ptr(x), ptr(wd), ptr(gs), ptr(both), C, ops.NREP, ptr(slab), Ct, ptr(sc), ptr(sh), ptr(gs), Ct,
             B, H, W, K, K, H, W, C, Ct, 1, 1, 1, 0, 0, groups, 1, dt, stream_ptr())
        assert last_path().startswith("fast(8x32" if "SDHIP_CONV_BIG" in env else "fast(4x16"), (last_path(), env)
        torch.cuda.synchronize()
    a, b = gs[:, :C].float(), gs_ref.float()
    err, bound = (a - b).abs().max().item(), 3e-2 * b.abs().max().item()
    print("mode 1 y: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    _check_guards(whole, npix, C)                                              # channels beyond C untouched, too
    ra, rb = both.double().sum(1), both0.double().sum(1)
    err, bound = (ra - rb).abs().max().item(), 2e-2 * rb.abs().max().item()
    print("mode 1 sums: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound


# ---- 4 x 16 tile, ragged both ways (5 = 4 + 1 rows, 19 = 16 + 3 columns); the group comes from the image index ----
@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("B,groups", [(2, 1), (4, 2)])
def test_small_tile_ragged(B, groups, with_add):
    _run_mode0(B, 5, 19, 32, 128, groups, with_add, SMALL)


# ---- Cout = 36: a multiple of 4, not of 16 — the last lanes' channel group lies past Cout, and n0 + BN > Cout ----
@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
def test_channel_tail_mode0(with_add):
    _run_mode0(2, 4, 16, 32, 36, 1, with_add, SMALL)


@pytest.mark.gpu
def test_channel_tail_mode1():
    _run_mode1(2, 4, 16, 128, 36, 64, 1, SMALL)


# ---- every width the step uses on the small tile: 64-byte rows (Cin 32, 3x3) and 128-byte rows (Cin 128, 1x1, in place) ----
@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("Cout", [32, 64, 128])
def test_every_width_ks1(Cout, with_add):
    _run_mode0(2, 3, 17, 32, Cout, 1, with_add, WIDE)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [32, 64, 128, 96])     # 96: the 128-wide form with a quarter of its channel groups past Cout
def test_every_width_ks2_in_place(C):
    _run_mode1(2, 3, 17, 128, C, 160, 1, WIDE)


# ---- 8 x 32 tile (SDHIP_CONV_BIG, re-read in process): 9 x 33 = one row and one column past a tile, 8 x 32 = interior ----
@pytest.mark.gpu
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("H,W", [(9, 33), (8, 32)])
def test_big_tile_mode0(H, W, with_add):
    _run_mode0(2, H, W, 32, 128, 1, with_add, BIG)


@pytest.mark.gpu
def test_big_tile_mode0_two_groups():
    _run_mode0(4, 9, 33, 32, 128, 2, True, BIG)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(9, 33), (8, 32)])
def test_big_tile_mode1_in_place(H, W):
    _run_mode1(2, H, W, 128, 128, 160, 1, BIG)


# ---- one image row: every pixel of tile rows 1 .. is clamped onto row 0 ----
@pytest.mark.gpu
@pytest.mark.parametrize("env", [SMALL, BIG], ids=["small", "big"])
@pytest.mark.parametrize("with_add", [False, True])
def test_one_row_mode0(with_add, env):
    _run_mode0(2, 1, 40, 32, 128, 1, with_add, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [SMALL, BIG], ids=["small", "big"])
def test_one_row_mode1(env):
    _run_mode1(2, 1, 40, 128, 96, 160, 1, env)
