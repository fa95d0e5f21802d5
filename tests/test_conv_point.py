"""The pointwise split-K convolution of csrc/conv_point.h (bf16 1x1 with an input prologue over >= 128 channels on small maps:
conv1 of the DenseNet bottlenecks), through sdhip_conv2d_fwd (given in_scale / in_shift) and sdhip_conv2d_fwd_bnpro (the
consumer-side BatchNorm finalize), against the float64 references and bounds of tests/test_conv_kernels.py.

Without a GPU: the library's own dispatch, asked in dry mode (test_conv_kernels.chosen: sdhip_dispatch_dry / sdhip_last_path),
takes the kernel for every case below, declines each single violation of path_point's predicate and every case of the
tables of test_conv_kernels.py.
With a GPU: tensors are channel slices of NaN-filled slabs (x inside a 1024-channel slab as in a dense block: a NaN in y is
a lane past Cin or a pixel row past the image that reached an MFMA), shapes are the smallest at which the kernel takes
another path: a k-step tail inside a 64-channel weight row (160, 288, 992), fewer k-steps than waves (128, 160), uneven
k-step counts per wave (288, 992), 1 .. 4 k-steps per wave (128 / 512 / 992 / 1024), a 15-pixel tile, a tile of one pixel.

The statistics bound is test_conv_kernels.stats_bound with a (4, 16) tile: the kernel sums 64 stored values in f32 (16 by
DPP, four 16-pixel tiles through LDS) before its f64 atomic.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convops_ref as CR  # noqa: E402
import rowops_ref as R  # noqa: E402
import test_conv_kernels as K  # noqa: E402
from rowops_ref import U32, check  # noqa: E402
from test_conv_kernels import (BF16, BNPRO_COMBOS, EPS32, F32, MOM32, P, StatBuf, Table, Vol, bits, check_stats, code, dev, draw, draw_bnpro,  # noqa: E402
                               fwd_ref, gpu_fwd, isbf, mk, pro_err, run, st)

NO_POINT = {"SDHIP_CONV_NO_POINT": "1"}
SLAB = (0, 1024)        # x as the first Cin channels of a 1024-channel slab


def pt(name, **kw):
    base = dict(kh=1, kw=1, B=4, H=8, W=16, Cin=128, Cout=128, pro="relu", groups=2, lx=SLAB, ly="slab8", stats=(2, 1))
    base.update(kw)
    return mk(name, **base)


CASES = [pt("cin%d" % ci, Cin=ci) for ci in (128, 160, 288, 512, 992, 1024)]
CASES += [pt("map3x5", H=3, W=5, Cin=160, lx="slab8"), pt("map5x13", H=5, W=13, Cin=288, lx="slab8"),
          pt("cout256", Cout=256, Cin=160), pt("G1", groups=1, Cin=288, stats=(3, 0)), pt("G1_B2", groups=1, B=2, stats=(1, 0)),
          pt("lin", pro="lin", Cin=160), pt("lin_map3x5", pro="lin", H=3, W=5, Cin=992, ly="dense")]
BYNAME = {c.name: c for c in CASES}


def on_point(c, dtype, env=None):
    """Does the dispatch of sdhip_conv2d_fwd (csrc/conv_fwd.hip: path_point) run the case on conv_point.h?"""
    return K.chosen(c, dtype, env) == "point"


def test_point_predicate():
    for c in CASES:
        assert on_point(c, BF16), c.name
        assert not on_point(c, F32), c.name
        assert not on_point(c, BF16, NO_POINT) and not on_point(c, BF16, K.GENERIC_ENV), c.name
    for tag, kw in (("cin96", dict(Cin=96)), ("cout24", dict(Cout=24)), ("cout136", dict(Cout=136)), ("k3", dict(kh=3, kw=3)),
                    ("stride2", dict(stride=2)), ("nopro", dict(pro=None)), ("acc", dict(acc=1)), ("bias", dict(bias=1)),
                    ("ldodd", dict(lx="ldodd")), ("cin1032", dict(Cin=1032, lx="dense")), ("pixels", dict(B=4, H=128, W=128)),
                    ("act", dict(act=1)), ("nostats", dict(stats=None)), ("ly_ldodd", dict(ly="ldodd")), ("lx_misal", dict(lx="misal"))):
        assert not on_point(pt(tag, **kw), BF16), tag
    assert on_point(pt("block3", B=16, H=16, W=32, Cin=992), BF16)                  # 512 workgroups: the limit
    assert not on_point(pt("block2", B=16, H=32, W=64, Cin=480), BF16)              # 2048
    assert not on_point(pt("transition3", B=16, H=16, W=32, Cin=1024, Cout=512), BF16)
    assert not on_point(pt("cout512", Cin=1024, Cout=512), BF16) and not on_point(pt("map32x32", H=32, W=32), BF16)
    for dtype in (F32, BF16):
        for c in K.FWD:
            assert not on_point(c, dtype), c.name
        for Cin in (32, 96, 160):        # the shapes of test_conv_kernels.test_conv2d_fwd_bnpro
            for kh in (1, 3):
                assert not on_point(mk("bnpro", kh=kh, kw=kh, Cin=Cin, Cout=24, pro="relu", lx="slab8", ly="slab8"), dtype)


# =========================================================================== GPU: sdhip_conv2d_fwd with in_scale / in_shift
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_conv_point_fwd(name):
    """New kernel and the kernel it replaces (SDHIP_CONV_NO_POINT) against the same reference and against each other: y within
    the bound with no element excluded, the slab around y untouched, the statistics the sums of the stored y; a second launch
    of the new kernel gives the same y bits."""
    c = BYNAME[name]
    d = draw(c, BF16)
    assert np.abs(d.sh).min() >= 0.25 and (d.sc < 0).any() and (d.sh < 0).any() and (d.sh > 0).any()
    ref, bound = fwd_ref(c, BF16, d)
    got, ybits = {}, {}
    for tag, env in (("point", {}), ("fast", NO_POINT), ("point again", {})):
        y, sb = gpu_fwd(c, BF16, d, env)
        assert K.family(K.last_path()) == tag.split()[0], (name, tag, K.last_path())
        label = "point %s %s" % (name, tag)
        got[tag] = y.np()
        check(label, got[tag], ref, bound)
        assert y.pads_intact(), label
        if sb:
            check_stats(label + " stats", sb, got[tag], c.groups, (4, 16))
        ybits[tag] = bits(y.v)
    assert torch.equal(ybits["point"], ybits["point again"]), "point %s: y differs between two launches" % name
    check("point %s new against old" % name, got["point"], got["fast"], bound)


# =========================================================================== GPU: sdhip_conv2d_fwd_bnpro
@pytest.mark.gpu
@pytest.mark.parametrize("Cin", [128, 160, 1024])
def test_conv_point_bnpro(Cin):
    """The assertions of test_conv_kernels.test_conv2d_fwd_bnpro on the shapes that take the new kernel (1x1, Cout 128)."""
    from test_bn_kernels import b_finalize
    dtype, kh, pad = BF16, 1, 0
    for (G, nrep, pend_nrep, running, out_stats) in BNPRO_COMBOS:
        d = draw_bnpro(kh, Cin, G, nrep, pend_nrep, running, dtype, Cout=128)
        c0 = Cin - 32
        r = CR.bnpro(d.x, d.w, d.in_stats, d.count, d.gamma, d.beta, d.rm0, d.rv0, EPS32, MOM32, G, d.pend, c0, pad, pad)
        S = r["in_stats"].sum(0)[:, :, :Cin] if pend_nrep else R.replica_sum(d.in_stats)
        bf_ = b_finalize(S, d.count, d.gamma, d.beta, d.rm0, d.rv0)
        x = Vol((d.B, 1, d.H, d.W, Cin), dtype, "slab8", d.x)
        y = Vol((d.B, 1, d.H, d.W, d.Cout), dtype, "slab8")
        wp = dev(CR.pack_conv(d.w, isbf(dtype)), dtype)
        ld_in = Cin + 3
        ins = torch.full((nrep, G, 2, ld_in), -7.25, dtype=torch.float64, device="cuda")
        ins[..., :Cin] = torch.from_numpy(d.in_stats).cuda()
        ins0 = ins.clone()
        pend = None
        if pend_nrep:
            pend = torch.full((pend_nrep, G, 2, 37), float('nan'), dtype=torch.float64, device="cuda")
            pend[..., :32] = torch.from_numpy(d.pend).cuda()
        gam, bet = Table(d.gamma), Table(d.beta)
        rm, rv = (Table(d.rm0), Table(d.rv0)) if running else (None, None)
        outs = [torch.full((G * Cin + 16,), float('nan'), dtype=torch.float32, device="cuda") for _ in range(4)]
        sb = StatBuf(3, G, d.Cout, 1) if out_stats else None
        run("sdhip_conv2d_fwd_bnpro", x.p, P(wp), y.p, sb.p if sb else None, sb.ld if sb else 0, 3 if sb else 1,
            P(ins), ld_in, nrep, P(pend), 37, max(pend_nrep, 1), c0, 32 if pend_nrep else 0, gam.p, bet.p,
            rm.p if rm else None, rv.p if rv else None, P(outs[0], 32), P(outs[1], 32), P(outs[2], 32), P(outs[3], 32),
            ctypes.c_double(d.count), ctypes.c_float(EPS32), ctypes.c_float(MOM32),
            d.B, d.H, d.W, Cin, x.ld, d.H, d.W, d.Cout, y.ld, kh, kh, pad, pad, G, code(dtype))
        assert K.last_path() == "point", (Cin, G, K.last_path())
        label = "point bnpro Cin%d G%d nrep%d pend%d" % (Cin, G, nrep, pend_nrep)
        for key, o in zip(("scale", "shift", "mean", "invstd"), outs):
            check(label + " " + key, o[8:8 + G * Cin].double().cpu().numpy().reshape(G, Cin), r[key], bf_[key])
            assert bool(torch.isnan(o[:8]).all() and torch.isnan(o[8 + G * Cin:]).all())
        if running:
            check(label + " rmean", rm.t[8:8 + Cin].double().cpu().numpy(), r["rmean"], bf_["rmean"])
            check(label + " rvar", rv.t[8:8 + Cin].double().cpu().numpy(), r["rvar"], bf_["rvar"])
        want = ins0.clone()
        if pend_nrep:
            folded = ins[0, :, :, c0:Cin].cpu().numpy()
            check(label + " fold", folded, d.pend.sum(0), 2.0 ** -50 * np.abs(d.pend).sum(0) + 1e-300)
            want[0, :, :, c0:Cin] = ins[0, :, :, c0:Cin]
        assert torch.equal(bits(ins), bits(want)), label + ": in_stats outside the folded channels"
        A = CR.corr(np.abs(CR.prologue(d.x, r["scale"], r["shift"], 1, G)), np.abs(d.w), pad_t=pad, pad_l=pad)
        e = (Cin * kh * kh + 1) * U32 * A + CR.corr(pro_err(d.x, r["scale"], r["shift"], G, dtype, bf_["scale"], bf_["shift"]), np.abs(d.w), pad_t=pad, pad_l=pad)
        got = y.np()
        check(label + " y", got, r["y"], e + st(r["y"], dtype, e) + 1e-300)
        assert y.pads_intact(), label
        if sb:
            check_stats(label + " out_stats", sb, got, G, (4, 16))
