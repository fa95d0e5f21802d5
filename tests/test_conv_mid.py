"""The whole-weight-set 3x3 convolution of csrc/conv_mid.h (bf16 3x3 / stride 1 / pad 1, 64 -> 64, no prologue: the decoder
blocks on the 1/4-resolution maps), through sdhip_conv2d_fwd (plain and with the statistics epilogue) and
sdhip_conv2d_fwd_bnbwd mode 0 (the data gradient with the BatchNorm-backward sums, with and without an addend).

Without a GPU: the library's own dispatch, asked in dry mode (test_conv_kernels.chosen: sdhip_dispatch_dry / sdhip_last_path),
takes the kernel for every case below in every form, declines each single violation of path_mid's predicate, one step past
each of its limits (as shipped and as set by SDHIP_TUNE_MID_*) and every case of the tables of test_conv_kernels.py, and
takes those of the headline step's shapes it was measured faster on.
With a GPU: the operands are channel slices of NaN-filled slabs, so a NaN in y or in a sum is a padding lane, a dead pixel
or a channel past the slice that reached an MFMA or an epilogue.  The kernel keeps the halo-tile kernel's reduction order
per output element, so y must have the BITS of the same call under SDHIP_CONV_NO_MID=1; next to that it is held against
the float64 reference and bound of test_conv_kernels.fwd_ref.  The map limits of the dispatch (kMidMinMap .. kMidMaxMap:
the workload's 64x128 maps only) are lifted with SDHIP_TUNE_MID_MIN_MAP; the shapes are the smallest at which the kernel
takes another route: one tile with every border (8x32), four tiles sharing interior halo rows and columns (16x64), a
one-row and a one-column ragged tile with dead pixel rows (9x33), one ragged tile (5x13), a halo that is all padding (1x1),
the group taken from the image index (B 4 / two groups, B 2 / one), pixel strides other than 64 on x, y, u and the addend.

The statistics bound is test_conv_kernels.stats_bound with an (8, 32) tile: the kernel sums 256 stored values in f32 (two
per lane, 16 by DPP, the eight tile rows through LDS) before its f64 atomic.  A second launch must give the same bits of
the sums although the workgroups' atomics arrive in any order: every workgroup adds ONE f32-valued total per channel and
slot, and a handful of f32 values within a few binades of each other add exactly in f64, in any order.
The BatchNorm-backward sums are held against the f64 reduction over the stored y and u within the bound of
tests/test_conv.py::test_hip_dgrad_with_bn_backward_sums (2e-4 of the largest sum).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convops_ref as CR  # noqa: E402
import rowops_ref as R  # noqa: E402
import test_conv_kernels as K  # noqa: E402
from rowops_ref import check, diag_switches  # noqa: E402
from test_conv_kernels import BF16, F32, P, StatBuf, Table, Vol, bits, check_stats, code, dev, draw, fwd_ref, gpu_fwd, mk, run  # noqa: E402

NO_MID = {"SDHIP_CONV_NO_MID": "1"}
LIFT = {"SDHIP_TUNE_MID_MIN_MAP": "1"}        # the tests' maps are below kMidMinMap
SLICE = (64, 160)       # channels [64, 128) of a 160-channel slab


def md(name, **kw):
    base = dict(kh=3, kw=3, B=2, H=8, W=32, Cin=64, Cout=64, groups=1, lx="dense", ly="dense", lu="dense", la="dense", env=LIFT)
    base.update(kw)
    return mk(name, **base)


CASES = [md("map8x32"), md("map16x64", H=16, W=64), md("map9x33", H=9, W=33), md("map5x13", H=5, W=13), md("map1x1", H=1, W=1),
         md("G2_B4", B=4, groups=2, H=9, W=33), md("slabs", lx="slab8", ly=SLICE, lu="slab8", la=(24, 96), H=9, W=33)]
BYNAME = {c.name: c for c in CASES}


def on_mid(c, dtype, env=None, bx=False, addend=False, mode=0):
    """Does the dispatch (csrc/conv_fwd.hip: path_mid) run the case on conv_mid.h?  bx: through sdhip_conv2d_fwd_bnbwd;
    addend alone: sdhip_conv2d_fwd_add; neither: sdhip_conv2d_fwd."""
    return K.chosen(c, dtype, env, entry="bnbwd" if bx else "add" if addend else "fwd", addend=addend, mode=mode) == "mid"


def test_mid_predicate():
    for c in CASES:
        for kw in (dict(), dict(bx=True), dict(bx=True, addend=True)):
            assert on_mid(c, BF16, **kw), c.name
            assert not on_mid(c, F32, **kw), c.name
            assert not on_mid(c, BF16, NO_MID, **kw) and not on_mid(c, BF16, K.GENERIC_ENV, **kw), c.name
        assert not on_mid(c, BF16, bx=True, addend=True, mode=1) and not on_mid(c, BF16, addend=True), c.name
        stats = md(c.name, **dict({k: c[k] for k in ("B", "H", "W", "groups", "lx", "ly")}, stats=(2, 1)))
        assert on_mid(stats, BF16), c.name
    for tag, kw in (("k1", dict(kh=1, kw=1)), ("k5", dict(kh=5, kw=5)), ("stride2", dict(stride=2)), ("dil2", dict(dil=2)),
                    ("cin32", dict(Cin=32)), ("cin128", dict(Cin=128)), ("cout32", dict(Cout=32)), ("cout128", dict(Cout=128)),
                    ("pro", dict(pro="relu")), ("bias", dict(bias=1)), ("act", dict(act=1)), ("acc", dict(acc=1)),
                    ("lx_ldodd", dict(lx="ldodd")), ("ly_ldodd", dict(ly="ldodd")), ("lx_misal", dict(lx="misal")), ("ly_misal", dict(ly="misal")),
                    ("vol", dict(D=4, kd=3, pad_d=1))):
        assert not on_mid(md(tag, **kw), BF16), tag
    pad0 = md("pad0")
    pad0.update(pad_t=0, pad_l=0)
    assert not on_mid(pad0, BF16)
    # one step past each limit, with the limits as shipped (no override) and as set
    assert on_mid(md("at", B=8, H=64, W=128, env={}), BF16)
    assert not on_mid(md("below", B=8, H=64, W=127, env={}), BF16) and not on_mid(md("above", B=7, H=64, W=129, env={}), BF16)
    assert not on_mid(md("grid", B=9, H=64, W=128, env={}), BF16)
    assert on_mid(md("wg", B=256), BF16) and not on_mid(md("wg+1", B=257), BF16)
    assert on_mid(md("max", env={"SDHIP_TUNE_MID_MIN_MAP": "1", "SDHIP_TUNE_MID_MAX_MAP": "256"}), BF16)
    assert not on_mid(md("max+1", H=1, W=257, env={"SDHIP_TUNE_MID_MIN_MAP": "1", "SDHIP_TUNE_MID_MAX_MAP": "256"}), BF16)
    assert not on_mid(md("min-1", H=1, W=255, env={"SDHIP_TUNE_MID_MIN_MAP": "256"}), BF16)
    # the headline step (8 images, one group): the 64 -> 64 layers on the 64x128 maps are taken in every form; the 32x64 maps,
    # the 128 -> 64 c1 layers, Cout 128 and a batch of 16 (512 workgroups) are not
    for kw in (dict(), dict(bx=True), dict(bx=True, addend=True)):
        assert on_mid(md("quarter", B=8, H=64, W=128, env={}), BF16, **kw)
        assert not on_mid(md("eighth", B=8, H=32, W=64, env={}), BF16, **kw)
        assert not on_mid(md("c1", B=8, H=64, W=128, Cin=128, env={}), BF16, **kw)
        assert not on_mid(md("downup3", B=8, H=64, W=128, Cout=128, env={}), BF16, **kw)
        assert not on_mid(md("B16", B=16, H=64, W=128, env={}), BF16, **kw)
    assert on_mid(md("quarter_stats", B=8, H=64, W=128, stats=(32, 0), env={}), BF16)
    # the tables of test_conv_kernels.py: none of their cases is taken, with or without the lifted limits
    taken = {}
    for dtype in (F32, BF16):
        for c in K.FWD:
            taken[(c.name, dtype)] = on_mid(c, dtype) or on_mid(c, dtype, LIFT)
        for Cin in (32, 96, 160):        # the shapes of test_conv_kernels.test_conv2d_fwd_bnpro
            for kh in (1, 3):
                taken[("bnpro%d_%d" % (Cin, kh), dtype)] = on_mid(mk("bnpro", kh=kh, kw=kh, Cin=Cin, Cout=24, pro="relu", lx="slab8", ly="slab8", stats=(3, 1)), dtype, LIFT)
    assert not any(taken.values()), sorted(k for k, v in taken.items() if v)
    # the existing GPU tests with 3x3 64 -> 64 shapes stay on the kernels they were written for (maps below kMidMinMap)
    assert not on_mid(md("test_band", B=3, H=48, W=64, env={}), BF16) and not on_mid(md("test_conv", B=2, H=20, W=36, env={}), BF16, bx=True)


# =========================================================================== GPU
@functools.lru_cache(maxsize=None)
def _problem(name):
    """(draw, y reference, bound) of a case: computed once, shared by the tests, never written."""
    c = BYNAME[name]
    d = draw(c, BF16)
    ref, bound = fwd_ref(c, BF16, d)
    return d, ref, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_conv_mid_plain(name):
    """y has the bits of the halo-tile kernel's and lies within the f64 bound; the slab around y is untouched."""
    c = BYNAME[name]
    d, ref, bound = _problem(name)
    ybits = {}
    for tag, env in (("mid", {}), ("fast", NO_MID)):
        assert on_mid(c, BF16, env) == (tag == "mid")
        y, _ = gpu_fwd(c, BF16, d, env)
        assert K.family(K.last_path()) == tag, (name, tag, K.last_path())
        check("mid plain %s %s" % (name, tag), y.np(), ref, bound)
        assert y.pads_intact(), (name, tag)
        ybits[tag] = bits(y.v)
    assert torch.equal(ybits["mid"], ybits["fast"]), "mid plain %s: y differs from the halo-tile kernel's" % name


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_conv_mid_stats(name):
    """y as in the plain launch; the statistics are the sums of the stored y within stats_bound for an (8, 32) tile, leave
    the sentinel columns alone and come to the same bits on a second launch (module docstring)."""
    base = BYNAME[name]
    c = md(name, **dict({k: base[k] for k in ("B", "H", "W", "groups", "lx", "ly")}, stats=(3, 1)))      # the draw depends on the name only
    d, ref, bound = _problem(name)
    ybits, sbits = {}, {}
    for tag, env in (("mid", {}), ("fast", NO_MID), ("mid again", {})):
        assert on_mid(c, BF16, env) == (tag != "fast")
        y, sb = gpu_fwd(c, BF16, d, env)
        assert K.family(K.last_path()) == tag.split()[0], (name, tag, K.last_path())
        label = "mid stats %s %s" % (name, tag)
        got = y.np()
        check(label, got, ref, bound)
        assert y.pads_intact(), label
        check_stats(label + " sums", sb, got, c.groups, (8, 32) if tag != "fast" else (4, 16))
        ybits[tag], sbits[tag] = bits(y.v), bits(sb.t)
    assert torch.equal(ybits["mid"], ybits["fast"]) and torch.equal(ybits["mid"], ybits["mid again"]), "mid stats %s: y bits" % name
    assert torch.equal(sbits["mid"], sbits["mid again"]), "mid stats %s: the sums differ between two launches" % name


def gpu_bnbwd(c, d, u, sc, sh, add, env):
    """One launch of sdhip_conv2d_fwd_bnbwd mode 0 on the case's tensors; returns (y Vol, StatBuf)."""
    with diag_switches(**dict(c.env, **env)):
        x = Vol((c.B, 1, c.H, c.W, 64), BF16, c.lx, d.x)
        y = Vol((c.B, 1, c.H, c.W, 64), BF16, c.ly)
        uv = Vol((c.B, 1, c.H, c.W, 64), BF16, c.lu, u)
        av = Vol((c.B, 1, c.H, c.W, 64), BF16, c.la, add) if add is not None else None
        wp = dev(CR.pack_conv(d.w, True), BF16)
        tsc, tsh = Table(sc), Table(sh)
        sb = StatBuf(3, c.groups, 64, 1)
        run("sdhip_conv2d_fwd_bnbwd", x.p, P(wp), y.p, sb.p, sb.ld, 3, uv.p, uv.ld, tsc.p, tsh.p, av.p if av else None, av.ld if av else 0,
            c.B, c.H, c.W, 64, x.ld, c.H, c.W, 64, y.ld, 3, 3, 1, 1, 1, c.groups, 0, code(BF16))
    return y, sb


@pytest.mark.gpu
@pytest.mark.parametrize("addend", [0, 1])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_conv_mid_bnbwd(name, addend):
    """The data-gradient form: y (= conv, + addend summed in f32 and rounded once) has the bits of the halo-tile kernel's; the
    sums are sum(gm u) and sum(gm), gm = y where u scale + shift > 0, over the STORED y, in f64, within 2e-4 of the largest."""
    c = BYNAME[name]
    d, ref, bound = _problem(name)
    rng = K.rng_for(c, BF16, salt=7 + addend)
    G = c.groups
    u = R.quant(rng.standard_normal((c.B, 1, c.H, c.W, 64)), BF16)
    add = R.quant(rng.standard_normal((c.B, 1, c.H, c.W, 64)), BF16) if addend else None
    sc = K.f32(rng.uniform(0.5, 1.5, (G, 64)) * rng.choice([-1, 1], (G, 64)))
    sh = K.f32(rng.standard_normal((G, 64)) * 0.3)
    out = {}
    for tag, env in (("mid", {}), ("fast", NO_MID)):
        assert on_mid(c, BF16, env, bx=True, addend=bool(addend)) == (tag == "mid")
        y, sb = gpu_bnbwd(c, d, u, sc, sh, add, env)
        assert K.family(K.last_path()) == tag, (name, tag, K.last_path())
        label = "mid bnbwd %s add%d %s" % (name, addend, tag)
        ys = y.np()
        if addend:
            e = bound + R.U32 * (np.abs(ref) + np.abs(add))
            check(label, ys, ref + add, e + K.st(ref + add, BF16, e))
        else:
            check(label, ys, ref, bound)
        assert y.pads_intact() and sb.pads_intact(), label
        g = CR.group_of(c.B, G)
        z = u * sc[g][:, None, None, None, :] + sh[g][:, None, None, None, :]       # exact product, one f64 rounding: the sign of the f32 fma
        gm = np.where(z > 0, ys, 0.0)
        want = np.stack([(gm * u).reshape(G, -1, 64).sum(1), gm.reshape(G, -1, 64).sum(1)], 1)      # [G][2][C]
        got = sb.added()
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print("ratio %-44s %.3g" % (label + " sums", err / (2e-4 * scale + 1e-300)))
        assert err <= 2e-4 * scale, label
        out[tag] = bits(y.v)
    assert torch.equal(out["mid"], out["fast"]), "mid bnbwd %s add%d: y differs from the halo-tile kernel's" % (name, addend)
