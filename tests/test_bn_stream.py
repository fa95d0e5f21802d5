"""The streaming bodies and the replica folds of pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/bn_act.hip at the
shapes where they can go wrong, against the float64 references of tests/rowops_ref.py within the bounds of
tests/test_bn_kernels.py (imported, not copied: its `plan` mirror, its bounds and its case runners).

A streaming trip of affine_act_bwd, bn_bwd_apply and bn_bwd_apply_fin issues the loads of 4 pixels of every input tensor
before it uses any (act_out_bwd: 2; the other kernels walk one pixel per trip, and so do the 4-pixel ones on a map with one
pixel per thread); full trips run without a guard, the last, ragged one loads a pixel past the end from the trip's own first
row and drops the result.  With two or more statistics groups a fold issues a window of 16 replica loads per thread and
its per-channel parameters before it waits, walks replicas beyond the window in a plain loop, and folds up to two groups
into one barrier pair; with one group it is the plain loop.

Every tensor here is a channel slice of a NaN-filled slab that goes on for at least one trip's worth of NaN rows after the
last pixel (TailRows): a load that runs past the end poisons a result instead of leaving the allocation, and a row that only
stands in for a missing pixel must not reach an output or a sum.

  ragged trips   pixel counts per group 1, ty - 1, ty + 1, 2 full trips + 37 (the last trip's k = 0 partly valid, k >= 1
                 empty; where a trip's k holds 37 pixels or fewer: all but 3 of them), 1 full trip + one full k + 3.
                 affine_act_bn / bn_bwd_apply_fin: C = 64 and C = 8 (tx = 1 in bf16) with SDHIP_TUNE_FUSED_BLOCKS = 2;
                 the kernels without that switch: the small counts at C = 64, the two large ones at C = 520 at their caps
  in place       gx == gy for bn_bwd_apply_fin, bn_bwd_apply and stats_fix at those counts
  accumulate     affine_act_bwd with gx += and with gx NULL (sums only) at those counts
  folds          nrep 1, 2, 3, 32, 40 (40 goes past the window at C = 128); groups 1, 2, 3 (3 takes the serial walk);
                 C = 8, 72, 128, 520; strided statistics; f32 and f64 sums; accumulate_params with param_scale 0.5
  stats_fix_fin  Cf = 64, 96, 1024 with the slice first, in the middle and last; groups 1 and 2 (3 in one case); one case
                 at the cap of 2048 workgroups

The cases at the caps cannot be smaller than a full trip of a capped grid (1024 or 2048 workgroups x 256 threads x 4 pixels
x 16 bytes per tensor): one kernel at one of the two large counts per case, each up to about a second, most of it the
float64 reference and bound on the CPU; everything else is a few milliseconds per call."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from rowops_ref import U32, Rows, check, quant, diag_switches  # noqa: E402
import test_bn_kernels as K  # noqa: E402

F32, BF16 = K.F32, K.BF16
DTYPES = K.DTYPES
KTRIP = 4                      # pixels per trip of every streaming body
NREPS = [1, 2, 3, 32, 40]
P, dev, run, code, f32, rng_for = K.P, K.dev, K.run, K.code, K.f32, K.rng_for


class TailRows(Rows):
    """Rows whose slab goes on for `tail` NaN rows after the last pixel, inside the same allocation."""
    tail = 0

    def __init__(self, n, C, dtype, lay="dense", vals=None):
        self.k, self.ld = R.layout(lay, C) if isinstance(lay, str) else lay
        self.C, self.n = C, n
        self.slab = torch.full((n + TailRows.tail, self.ld), float('nan'), dtype=dtype, device="cuda")
        self.v = self.slab[:n, self.k:self.k + C]
        if vals is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64).reshape(n, C)).to(dtype))
        self.before = self.slab.clone()

    def pads_intact(self):
        bits = torch.int32 if self.slab.element_size() == 4 else torch.int16
        a, b = self.slab.clone(), self.before.clone()
        a[:self.n, self.k:self.k + self.C] = 0
        b[:self.n, self.k:self.k + self.C] = 0
        return bool(torch.equal(a.view(bits), b.view(bits)))


@pytest.fixture
def tail(monkeypatch):
    """The case runners of test_bn_kernels.py build their tensors as TailRows; tail(rows) sets the NaN rows after the end."""
    monkeypatch.setattr(K, "Rows", TailRows)

    def set_tail(rows):
        TailRows.tail = int(rows)
    yield set_tail
    TailRows.tail = 0


def units(dtype, C):
    return C // K.vecn(dtype) if C % K.vecn(dtype) == 0 else C


def ragged(ty, gx):
    """Pixel counts per group for a grid of gx workgroups of ty pixel rows."""
    per = gx * ty                                  # pixels of one k of a trip
    r = 37 if per > 37 else max(per - 3, 1)
    return [1, ty - 1, ty + 1, 2 * KTRIP * per + r, KTRIP * per + per + 3]


# ------------------------------------------------------------------ case runners the other file does not have
def act_bwd_case(dtype, C, n, G, nrep, act, mode, rng, label, max_blocks=1024):
    """affine_act_bwd: mode 'accumulate' (gx += on top of old values), 'red only' (gx NULL) or 'gx+red'."""
    x, gy, sc, sf = K.draw(rng, n, C, G, dtype)
    old = quant(rng.standard_normal((n, C)), dtype) if mode == "accumulate" else None
    xd, gd = TailRows(n, C, dtype, "dense", x), TailRows(n, C, dtype, "dense", gy)
    gxd = TailRows(n, C, dtype, "dense", old) if mode != "red only" else None
    ds = torch.full((nrep, G, C), float('nan'), device="cuda")
    dh = torch.full((nrep, G, C), float('nan'), device="cuda")
    run("sdhip_affine_act_bwd", gd.p, gd.ld, xd.p, xd.ld, gxd.p if gxd else None, gxd.ld if gxd else 0, P(dev(sc)), P(dev(sf)),
        P(ds), P(dh), nrep, n, C, G, act, int(mode == "accumulate"), 0, code(dtype))
    rows = [gd, xd] + ([gxd] if gxd else [])
    _, ty, gx, _, n_t = K.geom(dtype, C, n, G, max_blocks, *rows)
    gxr, dsr, dhr = R.affine_act_bwd(gy, x, sc, sf, G, act)
    e_gx, e_ds, e_dh, keep = K.b_act_bwd(gy, x, sc, sf, G, act, dtype, n_t + ty + -(-gx // nrep), old)
    K._finite_and_intact(*rows)
    if gxd:
        check(label + " gx", gxd.np(), gxr + (old if old is not None else 0), e_gx, keep)
    assert bool(torch.isfinite(ds).all() and torch.isfinite(dh).all()), "a row that is no pixel reached the sums"
    check(label + " dscale", ds.double().sum(0).cpu().numpy(), dsr, e_ds)
    check(label + " dshift", dh.double().sum(0).cpu().numpy(), dhr, e_dh)


def apply_fix_in_place_case(dtype, C, n, G, act, rng, label, which=("stats_fix", "bn_bwd_apply")):
    """stats_fix and bn_bwd_apply with the output on top of the incoming gradient."""
    x, gy, sc, sf = K.draw(rng, n, C, G, dtype)
    dSv = rng.standard_normal((G, 2, C)) * 0.1
    dS = K.Stats(1, G, C, True, dSv[None])
    xd = TailRows(n, C, dtype, "dense", x)
    if "stats_fix" in which:
        gd = TailRows(n, C, dtype, "dense", gy)
        run("sdhip_stats_fix", gd.p, gd.ld, xd.p, xd.ld, gd.p, gd.ld, dS.p, dS.ld, n, C, G, code(dtype))
        K._finite_and_intact(xd, gd, dS)
        check(label + " stats_fix in place", gd.np(), R.stats_fix(gy, x, dSv, G), K.b_stats_fix(gy, x, dSv, G, dtype))
    if "bn_bwd_apply" in which:
        gd = TailRows(n, C, dtype, "dense", gy)
        run("sdhip_bn_bwd_apply", gd.p, gd.ld, xd.p, xd.ld, gd.p, gd.ld, P(dev(sc)), P(dev(sf)), dS.p, dS.ld, n, C, G, act, code(dtype))
        K._finite_and_intact(xd, gd, dS)
        bound, keep = K.b_bwd_apply(gy, x, sc, sf, dSv, G, act, dtype)
        check(label + " bn_bwd_apply in place", gd.np(), R.bn_bwd_apply(gy, x, sc, sf, dSv, G, act), bound, keep)


def bwd_fin_in_place_case(dtype, C, n, G, nrep, act, acc, pscale, f64_sums, rng, label):
    """K._bwd_fin_case with gx == gy."""
    count, gamma, mean, invstd, ds, dh = K._bwd_inputs(rng, G, C, nrep, n)
    x, gy, sc, sf = K.draw(rng, n, C, G, dtype)
    dg0, db0 = f32(rng.standard_normal(C)), f32(rng.standard_normal(C))
    nan = lambda: torch.full((C,), float('nan'), device="cuda")
    dgd, dbd = (dev(dg0), dev(db0)) if acc else (nan(), nan())
    xd, gd = TailRows(n, C, dtype, "dense", x), TailRows(n, C, dtype, "dense", gy)
    head = (gd.p, gd.ld, xd.p, xd.ld, gd.p, gd.ld, P(dev(sc)), P(dev(sf)))
    tl = (nrep, P(dev(gamma)), P(dev(mean)), P(dev(invstd)), P(dgd), P(dbd), int(acc), pscale, n, C, G, float(count), act, code(dtype))
    g64 = lambda v: np.asarray(v, np.float64)
    if f64_sums:
        sums = np.stack([rng.standard_normal((nrep, G, C)) * math.sqrt(count), rng.standard_normal((nrep, G, C)) * math.sqrt(count)], 2)
        run("sdhip_bn_bwd_apply_fin_d", *head, P(dev(sums, np.float64)), *tl)
        dsv, dhv = sums[:, :, 0], sums[:, :, 1]
    else:
        run("sdhip_bn_bwd_apply_fin", *head, P(dev(ds)), P(dev(dh)), *tl)
        dsv, dhv = g64(ds), g64(dh)
    dgr, dbr, dSr = R.bn_finalize_bwd(dsv.sum(0), dhv.sum(0), g64(gamma), g64(mean), g64(invstd), count)
    e_dg, e_db, e_dmu, e_dvar = K.b_finalize_bwd(dsv, dhv, g64(gamma), g64(mean), g64(invstd), count)
    p32 = float(np.float32(pscale))
    dgr, dbr, e_dg, e_db = dgr * p32, dbr * p32, e_dg * p32 + U32 * np.abs(dgr * p32), e_db * p32 + U32 * np.abs(dbr * p32)
    if acc:
        dgr, dbr = dgr + dg0, dbr + db0
        e_dg, e_db = e_dg + U32 * (np.abs(dg0) + np.abs(dgr)), e_db + U32 * (np.abs(db0) + np.abs(dbr))
    K._finite_and_intact(xd, gd)
    check(label + " dgamma", dgd.double().cpu().numpy(), dgr, e_dg)
    check(label + " dbeta", dbd.double().cpu().numpy(), dbr, e_db)
    bound, keep = K.b_bwd_apply(gy, x, sc, sf, dSr, G, act, dtype, e_dmu, e_dvar)
    check(label + " gx in place act%d" % act, gd.np(), R.bn_bwd_apply(gy, x, sc, sf, dSr, G, act), bound, keep)


def stats_fix_fin_case(dtype, Cf, cs, n, G, nrep, acc, pscale, in_place, rng, label, lay=None):
    """The body of K.test_stats_fix_fin for one case, on TailRows, optionally with gout == gin."""
    count, gamma, mean, invstd, ds, dh = K._bwd_inputs(rng, G, Cf, nrep, n)
    x, gin = K.make_x(rng, n, 32, dtype), quant(rng.standard_normal((n, 32)), dtype)
    ldc = Cf + 3
    dS0 = rng.standard_normal((G, 2, ldc)) * 0.05
    dSd = torch.from_numpy(dS0).cuda()
    dg0, db0 = f32(rng.standard_normal(Cf)), f32(rng.standard_normal(Cf))
    nan = lambda: torch.full((Cf,), float('nan'), device="cuda")
    dgd, dbd = (dev(dg0), dev(db0)) if acc else (nan(), nan())
    lay = (cs, Cf + 8) if lay is None else lay
    xd, gd = TailRows(n, 32, dtype, lay, x), TailRows(n, 32, dtype, lay, gin)
    od = gd if in_place else TailRows(n, 32, dtype, lay)
    run("sdhip_stats_fix_fin", gd.p, gd.ld, xd.p, xd.ld, od.p, od.ld, n, P(dSd), ldc, cs, P(dev(ds)), P(dev(dh)), nrep,
        P(dev(gamma)), P(dev(mean)), P(dev(invstd)), P(dgd), P(dbd), int(acc), pscale, Cf, G, float(count), code(dtype))
    g64 = lambda v: np.asarray(v, np.float64)
    dgr, dbr, dSr = R.bn_finalize_bwd(g64(ds).sum(0), g64(dh).sum(0), g64(gamma), g64(mean), g64(invstd), count)
    e_dg, e_db, e_dmu, e_dvar = K.b_finalize_bwd(g64(ds), g64(dh), g64(gamma), g64(mean), g64(invstd), count)
    p32 = float(np.float32(pscale))
    dgr, dbr, e_dg, e_db = dgr * p32, dbr * p32, e_dg * p32 + U32 * np.abs(dgr * p32), e_db * p32 + U32 * np.abs(dbr * p32)
    if acc:
        dgr, dbr = dgr + dg0, dbr + db0
        e_dg, e_db = e_dg + U32 * (np.abs(dg0) + np.abs(dgr)), e_db + U32 * (np.abs(db0) + np.abs(dbr))
    K._finite_and_intact(xd, gd, od)
    check(label + " dgamma", dgd.double().cpu().numpy(), dgr, e_dg)
    check(label + " dbeta", dbd.double().cpu().numpy(), dbr, e_db)
    got = dSd.cpu().numpy()
    sl = np.zeros(ldc, bool); sl[cs:cs + 32] = True
    out = np.zeros(ldc, bool); out[:Cf] = True; out &= ~sl
    assert np.array_equal(got[:, :, sl], dS0[:, :, sl]) and np.array_equal(got[:, :, Cf:], dS0[:, :, Cf:]), "dS changed inside the slice or past Cf"
    full = dS0[:, :, :Cf] + dSr
    check(label + " dS", got[:, :, out], full[:, :, out[:Cf]], (np.stack([e_dmu, e_dvar], 1) + K.F64EPS * np.abs(full))[:, :, out[:Cf]])
    dsl = full[:, :, cs:cs + 32]
    check(label + " gout", od.np(), R.stats_fix(gin, x, dsl, G), K.b_stats_fix(gin, x, dsl, G, dtype, e_dmu[:, cs:cs + 32], e_dvar[:, cs:cs + 32]))


# ------------------------------------------------------------------ ragged trips
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,G", [(64, 1), (64, 2), (8, 1)])
def test_fused_kernels_ragged_trips(dtype, C, G, tail):
    """affine_act_bn (with and without a residual) and bn_bwd_apply_fin (in place; f32 and f64 sums) with the grid held at
    2 workgroups per block row: every count of ragged()."""
    with diag_switches(SDHIP_TUNE_FUSED_BLOCKS=2):
        tx, ty, _, gy, _ = K.plan(units(dtype, C), 1 << 30, G, 2)
        gx = max(2 // (gy * G), 1)
        tail(KTRIP * gx * ty)
        for i, npix_g in enumerate(ragged(ty, gx)):
            n = npix_g * G
            assert K.plan(units(dtype, C), npix_g, G, 2)[2] == min(gx, -(-npix_g // ty))
            K._affine_act_bn_case(dtype, C, "dense", n, G, 3, i % 2 == 1, i % 3, i % 2 == 0, "all", rng_for(C, G, i, 31),
                                  "affine_act_bn n=%d" % npix_g)
            bwd_fin_in_place_case(dtype, C, n, G, 3, (1, 0, 2)[i % 3], i % 2 == 0, 0.5, i % 2 == 1, rng_for(C, G, i, 32),
                                  "bn_bwd_apply_fin n=%d" % npix_g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 8])
def test_plain_kernels_short_counts(dtype, C, tail):
    """The kernels without a grid switch at 1, ty - 1 and ty + 1 pixels per group (only the ragged trip runs), groups 1
    and 2: affine_act, affine_act_bwd accumulating and with gx NULL, stats_fix and bn_bwd_apply in place."""
    tx, ty, _, _, _ = K.plan(units(dtype, C), 1 << 30, 1)
    tail(KTRIP * 2 * ty)
    for G in (1, 2):
        for i, npix_g in enumerate(ragged(ty, 1)[:3]):
            n = npix_g * G
            rng = rng_for(C, G, i, 33)
            x, res = K.make_x(rng, n, C, dtype), quant(rng.standard_normal((n, C)), dtype)
            sc, sf = K._coeffs(rng, G, C)
            xd, rd, yd = TailRows(n, C, dtype, "dense", x), TailRows(n, C, dtype, "dense", res), TailRows(n, C, dtype)
            run("sdhip_affine_act", xd.p, xd.ld, yd.p, yd.ld, rd.p, rd.ld, P(dev(sc)), P(dev(sf)), n, C, G, i % 3, code(dtype))
            K._finite_and_intact(xd, rd, yd)
            check("affine_act n=%d" % npix_g, yd.np(), R.affine_act(x, sc, sf, G, i % 3, res), K.b_affine_act(x, sc, sf, G, i % 3, res, dtype))
            act_bwd_case(dtype, C, n, G, 3, (1, 2, 0)[i], "accumulate", rng_for(C, G, i, 34), "affine_act_bwd += n=%d" % npix_g)
            act_bwd_case(dtype, C, n, G, 2, (0, 1, 2)[i], "red only", rng_for(C, G, i, 35), "affine_act_bwd sums n=%d" % npix_g)
            apply_fix_in_place_case(dtype, C, n, G, i % 3, rng_for(C, G, i, 36), "n=%d" % npix_g)


def _capped_count(dtype, max_blocks, which):
    """C = 520, groups 1, at the cap: (pixels of one k of a trip, the `which`-th large count of ragged())."""
    tx, ty, gx, gy, _ = K.plan(units(dtype, 520), 1 << 30, 1, max_blocks)
    return gx * ty, ragged(ty, gx)[3 + which]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1], ids=["2trips+37", "1trip+1k+3"])
@pytest.mark.parametrize("kern", ["accumulate", "sums", "stats_fix", "bn_bwd_apply", "affine_act"])
def test_plain_kernels_ragged_trips_at_the_cap(dtype, which, kern, tail):
    """C = 520 at the caps (1024 workgroups for affine_act_bwd and bn_bwd_apply, 2048 for affine_act and stats_fix), where a
    thread of these kernels has more than one trip.  Both large counts for each of: affine_act_bwd accumulating and with
    gx NULL, stats_fix and bn_bwd_apply in place, affine_act with a residual."""
    C, G = 520, 1
    per1, n1 = _capped_count(dtype, 1024, which)
    per2, n2 = _capped_count(dtype, 2048, which)
    tail(KTRIP * per2)
    assert n1 % (KTRIP * per1) == (37 if which == 0 else per1 + 3) and n2 % (KTRIP * per2) == (37 if which == 0 else per2 + 3)
    if kern == "accumulate":
        act_bwd_case(dtype, C, n1, G, 3, 1, "accumulate", rng_for(which, 37), "affine_act_bwd += capped")
    elif kern == "sums":
        act_bwd_case(dtype, C, n1, G, 3, 0, "red only", rng_for(which, 47), "affine_act_bwd sums capped")
    elif kern == "stats_fix":
        apply_fix_in_place_case(dtype, C, n2, G, 0, rng_for(which, 38), "capped", which=("stats_fix",))
    elif kern == "bn_bwd_apply":
        apply_fix_in_place_case(dtype, C, n1, G, 1, rng_for(which, 48), "capped", which=("bn_bwd_apply",))
    else:
        rng = rng_for(which, 39)
        x, res = K.make_x(rng, n2, C, dtype), quant(rng.standard_normal((n2, C)), dtype)
        sc, sf = K._coeffs(rng, G, C)
        xd, rd, yd = TailRows(n2, C, dtype, "dense", x), TailRows(n2, C, dtype, "dense", res), TailRows(n2, C, dtype)
        run("sdhip_affine_act", xd.p, C, yd.p, C, rd.p, C, P(dev(sc)), P(dev(sf)), n2, C, G, 1, code(dtype))
        K._finite_and_intact(xd, rd, yd)
        check("affine_act capped", yd.np(), R.affine_act(x, sc, sf, G, 1, res), K.b_affine_act(x, sc, sf, G, 1, res, dtype))


# ------------------------------------------------------------------ folds
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 72, 128, 520])
def test_folds(dtype, C, tail):
    """affine_act_bn and bn_bwd_apply_fin over nrep x groups: scale, shift, mean, invstd and the running statistics (updated
    for the groups in order), dgamma / dbeta (written or accumulated, scaled by param_scale), y and gx.  Statistics strided
    (ldc = C + 5) in every other case; the f64 and the f32 sums of bn_bwd_apply_fin alternate."""
    tail(KTRIP * 64)
    i = 0
    for nrep in NREPS:
        for G in (1, 2, 3):
            n = 37 * G
            K._affine_act_bn_case(dtype, C, "dense", n, G, nrep, i % 2 == 0, i % 3, i % 2 == 1, ("all", "all", "nogamma", "norunning")[i % 4],
                                  rng_for(C, i, 40), "affine_act_bn nrep=%d G=%d" % (nrep, G))
            K._bwd_fin_case(dtype, C, "dense", n, G, nrep, (i + 1) % 3, i % 2 == 0, 0.5, (i // 3) % 2 == 0, rng_for(C, i, 41),
                            "bn_bwd_apply_fin%s nrep=%d G=%d" % ("_d" if (i // 3) % 2 == 0 else "", nrep, G))
            K._bwd_fin_case(dtype, C, "dense", n, G, nrep, i % 3, i % 2 == 1, 1.0, (i // 3) % 2 == 1, rng_for(C, i, 42),
                            "bn_bwd_apply_fin%s nrep=%d G=%d" % ("_d" if (i // 3) % 2 == 1 else "", nrep, G))
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cf", [64, 96, 1024])
def test_stats_fix_fin_folds(dtype, Cf, tail):
    """The slice first, in the middle and last; groups 1 and 2 (and 3 once: the serial walk); every nrep; in place in every
    other case; pixel counts around one row of workgroups (32 channels: ty = 32 in f32, 64 in bf16)."""
    ty = K.plan(units(dtype, 32), 1 << 30, 1)[1]
    tail(KTRIP * 2 * ty)
    i = 0
    for cs in (0, (Cf // 64) * 32, Cf - 32):
        for G in (1, 2):
            nrep = NREPS[i % 5]
            npix_g = (1, ty - 1, ty + 1, 70, 37)[i % 5]
            stats_fix_fin_case(dtype, Cf, cs, npix_g * G, G, nrep, i % 2 == 1, 0.5 if i % 3 == 0 else 1.0, i % 2 == 0, rng_for(Cf, i, 43),
                               "stats_fix_fin cs=%d G=%d nrep=%d" % (cs, G, nrep))
            i += 1
    for nrep in NREPS:           # every nrep at two groups, and three groups once
        stats_fix_fin_case(dtype, Cf, Cf - 32, 2 * (ty + 1), 2, nrep, True, 1.0, True, rng_for(Cf, nrep, 44), "stats_fix_fin nrep=%d" % nrep)
    stats_fix_fin_case(dtype, Cf, 32, 3 * 37, 3, 32, False, 1.0, False, rng_for(Cf, 45), "stats_fix_fin G=3")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_fix_fin_ragged_trips_at_the_cap(dtype, tail):
    """32 dense channels, groups 2, at the cap of 2048 workgroups: 1 full trip + one full k + 3 pixels per group, in place."""
    G = 2
    tx, ty, gx, gy, _ = K.plan(units(dtype, 32), 1 << 30, G)
    per = gx * ty
    tail(KTRIP * per)
    stats_fix_fin_case(dtype, 32, 0, ragged(ty, gx)[4] * G, G, 3, False, 1.0, True, rng_for(46), "stats_fix_fin capped", lay="dense")
