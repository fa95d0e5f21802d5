"""The BatchNorm entry points of pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/bn_act.hip, one by one, against the float64 references of tests/rowops_ref.py.

Without a GPU: the references compose to nn.BatchNorm2d (+ activation) and to autograd's gradients, and the comparator
rejects a set of plausible wrong references at the very bounds the GPU tests use.  With a GPU (marker `gpu`): every entry
point is called through the C ABI on inputs rounded to the dtype under test, each stage on exact inputs, tensors as channel
slices of NaN-filled slabs, and compared with the reference within a bound derived from the operation's rounding model.

Branches (the case lists below reach each of them for every kernel that has it):
  scalar / vector units   C = 3, 5 scalar in both dtypes (tx = 3, 5: the magic division by a non power of two); C = 12 vector
                          in f32 and scalar in bf16; C = 8, 72, 520 vector; layouts `ldodd` and `misal` force the scalar kernel
  partial last unit group C = 72 scalar (72 units = 64 + 8), C = 520 (f32: 130 units = 64 + 64 + 2; bf16: 65 = 64 + 1)
  cb > 0                  C = 520 bf16 vector: block row 0 holds 512 channels, ncp = 256, two trips of the fold loop
  nrep > 1, groups > 1    NREPS, SHAPES
  strided statistics      stats_ld = C + 5 in every other case
  capped grid             test_*_capped_grid
"""
import ctypes
import math
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
CS = [3, 5, 8, 12, 72, 520]
SHAPES = [(2, 5, 7, 1), (2, 5, 7, 2), (4, 9, 13, 1), (4, 9, 13, 2), (4, 9, 13, 4)]    # (B, H, W, groups)
NREPS = [1, 3, 4, 32]
EPS, MOM = 1e-5, 0.1
EPS32 = float(np.float32(EPS))         # the kernels take eps as a float
MOM32 = float(np.float32(MOM))
F64EPS = 2.0 ** -40                    # f64 accumulation of at most 2^13 terms (2^-53 each): negligible, kept for honesty


def cases(C):
    """(layout, npix, groups, nrep, strided statistics?) — dense at every shape, the other layouts at two shapes each."""
    out, i = [], 0
    for li, lay in enumerate(("dense", "slab8", "ldodd", "misal")):
        shapes = SHAPES if lay == "dense" else [SHAPES[li % 5], SHAPES[(li + 3) % 5]]
        for (B, H, W, G) in shapes:
            out.append((lay, B * H * W, G, NREPS[i % 4], i % 2 == 1))
            i += 1
    return out


def vecn(dtype):
    return 4 if dtype == F32 else 8


def plan(units, npix_g, G, max_blocks=2048):
    """Mirror of plan() / row_geom() in pmt_learning_for_semantic_segmentation_and_disparity_amd/csrc/bn_act.hip, for the
    partial-sum lengths the bounds need:
    (tx, ty, grid x, grid y, pixel trips per thread)."""
    tx = min(units, 64)
    ty = 256 // tx
    gy = -(-units // tx)
    gx = max(1, min(-(-npix_g // ty), max(max_blocks // (gy * G), 1)))
    return tx, ty, gx, gy, -(-npix_g // (gx * ty))


def geom(dtype, C, npix, G, max_blocks, *rows):
    vec = all(r.vec(vecn(dtype)) for r in rows)
    return plan(C // vecn(dtype) if vec else C, npix // G, G, max_blocks)


def st(ref, dtype, e=0.0):
    """Rounding of the stored output: half an ulp of the bf16 value that is rounded, which lies within e (the error bound
    before the store) of ref — at a binade's edge that may be the larger half ulp.  An f32 store is part of the operation's own
    bound."""
    return R.half_ulp_bf16(np.abs(ref) + e) if dtype == BF16 else 0.0


def rng_for(*key):
    return np.random.default_rng([int(k) for k in key])


def make_x(rng, n, C, dtype):
    """N(0,1) rows with a per-channel gain in [0.5, 2] and offset in [-1, 1], rounded to dtype."""
    return quant(rng.standard_normal((n, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1, 1, C), dtype)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _coeffs(rng, G, C, identity=False):
    if identity:
        return None, None
    return f32(rng.uniform(0.5, 1.5, (G, C)) * rng.choice([-1, 1], (G, C))), f32(rng.uniform(-1, 1, (G, C)))


def draw(rng, n, C, G, dtype):
    """x, gy (rounded to dtype) and f32 (scale, shift) of one backward case, always drawn in this order."""
    x, gy = make_x(rng, n, C, dtype), quant(rng.standard_normal((n, C)), dtype)
    return (x, gy) + _coeffs(rng, G, C)


_ALIVE = []     # device copies made for one call: held until it has run (P() keeps only the address)


def dev(a, dt=np.float32):
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda())
    return _ALIVE[-1]


def run(name, *args):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())
    torch.cuda.synchronize()
    del _ALIVE[:]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def code(dtype):
    return 0 if dtype == F32 else 1


class Stats:
    """f64 statistics [nrep][G][2][ld] on the GPU; strided: the C logical columns sit at column 2 of rows of C + 5, the rest
    holds a sentinel that must survive."""

    def __init__(self, nrep, G, C, strided, vals=None, fill=float('nan')):
        self.ld, self.k = (C + 5, 2) if strided else (C, 0)
        self.C = C
        self.t = torch.full((nrep, G, 2, self.ld), fill, dtype=torch.float64, device="cuda")
        if strided:
            self.t[...] = -7.25
            self.t[..., self.k:self.k + C] = fill
        if vals is not None:
            self.t[..., self.k:self.k + C] = torch.from_numpy(np.asarray(vals, np.float64)).cuda()
        self.before = self.t.clone()

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr() + 8 * self.k)

    def np(self):
        return self.t[..., self.k:self.k + self.C].cpu().numpy()

    def pads_intact(self):
        a, b = self.t.clone(), self.before.clone()
        a[..., self.k:self.k + self.C] = 0
        b[..., self.k:self.k + self.C] = 0
        return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


# =========================================================================== bounds (numpy; used on the CPU and on the GPU)
def b_stats(x, G, n_t):
    """channel_stats: every thread adds n_t values (and n_t fused x*x + acc) in f32, each step rounding a partial sum that is
    at most sum |terms| -> n_t u sum|terms| (+ u for the f32 -> f64 hand-over being exact: nothing); rows, workgroups and
    replicas are then added in f64."""
    xa = R._grp(np.abs(x), G)
    return np.stack([xa.sum(1), (xa * xa).sum(1)], 1) * (n_t * U32 + F64EPS)


def b_finalize(S, count, gamma, beta, rm0=None, rv0=None, G_order=True):
    """bn_finalize and its fused forms compute mean, var, invstd in f64 and round once to f32:
      mean    u |mean|
      invstd  u invstd + invstd^3 / 2 * e_var, e_var = 8 * 2^-53 (S2/n + mean^2): the f64 cancellation of S2/n - mean^2, which
              the kernel and this reference both carry
      scale   = fl32(gamma * invstd): |gamma| e_invstd + u |scale|
      shift   = fl32(beta - mean * scale) with the ROUNDED scale: u |shift| + |mean| e_scale
      running r <- fl((1 - m) r) + fl(m * fl(stat)) per group, f32: each group adds 4 u (|r| + m |stat|) + m e_stat;
              stat = mean, or the unbiased variance (e_var n/(n-1) + u var_unb)."""
    S = np.asarray(S, np.float64)
    G, _, C = S.shape
    gamma = np.ones(C) if gamma is None else gamma
    beta = np.zeros(C) if beta is None else beta
    ref = R.bn_finalize(S, count, gamma, beta, eps=EPS32)
    mu, inv = ref["mean"], ref["invstd"]
    e_var = 8 * 2.0 ** -53 * (S[:, 1] / count + mu * mu)
    e_inv = U32 * inv + 0.5 * inv ** 3 * e_var
    e_sc = np.abs(gamma)[None] * e_inv + U32 * np.abs(ref["scale"])
    e_sh = U32 * np.abs(ref["shift"]) + np.abs(mu) * e_sc + F64EPS * (np.abs(beta)[None] + np.abs(mu * ref["scale"]))
    out = dict(mean=U32 * np.abs(mu) + 1e-300, invstd=e_inv, scale=e_sc + 1e-300, shift=e_sh + 1e-300)
    if rm0 is not None:
        unb = ref["var"] * (count / (count - 1.0) if count > 1 else 1.0)
        e_unb = e_var * (count / (count - 1.0) if count > 1 else 1.0) + U32 * unb
        em, ev, mm, mv = 0.0, 0.0, np.abs(rm0), np.abs(rv0)
        for g in range(G):
            em = em + 4 * U32 * (mm + MOM * np.abs(mu[g])) + MOM * U32 * np.abs(mu[g])
            ev = ev + 4 * U32 * (mv + MOM * unb[g]) + MOM * e_unb[g]
            mm, mv = mm + MOM * np.abs(mu[g]), mv + MOM * unb[g]
        out.update(rmean=em + 1e-300, rvar=ev + 1e-300)
    return out


def sig_err(z, dz):
    """sigmoid as 1 / (1 + __expf(-z)) in f32 with z off by dz: e = exp(-z) carries the intrinsic's documented error, taken
    as (2 + 1.5 |z|) ulp = (4 + 3 |z|) u relative (exponent product rounded once, hardware exp2 to 1 ulp), plus dz relative
    from the argument; ds/de = -s^2, s^2 e = s (1 - s); the add and the division round once each, a divide built on a
    reciprocal a little more: 6 u s."""
    s = R.sigmoid(z)
    return s * (1 - s) * ((4 + 3 * np.abs(z)) * U32 + dz) + 6 * U32 * s


def b_affine_act(x, scale, shift, G, act, res, dtype, e_sc=0.0, e_sh=0.0):
    """y = act(fma(x, scale, shift)) (+ res): the fma rounds once, u (|x scale| + |shift|); coefficient errors enter as
    |x| e_scale + e_shift; ReLU is exact and 1-Lipschitz; sigmoid: sig_err; the residual add rounds once more."""
    z, sc = R.pre_act(x, scale, shift, G)
    n, C = z.shape
    dz = U32 * (np.abs(x * sc) + np.abs(z - x * sc))
    if np.ndim(e_sc):
        dz = dz + np.abs(x) * R._coef(e_sc, G, n, C) + R._coef(e_sh, G, n, C)
    y = R.act_fwd(z, act)
    e = sig_err(z, dz) if act == 2 else dz
    if res is not None:
        e = e + U32 * (np.abs(y) + np.abs(res))
        y = y + res
    return e + st(y, dtype, e) + 1e-300


def relu_keep(z, act, rel=1e-5):
    """ReLU masks flip when z rounds across zero: elements with |z| < rel * max|z| leave the elementwise comparison (their
    share is asserted < 0.5 %) and enter the bounds of the reductions as terms that may be present or absent."""
    if act != 1:
        return np.ones(z.shape, bool)
    keep = np.abs(z) >= rel * np.abs(z).max()
    assert 1.0 - keep.mean() <= 0.005, 1.0 - keep.mean()
    return keep


def gm_err(gy, x, scale, shift, G, act):
    """gm = gy * act'(z), z = fma(x, scale, shift): (gm, its error bound, z, scale rows).  act' is exact for act 0 and 1 (off
    the excluded band); act 2: |d(s (1 - s))| <= |1 - 2 s| e_s + 3 u s (1 - s) <= e_s + 3 u s (1 - s); act 4 (z is the
    output): |1 - 2 z| dz + 3 u |z (1 - z)|; the product with gy rounds once."""
    z, sc = R.pre_act(x, scale, shift, G)
    dz = U32 * (np.abs(x * sc) + np.abs(z - x * sc))
    a = R.act_grad(z, act)
    if act == 2:
        da = sig_err(z, dz) + 3 * U32 * a
    elif act == 4:
        da = np.abs(1 - 2 * z) * dz + 3 * U32 * np.abs(a)
    else:
        da = np.zeros_like(z)
    gm = gy * a
    return gm, np.abs(gy) * da + U32 * np.abs(gm), z, sc


def b_act_bwd(gy, x, scale, shift, G, act, dtype, L, old=None):
    """affine_act_bwd.  gx = fl(gm * scale) (+ old, one more f32 add), stored in dtype.  dscale / dshift: f32 sums of L links
    (per-thread trips, then the ty rows of the workgroup, then the workgroups that share a replica by atomics), each link
    rounding a partial sum <= sum|terms|: (L + 1) u sum|terms| (+1: the product gm * x inside the fma chain); the error of gm
    itself adds sum e_gm |x|; an element inside the excluded ReLU band may flip: its whole term is added."""
    gm, e_gm, z, sc = gm_err(gy, x, scale, shift, G, act)
    keep = relu_keep(z, act)
    gx = gm * sc
    e_gx = np.abs(sc) * e_gm + U32 * np.abs(gx)
    if old is not None:
        e_gx = e_gx + U32 * (np.abs(old) + np.abs(gx))
        gx = gx + old
    flip = np.where(keep, 0.0, np.abs(gy))
    e_ds = R._grp((L + 1) * U32 * np.abs(gm * x) + e_gm * np.abs(x) + flip * np.abs(x), G).sum(1)
    e_dh = R._grp((L + 1) * U32 * np.abs(gm) + e_gm + flip, G).sum(1)
    return e_gx + st(gx, dtype, e_gx) + 1e-300, e_ds + 1e-300, e_dh + 1e-300, keep


def b_stats_fix(gin, x, dS, G, dtype, e_a=0.0, e_b=0.0, e_in=0.0):
    """gout = gin + fma(x, b2, a), a = fl32(dS0), b2 = fl32(2 dS1): u |a| + u |x b2| from the two casts, u (|x b2| + |a|) from
    the fma, u (|gin| + |x b2| + |a|) from the add -> 3 u (|gin| + |a| + |x b2|); errors of dS0 / dS1 enter as e_a + 2 |x| e_b,
    an error of gin as e_in."""
    n, C = x.shape
    a, b2 = R._coef(dS[:, 0], G, n, C), 2 * R._coef(dS[:, 1], G, n, C)
    e = 3 * U32 * (np.abs(gin) + np.abs(a) + np.abs(x * b2)) + e_in
    if np.ndim(e_a):
        e = e + R._coef(e_a, G, n, C) + 2 * np.abs(x) * R._coef(e_b, G, n, C)
    return e + st(gin + a + x * b2, dtype, e) + 1e-300


def b_bwd_apply(gy, x, scale, shift, dS, G, act, dtype, e_a=0.0, e_b=0.0):
    """bn_bwd_apply = stats_fix of the gx that affine_act_bwd would have STORED: the kernels round the first term to dtype on
    purpose before the statistics path is added (Elem<T>::rnd in bn_bwd_apply_kernel and bn_bwd_apply_fin_kernel, whose comment
    reads "the first-phase result the one-pass form would have stored is rounded to T"), so that the one-pass and the two-pass
    backward give the same bits.  include/sdhip.h does not state this; the bound follows the kernel comment and holds, in bf16,
    half an ulp of gy act' scale for that store besides the half ulp of the final gx.  In f32 the term is nothing."""
    gm, e_gm, z, sc = gm_err(gy, x, scale, shift, G, act)
    keep = relu_keep(z, act)
    g1 = gm * sc
    e1 = np.abs(sc) * e_gm + U32 * np.abs(g1)
    return b_stats_fix(g1, x, dS, G, dtype, e_a, e_b, e1 + st(g1, dtype, e1)), keep


def b_finalize_bwd(ds_rep, dh_rep, gamma, mean, invstd, count):
    """bn_finalize_bwd and its fused forms: ds, dh = f32 sums of nrep replicas (any order: < nrep u sum|replica|);
    t = fl(ds - fl(mean dh)): e_t = e_ds + |mean| e_dh + 2 u (|ds| + |mean dh|) — an absolute bound, t may cancel;
    dgamma = sum_g fl(invstd t): invstd e_t + 2 u |invstd t| per group; dbeta = sum_g dh: e_dh + u |dh| per group;
    dS in f64 from the f32 t, dh: dvar = -gamma t invstd^3 / 2n, dmean = -gamma invstd dh / n - 2 mean dvar."""
    nrep = ds_rep.shape[0]
    ds, dh = ds_rep.sum(0), dh_rep.sum(0)
    e_ds, e_dh = nrep * U32 * np.abs(ds_rep).sum(0), nrep * U32 * np.abs(dh_rep).sum(0)
    gam = np.ones(ds.shape[1]) if gamma is None else gamma
    e_t = e_ds + np.abs(mean) * e_dh + 2 * U32 * (np.abs(ds) + np.abs(mean * dh))
    t = ds - mean * dh
    e_dg = (invstd * e_t + 2 * U32 * np.abs(invstd * t)).sum(0) + U32 * np.abs(invstd * t).sum(0)
    e_db = (e_dh + U32 * np.abs(dh)).sum(0)
    e_dvar = 0.5 * np.abs(gam)[None] * invstd ** 3 * e_t / count
    e_dmu = np.abs(gam)[None] * invstd * e_dh / count + 2 * np.abs(mean) * e_dvar
    return e_dg + 1e-300, e_db + 1e-300, e_dmu * (1 + F64EPS) + 1e-300, e_dvar * (1 + F64EPS) + 1e-300


# =========================================================================== CPU: the references are the torch operations
COMPOSE = [(2, 3, 5, 7, 1, 1), (4, 5, 9, 13, 2, 0), (4, 12, 4, 6, 4, 2), (6, 8, 3, 5, 3, 1), (2, 72, 2, 3, 1, 2)]   # B C H W G act


def _rows(t):      # NCHW torch f64 -> [npix][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _tact(z, act):
    return z if act == 0 else torch.relu(z) if act == 1 else torch.sigmoid(z)


@pytest.mark.parametrize("B,C,H,W,G,act", COMPOSE)
def test_references_compose_to_batch_norm(B, C, H, W, G, act):
    """stats -> finalize -> affine_act is F.batch_norm(training=True) + activation per sub-batch, in f64; the running
    statistics are those of nn.BatchNorm2d fed the sub-batches in order, after one and after two steps."""
    torch.manual_seed(B * 100 + C)
    x = torch.randn(B, C, H, W, dtype=torch.float64) * 1.5 + 0.3
    gamma, beta = torch.rand(C, dtype=torch.float64) + 0.5, torch.randn(C, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double().train()
    bn.weight.data.copy_(gamma); bn.bias.data.copy_(beta)
    rm, rv = np.zeros(C), np.ones(C)
    per = B // G
    count = per * H * W
    for step in range(2):
        xs = x * (1 + step)
        want = torch.cat([_tact(bn(xs[g * per:(g + 1) * per]), act) for g in range(G)])
        want_fn = torch.cat([_tact(F.batch_norm(xs[g * per:(g + 1) * per], None, None, gamma, beta, True, MOM, EPS), act) for g in range(G)])
        S = R.channel_stats(_rows(xs), G)
        fin = R.bn_finalize(S, count, gamma.numpy(), beta.numpy(), rm, rv, EPS, MOM)
        y = R.affine_act(_rows(xs), fin["scale"], fin["shift"], G, act)
        rm, rv = fin["rmean"], fin["rvar"]
        assert np.allclose(y, _rows(want.detach()), rtol=1e-11, atol=1e-11)
        assert np.allclose(y, _rows(want_fn), rtol=1e-11, atol=1e-11)
        assert np.allclose(rm, bn.running_mean.numpy(), rtol=1e-12, atol=1e-13), step
        assert np.allclose(rv, bn.running_var.numpy(), rtol=1e-12, atol=1e-13), step
    ev = R.bn_finalize_eval(G, gamma.numpy(), beta.numpy(), rm, rv, EPS)
    want = _tact(bn.eval()(x), act)
    assert np.allclose(R.affine_act(_rows(x), ev["scale"], ev["shift"], G, act), _rows(want.detach()), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("B,C,H,W,G,act", COMPOSE)
def test_references_compose_to_autograd(B, C, H, W, G, act):
    """reductions -> finalize_bwd -> bn_bwd_apply gives autograd's x.grad / weight.grad / bias.grad of the per-sub-batch
    BatchNorm (+ activation); so does the stats_fix form (affine_act_bwd with gx, then stats_fix); act 4 = act 2 given y."""
    torch.manual_seed(B * 100 + C + 1)
    x = (torch.randn(B, C, H, W, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(B, C, H, W, dtype=torch.float64)
    per = B // G
    count = per * H * W
    y = torch.cat([_tact(F.batch_norm(x[g * per:(g + 1) * per], None, None, gamma, beta, True, MOM, EPS), act) for g in range(G)])
    y.backward(gy)
    xr, gr = _rows(x.detach()), _rows(gy)
    fin = R.bn_finalize(R.channel_stats(xr, G), count, gamma.detach().numpy(), beta.detach().numpy(), eps=EPS)
    gx1, ds, dh = R.affine_act_bwd(gr, xr, fin["scale"], fin["shift"], G, act)
    dgamma, dbeta, dS = R.bn_finalize_bwd(ds, dh, gamma.detach().numpy(), fin["mean"], fin["invstd"], count)
    for gx in (R.bn_bwd_apply(gr, xr, fin["scale"], fin["shift"], dS, G, act), R.stats_fix(gx1, xr, dS, G)):
        assert np.allclose(gx, _rows(x.grad), rtol=1e-9, atol=1e-11)
    assert np.allclose(dgamma, gamma.grad.numpy(), rtol=1e-9, atol=1e-11)
    assert np.allclose(dbeta, beta.grad.numpy(), rtol=1e-9, atol=1e-11)
    if act == 2:
        yr = R.affine_act(xr, fin["scale"], fin["shift"], G, 2)
        gx4, _, _ = R.affine_act_bwd(gr, yr, None, None, G, 4)
        gx2, _, _ = R.affine_act_bwd(gr, xr * R._coef(fin["scale"], G, *xr.shape) + R._coef(fin["shift"], G, *xr.shape), None, None, G, 2)
        assert np.allclose(gx4, gx2, rtol=1e-12, atol=1e-14)
    # eval mode: the statistics are constants
    dg0, db0, dS0 = R.bn_finalize_bwd(ds, dh, gamma.detach().numpy(), fin["mean"], fin["invstd"], count, train=False)
    assert not dS0.any() and np.array_equal(dg0, dgamma) and np.array_equal(db0, dbeta)


def _synthetic_stats(rng, G, C, count):
    """f64 (sum, sum of squares) of plausible channels; channel 0 is constant (variance exactly at the clamp)."""
    mean, var = rng.uniform(-2, 2, (G, C)), rng.uniform(0.2, 3, (G, C))
    mean[:, 0], var[:, 0] = 3.0, 0.0
    return np.stack([mean * count, (var + mean * mean) * count], 1)


def test_comparator_rejects_wrong_batchnorm_references():
    """Each plausible mistake, played as a wrong reference against the right one, must exceed the bound the GPU test of that
    quantity uses — and the right one must pass at ratio 0."""
    rng = np.random.default_rng(7)
    G, C, n = 2, 12, 140
    count = n // G
    x = make_x(rng, n, C, BF16)
    gy = quant(rng.standard_normal((n, C)), BF16)
    gamma, beta = f32(rng.uniform(0.5, 1.5, C)).astype(np.float64), f32(rng.standard_normal(C)).astype(np.float64)
    S = R.channel_stats(x, G)
    rm0, rv0 = np.zeros(C), np.ones(C)
    fin = R.bn_finalize(S, count, gamma, beta, rm0, rv0, EPS32, MOM32)
    bf = b_finalize(S, count, gamma, beta, rm0, rv0)
    assert R.worst_ratio(fin["rvar"], fin["rvar"], bf["rvar"]) == 0.0
    # biased instead of unbiased running_var
    rv = rv0.copy()
    for g in range(G):
        rv = (1 - MOM32) * rv + MOM32 * fin["var"][g]
    assert R.worst_ratio(rv, fin["rvar"], bf["rvar"]) > 1
    # groups pooled into one
    pooled = R.bn_finalize(S.sum(0, keepdims=True), n, gamma, beta, rm0, rv0, EPS32, MOM32)
    for k in ("scale", "shift", "mean", "invstd"):
        assert R.worst_ratio(np.repeat(pooled[k], G, 0), fin[k], bf[k]) > 1, k
    assert R.worst_ratio(pooled["rmean"], fin["rmean"], bf["rmean"]) > 1
    # running statistics updated once instead of once per group
    once = R.bn_finalize(S[:1], count, gamma, beta, rm0, rv0, EPS32, MOM32)
    assert R.worst_ratio(once["rmean"], fin["rmean"], bf["rmean"]) > 1 and R.worst_ratio(once["rvar"], fin["rvar"], bf["rvar"]) > 1
    # only replica 0 summed: the statistics of the rows that replica 0 received (every third workgroup's)
    part = R.channel_stats(np.where((np.arange(n) % 3 == 0)[:, None], x, 0.0), G)
    assert R.worst_ratio(part, S, b_stats(x, G, 4)) > 1
    # dS[.][1] applied without the factor 2
    sc, sf = f32(fin["scale"]).astype(np.float64), f32(fin["shift"]).astype(np.float64)
    for dtype in (F32, BF16):
        _, ds, dh = R.affine_act_bwd(gy, x, sc, sf, G, 1)
        _, _, dS = R.bn_finalize_bwd(ds, dh, gamma, fin["mean"], fin["invstd"], count)
        assert R.worst_ratio(R.stats_fix(gy, x, dS, G, factor=1.0), R.stats_fix(gy, x, dS, G), b_stats_fix(gy, x, dS, G, dtype)) > 1
        # sigmoid' taken at the output for act = 2
        good = R.affine_act_bwd(gy, x, sc, sf, G, 2)
        bad = R.affine_act_bwd(gy, x, sc, sf, G, 2, at_output=True)
        e_gx, e_ds, e_dh, keep = b_act_bwd(gy, x, sc, sf, G, 2, dtype, L=40)
        assert R.worst_ratio(bad[0], good[0], e_gx, keep) > 1 and R.worst_ratio(bad[1], good[1], e_ds) > 1
        assert R.worst_ratio(bad[2], good[2], e_dh) > 1
        assert R.worst_ratio(good[0], good[0], e_gx, keep) == 0.0
    # a got that is not finite, or off where the bound is tight, is rejected whatever the rest looks like
    bad = fin["scale"].copy(); bad[0, 3] = np.nan
    assert R.worst_ratio(bad, fin["scale"], bf["scale"]) == np.inf


def test_relu_band_is_small_for_the_seeds_in_use():
    """The share of elements inside the excluded ReLU band (|z| < 1e-5 max|z|) stays far below the 0.5 % cap for the very
    data every ReLU case of the GPU tests draws (relu_keep asserts the cap itself on every case as well)."""
    worst = 0.0
    for dtype in (F32, BF16):
        for C in CS:
            for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
                zs = []
                if ci % 4 == 1:                                                     # test_affine_act_bwd
                    zs.append(draw(rng_for(C, ci, 8), n, C, G, dtype))
                if ci % 3 == 1:                                                     # test_stats_fix_and_bn_bwd_apply, test_bn_bwd_apply_fin
                    zs.append(draw(rng_for(C, ci, 9), n, C, G, dtype))
                    rng = rng_for(C, ci, 12)
                    _bwd_inputs(rng, G, C, nrep, n)
                    zs.append(draw(rng, n, C, G, dtype))
                for x, _, sc, sf in zs:
                    z, _ = R.pre_act(x, sc, sf, G)
                    worst = max(worst, 1.0 - float(relu_keep(z, 1).mean()))
        # test_elementwise_capped_grid (affine_act_bwd and bn_bwd_apply with ReLU on its second data set)
        _, _, _, sc, sf, _, _, x2, _ = _elementwise_capped_data(dtype)
        worst = max(worst, 1.0 - float(relu_keep(R.pre_act(x2, sc, sf, 1)[0], 1).mean()))
        # test_fused_kernels_capped_grid: its ReLU backward case (seed 14; seed 15 is a sigmoid)
        for C in (12, 520):
            rng = rng_for(C, 14)
            _bwd_inputs(rng, 1, C, 3, 468)
            x, _, sc, sf = draw(rng, 468, C, 1, dtype)
            worst = max(worst, 1.0 - float(relu_keep(R.pre_act(x, sc, sf, 1)[0], 1).mean()))
        # the chain: coefficients derived from the data, band 1e-4 max|z|
        x, _, gamma, beta = _chain_data(dtype)
        G = CHAIN[4]
        fin = R.bn_finalize(R.channel_stats(x, G), x.shape[0] // G, gamma.astype(np.float64), beta.astype(np.float64), eps=EPS32)
        worst = max(worst, 1.0 - float(relu_keep(R.pre_act(x, fin["scale"], fin["shift"], G)[0], 1, 1e-4).mean()))
    assert worst <= 0.005, worst


# =========================================================================== GPU
def _finite_and_intact(*outs):
    for o in outs:
        if isinstance(o, (Rows, Stats)):
            assert o.pads_intact(), "a pad element changed"
        if isinstance(o, Rows):
            assert np.isfinite(o.np()).all(), "a logical output element is not finite"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_channel_stats(dtype, C):
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        rng = rng_for(C, ci, 2)
        x = make_x(rng, n, C, dtype)
        if C >= 5:
            x[:, 1] = quant(50.0 + 0.5 * rng.standard_normal(n), dtype)     # large mean: the sums themselves are compared
            x[:, 2] = quant(np.full(n, 1.7), dtype)                          # constant channel
        xd = Rows(n, C, dtype, lay, x)
        _, ty, gx, _, n_t = geom(dtype, C, n, G, 1024, xd)
        S = Stats(nrep, G, C, strided)                                       # NaN: zero_first must clear exactly the C columns
        run("sdhip_channel_stats", xd.p, xd.ld, S.p, S.ld, nrep, n, C, G, 1, code(dtype))
        ref, bound = R.channel_stats(x, G), b_stats(x, G, n_t)
        _finite_and_intact(xd, S)
        check("channel_stats", S.np().sum(0), ref, bound)
        if nrep > 1 and gx > 1:
            assert np.count_nonzero(np.abs(S.np()[:, 0, 1]).sum(-1)) == min(nrep, gx), "replica = workgroup % nrep"
        # zero_first = 0 accumulates onto what is there
        base = rng.standard_normal((nrep, G, 2, C)) * 10
        S2 = Stats(nrep, G, C, strided, base)
        run("sdhip_channel_stats", xd.p, xd.ld, S2.p, S2.ld, nrep, n, C, G, 0, code(dtype))
        _finite_and_intact(S2)
        check("channel_stats accumulate", S2.np().sum(0), ref + base.sum(0), bound + F64EPS * np.abs(base).sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_stats_capped_grid(dtype):
    """C = 520, groups 1, cap 1024 workgroups: bf16 65 units -> tx 64, ty 4, 2 block rows -> 512 x 4 = 2048 pixels per trip;
    f32 130 units -> 3 block rows -> 341 x 4 = 1364 per trip.  2 trips + 5 pixels: a third, ragged trip."""
    C = 520
    n = 2 * (2048 if dtype == BF16 else 1364) + 5
    rng = rng_for(C, 3)
    x = make_x(rng, n, C, dtype)
    xd = Rows(n, C, dtype, "dense", x)
    _, ty, gx, gy, n_t = geom(dtype, C, n, 1, 1024, xd)
    assert n_t == 3 and gx * gy <= 1024 and n % (gx * ty) == 5
    S = Stats(3, 1, C, False)
    run("sdhip_channel_stats", xd.p, xd.ld, S.p, S.ld, 3, n, C, 1, 1, code(dtype))
    check("channel_stats capped", S.np().sum(0), R.channel_stats(x, 1), b_stats(x, 1, n_t))


def _fin_inputs(rng, G, C, nrep, count):
    S = _synthetic_stats(rng, G, C, count)
    w = rng.dirichlet(np.ones(nrep), (G, 2, C)).transpose(3, 0, 1, 2)        # the sums spread over the replicas
    gamma, beta = f32(rng.uniform(0.5, 1.5, C)), f32(rng.standard_normal(C))
    rm0, rv0 = f32(rng.standard_normal(C)), f32(rng.uniform(0.5, 2, C))
    return S[None] * w, gamma, beta, rm0, rv0


def _check_fin(label, got, S, count, gamma, beta, rm0, rv0, running=True):
    """got: dict of numpy outputs; S the f64 statistics the kernel read (replicas summed)."""
    g64 = lambda v: None if v is None else np.asarray(v, np.float64)
    ref = R.bn_finalize(S, count, g64(gamma), g64(beta), g64(rm0) if running else None, g64(rv0) if running else None, EPS32, MOM32)
    bnd = b_finalize(S, count, g64(gamma), g64(beta), g64(rm0) if running else None, g64(rv0) if running else None)
    for k in ("scale", "shift", "mean", "invstd") + (("rmean", "rvar") if running else ()):
        check("%s %s" % (label, k), got[k], ref[k], bnd[k])
    assert (ref["var"][:, 0] < 1e-12).all() and np.allclose(got["invstd"][:, 0], 1 / math.sqrt(EPS32), rtol=2 * U32), \
        "variance clamp of the constant channel"
    return ref, bnd


@pytest.mark.gpu
@pytest.mark.parametrize("C", CS)
def test_bn_finalize_and_replica_sum(C):
    for ci, (G, nrep, strided, count, opt) in enumerate([(1, 1, False, 70.0, "all"), (2, 3, True, 35.0, "all"), (4, 32, True, 117.0, "nogamma"),
                                                          (2, 4, False, 1.0, "norunning"), (1, 32, True, 1000.0, "all")]):
        rng = rng_for(C, ci, 4)
        Srep, gamma, beta, rm0, rv0 = _fin_inputs(rng, G, C, nrep, count)
        if count == 1.0:          # one sample: S2 = S1^2, the biased variance is 0 and the unbiased one is not formed
            Srep[:, :, 1] = 0
            Srep[0, :, 1] = Srep.sum(0)[:, 0] ** 2
        S = Stats(nrep, G, C, strided, Srep)
        Sref = S.np().sum(0)
        if opt == "nogamma":
            gamma = beta = None
        running = opt != "norunning"
        o = {k: torch.full((G, C), float('nan'), device="cuda") for k in ("scale", "shift", "mean", "invstd")}
        rm, rv = (dev(rm0), dev(rv0)) if running else (None, None)
        run("sdhip_bn_finalize", S.p, S.ld, nrep, P(dev(gamma)) if gamma is not None else None, P(dev(beta)) if beta is not None else None,
            P(rm), P(rv), P(o["scale"]), P(o["shift"]), P(o["mean"]), P(o["invstd"]), C, G, count, EPS, MOM)
        got = {k: v.double().cpu().numpy() for k, v in o.items()}
        if running:
            got.update(rmean=rm.double().cpu().numpy(), rvar=rv.double().cpu().numpy())
        assert all(np.isfinite(v).all() for v in got.values()) and S.pads_intact()
        _check_fin("bn_finalize", got, Sref, count, gamma, beta, rm0, rv0, running)
        # stats_replica_sum: out += the replicas, f64 (nrep adds of 2^-53 each)
        base = rng.standard_normal((G, 2, C))
        out = Stats(1, G, C, not strided, base[None])
        run("sdhip_stats_replica_sum", S.p, out.p, nrep, G, C, S.ld, out.ld)
        assert out.pads_intact()
        check("stats_replica_sum", out.np()[0], base + Sref, (nrep + 1) * 2.0 ** -53 * (np.abs(Srep).sum(0) + np.abs(base)) + 1e-300)
        # eval mode: scale / shift from the running statistics (f32: 1/sqrtf and two products, 4 u each side of the subtraction)
        if running:
            e = {k: torch.full((G, C), float('nan'), device="cuda") for k in ("scale", "shift", "mean", "invstd")}
            run("sdhip_bn_finalize", None, 0, 1, P(dev(gamma)) if gamma is not None else None, P(dev(beta)) if beta is not None else None,
                P(dev(rm0)), P(dev(rv0)), P(e["scale"]), P(e["shift"]), P(e["mean"]), P(e["invstd"]), C, G, count, EPS, MOM)
            g64 = lambda v: None if v is None else np.asarray(v, np.float64)
            ev = R.bn_finalize_eval(G, g64(gamma), g64(beta), g64(rm0), g64(rv0), EPS32)
            b = 0.0 if beta is None else np.abs(g64(beta))[None]
            for k, bound in (("invstd", 3 * U32 * ev["invstd"]), ("scale", 4 * U32 * np.abs(ev["scale"])), ("mean", 1e-300),
                             ("shift", 6 * U32 * (b + np.abs(ev["mean"] * ev["scale"])) + 1e-300)):
                check("bn_finalize eval %s" % k, e[k].double().cpu().numpy(), ev[k], bound)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,c_new0,C,ldc", [(32, 64, 96, 128), (32, 64, 128, 131), (8, 3, 20, 25), (5, 0, 5, 5)])
def test_bn_fold_finalize(Cn, c_new0, C, ldc):
    """The fold touches S only in [c_new0, c_new0 + Cn); C > c_new0 + Cn finalizes channels beyond the fresh ones from S as is."""
    for ci, (G, nrep, count) in enumerate([(1, 3, 70.0), (2, 32, 35.0), (4, 1, 117.0)]):
        rng = rng_for(Cn, C, ci, 5)
        S0 = np.zeros((G, 2, ldc))
        S0[:, :, :C] = _synthetic_stats(rng, G, C, count)
        S0[:, :, C:] = -7.25
        fresh = S0[:, :, c_new0:c_new0 + Cn].copy()
        S0[:, :, c_new0:c_new0 + Cn] = fresh * 0.25                             # a quarter is there, the rest in the replicas
        w = rng.dirichlet(np.ones(nrep), (G, 2, Cn)).transpose(3, 0, 1, 2)
        ws = Stats(nrep, G, Cn, True, 0.75 * fresh[None] * w)
        Sd = torch.from_numpy(S0).cuda()
        gamma, beta = f32(rng.uniform(0.5, 1.5, C)), f32(rng.standard_normal(C))
        rm0, rv0 = f32(rng.standard_normal(C)), f32(rng.uniform(0.5, 2, C))
        rm, rv = dev(rm0), dev(rv0)
        o = {k: torch.full((G, C), float('nan'), device="cuda") for k in ("scale", "shift", "mean", "invstd")}
        run("sdhip_bn_fold_finalize", ws.p, nrep, ws.ld, c_new0, Cn, P(Sd), ldc, P(dev(gamma)), P(dev(beta)), P(rm), P(rv),
            P(o["scale"]), P(o["shift"]), P(o["mean"]), P(o["invstd"]), C, G, count, EPS, MOM)
        Sref, _ = R.bn_fold_finalize(ws.np(), c_new0, S0, count, C)
        Sgot = Sd.cpu().numpy()
        keep = np.zeros(ldc, bool); keep[c_new0:c_new0 + Cn] = True
        assert np.array_equal(Sgot[:, :, ~keep], S0[:, :, ~keep]) and ws.pads_intact(), "S changed outside the fresh columns"
        check("bn_fold_finalize S", Sgot[:, :, keep], Sref[:, :, keep], (nrep + 1) * 2.0 ** -53 * np.abs(fresh) * 2 + 1e-300)
        got = {k: v.double().cpu().numpy() for k, v in o.items()}
        got.update(rmean=rm.double().cpu().numpy(), rvar=rv.double().cpu().numpy())
        _check_fin("bn_fold_finalize", got, Sgot[:, :, :C], count, gamma, beta, rm0, rv0)      # from the S it wrote


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_affine_act(dtype, C):
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        rng = rng_for(C, ci, 6)
        act, with_res, ident = ci % 3, ci % 2 == 0, ci % 5 == 4
        x = make_x(rng, n, C, dtype)
        sc, sf = _coeffs(rng, G, C, ident)
        res = quant(rng.standard_normal((n, C)), dtype) if with_res else None
        xd, yd = Rows(n, C, dtype, lay, x), Rows(n, C, dtype, lay)
        rd = Rows(n, C, dtype, lay, res) if with_res else None
        run("sdhip_affine_act", xd.p, xd.ld, yd.p, yd.ld, rd.p if rd else None, rd.ld if rd else 0,
            P(dev(sc)) if sc is not None else None, P(dev(sf)) if sf is not None else None, n, C, G, act, code(dtype))
        _finite_and_intact(xd, yd)
        check("affine_act act%d" % act, yd.np(), R.affine_act(x, sc, sf, G, act, res), b_affine_act(x, sc, sf, G, act, res, dtype))


def _capped_rows(dtype, per_trip_bf16, per_trip_f32, trips):
    return trips * (per_trip_bf16 if dtype == BF16 else per_trip_f32) + 5


def _elementwise_capped_data(dtype):
    """The two data sets of test_elementwise_capped_grid (the CPU test of the ReLU band draws them as well)."""
    C, G = 520, 1
    rng = rng_for(C, 7)
    n = _capped_rows(dtype, 4096, 2728, 2)
    x, gin = make_x(rng, n, C, dtype), quant(rng.standard_normal((n, C)), dtype)
    sc, sf = _coeffs(rng, G, C)
    dS = rng.standard_normal((G, 2, C)) * 0.1
    n2 = _capped_rows(dtype, 2048, 1364, 6)
    x2, gy = make_x(rng, n2, C, dtype), quant(rng.standard_normal((n2, C)), dtype)
    return n, x, gin, sc, sf, dS, n2, x2, gy


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise_capped_grid(dtype):
    """affine_act and stats_fix (cap 2048, one pixel per trip): C = 520, groups 1: bf16 2 block rows -> 1024 x 4 = 4096 pixels
    per trip, f32 3 block rows -> 682 x 4 = 2728; 2 trips + 5.  affine_act_bwd and bn_bwd_apply (cap 1024, 4 pixels per
    unrolled trip): 2048 / 1364 pixels per trip; 6 trips + 5 = one full unrolled trip, then one whose last slot is ragged."""
    C, G = 520, 1
    n, x, gin, sc, sf, dS, n2, x2, gy = _elementwise_capped_data(dtype)
    xd, gd, yd = Rows(n, C, dtype, "dense", x), Rows(n, C, dtype, "dense", gin), Rows(n, C, dtype)
    assert geom(dtype, C, n, G, 2048, xd)[4] == 3
    run("sdhip_affine_act", xd.p, C, yd.p, C, None, 0, P(dev(sc)), P(dev(sf)), n, C, G, 2, code(dtype))
    check("affine_act capped", yd.np(), R.affine_act(x, sc, sf, G, 2), b_affine_act(x, sc, sf, G, 2, None, dtype))
    yd = Rows(n, C, dtype)
    run("sdhip_stats_fix", gd.p, C, xd.p, C, yd.p, C, P(dev(dS, np.float64)), C, n, C, G, code(dtype))
    check("stats_fix capped", yd.np(), R.stats_fix(gin, x, dS, G), b_stats_fix(gin, x, dS, G, dtype))
    n, x = n2, x2
    xd, gd, yd = Rows(n, C, dtype, "dense", x), Rows(n, C, dtype, "dense", gy), Rows(n, C, dtype)
    _, ty, gx, _, n_t = geom(dtype, C, n, G, 1024, xd)
    assert n_t == 7
    nrep = 3
    ds, dh = torch.full((nrep, G, C), float('nan'), device="cuda"), torch.full((nrep, G, C), float('nan'), device="cuda")
    run("sdhip_affine_act_bwd", gd.p, C, xd.p, C, yd.p, C, P(dev(sc)), P(dev(sf)), P(ds), P(dh), nrep, n, C, G, 1, 0, 0, code(dtype))
    gxr, dsr, dhr = R.affine_act_bwd(gy, x, sc, sf, G, 1)
    e_gx, e_ds, e_dh, keep = b_act_bwd(gy, x, sc, sf, G, 1, dtype, n_t + ty + -(-gx // nrep))
    check("affine_act_bwd capped gx", yd.np(), gxr, e_gx, keep)
    check("affine_act_bwd capped dscale", ds.double().sum(0).cpu().numpy(), dsr, e_ds)
    check("affine_act_bwd capped dshift", dh.double().sum(0).cpu().numpy(), dhr, e_dh)
    yd = Rows(n, C, dtype)
    run("sdhip_bn_bwd_apply", gd.p, C, xd.p, C, yd.p, C, P(dev(sc)), P(dev(sf)), P(dev(dS, np.float64)), C, n, C, G, 1, code(dtype))
    bound, keep = b_bwd_apply(gy, x, sc, sf, dS, G, 1, dtype)
    check("bn_bwd_apply capped", yd.np(), R.bn_bwd_apply(gy, x, sc, sf, dS, G, 1), bound, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_affine_act_bwd(dtype, C):
    """acts 0, 1, 2, 4; gx NULL / written / accumulated; replicas zeroed by the call or by the caller; dscale / dshift NULL."""
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        rng = rng_for(C, ci, 8)
        act = (0, 1, 2, 4)[ci % 4]
        mode = ("gx+red", "red only", "accumulate", "gx only", "prezeroed")[ci % 5]
        x, gy, sc, sf = draw(rng, n, C, G, dtype)
        if act == 4:                       # x holds a sigmoid's output, the affine map is the identity
            x, sc, sf = quant(R.sigmoid(x), dtype), None, None
        old = quant(rng.standard_normal((n, C)), dtype)
        xd, gd = Rows(n, C, dtype, lay, x), Rows(n, C, dtype, lay, gy)
        want_gx, want_red = mode != "red only", mode != "gx only"
        gxd = Rows(n, C, dtype, lay, old if mode == "accumulate" else None) if want_gx else None
        # prezeroed = 1: the call must not clear the replicas, so what the caller left there (here: known non-zero values
        # instead of zeros) stays in the sums; otherwise NaN, which only a clear by the call removes
        base = f32(rng.standard_normal((2, nrep, G, C)) * 3).astype(np.float64) if mode == "prezeroed" else None
        ds = (dev(base[0]).clone() if base is not None else torch.full((nrep, G, C), float('nan'), device="cuda")) if want_red else None
        dh = (dev(base[1]).clone() if base is not None else torch.full((nrep, G, C), float('nan'), device="cuda")) if want_red else None
        run("sdhip_affine_act_bwd", gd.p, gd.ld, xd.p, xd.ld, gxd.p if gxd else None, gxd.ld if gxd else 0,
            P(dev(sc)) if sc is not None else None, P(dev(sf)) if sf is not None else None, P(ds), P(dh), nrep, n, C, G, act,
            int(mode == "accumulate"), int(mode == "prezeroed"), code(dtype))
        rows = [gd, xd] + ([gxd] if gxd else [])
        _, ty, gx, _, n_t = geom(dtype, C, n, G, 1024, *rows)
        gxr, dsr, dhr = R.affine_act_bwd(gy, x, sc, sf, G, act)
        L = n_t + ty + -(-gx // nrep)
        e_gx, e_ds, e_dh, keep = b_act_bwd(gy, x, sc, sf, G, act, dtype, L, old if mode == "accumulate" else None)
        if base is not None:           # the atomics of a replica add onto its old value: that many more roundings of a sum holding it
            dsr, dhr = dsr + base[0].sum(0), dhr + base[1].sum(0)
            e_ds, e_dh = e_ds + L * U32 * np.abs(base[0]).sum(0), e_dh + L * U32 * np.abs(base[1]).sum(0)
        _finite_and_intact(*rows)
        label = "affine_act_bwd act%d" % act
        if want_gx:
            check(label + " gx", gxd.np(), gxr + (old if mode == "accumulate" else 0), e_gx, keep)
        if want_red:
            assert bool(torch.isfinite(ds).all() and torch.isfinite(dh).all())
            check(label + " dscale", ds.double().sum(0).cpu().numpy(), dsr, e_ds)
            check(label + " dshift", dh.double().sum(0).cpu().numpy(), dhr, e_dh)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_stats_fix_and_bn_bwd_apply(dtype, C):
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        rng = rng_for(C, ci, 9)
        act = ci % 3
        x, gy, sc, sf = draw(rng, n, C, G, dtype)
        dSv = rng.standard_normal((G, 2, C)) * 0.1
        dS = Stats(1, G, C, strided, dSv[None])
        xd, gd = Rows(n, C, dtype, lay, x), Rows(n, C, dtype, lay, gy)
        o1, o2 = Rows(n, C, dtype, lay), Rows(n, C, dtype, lay)
        run("sdhip_stats_fix", gd.p, gd.ld, xd.p, xd.ld, o1.p, o1.ld, dS.p, dS.ld, n, C, G, code(dtype))
        run("sdhip_bn_bwd_apply", gd.p, gd.ld, xd.p, xd.ld, o2.p, o2.ld, P(dev(sc)), P(dev(sf)), dS.p, dS.ld, n, C, G, act, code(dtype))
        _finite_and_intact(xd, gd, o1, o2, dS)
        check("stats_fix", o1.np(), R.stats_fix(gy, x, dSv, G), b_stats_fix(gy, x, dSv, G, dtype))
        bound, keep = b_bwd_apply(gy, x, sc, sf, dSv, G, act, dtype)
        check("bn_bwd_apply act%d" % act, o2.np(), R.bn_bwd_apply(gy, x, sc, sf, dSv, G, act), bound, keep)


def _bwd_inputs(rng, G, C, nrep, n):
    """Replicated (dscale, dshift) of a plausible layer and its f32 side outputs."""
    count = n // G
    gamma = f32(rng.uniform(0.5, 1.5, C))
    mean, invstd = f32(rng.uniform(-1, 1, (G, C))), f32(rng.uniform(0.5, 2, (G, C)))
    w = rng.dirichlet(np.ones(nrep), (2, G, C)).transpose(3, 0, 1, 2)
    ds = f32(rng.standard_normal((G, C)) * math.sqrt(count) * w[:, 0])
    dh = f32(rng.standard_normal((G, C)) * math.sqrt(count) * w[:, 1])
    return count, gamma, mean, invstd, ds, dh


@pytest.mark.gpu
@pytest.mark.parametrize("C", CS)
def test_bn_finalize_bwd(C):
    """Both bits of accumulate_flags, train = 0, gamma NULL, strided dstats."""
    for ci, (G, nrep, flags, train, strided) in enumerate([(1, 1, 0, 1, False), (2, 3, 1, 1, True), (4, 32, 2, 1, True), (2, 4, 3, 1, False),
                                                           (2, 32, 0, 0, True), (1, 3, 1, 0, False)]):
        rng = rng_for(C, ci, 10)
        count, gamma, mean, invstd, ds, dh = _bwd_inputs(rng, G, C, nrep, 70 * G)
        if ci == 3:
            gamma = None
        dg0, db0, dS0 = f32(rng.standard_normal(C)), f32(rng.standard_normal(C)), rng.standard_normal((G, 2, C))
        dgd, dbd = dev(dg0), dev(db0)
        dS = Stats(1, G, C, strided, dS0[None] if flags & 1 else None)
        run("sdhip_bn_finalize_bwd", P(dev(ds)), P(dev(dh)), nrep, P(dev(gamma)) if gamma is not None else None, P(dev(mean)), P(dev(invstd)),
            P(dgd), P(dbd), dS.p, dS.ld, flags, C, G, float(count), train)
        g64 = lambda v: None if v is None else np.asarray(v, np.float64)
        dgr, dbr, dSr = R.bn_finalize_bwd(g64(ds).sum(0), g64(dh).sum(0), g64(gamma), g64(mean), g64(invstd), count, bool(train))
        e_dg, e_db, e_dmu, e_dvar = b_finalize_bwd(g64(ds), g64(dh), g64(gamma), g64(mean), g64(invstd), count)
        if flags & 2:      # one more f32 add onto the old value
            dgr, dbr = dgr + dg0, dbr + db0
            e_dg, e_db = e_dg + U32 * (np.abs(dg0) + np.abs(dgr)), e_db + U32 * (np.abs(db0) + np.abs(dbr))
        if flags & 1:
            dSr = dSr + dS0
        assert dS.pads_intact()
        check("bn_finalize_bwd dgamma", dgd.double().cpu().numpy(), dgr, e_dg)
        check("bn_finalize_bwd dbeta", dbd.double().cpu().numpy(), dbr, e_db)
        check("bn_finalize_bwd dstats", dS.np()[0], dSr, np.stack([e_dmu, e_dvar], 1) + F64EPS * np.abs(dSr))


def _affine_act_bn_case(dtype, C, lay, n, G, nrep, strided, act, with_res, opt, rng, label):
    count = float(n // G)
    x = make_x(rng, n, C, dtype)
    x[:, 0] = quant(np.full(n, 3.0), dtype)                  # constant channel: variance clamp inside the fused kernel
    res = quant(rng.standard_normal((n, C)), dtype) if with_res else None
    Sv = R.channel_stats(x, G)
    w = rng.dirichlet(np.ones(nrep), (G, 2, C)).transpose(3, 0, 1, 2)
    S = Stats(nrep, G, C, strided, Sv[None] * w)
    Sref = S.np().sum(0)
    gamma, beta = (None, None) if opt == "nogamma" else (f32(rng.uniform(0.5, 1.5, C)), f32(rng.standard_normal(C)))
    running = opt != "norunning"
    rm0, rv0 = f32(rng.standard_normal(C)), f32(rng.uniform(0.5, 2, C))
    rm, rv = (dev(rm0), dev(rv0)) if running else (None, None)
    o = {k: torch.full((G, C), float('nan'), device="cuda") for k in ("scale", "shift", "mean", "invstd")}
    xd, yd = Rows(n, C, dtype, lay, x), Rows(n, C, dtype, lay)
    rd = Rows(n, C, dtype, lay, res) if with_res else None
    run("sdhip_affine_act_bn", xd.p, xd.ld, yd.p, yd.ld, rd.p if rd else None, rd.ld if rd else 0, S.p, S.ld, nrep,
        P(dev(gamma)) if gamma is not None else None, P(dev(beta)) if beta is not None else None, P(rm), P(rv),
        P(o["scale"]), P(o["shift"]), P(o["mean"]), P(o["invstd"]), n, C, G, count, EPS, MOM, act, code(dtype))
    _finite_and_intact(xd, yd, S)
    got = {k: v.double().cpu().numpy() for k, v in o.items()}
    if running:
        got.update(rmean=rm.double().cpu().numpy(), rvar=rv.double().cpu().numpy())
    assert all(np.isfinite(v).all() for v in got.values())
    ref, bnd = _check_fin(label, got, Sref, count, gamma, beta, rm0, rv0, running)
    check(label + " y act%d" % act, yd.np(), R.affine_act(x, ref["scale"], ref["shift"], G, act, res),
          b_affine_act(x, ref["scale"], ref["shift"], G, act, res, dtype, bnd["scale"], bnd["shift"]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_affine_act_bn(dtype, C):
    """y, the four side outputs and the running statistics over the groups, from the same f64 statistics."""
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        opt = ("all", "nogamma", "norunning")[ci % 3]           # 11 cases: each option at least three times
        _affine_act_bn_case(dtype, C, lay, n, G, nrep, strided, ci % 3, ci % 2 == 0, opt, rng_for(C, ci, 11), "affine_act_bn")


def _bwd_fin_case(dtype, C, lay, n, G, nrep, act, acc, pscale, f64_sums, rng, label):
    count, gamma, mean, invstd, ds, dh = _bwd_inputs(rng, G, C, nrep, n)
    x, gy, sc, sf = draw(rng, n, C, G, dtype)
    dg0, db0 = f32(rng.standard_normal(C)), f32(rng.standard_normal(C))
    dgd, dbd = (dev(dg0), dev(db0)) if acc else (torch.full((C,), float('nan'), device="cuda"), torch.full((C,), float('nan'), device="cuda"))
    xd, gd, od = Rows(n, C, dtype, lay, x), Rows(n, C, dtype, lay, gy), Rows(n, C, dtype, lay)
    head = (gd.p, gd.ld, xd.p, xd.ld, od.p, od.ld, P(dev(sc)), P(dev(sf)))
    tail = (nrep, P(dev(gamma)), P(dev(mean)), P(dev(invstd)), P(dgd), P(dbd), int(acc), pscale, n, C, G, float(count), act, code(dtype))
    g64 = lambda v: np.asarray(v, np.float64)
    if f64_sums:       # [nrep][G][2][C] f64: the sums are added in f64 and rounded to f32 once (u each, inside e_ds / e_dh)
        sums = np.stack([rng.standard_normal((nrep, G, C)) * math.sqrt(count), rng.standard_normal((nrep, G, C)) * math.sqrt(count)], 2)
        run("sdhip_bn_bwd_apply_fin_d", *head, P(dev(sums, np.float64)), *tail)
        dsv, dhv = sums[:, :, 0], sums[:, :, 1]
    else:
        run("sdhip_bn_bwd_apply_fin", *head, P(dev(ds)), P(dev(dh)), *tail)
        dsv, dhv = g64(ds), g64(dh)
    dgr, dbr, dSr = R.bn_finalize_bwd(dsv.sum(0), dhv.sum(0), g64(gamma), g64(mean), g64(invstd), count)
    e_dg, e_db, e_dmu, e_dvar = b_finalize_bwd(dsv, dhv, g64(gamma), g64(mean), g64(invstd), count)
    p32 = float(np.float32(pscale))
    dgr, dbr, e_dg, e_db = dgr * p32, dbr * p32, e_dg * p32 + U32 * np.abs(dgr * p32), e_db * p32 + U32 * np.abs(dbr * p32)
    if acc:
        dgr, dbr = dgr + dg0, dbr + db0
        e_dg, e_db = e_dg + U32 * (np.abs(dg0) + np.abs(dgr)), e_db + U32 * (np.abs(db0) + np.abs(dbr))
    _finite_and_intact(xd, gd, od)
    check(label + " dgamma", dgd.double().cpu().numpy(), dgr, e_dg)      # NaN-prefilled unless accumulating: written exactly once
    check(label + " dbeta", dbd.double().cpu().numpy(), dbr, e_db)
    bound, keep = b_bwd_apply(gy, x, sc, sf, dSr, G, act, dtype, e_dmu, e_dvar)
    check(label + " gx act%d" % act, od.np(), R.bn_bwd_apply(gy, x, sc, sf, dSr, G, act), bound, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CS)
def test_bn_bwd_apply_fin(dtype, C):
    """bn_bwd_apply_fin and _fin_d equal the f64 composition finalize_bwd -> bn_bwd_apply; dgamma / dbeta are summed over the
    groups, scaled by param_scale and written (or added) exactly once."""
    for ci, (lay, n, G, nrep, strided) in enumerate(cases(C)):
        _bwd_fin_case(dtype, C, lay, n, G, nrep, ci % 3, ci % 2 == 1, 0.5 if ci % 3 == 0 else 1.0, strided, rng_for(C, ci, 12),
                      "bn_bwd_apply_fin_d" if strided else "bn_bwd_apply_fin")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_kernels_capped_grid(dtype):
    """SDHIP_TUNE_FUSED_BLOCKS = 1 leaves one workgroup per block row and group.  (4, 9, 13) pixels, groups 1, C = 12: f32
    3 vector units -> ty = 85, bf16 12 scalar units -> ty = 21: 468 pixels are 6 / 23 trips of the plain loop and 2 / 6 trips
    of the 4-pixel unrolled one, the last of them ragged (468 = 5 x 85 + 43 = 22 x 21 + 6).  C = 520 bf16 keeps cb > 0 in it."""
    with R.diag_switches(SDHIP_TUNE_FUSED_BLOCKS=1):
        for C in (12, 520):
            n, G = 468, 1
            assert geom(dtype, C, n, G, 1, Rows(n, C, dtype))[2] == 1
            _affine_act_bn_case(dtype, C, "dense", n, G, 3, True, 1, True, "all", rng_for(C, 13), "affine_act_bn capped")
            _bwd_fin_case(dtype, C, "dense", n, G, 3, 1, False, 1.0, False, rng_for(C, 14), "bn_bwd_apply_fin capped")
            _bwd_fin_case(dtype, C, "dense", n, G, 32, 2, True, 1.0, True, rng_for(C, 15), "bn_bwd_apply_fin_d capped")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cf,cs", [(32, 0), (96, 0), (96, 32), (96, 64), (200, 0), (200, 88), (200, 168)])
def test_stats_fix_fin(dtype, Cf, cs):
    """finalize_bwd of the Cf slab channels + stats_fix of the 32 channels [cs, cs + 32), which sit in a slab of pixel stride
    Cf + 8 at channel cs (16-byte aligned rows).  dS changes only outside the slice."""
    for ci, (n, G, nrep, acc, pscale) in enumerate([(70, 1, 1, False, 1.0), (70, 2, 3, True, 0.5), (468, 4, 32, False, 1.0), (468, 2, 4, True, 1.0)]):
        rng = rng_for(Cf, cs, ci, 16)
        count, gamma, mean, invstd, ds, dh = _bwd_inputs(rng, G, Cf, nrep, n)
        x, gin = make_x(rng, n, 32, dtype), quant(rng.standard_normal((n, 32)), dtype)
        ldc = Cf + 3
        dS0 = rng.standard_normal((G, 2, ldc)) * 0.05
        dSd = torch.from_numpy(dS0).cuda()
        dg0, db0 = f32(rng.standard_normal(Cf)), f32(rng.standard_normal(Cf))
        dgd, dbd = (dev(dg0), dev(db0)) if acc else (torch.full((Cf,), float('nan'), device="cuda"), torch.full((Cf,), float('nan'), device="cuda"))
        lay = (cs, Cf + 8)
        xd, gd, od = Rows(n, 32, dtype, lay, x), Rows(n, 32, dtype, lay, gin), Rows(n, 32, dtype, lay)
        run("sdhip_stats_fix_fin", gd.p, gd.ld, xd.p, xd.ld, od.p, od.ld, n, P(dSd), ldc, cs, P(dev(ds)), P(dev(dh)), nrep,
            P(dev(gamma)), P(dev(mean)), P(dev(invstd)), P(dgd), P(dbd), int(acc), pscale, Cf, G, float(count), code(dtype))
        g64 = lambda v: np.asarray(v, np.float64)
        dgr, dbr, dSr = R.bn_finalize_bwd(g64(ds).sum(0), g64(dh).sum(0), g64(gamma), g64(mean), g64(invstd), count)
        e_dg, e_db, e_dmu, e_dvar = b_finalize_bwd(g64(ds), g64(dh), g64(gamma), g64(mean), g64(invstd), count)
        p32 = float(np.float32(pscale))
        dgr, dbr, e_dg, e_db = dgr * p32, dbr * p32, e_dg * p32 + U32 * np.abs(dgr * p32), e_db * p32 + U32 * np.abs(dbr * p32)
        if acc:
            dgr, dbr = dgr + dg0, dbr + db0
            e_dg, e_db = e_dg + U32 * (np.abs(dg0) + np.abs(dgr)), e_db + U32 * (np.abs(db0) + np.abs(dbr))
        _finite_and_intact(xd, gd, od)
        check("stats_fix_fin dgamma", dgd.double().cpu().numpy(), dgr, e_dg)
        check("stats_fix_fin dbeta", dbd.double().cpu().numpy(), dbr, e_db)
        got = dSd.cpu().numpy()
        sl = np.zeros(ldc, bool); sl[cs:cs + 32] = True
        out = np.zeros(ldc, bool); out[:Cf] = True; out &= ~sl
        assert np.array_equal(got[:, :, sl], dS0[:, :, sl]) and np.array_equal(got[:, :, Cf:], dS0[:, :, Cf:]), "dS changed inside the slice or past Cf"
        full = dS0[:, :, :Cf] + dSr
        check("stats_fix_fin dS", got[:, :, out], full[:, :, out[:Cf]], (np.stack([e_dmu, e_dvar], 1) + F64EPS * np.abs(full))[:, :, out[:Cf]])
        dsl = full[:, :, cs:cs + 32]
        check("stats_fix_fin gout", od.np(), R.stats_fix(gin, x, dsl, G),
              b_stats_fix(gin, x, dsl, G, dtype, e_dmu[:, cs:cs + 32], e_dvar[:, cs:cs + 32]))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_fix_fin_capped_grid(dtype):
    """32 channels are 8 (f32) / 4 (bf16) vector units -> ty = 32 / 64 and a cap of 2048 workgroups: 65536 / 131072 pixels per
    trip; 2 trips + 5 pixels of 32 channels in a dense tensor (17 MB in either dtype)."""
    per = 65536 if dtype == F32 else 131072
    n, G, Cf, cs, nrep = 2 * per + 5, 1, 32, 0, 3
    rng = rng_for(17)
    count, gamma, mean, invstd, ds, dh = _bwd_inputs(rng, G, Cf, nrep, n)
    x, gin = make_x(rng, n, 32, dtype), quant(rng.standard_normal((n, 32)), dtype)
    dS0 = rng.standard_normal((G, 2, Cf)) * 0.05
    dSd = torch.from_numpy(dS0).cuda()
    dgd, dbd = torch.full((Cf,), float('nan'), device="cuda"), torch.full((Cf,), float('nan'), device="cuda")
    xd, gd, od = Rows(n, 32, dtype, "dense", x), Rows(n, 32, dtype, "dense", gin), Rows(n, 32, dtype)
    assert geom(dtype, 32, n, G, 2048, xd)[4] == 3
    run("sdhip_stats_fix_fin", gd.p, 32, xd.p, 32, od.p, 32, n, P(dSd), Cf, cs, P(dev(ds)), P(dev(dh)), nrep, P(dev(gamma)), P(dev(mean)),
        P(dev(invstd)), P(dgd), P(dbd), 0, 1.0, Cf, G, float(count), code(dtype))
    g64 = lambda v: np.asarray(v, np.float64)
    _, _, dSr = R.bn_finalize_bwd(g64(ds).sum(0), g64(dh).sum(0), g64(gamma), g64(mean), g64(invstd), count)
    _, _, e_dmu, e_dvar = b_finalize_bwd(g64(ds), g64(dh), g64(gamma), g64(mean), g64(invstd), count)
    assert np.array_equal(dSd.cpu().numpy(), dS0)
    check("stats_fix_fin capped gout", od.np(), R.stats_fix(gin, x, dS0 + dSr, G), b_stats_fix(gin, x, dS0 + dSr, G, dtype, e_dmu, e_dvar))


CHAIN = (4, 12, 9, 13, 2)      # B, C, H, W, groups


def _chain_data(dtype):
    B, C, H, W, G = CHAIN
    n = B * H * W
    rng = rng_for(18)
    x = quant(rng.standard_normal((n, C)) * rng.uniform(0.7, 1.5, C) + rng.uniform(-0.5, 0.5, C), dtype)
    gy = quant(rng.standard_normal((n, C)), dtype)
    return x, gy, f32(rng.uniform(0.5, 1.5, C)), f32(rng.uniform(-0.5, 0.5, C))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_short_chain_matches_the_torch_module(dtype):
    """channel_stats -> affine_act_bn -> (loss gradient) -> affine_act_bwd -> bn_bwd_apply_fin on well-conditioned data against
    nn.BatchNorm2d + ReLU in f64: the pieces fit together.  Every stage above is held to its own bound on exact inputs; here the
    errors compound, so the bound is the first-order propagation for THIS data (|x| < 6, invstd < 2.1, |gamma| <= 1.5, n = 234
    rows per group): the f32 coefficients carry ~4 u, z = x scale + shift 6 x 4 u + u (|z| + ...) < 40 u max|z|; in bf16 y adds
    its store (<= 2^-8 relative).  The gradient passes x (given exactly) and gy through two reductions of 234 terms whose errors
    (<= 300 u relative to sum|terms|, and one bf16 store each of gx's two phases) come back multiplied by
    |gamma| invstd (1 + |xhat|^2) / n-normalised terms < 12: 12 x 300 u in f32, 3 x 2^-8 + that in bf16, relative to the
    largest magnitude of the quantity.  ReLU band: 1e-4 max|z| (the coefficients are derived in the kernels)."""
    B, C, H, W, G = CHAIN
    n = B * H * W
    x, gy, gamma, beta = _chain_data(dtype)
    count = float(n // G)
    # torch, f64, one module call per sub-batch
    bn = torch.nn.BatchNorm2d(C, eps=EPS32, momentum=MOM32).double().train()
    bn.weight.data.copy_(torch.from_numpy(gamma)); bn.bias.data.copy_(torch.from_numpy(beta))
    xt = torch.from_numpy(x).reshape(B, H, W, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    zs = [bn(xt[g * 2:(g + 1) * 2]) for g in range(G)]
    yt = torch.relu(torch.cat(zs))
    yt.backward(torch.from_numpy(gy).reshape(B, H, W, C).permute(0, 3, 1, 2))
    z_ref = _rows(torch.cat(zs).detach())
    keep = relu_keep(z_ref, 1, 1e-4)
    # the kernels
    nrep = 4
    xd, gd, yd, gxd = Rows(n, C, dtype, "slab8", x), Rows(n, C, dtype, "slab8", gy), Rows(n, C, dtype, "slab8"), Rows(n, C, dtype, "slab8")
    S = Stats(nrep, G, C, False)
    run("sdhip_channel_stats", xd.p, xd.ld, S.p, S.ld, nrep, n, C, G, 1, code(dtype))
    o = {k: torch.full((G, C), float('nan'), device="cuda") for k in ("scale", "shift", "mean", "invstd")}
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    run("sdhip_affine_act_bn", xd.p, xd.ld, yd.p, yd.ld, None, 0, S.p, S.ld, nrep, P(dev(gamma)), P(dev(beta)), P(rm), P(rv),
        P(o["scale"]), P(o["shift"]), P(o["mean"]), P(o["invstd"]), n, C, G, count, EPS, MOM, 1, code(dtype))
    ds, dh = torch.full((nrep, G, C), float('nan'), device="cuda"), torch.full((nrep, G, C), float('nan'), device="cuda")
    run("sdhip_affine_act_bwd", gd.p, gd.ld, xd.p, xd.ld, None, 0, P(o["scale"]), P(o["shift"]), P(ds), P(dh), nrep, n, C, G, 1, 0, 0, code(dtype))
    dg, db = torch.full((C,), float('nan'), device="cuda"), torch.full((C,), float('nan'), device="cuda")
    run("sdhip_bn_bwd_apply_fin", gd.p, gd.ld, xd.p, xd.ld, gxd.p, gxd.ld, P(o["scale"]), P(o["shift"]), P(ds), P(dh), nrep, P(dev(gamma)),
        P(o["mean"]), P(o["invstd"]), P(dg), P(db), 0, 1.0, n, C, G, count, 1, code(dtype))
    _finite_and_intact(xd, gd, yd, gxd)
    ub = UBF if dtype == BF16 else 0.0
    yr, gxr = _rows(yt.detach()), _rows(xt.grad)
    xhat = (z_ref - beta) / gamma
    # an element inside the band may flip its mask: its whole term enters the two reductions, and through them every gx of its
    # channel and group (dL/dx holds -(gamma invstd / n) (dbeta + xhat dgamma); gamma invstd < 3.2 here)
    f_dg, f_db = np.where(keep, 0.0, np.abs(gy * xhat)).sum(0), np.where(keep, 0.0, np.abs(gy)).sum(0)
    check("chain y", yd.np(), yr, (40 * U32 + ub) * np.abs(z_ref).max(), keep)
    check("chain gx", gxd.np(), gxr, (12 * 300 * U32 + 3 * ub) * np.abs(gxr).max() + 3.2 / count * (f_db + np.abs(xhat) * f_dg), keep)
    check("chain dgamma", dg.double().cpu().numpy(), bn.weight.grad.numpy(), 300 * U32 * np.abs(gy * xhat).sum(0) + f_dg + 1e-300)
    check("chain dbeta", db.double().cpu().numpy(), bn.bias.grad.numpy(), 300 * U32 * np.abs(gy).sum(0) + f_db + 1e-300)
    check("chain running_mean", rm.double().cpu().numpy(), bn.running_mean.numpy(), 40 * U32 * (1 + np.abs(bn.running_mean.numpy())))
    check("chain running_var", rv.double().cpu().numpy(), bn.running_var.numpy(), 40 * U32 * (1 + np.abs(bn.running_var.numpy())))


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    """Only arguments SDHIP_CHECK_ARG rejects before a launch: a negative code and a message, outputs untouched."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    lib, sp = _lib._lib, _lib.stream_ptr()
    n, C = 70, 8
    x, y = Rows(n, C, F32, "dense", np.ones((n, C))), Rows(n, C, F32)
    S = Stats(1, 1, C, False)
    v = torch.zeros(200, device="cuda")
    bad = [
        ("sdhip_affine_act", (x.p, C - 1, y.p, C, None, 0, None, None, n, C, 1, 0, 0, sp)),                                  # ld < C
        ("sdhip_affine_act", (x.p, C, y.p, C, None, 0, None, None, n, C, 3, 0, 0, sp)),                                      # npix % groups
        ("sdhip_affine_act", (x.p, C, y.p, C, None, 0, None, None, n, C, 1, 0, 7, sp)),                                      # unknown dtype
        ("sdhip_channel_stats", (x.p, C - 1, S.p, C, 1, n, C, 1, 1, 0, sp)),
        ("sdhip_affine_act_bwd", (x.p, C, x.p, C, y.p, C, None, None, P(v), None, 1, n, C, 1, 0, 0, 0, 0, sp)),              # dscale without dshift
        ("sdhip_stats_fix_fin", (x.p, 32, x.p, 32, y.p, 32, n, S.p, 40, 16, P(v), P(v), 1, P(v), P(v), P(v), P(v), P(v), 0, 1.0, 40, 1, 70.0, 0, sp)),   # cs + 32 > Cf
        ("sdhip_stats_fix", (x.p, C, x.p, C, y.p, C - 1, S.p, C, n, C, 1, 0, sp)),
        ("sdhip_bn_bwd_apply", (x.p, C, x.p, C, y.p, C, P(v), P(v), S.p, C, n, C, 1, 3, 0, sp)),                             # unknown activation
    ]
    for name, args in bad:
        rc = getattr(lib, name)(*args)
        assert rc < 0 and lib.sdhip_last_error().decode(), name
    torch.cuda.synchronize()
    assert y.pads_intact() and bool(torch.isnan(y.slab).all()) and S.pads_intact()
