"""Plain float64 references of the BatchNorm / pooling / resize entry points of include/sdhip.h, and the comparator.

Everything here is numpy on the CPU, written from the formulas in the header (and from what nn.BatchNorm2d, F.max_pool2d,
F.avg_pool2d and F.interpolate define) — not from the kernels.  tests/test_bn_kernels.py and tests/test_resample.py check,
without a GPU, that these functions compose to the torch operations, and then compare the HIP kernels with them.

Layouts: BatchNorm tensors are [npix][C] row matrices, rows of statistics group g are the g-th npix/G rows; statistics are
[G][2][C] (sum, sum of squares), per-group coefficients [G][C].  Pool / resize tensors are NHWC [B][H][W][C].
"""
import numpy as np

U32 = 2.0 ** -24      # unit roundoff of f32 (round to nearest)
UBF = 2.0 ** -8       # unit roundoff of bf16 (8 significant bits): the largest half ulp relative to the value


def half_ulp_bf16(ref):
    """Half an ulp of the bf16 number nearest `ref`: 2^(e - 8) for 2^e <= |ref| < 2^(e + 1) — what a correctly rounded
    store may add.  Relative to |ref| that is 2^-9 only at the top of a binade and 2^-8 at its bottom."""
    _, e = np.frexp(np.abs(np.asarray(ref, np.float64)))          # |ref| = m 2^e, m in [0.5, 1)
    return np.where(np.asarray(ref) == 0, 0.0, np.ldexp(1.0, e - 9))


# --------------------------------------------------------------------------- BatchNorm forward
def _grp(x, G):
    return x.reshape(G, x.shape[0] // G, x.shape[1])


def channel_stats(x, G):
    """S[g][0][c] = sum x, S[g][1][c] = sum x^2 over the rows of group g."""
    xg = _grp(np.asarray(x, np.float64), G)
    return np.stack([xg.sum(1), (xg * xg).sum(1)], 1)


def replica_sum(ws):
    """[nrep][G][2][C] -> [G][2][C]."""
    return np.asarray(ws, np.float64).sum(0)


def bn_finalize(S, count, gamma=None, beta=None, rmean=None, rvar=None, eps=1e-5, momentum=0.1):
    """Train mode.  Returns dict(scale, shift, mean, invstd: [G][C]; rmean, rvar: [C] or None).  The variance that
    normalises is biased and clamped at 0; running_var takes the unbiased one (count > 1); groups update in order."""
    S = np.asarray(S, np.float64)
    G, _, C = S.shape
    gamma = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    mean = S[:, 0] / count
    var = np.maximum(S[:, 1] / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma[None] * invstd
    shift = beta[None] - mean * scale
    out = dict(scale=scale, shift=shift, mean=mean, invstd=invstd, var=var, rmean=None, rvar=None)
    if rmean is not None:
        rm, rv = np.asarray(rmean, np.float64).copy(), np.asarray(rvar, np.float64).copy()
        for g in range(G):
            unb = var[g] * count / (count - 1.0) if count > 1 else var[g]
            rm = (1.0 - momentum) * rm + momentum * mean[g]
            rv = (1.0 - momentum) * rv + momentum * unb
        out.update(rmean=rm, rvar=rv)
    return out


def bn_finalize_eval(G, gamma, beta, rmean, rvar, eps=1e-5):
    """Eval mode: scale / shift from the running statistics, the same for every group."""
    rmean, rvar = np.asarray(rmean, np.float64), np.asarray(rvar, np.float64)
    C = rmean.shape[0]
    gamma = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    beta = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    invstd = 1.0 / np.sqrt(rvar + eps)
    t = lambda v: np.repeat(v[None], G, 0)
    return dict(scale=t(gamma * invstd), shift=t(beta - rmean * gamma * invstd), mean=t(rmean), invstd=t(invstd))


def bn_fold_finalize(ws, c_new0, S, count, C, **kw):
    """S (a [G][2][ldc] slab, updated copy returned) += replica sum of ws in columns [c_new0, c_new0 + Cn); then
    bn_finalize of the first C columns."""
    S = np.asarray(S, np.float64).copy()
    add = replica_sum(ws)
    S[:, :, c_new0:c_new0 + add.shape[2]] += add
    return S, bn_finalize(S[:, :, :C], count, **kw)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def act_fwd(z, act):
    return z if act == 0 else np.maximum(z, 0.0) if act == 1 else sigmoid(z)


def act_grad(z, act, at_output=False):
    """d act / dz at z.  act 4: z IS the sigmoid's output.  at_output (the wrong reference of the comparator test):
    sigmoid' of act 2 evaluated as if z were the output."""
    if act == 0:
        return np.ones_like(z)
    if act == 1:
        return (z > 0).astype(np.float64)
    if act == 4 or at_output:
        return z * (1.0 - z)
    s = sigmoid(z)
    return s * (1.0 - s)


def _coef(v, G, n, C):
    """[G][C] (or None -> fill) broadcast to the rows."""
    return np.repeat(np.asarray(v, np.float64).reshape(G, 1, C), n // G, 1).reshape(n, C)


def pre_act(x, scale, shift, G):
    x = np.asarray(x, np.float64)
    n, C = x.shape
    sc = _coef(scale, G, n, C) if scale is not None else np.ones((n, C))
    sf = _coef(shift, G, n, C) if shift is not None else np.zeros((n, C))
    return x * sc + sf, sc


def affine_act(x, scale, shift, G, act, res=None):
    z, _ = pre_act(x, scale, shift, G)
    y = act_fwd(z, act)
    return y if res is None else y + np.asarray(res, np.float64)


# --------------------------------------------------------------------------- BatchNorm backward
def affine_act_bwd(gy, x, scale, shift, G, act, at_output=False):
    """gx = gy * act' * scale; dscale[g][c] = sum gy * act' * x; dshift[g][c] = sum gy * act'."""
    x = np.asarray(x, np.float64)
    z, sc = pre_act(x, scale, shift, G)
    gm = np.asarray(gy, np.float64) * act_grad(z, act, at_output)
    return gm * sc, _grp(gm * x, G).sum(1), _grp(gm, G).sum(1)


def bn_finalize_bwd(dscale, dshift, gamma, mean, invstd, count, train=True):
    """(dscale, dshift)[G][C] -> dgamma[C], dbeta[C], dS[G][2][C].
    scale = gamma * invstd, shift = beta - mean * scale, invstd = (var + eps)^-1/2, var = S2/n - mean^2, mean = S1/n:
      dL/dinvstd = gamma * (dscale - mean * dshift), dL/dvar = -invstd^3 / 2 * dL/dinvstd,
      dL/dmean = -gamma * invstd * dshift (through shift; the part through var is -2 mean dL/dvar),
      dL/dS2 = dL/dvar / n, dL/dS1 = (dL/dmean - 2 mean dL/dvar) / n.  Eval mode: the statistics are constants, dS = 0."""
    dscale, dshift = np.asarray(dscale, np.float64), np.asarray(dshift, np.float64)
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    C = dscale.shape[1]
    gamma = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    t = dscale - mean * dshift
    dgamma, dbeta = (invstd * t).sum(0), dshift.sum(0)
    dvar = -0.5 * invstd ** 3 * gamma[None] * t
    dmean = -gamma[None] * invstd * dshift - 2.0 * mean * dvar
    dS = np.stack([dmean / count, dvar / count], 1)
    return dgamma, dbeta, dS if train else np.zeros_like(dS)


def stats_fix(gin, x, dS, G, factor=2.0):
    """gout = gin + dS[g][0][c] + 2 x dS[g][1][c]  (d sum x^2 / dx = 2x).  factor: the comparator test drops the 2."""
    x = np.asarray(x, np.float64)
    n, C = x.shape
    dS = np.asarray(dS, np.float64)
    return np.asarray(gin, np.float64) + _coef(dS[:, 0], G, n, C) + factor * x * _coef(dS[:, 1], G, n, C)


def bn_bwd_apply(gy, x, scale, shift, dS, G, act):
    gx, _, _ = affine_act_bwd(gy, x, scale, shift, G, act)
    return stats_fix(gx, x, dS, G)


# --------------------------------------------------------------------------- pooling / broadcast
def maxpool3s2(x, pad=-np.inf, last_wins=False):
    """3x3 / stride 2 / pad 1 max pool of NHWC x -> (y, tap): tap = kh * 3 + kw of the FIRST maximum in row-major order;
    a NaN wins over everything (ATen).  pad / last_wins: the wrong references of the comparator test."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((B, H + 2, W + 2, C), pad)
    xp[:, 1:H + 1, 1:W + 1] = x
    real = np.zeros((H + 2, W + 2), bool)
    real[1:H + 1, 1:W + 1] = True
    y = np.full((B, Ho, Wo, C), -np.inf)
    tap = np.zeros((B, Ho, Wo, C), np.int64)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:, :Ho, :Wo]
            ok = real[kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:Ho, :Wo][None, :, :, None] | (pad != -np.inf)
            with np.errstate(invalid='ignore'):
                take = ((v >= y) if last_wins else (v > y)) | np.isnan(v)
            take &= ok
            y = np.where(take, v, y)
            tap = np.where(take, kh * 3 + kw, tap)
    return y, tap


def maxpool3s2_bwd(gy, tap, H, W):
    gy = np.asarray(gy, np.float64)
    B, Ho, Wo, C = gy.shape
    gx = np.zeros((B, H + 2, W + 2, C))
    for kh in range(3):
        for kw in range(3):
            gx[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][:, :Ho, :Wo] += np.where(tap == kh * 3 + kw, gy, 0.0)
    return gx[:, 1:H + 1, 1:W + 1]


def avgpool(x, k):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    Ho, Wo = H // k, W // k
    return x[:, :Ho * k, :Wo * k].reshape(B, Ho, k, Wo, k, C).mean((2, 4))


def avgpool_bwd(gy, H, W, k, fill_leftover=False):
    """Floor mode: the rows / columns past Ho * k belong to no window and get zero.  fill_leftover: wrong reference."""
    gy = np.asarray(gy, np.float64)
    B, Ho, Wo, C = gy.shape
    gx = np.zeros((B, H, W, C))
    hi = np.minimum(np.arange(H) // k, Ho - 1) if fill_leftover else np.arange(Ho * k) // k
    wi = np.minimum(np.arange(W) // k, Wo - 1) if fill_leftover else np.arange(Wo * k) // k
    gx[:, :len(hi), :len(wi)] = gy[:, hi][:, :, wi] / (k * k)
    return gx


def mul_bcast(a, m):
    return np.asarray(a, np.float64) * np.asarray(m, np.float64)[..., None]


def mul_bcast_bwd(g, a, m):
    g = np.asarray(g, np.float64)
    return g * np.asarray(m, np.float64)[..., None], (g * np.asarray(a, np.float64)).sum(-1)


# --------------------------------------------------------------------------- resize
def resize_matrix(n_in, n_out, mode, scale=0.0, shifted_window=True):
    """[n_out][n_in] matrix of one axis.  mode 0 nearest: src = min(floor(d * s), in - 1); 1 bilinear align_corners=False:
    src = max((d + 0.5) * s - 0.5, 0); 2 bilinear align_corners=True: src = d * (in - 1) / (out - 1) (0 if out == 1);
    s = `scale` if > 0 (F.interpolate(scale_factor=f) passes 1/f) else in / out.  The nearest index is taken in f32 as ATen
    does for every dtype; the bilinear coordinate in f64 as ATen does for a double tensor.
    shifted_window=False: the wrong reference of the comparator test — a gather backward of mode 1 that looks for the
    destinations of source i only in [(i - 1) / s - 2, (i + 1) / s + 2], forgetting that the half-pixel sampling shifts that
    window by 0.5 / s - 0.5 destinations."""
    M = np.zeros((n_out, n_in))
    d = np.arange(n_out)
    if mode == 0:
        s = np.float32(scale) if scale > 0 else np.float32(n_in) / np.float32(n_out)
        src = np.minimum(np.floor(d.astype(np.float32) * s).astype(np.int64), n_in - 1)
        M[d, src] = 1.0
        return M
    if mode == 2:
        pos = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        s = float(scale) if scale > 0 else n_in / n_out
        pos = np.maximum((d + 0.5) * s - 0.5, 0.0)
    i0 = np.minimum(np.floor(pos).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(pos - i0, 0.0, 1.0)
    np.add.at(M, (d, i0), 1.0 - l1)
    np.add.at(M, (d, i1), l1)
    if mode == 1 and not shifted_window:
        i = np.arange(n_in)[None]
        M[(d[:, None] < np.floor((i - 1) / s) - 2) | (d[:, None] > np.ceil((i + 1) / s) + 2)] = 0.0
    return M


def resize(x, Ho, Wo, mode, scale_h=0.0, scale_w=0.0):
    x = np.asarray(x, np.float64)
    Mh, Mw = resize_matrix(x.shape[1], Ho, mode, scale_h), resize_matrix(x.shape[2], Wo, mode, scale_w)
    return np.einsum('oh,bhwc,pw->bopc', Mh, x, Mw, optimize=True)


def resize_bwd(gy, H, W, mode, scale_h=0.0, scale_w=0.0, shifted_window=True):
    gy = np.asarray(gy, np.float64)
    Mh = resize_matrix(H, gy.shape[1], mode, scale_h, shifted_window)
    Mw = resize_matrix(W, gy.shape[2], mode, scale_w, shifted_window)
    return np.einsum('oh,bopc,pw->bhwc', Mh, gy, Mw, optimize=True)


# --------------------------------------------------------------------------- comparator
def worst_ratio(got, ref, bound, keep=None):
    """max |got - ref| / bound over the kept elements (inf if a kept element of got is not finite, or a bound is not
    positive).  An equal NaN / inf pair counts as exact."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    keep = np.ones(ref.shape, bool) if keep is None else np.asarray(keep, bool)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(same, 0.0, np.abs(got - ref) / bound)
    r = np.where(np.isnan(r) | (bound <= 0) & ~same, np.inf, r)
    r = r[keep]
    return float(r.max()) if r.size else 0.0


def check(label, got, ref, bound, keep=None):
    """Assert worst_ratio <= 1, after printing it: `pytest -s` leaves every measured error / bound in the log (the tables in
    the docstrings of the two test files were taken from such a run)."""
    r = worst_ratio(got, ref, bound, keep)
    print("ratio %-44s %.3g" % (label, r))
    assert r <= 1.0, "%s: worst |error| / bound = %.4g" % (label, r)
    return r


# --------------------------------------------------------------------------- plumbing shared by the two GPU test files
def quant(a, dtype):
    """`a` rounded to the torch dtype under test, back in float64: the values the kernel is given."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).double().numpy()


def layout(name, C):
    """(first channel k, pixel stride ld) of a [rows][C] tensor inside a NaN-filled slab:
    dense; slab8: ld a multiple of 8 and a 16-byte aligned offset (vector kernels stay possible); ldodd: ld odd, so no
    vector width divides it; misal: ld a multiple of 8 but the slice starts one element in, which breaks 16-byte alignment."""
    r8 = (C + 7) // 8 * 8
    return {"dense": (0, C), "slab8": (8, r8 + 16), "ldodd": (0, r8 + 9), "misal": (1, r8 + 8)}[name]


class Rows:
    """A [n][C] tensor of `dtype` on the GPU as channels [k, k + C) of a NaN-filled [n][ld] slab.  vals=None: an output,
    NaN everywhere.  After the kernel ran: np() = the logical values in f64, pads_intact() = every other element of the
    slab has the bits it had."""

    def __init__(self, n, C, dtype, lay="dense", vals=None):
        import torch
        self.k, self.ld = layout(lay, C) if isinstance(lay, str) else lay
        self.C = C
        self.slab = torch.full((n, self.ld), float('nan'), dtype=dtype, device="cuda")
        self.v = self.slab[:, self.k:self.k + C]
        if vals is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64).reshape(n, C)).to(dtype))
        self.before = self.slab.clone()

    @property
    def p(self):
        import ctypes
        return ctypes.c_void_p(self.v.data_ptr())

    def vec(self, n):
        """Can a kernel read these rows n elements (16 bytes) at a time?"""
        return self.C % n == 0 and self.ld % n == 0 and self.v.data_ptr() % 16 == 0

    def np(self):
        return self.v.double().cpu().numpy()

    def pads_intact(self):
        import torch
        bits = torch.int32 if self.slab.element_size() == 4 else torch.int16 if self.slab.element_size() == 2 else torch.int64
        a, b = self.slab.clone(), self.before.clone()
        a[:, self.k:self.k + self.C] = 0
        b[:, self.k:self.k + self.C] = 0
        return bool(torch.equal(a.view(bits), b.view(bits)))


class diag_switches:
    """`with diag_switches(SDHIP_CONV_GENERIC="1", SDHIP_CONV_BIG=None):` sets (None: unsets) diagnostic environment
    switches and has the library re-read them; on the way out — by an exception too — the environment is what it was and the
    library has re-read it again, so a failing assert cannot leak a switch into the later tests of the process."""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        import os
        from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
        self.old = {k: os.environ.get(k) for k in self.env}
        self._set(self.env)
        _lib.reload_diag()
        return self

    def __exit__(self, *exc):
        from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
        self._set(self.old)
        _lib.reload_diag()
        return False

    @staticmethod
    def _set(env):
        import os
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
