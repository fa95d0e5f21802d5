"""Plain float64 references of the loss / optimizer / PSMNet / HANet row entry points of include/sdhip.h.

Everything here is numpy on the CPU, written from the formulas in the header (and from what torch.optim.Adam, F.log_softmax,
F.l1_loss, F.adaptive_max_pool2d and the slice loop of the PSMNet cost volume define) — not from the kernels.
tests/test_tail_kernels.py checks, without a GPU, that these functions compose to the torch operations, and then compares the
HIP kernels with them.  The comparator, the slab layouts and the rounding units are those of tests/rowops_ref.py.

Layouts: loss / log-softmax tensors are [npix][C] row matrices; PSMNet volumes [N][D][H][W][C]; HANet tensors NHWC.
Every `wrong=` argument selects a plausible WRONG formula: the comparator tests show that the bounds reject it.
"""
import numpy as np

from rowops_ref import U32, UBF, Rows, check, half_ulp_bf16, layout, quant, worst_ratio  # noqa: F401  (one copy, re-exported)


def _f64(a):
    return np.asarray(a, np.float64)


# --------------------------------------------------------------------------- log-softmax
def log_softmax(x):
    x = _f64(x)
    z = x - x.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def log_softmax_bwd(gy, y, wrong=None):
    """gx = gy - exp(y) * sum_c gy.  wrong 'elementwise': gy - exp(y) * gy."""
    gy, y = _f64(gy), _f64(y)
    return gy - np.exp(y) * (gy if wrong == "elementwise" else gy.sum(-1, keepdims=True))


# --------------------------------------------------------------------------- losses
def ce_loss(y, t, weight, wrong=None):
    """(weight * mean_p sum_c -t log_softmax(y), gradient weight / npix * (softmax * sum_c t - t)).
    wrong: 'no_tsum' (softmax - t), 'mean_all' (mean over npix * C), 'weight_twice'."""
    y, t = _f64(y), _f64(t)
    npix, C = y.shape
    ls = log_softmax(y)
    den = npix * C if wrong == "mean_all" else npix
    w = weight * weight if wrong == "weight_twice" else weight
    ts = 1.0 if wrong == "no_tsum" else t.sum(-1, keepdims=True)
    return w * float(-(t * ls).sum()) / den, w / den * (np.exp(ls) * ts - t)


def l1_loss(a, b, weight, mask_nonpositive, wrong=None):
    """(weight * mean |a - b|, weight / n * sign(a - b)); mask_nonpositive: elements with b <= 0 count as zero difference
    and stay in the mean.  wrong: 'denominator' (masked elements leave the mean), 'sign0' (sign(0) = +1), 'mask_ge'."""
    a, b = _f64(a), _f64(b)
    m = ((b >= 0) if wrong == "mask_ge" else (b > 0)) if mask_nonpositive else np.ones(b.shape, bool)
    d = np.where(m, a - b, 0.0)
    n = max(int(m.sum()), 1) if wrong == "denominator" else d.size
    sg = np.where(d >= 0, 1.0, -1.0) if wrong == "sign0" else np.sign(d)
    return weight * float(np.abs(d).sum()) / n, weight / n * sg


# --------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, t, lr, b1, b2, eps, wd, gs, wrong=None):
    """Step t (1-based) of torch.optim.Adam on the gradient g * gs (+ wd * p: coupled weight decay) -> (p, m, v).
    wrong: 'eps_in_sqrt', 'no_bc2', 'decoupled_wd' (AdamW), 'scale_after_wd'."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    if wrong == "decoupled_wd":
        p = p * (1.0 - lr * wd)
        gr = g * gs
    elif wrong == "scale_after_wd":
        gr = (g + wd * p) * gs
    else:
        gr = g * gs + wd * p
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if wrong == "no_bc2":
        bc2 = 1.0
    den = np.sqrt(v / bc2 + eps) if wrong == "eps_in_sqrt" else np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m / den, m, v


# --------------------------------------------------------------------------- dropout
def dropout_kept(x, p, wrong=None):
    """Value of a kept element, x / (1 - p).  wrong 'scale_p': x / p."""
    return _f64(x) / (p if wrong == "scale_p" else 1.0 - p)


# --------------------------------------------------------------------------- PSMNet
def stuff(x, sd, s, wrong=None):
    """z[n, d*sd, h*s, w*s, :] = x[n, d, h, w, :], zero elsewhere.  wrong 'depth_s': the depth stride taken from s."""
    x = _f64(x)
    N, D, H, W, C = x.shape
    if wrong == "depth_s":
        sd = s
    z = np.zeros((N, (D - 1) * sd + 1, (H - 1) * s + 1, (W - 1) * s + 1, C))
    z[:, ::sd, ::s, ::s] = x
    return z


def unstuff(z, sd, s, wrong=None):
    if wrong == "depth_s":
        sd = s
    return _f64(z)[:, ::sd, ::s, ::s]


def cost_volume(L, R, D, wrong=None):
    """vol[b,i,h,w,:C] = L[b,h,w], vol[b,i,h,w,C:] = R[b,h,w-i] for w >= i, else 0.
    wrong: 'shift_plus' (right tower at w + i), 'zero_gt' (the valid region taken as w > i)."""
    L, R = _f64(L), _f64(R)
    B, H, W, C = L.shape
    vol = np.zeros((B, D, H, W, 2 * C))
    w = np.arange(W)
    for i in range(D):
        ok = w[(w > i) if wrong == "zero_gt" else (w >= i)]
        if wrong == "shift_plus":
            ok = ok[ok + i < W]
            src = ok + i
        else:
            src = ok - i
        vol[:, i, :, ok, :C] = L[:, :, ok].transpose(2, 0, 1, 3)
        vol[:, i, :, ok, C:] = R[:, :, src].transpose(2, 0, 1, 3)
    return vol


def cost_volume_bwd(g, wrong=None):
    """gL[b,h,w] = sum_{i <= w} g[b,i,h,w,:C]; gR[b,h,w] = sum_{i: w+i < W} g[b,i,h,w+i,C:].
    wrong 'gr_nolimit': the w + i < W limit forgotten, the column index wraps into the row."""
    g = _f64(g)
    B, D, H, W, C2 = g.shape
    C = C2 // 2
    gL, gR = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for i in range(D):
        if i < W:
            gL[:, :, i:] += g[:, i, :, i:, :C]
            gR[:, :, :W - i] += g[:, i, :, i:, C:]
        if wrong == "gr_nolimit" and i > 0:
            k = min(i, W)
            gR[:, :, W - k:] += g[:, i, :, (np.arange(W - k, W) + i) % W, C:].transpose(1, 2, 0, 3)
    return gL, gR


# --------------------------------------------------------------------------- HANet
def rowpool_bins(H, OH, wrong=None):
    """Rows [h0, h1) of bin i: floor(i H / OH) .. ceil((i + 1) H / OH).  wrong 'floor_end': the end floored (never empty)."""
    out = []
    for i in range(OH):
        h0 = i * H // OH
        h1 = (i + 1) * H // OH if wrong == "floor_end" else -(-(i + 1) * H // OH)
        out.append((h0, max(h1, h0 + 1)))
    return out


def rowpool_max(x, OH, wrong=None):
    """nn.AdaptiveMaxPool2d((OH, 1)) of NHWC x -> (y [B][OH][C], idx [B][OH][C] = h * W + w).  The scan is ATen's: row-major
    over the bin, `v > best || isnan(v)` takes v, starting from (-inf, index of the bin's first element): the first maximum
    wins, a NaN wins over everything and a later NaN over an earlier one.  wrong: 'last_wins' (v >= best), 'floor_end'."""
    x = _f64(x)
    B, H, W, C = x.shape
    y = np.full((B, OH, C), -np.inf)
    idx = np.zeros((B, OH, C), np.int64)
    for i, (h0, h1) in enumerate(rowpool_bins(H, OH, wrong)):
        best, bi = np.full((B, C), -np.inf), np.full((B, C), h0 * W, np.int64)
        for h in range(h0, h1):
            for w in range(W):
                v = x[:, h, w]
                with np.errstate(invalid='ignore'):
                    take = ((v >= best) if wrong == "last_wins" else (v > best)) | np.isnan(v)
                best = np.where(take, v, best)
                bi = np.where(take, h * W + w, bi)
        y[:, i], idx[:, i] = best, bi
    return y, idx


def rowpool_max_bwd(gy, idx, H, W, count=False):
    """gx[b, idx[b,i,c], c] += gy[b,i,c] -> [B][H][W][C].  count: the number of bins that land on each element instead."""
    gy = _f64(gy)
    B, OH, C = gy.shape
    gx = np.zeros((B, H * W, C))
    b, _, c = np.meshgrid(np.arange(B), np.arange(OH), np.arange(C), indexing="ij")
    np.add.at(gx, (b, np.asarray(idx), c), np.ones_like(gy) if count else gy)
    return gx.reshape(B, H, W, C)


def mul_rows(a, att):
    """y[b,h,w,c] = a[b,h,w,c] * att[b,h,c]."""
    return _f64(a) * _f64(att)[:, :, None, :]


def mul_rows_bwd(g, a, att, wrong=None):
    """ga = g * att; gatt[b,h,c] = sum_w g * a.  wrong 'sum_h': gatt summed over h as well."""
    g, a, att = _f64(g), _f64(a), _f64(att)
    gatt = (g * a).sum(2)
    if wrong == "sum_h":
        gatt = np.repeat(gatt.sum(1, keepdims=True), g.shape[1], 1)
    return g * att[:, :, None, :], gatt
