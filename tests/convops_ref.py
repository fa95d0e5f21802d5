"""Plain float64 references of the convolution entry points of include/sdhip.h (weight packing, forward, statistics,
BatchNorm-prologue forward, transposed-convolution phases, weight gradient).

Everything here is numpy on the CPU, written from the formulas in the header — explicit loops over the kernel taps, no call
to F.conv2d — and tests/test_conv_kernels.py checks without a GPU that these functions compose to the torch operations.

Layouts: activations NDHWC [B][D][H][W][C] (a 4-D array is taken as D = 1 and a 4-D result is returned for it); logical
weights w[kd][M][K][kh][kw] (a 4-D w is kd = 1); per-group coefficients [G][C]; statistics [G][2][C].
"""
import numpy as np

import rowops_ref as R


def ck_of(bf16):
    """Reduction channels per packed 128-byte row."""
    return 64 if bf16 else 32


def packed_elems(M, K, T, bf16):
    ck = ck_of(bf16)
    return -(-K // ck) * T * (-(-M // 16) * 16) * ck


# --------------------------------------------------------------------------- packing
def pack(src, M, K, T, sm, sk, flip, bf16, rnd=None):
    """packed[q][t][m][c] = src[m*sm + (q*CK + c)*sk + (T-1-t if flip else t)] for m < M and q*CK + c < K, else 0;
    m < Mpad = roundup(M, 16), c < CK = 64 (bf16) / 32 (f32).  src: the flat f32 parameter.  rnd: rounding to the pack
    dtype (values -> values), applied to the gathered values."""
    src = np.asarray(src, np.float64).ravel()
    ck, Mpad = ck_of(bf16), -(-M // 16) * 16
    nq = -(-K // ck)
    out = np.zeros((nq, T, Mpad, ck))
    for q in range(nq):
        for t in range(T):
            tt = T - 1 - t if flip else t
            for c in range(min(ck, K - q * ck)):
                out[q, t, :M, c] = src[np.arange(M) * sm + (q * ck + c) * sk + tt]
    return out if rnd is None else rnd(out)


def unpack(acc, M, K, T, sm, sk, flip, bf16, grad=None, size=None):
    """Inverse of pack for the f32 gradient: grad[m*sm + k*sk + t] (+)= acc[k / CK][T-1-t if flip else t][m][k % CK].
    grad=None: a zero array of `size` elements is written (the other elements stay 0); else added to a copy of grad."""
    acc = np.asarray(acc, np.float64)
    ck = ck_of(bf16)
    out = np.zeros(size) if grad is None else np.asarray(grad, np.float64).copy()
    for k in range(K):
        for t in range(T):
            tt = T - 1 - t if flip else t
            idx = np.arange(M) * sm + k * sk + t
            v = acc[k // ck, tt, :M, k % ck]
            out[idx] = v if grad is None else out[idx] + v
    return out


def pack_conv(w, bf16, rnd=None):
    """Logical w[kd][M][K][kh][kw] -> [kd][q][t][m][c]: every depth tap packed as a Conv2d forward weight."""
    w = _w5(w)
    kd, M, K, kh, kw = w.shape
    T = kh * kw
    return np.stack([pack(w[i].ravel(), M, K, T, K * T, T, 0, bf16, rnd) for i in range(kd)])


def unpack_conv(acc, M, K, kd, kh, kw, bf16):
    """[kd][q][t][m][c] -> dW[kd][M][K][kh][kw]."""
    T = kh * kw
    acc = np.asarray(acc, np.float64).reshape(kd, -(-K // ck_of(bf16)), T, -(-M // 16) * 16, ck_of(bf16))
    return np.stack([unpack(acc[i], M, K, T, K * T, T, 0, bf16, size=M * K * T).reshape(M, K, kh, kw) for i in range(kd)])


# --------------------------------------------------------------------------- forward
def _x5(x):
    x = np.asarray(x, np.float64)
    return x[:, None] if x.ndim == 4 else x


def _w5(w):
    w = np.asarray(w, np.float64)
    return w[None] if w.ndim == 4 else w


def group_of(B, groups, mod=False):
    """Statistics group of every image: b / (B / groups).  mod: the wrong reference b % groups."""
    b = np.arange(B)
    return b % groups if mod else b // (B // groups)


def prologue(x, in_scale, in_shift, in_relu, groups, group_mod=False):
    """pro(x) = relu?(x * in_scale[g][k] + in_shift[g][k]), g the group of the image; x itself without coefficients."""
    x = _x5(x)
    if in_scale is None:
        return x
    g = group_of(x.shape[0], groups, group_mod)
    sc = np.asarray(in_scale, np.float64)[g][:, None, None, None, :]
    sh = np.asarray(in_shift, np.float64)[g][:, None, None, None, :]
    z = x * sc + sh
    return np.maximum(z, 0.0) if in_relu else z


def _axis(n, no, k, s, d, pad):
    """Extent of the padded axis and the offset of element 0 inside it: output o, tap j reads o*s + j*d - pad."""
    lo = min(0, -pad)
    hi = max(n - 1, (no - 1) * s + (k - 1) * d - pad)
    return hi - lo + 1, -lo


def padded(xe, w_shape, stride, dil, pad_t, pad_l, Ho, Wo, sd=1, pad_d=0, Do=None, fill=None):
    """xe inside the zero frame every tap of every output needs (bottom / right / back padding implied by the output
    extent).  fill: [B][C] values for the frame instead of zero (the wrong reference that pads before the prologue).
    Returns (array, (od, oh, ow) offsets of element 0)."""
    B, D, H, W, C = xe.shape
    kd, _, _, kh, kw = w_shape
    Do = D if Do is None else Do
    nd, od = _axis(D, Do, kd, sd, 1, pad_d)
    nh, oh = _axis(H, Ho, kh, stride, dil, pad_t)
    nw, ow = _axis(W, Wo, kw, stride, dil, pad_l)
    P = np.zeros((B, nd, nh, nw, C))
    if fill is not None:
        P[...] = np.asarray(fill, np.float64)[:, None, None, None, :]
    P[:, od:od + D, oh:oh + H, ow:ow + W] = xe
    return P, (od, oh, ow)


def corr(xe, w, stride=1, dil=1, pad_t=0, pad_l=0, Ho=None, Wo=None, sd=1, pad_d=0, Do=None, fill=None, taps=None,
         shift=None):
    """out[b,do,oh,ow,m] = sum over (jd, jh, jw, k) of w[jd][m][k][jh][jw] * xe[b, do*sd + jd - pad_d,
    oh*stride + jh*dil - pad_t, ow*stride + jw*dil - pad_l, k], zero outside xe (depth taps are never dilated).
    taps: boolean [kh][kw] selecting the taps that take part.  shift: {(jh, jw): pixels} moves those taps' column (the
    wrong reference of the comparator test)."""
    xe, w = _x5(xe), _w5(w)
    B, D, H, W, C = xe.shape
    kd, M, K, kh, kw = w.shape
    assert K == C, (K, C)
    Ho = H if Ho is None else Ho
    Wo = W if Wo is None else Wo
    Do = D if Do is None else Do
    extra = max([abs(v) for v in shift.values()], default=0) if shift else 0
    P, (od, oh, ow) = padded(xe, (kd, M, K, kh, kw + 0), stride, dil, pad_t, pad_l + extra, Ho, Wo + 2 * extra, sd, pad_d, Do, fill)
    ow -= extra
    out = np.zeros((B, Do, Ho, Wo, M))
    for jd in range(kd):
        d0 = od + jd - pad_d
        for jh in range(kh):
            h0 = oh + jh * dil - pad_t
            for jw in range(kw):
                if taps is not None and not taps[jh][jw]:
                    continue
                w0 = ow + extra + jw * dil - pad_l + (shift.get((jh, jw), 0) if shift else 0)
                xs = P[:, d0:d0 + (Do - 1) * sd + 1:sd, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride]
                out += xs @ w[jd, :, :, jh, jw].T
    return out


def conv_fwd(x, w, bias=None, in_scale=None, in_shift=None, in_relu=0, groups=1, stride=1, dil=1, pad_t=0, pad_l=0,
             Ho=None, Wo=None, sd=1, pad_d=0, Do=None, act=0, y_prev=None,
             pad_first=False, group_mod=False, act_before_bias=False, taps=None, shift=None):
    """y = act(bias + corr(pro(x), w)) (+ y_prev when accumulating); zero padding AFTER the prologue.  The last line of
    keywords are the wrong references of the comparator test."""
    squeeze = np.asarray(x).ndim == 4
    xe = prologue(x, in_scale, in_shift, in_relu, groups, group_mod)
    fill = None
    if pad_first and in_scale is not None:      # pro(0): what a kernel that pads first would feed the taps
        g = group_of(xe.shape[0], groups, group_mod)
        z = np.asarray(in_shift, np.float64)[g]
        fill = np.maximum(z, 0.0) if in_relu else z
    r = corr(xe, w, stride, dil, pad_t, pad_l, Ho, Wo, sd, pad_d, Do, fill, taps, shift)
    b = 0.0 if bias is None else np.asarray(bias, np.float64)
    y = R.act_fwd(r, act) + b if act_before_bias else R.act_fwd(r + b, act)
    if y_prev is not None:
        y = y + _x5(y_prev)
    return y[:, 0] if squeeze else y


def conv_stats(y_stored, groups):
    """[G][2][M]: sum and sum of squares of the stored values over the pixels (voxels) of every statistics group."""
    y = np.asarray(y_stored, np.float64)
    return R.channel_stats(y.reshape(-1, y.shape[-1]), groups)


# --------------------------------------------------------------------------- BatchNorm-prologue forward
def bnpro(x, w, in_stats, count, gamma=None, beta=None, rmean=None, rvar=None, eps=1e-5, momentum=0.1, groups=1,
          pend=None, pend_c0=0, pad_t=0, pad_l=0):
    """sdhip_conv2d_fwd_bnpro.  in_stats [nrep][G][2][ld] (ld >= Cin); pend [pend_nrep][G][2][pend_n] or None: the
    channels [pend_c0, pend_c0 + pend_n) take their sums from there, and in_stats (one replica) receives them.
    Returns dict(y, scale, shift, mean, invstd, rmean, rvar, in_stats (after the fold), fin (the bn_finalize dict))."""
    x5 = _x5(x)
    Cin = x5.shape[-1]
    S = np.asarray(in_stats, np.float64)
    if pend is not None:
        assert S.shape[0] == 1
        pend = np.asarray(pend, np.float64)
        Sf = S[0].copy()
        Sf[:, :, pend_c0:pend_c0 + pend.shape[3]] = R.replica_sum(pend)     # taken from the replicas, not added to the slab
        fin = R.bn_finalize(Sf[:, :, :Cin], count, gamma, beta, rmean, rvar, eps, momentum)
        S_after = Sf[None]
    else:
        fin = R.bn_finalize(R.replica_sum(S)[:, :, :Cin], count, gamma, beta, rmean, rvar, eps, momentum)
        S_after = S.copy()
    y = conv_fwd(x, w, None, fin["scale"], fin["shift"], 1, groups, 1, 1, pad_t, pad_l)
    return dict(y=y, scale=fin["scale"], shift=fin["shift"], mean=fin["mean"], invstd=fin["invstd"], rmean=fin["rmean"],
                rvar=fin["rvar"], in_stats=S_after, fin=fin)


# --------------------------------------------------------------------------- transposed-convolution phases
def phase_taps(off):
    """Kernel taps of one axis of ConvTranspose(k=3, s=2, p=1, output_padding=1) that reach output 2m + off, ordered by
    the input offset they read (m, m + 1): [1] for off = 0, [2, 0] for off = 1."""
    return [1] if off == 0 else [2, 0]


def phase(x, w_full, off_d, off_h, off_w):
    """x [B][D][H][W][Cin], w_full: the ConvTranspose3d weight [Cin][Cout][3][3][3] (2-D: [Cin][Cout][1][3][3] with
    off_d = 0 selecting its only depth tap).  Returns (w_sub [kd'][Cout][Cin][kh'][kw'] with taps input-offset-major, y_sub
    [B][D][H][W][Cout]): y_full[b, 2d + off_d, 2h + off_h, 2w + off_w] = y_sub[b, d, h, w]."""
    w_full = np.asarray(w_full, np.float64)
    td = [0] if w_full.shape[2] == 1 else phase_taps(off_d)
    th, tw = phase_taps(off_h), phase_taps(off_w)
    w_sub = w_full[:, :, td][:, :, :, th][:, :, :, :, tw].transpose(2, 1, 0, 3, 4)
    x5 = _x5(x)
    return w_sub, corr(x5, w_sub, 1, 1, 0, 0, x5.shape[2], x5.shape[3], 1, 0, x5.shape[1])


def phase_assemble(x, w_full, stored=None):
    """The whole [B][2D][2H][2W][Cout] volume from the 8 (2-D: 4) phases.  stored: rounding applied to every phase."""
    x5 = _x5(x)
    B, D, H, W, _ = x5.shape
    flat = np.asarray(w_full).shape[2] == 1
    out = np.full((B, D if flat else 2 * D, 2 * H, 2 * W, np.asarray(w_full).shape[1]), np.nan)
    for od in ([0] if flat else [0, 1]):
        for oh in (0, 1):
            for ow in (0, 1):
                _, ys = phase(x5, w_full, od, oh, ow)
                ys = ys if stored is None else stored(ys)
                if flat:
                    out[:, :, oh::2, ow::2] = ys
                else:
                    out[:, od::2, oh::2, ow::2] = ys
    return out


# --------------------------------------------------------------------------- weight gradient
def wgrad(x, dy, kd, kh, kw, in_scale=None, in_shift=None, in_relu=0, groups=1, stride=1, dil=1, pad_t=0, pad_l=0,
          sd=1, pad_d=0):
    """dW[jd][m][k][jh][jw] = sum over (b, do, oh, ow) of dy[b,do,oh,ow,m] * pro(x)[b, do*sd + jd - pad_d,
    oh*stride + jh*dil - pad_t, ow*stride + jw*dil - pad_l, k] (zero outside x, padding after the prologue);
    dbias[m] = sum dy.  Returns (dW, dbias)."""
    xe, dy = prologue(x, in_scale, in_shift, in_relu, groups), _x5(dy)
    B, Do, Ho, Wo, M = dy.shape
    K = xe.shape[-1]
    P, (od, oh, ow) = padded(xe, (kd, M, K, kh, kw), stride, dil, pad_t, pad_l, Ho, Wo, sd, pad_d, Do)
    dW = np.zeros((kd, M, K, kh, kw))
    dyf = dy.reshape(-1, M)
    for jd in range(kd):
        d0 = od + jd - pad_d
        for jh in range(kh):
            h0 = oh + jh * dil - pad_t
            for jw in range(kw):
                w0 = ow + jw * dil - pad_l
                xs = P[:, d0:d0 + (Do - 1) * sd + 1:sd, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride]
                dW[jd, :, :, jh, jw] = dyf.T @ xs.reshape(-1, K)
    return dW, dyf.sum(0)
