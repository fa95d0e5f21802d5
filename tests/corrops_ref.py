"""Plain float64 references of the correlation entry points of include/sdhip.h (sdhip_corr_fwd, sdhip_corr_bwd).

Everything here is numpy on the CPU, written from the formula in the header — one shift and one sum per displacement, zero
where the displaced pixel leaves the image — not from the kernels.  tests/test_corr_kernels.py checks without a GPU that
these functions agree with the plain-C oracle, with torch autograd and with a hand-checkable vector.

Layouts: maps NHWC [B][H][W][C]; the correlation [B][H][W][PH*PW], displacement index p = ph * PW + pw fastest, which pairs
in1[h, w] with in2[h + (ph - PH/2) * dil, w + (pw - PW/2) * dil].

The keywords after `dil` are the wrong references of the comparator test; the defaults are the operation.
"""
import numpy as np


def shifted(x, dy, dx, clamp=False):
    """y[b, h, w] = x[b, h + dy, w + dx], zero where that pixel lies outside the image (clamp: the nearest pixel inside)."""
    x = np.asarray(x, np.float64)
    _, H, W = x.shape[:3]
    hs, ws = np.arange(H) + dy, np.arange(W) + dx
    if clamp:
        return x[:, np.clip(hs, 0, H - 1)][:, :, np.clip(ws, 0, W - 1)]
    y = np.zeros_like(x)
    h, w = (hs >= 0) & (hs < H), (ws >= 0) & (ws < W)
    if h.any() and w.any():
        y[:, h.argmax():h.argmax() + h.sum(), w.argmax():w.argmax() + w.sum()] = x[:, hs[h][0]:hs[h][-1] + 1, ws[w][0]:ws[w][-1] + 1]
    return y


def displacements(PH, PW, dil, swap=False, sign=1, radius=0):
    """[(p, dy, dx)] of the patch.  swap: the patch taken as (PW, PH); sign -1: in2 read at -d; radius r: the centre
    taken r entries late on every axis longer than 1."""
    if swap:
        PH, PW = PW, PH
    out = []
    for ph in range(PH):
        for pw in range(PW):
            dy = (ph - PH // 2 - (radius if PH > 1 else 0)) * dil
            dx = (pw - PW // 2 - (radius if PW > 1 else 0)) * dil
            out.append((ph * PW + pw, sign * dy, sign * dx))
    return out


def _chan(C, drop_chunk):
    """Channels that take part: all, or all but the last 8-channel chunk."""
    return C if not drop_chunk else (C - 1) // 8 * 8


def corr_fwd(a, b, PH, PW, dil=1, swap=False, sign=1, radius=0, clamp=False, drop_chunk=False, term_round=None):
    """out[b,h,w,ph*PW+pw] = sum_c a[b,h,w,c] * b[b, h + (ph - PH/2) dil, w + (pw - PW/2) dil, c].
    term_round: a rounding (values -> values) applied to the running sum after every channel."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    B, H, W, C = a.shape
    n = _chan(C, drop_chunk)
    out = np.zeros((B, H, W, PH * PW))
    for p, dy, dx in displacements(PH, PW, dil, swap, sign, radius):
        t = a[..., :n] * shifted(b, dy, dx, clamp)[..., :n]
        if term_round is None:
            out[..., p] = t.sum(-1)
        else:
            acc = np.zeros((B, H, W))
            for c in range(n):
                acc = term_round(acc + t[..., c])
            out[..., p] = acc
    return out


def corr_fwd_abs(a, b, PH, PW, dil=1):
    """A = sum_c |a| |b| over the same terms."""
    return corr_fwd(np.abs(a), np.abs(b), PH, PW, dil)


def corr_bwd(a, b, g, PH, PW, dil=1, swap=False, sign=1, radius=0, clamp=False, drop_chunk=False, exchange=False, term_round=None):
    """gin1[x, c] = sum_p g[x, p] b[x + d(p), c];  gin2[x, c] = sum_p g[x - d(p), p] a[x - d(p), c], terms whose partner
    pixel lies outside the image absent.  drop_chunk: the last 8-channel chunk is left zero; exchange: the two results
    swapped; term_round: applied to the running sums after every displacement."""
    a, b, g = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(g, np.float64)
    B, H, W, C = a.shape
    g1, g2 = np.zeros_like(a), np.zeros_like(a)
    for p, dy, dx in displacements(PH, PW, dil, swap, sign, radius):
        gp = g[..., p:p + 1]
        g1 += gp * shifted(b, dy, dx, clamp)
        g2 += shifted(gp * a, -dy, -dx, clamp)
        if term_round is not None:
            g1, g2 = term_round(g1), term_round(g2)
    n = _chan(C, drop_chunk)
    g1[..., n:] = 0.0
    g2[..., n:] = 0.0
    return (g2, g1) if exchange else (g1, g2)


def corr_bwd_abs(a, b, g, PH, PW, dil=1):
    """(sum_p |g| |b|, sum_p |g| |a|) over the same terms."""
    return corr_bwd(np.abs(a), np.abs(b), np.abs(g), PH, PW, dil)
