"""sdhip_act_out_bwd: graw = gy * act'(y) * scale[g], the backward of a convolution whose FROZEN BatchNorm is folded into its
weight pack (`-freeze_bn 1`, torch_implementation.py:235-241): the derivative comes from the activation's OUTPUT.

CPU: the symbol is declared, exported and bound, and refuses bad arguments before any GPU work.
GPU: against f64 numpy on the grid C x rows x layout x groups x act x dtype below.  The destination is filled with NaN first:
the padding channels [C, ld) of every row must still hold it and every logical element must be finite.  ReLU positions with
y <= 0 (y = -0.0 included) are exactly 0.  Tolerances, relative per element: f32 is one chain of at most three f32 roundings
(y (1 - y) as one fma, times gy, times scale), bound 4 * 2^-24; bf16 is that f32 product rounded once to bf16 (2^-9) plus
the chain, bound 2^-8.  Which of the two code paths a case takes follows from the entry point's rule (C and the three pixel
strides multiples of a 16-byte chunk's elements, pointers 16-byte aligned); the grid is asserted to reach both."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (1, 3, 8, 19, 33, 64)
NPIX = (1, 7, 2 * (64 * 3 + 5))
ACTS = (0, 1, 2)
TOL = {torch.float32: 4 * 2.0 ** -24, torch.bfloat16: 2.0 ** -8}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_symbol_is_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sdhip_act_out_bwd\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sdhip_act_out_bwd")
    i, p, l = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert _lib.SIGNATURES["sdhip_act_out_bwd"] == [p, i, p, i, p, i, p, l, i, i, i, i, p]
    f = _lib._lib.sdhip_act_out_bwd
    a = ctypes.c_void_p(16)
    assert f(None, 8, a, 8, a, 8, a, 4, 8, 1, 1, 0, None) == _lib.ERR_ARG          # gy missing
    assert f(a, 8, a, 8, a, 8, None, 4, 8, 1, 1, 0, None) == _lib.ERR_ARG          # scale missing
    assert f(a, 7, a, 8, a, 8, a, 4, 8, 1, 1, 0, None) == _lib.ERR_ARG             # a pixel stride below C
    assert f(a, 8, a, 8, a, 8, a, 7, 8, 2, 1, 0, None) == _lib.ERR_ARG             # rows not divisible by the groups
    for act in (3, 4, 5, 6):                                                        # only none / ReLU / sigmoid have an output form
        assert f(a, 8, a, 8, a, 8, a, 4, 8, 1, act, 0, None) == _lib.ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- GPU
def _vec_rule(C, lds, ptrs, dtype):
    n = 4 if dtype == torch.float32 else 8
    return C % n == 0 and all(ld % n == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs)


def _rows(vals, ld, dtype, shift=0):
    """[n][C] values as rows of an [n][ld] device buffer whose padding holds NaN; shift: elements the base is moved by."""
    n, C = vals.shape
    buf = torch.full((n * ld + shift,), float("nan"), dtype=dtype, device="cuda")
    view = buf[shift:].view(n, ld)
    view[:, :C] = vals.to(dtype).cuda()
    return buf, view


def _case(C, n, G, act, dtype, lds, seed, shift=0):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    g = torch.Generator().manual_seed(seed)
    gy = torch.randn((n, C), generator=g).to(dtype)
    if act == 2:
        y = torch.sigmoid(2 * torch.randn((n, C), generator=g)).to(dtype)
    else:
        y = torch.randn((n, C), generator=g).to(dtype)
        flat = y.view(-1)
        flat[::5] = 0.0
        flat[1::7] = -0.0
    scale = (0.25 + 2 * torch.rand((G, C), generator=g)) * torch.where(torch.rand((G, C), generator=g) < 0.3, -1.0, 1.0)
    _, gv = _rows(gy, lds[0], dtype, shift)
    _, yv = _rows(y, lds[1], dtype, shift)
    out, ov = _rows(torch.full((n, C), float("nan")), lds[2], dtype, shift)
    sc = scale.cuda()
    vec = _vec_rule(C, lds, (gv.data_ptr(), yv.data_ptr(), ov.data_ptr()), dtype)
    _lib.call("sdhip_act_out_bwd", _lib.ptr(gv), lds[0], _lib.ptr(yv), lds[1], _lib.ptr(ov), lds[2], _lib.ptr(sc), n, C, G, act,
              _lib.BF16 if dtype == torch.bfloat16 else _lib.F32, _lib.stream_ptr())
    torch.cuda.synchronize()
    got = ov.float().cpu().numpy().astype(np.float64)
    what = (C, n, G, act, dtype, lds, shift)
    assert np.isfinite(got[:, :C]).all(), what
    assert np.isnan(got[:, C:]).all(), ("padding channels were written", what)
    assert bool(torch.isnan(out[:shift].float()).all())
    gy64, y64 = gy.double().numpy(), y.double().numpy()
    s64 = np.repeat(scale.double().numpy(), n // G, axis=0)
    d = {0: np.ones_like(y64), 1: (y64 > 0).astype(np.float64), 2: y64 * (1 - y64)}[act]
    want = gy64 * d * s64
    if act == 1:
        assert (got[:, :C][y64 <= 0] == 0).all(), what
        assert (y64 <= 0).any() or n * C < 5
    err = np.abs(got[:, :C] - want)
    assert (err <= TOL[dtype] * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))
    return vec


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("C", CS)
def test_act_out_bwd_matches_f64(C, padded, dtype):
    ld = (C + 7) & ~7
    lds = (ld, ld + 8, ld + 16) if padded else (C, C, C)
    paths = set()
    for npix in NPIX:
        # groups 1 over npix rows; groups 2 over npix rows per group, and over npix rows in all where that divides
        for G, n in [(1, npix), (2, 2 * npix)] + ([(2, npix)] if npix % 2 == 0 else []):
            for act in ACTS:
                paths.add(_case(C, n, G, act, dtype, lds, 1000 * C + 10 * n + act + G))
    chunk = 4 if dtype == torch.float32 else 8
    assert paths == {C % chunk == 0}, (paths, C, lds)      # strides of whole chunks in both layouts: C alone decides


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_both_paths_are_reached_and_a_misaligned_base_takes_the_scalar_one(dtype):
    """C = 8 / 64 with chunk strides take the 16-byte path, C = 19 / 33 never do, and the same C = 64 rows from a base moved by
    one element must not be read 16 bytes at a time (the rule includes the pointers)."""
    assert _case(64, 394, 2, 1, dtype, (64, 72, 80), 5) is True
    assert _case(8, 7, 1, 2, dtype, (8, 8, 8), 6) is True
    assert _case(19, 394, 2, 1, dtype, (24, 32, 40), 7) is False
    assert _case(64, 394, 2, 2, dtype, (64, 72, 80), 8, shift=1) is False
    assert _case(64, 394, 1, 1, dtype, (65, 72, 80), 9) is False      # one odd stride
