"""The three operators of the Ext_small edge networks (csrc/edge.hip: ops.grad_mag, ops.edge_loss, ops.gate_pair) against
fixtures made by the reference's own compute_grad_mag / lossEdge_fn (tests/golden/ext_small.npz, tools/make_golden_ext_small.py)
and against the closed forms of include/sdhip.h, restated here in plain torch in f64.

Bars.  grad_mag, f32: every element within 10 * gradmag.dev of the f64 closed form (gradmag.dev: the worst deviation of the
reference's own f32 run from it, 6.5e-8); bf16 output: 2^-8 * |want| on top (one rounding of an f32 result to bf16).
edge_loss, f32: value within bar * |want| + 1e-12, every gradient element within bar * max|want|, bar = 1e-5 unless ten times
the stored deviation of the reference's f32 run is larger (the generator found 1.2e-7 at worst, so no case is); bf16 logits: the
closed form on the bf16-rounded logits is the reference, the value meets the f32 bar, every gradient element lies within
2^-8 * |want| + 1e-5 * max|want| (tests/test_dispsmooth.py's rule).  gate_pair: torch autograd in f64 on the CPU is the
reference; the bar is ten times the worst deviation, relative to each tensor's largest element, of the same composition run in
f32 on the CPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.detweights import rand_input, randn_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 83                 # tools/make_golden_ext_small.py
BAR = 1e-5
_fix = {}


def _golden():
    if not _fix:
        z = np.load(os.path.join(ROOT, "tests", "golden", "ext_small.npz"))
        _fix.update({k: z[k] for k in z.files if not k.startswith("net.")})
        _fix["cases"] = json.loads(str(_fix["cases"]))
    return _fix


GM_CASES = {"tiny": (1, 1, 2, 2), "odd": (2, 3, 7, 9), "four": (2, 4, 5, 8), "big": (1, 3, 67, 131)}
EB_CASES = {"small": (2, 7, 9, "randn"), "p10": (2, 67, 131, "randn"), "mixed": (2, 7, 9, "randn"), "nopos": (2, 7, 9, "randn"),
            "allpos": (2, 7, 9, "randn"), "big80": (2, 67, 131, "pm80")}


def grad_mag_closed(E):
    """sqrt(Ox^2 + Oy^2 + 1e-6) of the zero-padded central differences, in f64."""
    P = F.pad(E.cpu().double(), (1, 1, 1, 1))
    ox = 0.5 * (P[:, :, 1:-1, 2:] - P[:, :, 1:-1, :-2])
    oy = 0.5 * (P[:, :, 2:, 1:-1] - P[:, :, :-2, 1:-1])
    return torch.sqrt(ox * ox + oy * oy + 1e-6)


def edge_closed(z, t):
    """(value, gradient) of lossEdge_fn in f64; the two weights are f32 quotients, as the reference's are."""
    z, t = z.detach().cpu().double(), t.cpu().double()
    pos, neg = int((t == 1).sum()), int((t == 0).sum())
    tot = pos + neg
    wp = float(np.float32(neg) / np.float32(tot)) if tot else 0.0
    wn = float(np.float32(pos) / np.float32(tot)) if tot else 0.0
    w = torch.where(t == 1, torch.full_like(t, wp), torch.where(t == 0, torch.full_like(t, wn), torch.zeros_like(t)))
    bce = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    n = z.numel()
    return float((w * bce).sum() / n), w * (torch.sigmoid(z) - t) / n


_inputs = {}


def _gm_case(name):
    if ("gm", name) not in _inputs:
        _inputs[("gm", name)] = rand_input(SEED, "gm:" + name, GM_CASES[name])
    return _inputs[("gm", name)]


def _eb_case(name):
    """(logits, target, want value, want gradient, bar) of a fixture case, CPU tensors; built once and left unchanged."""
    if ("eb", name) not in _inputs:
        g = _golden()
        B, H, W, zk = EB_CASES[name]
        shape = (B, 1, H, W)
        if zk == "pm80":
            z = torch.where(rand_input(SEED, "eb:%s:z" % name, shape) > 0.5, torch.tensor(80.0), torch.tensor(-80.0))
        else:
            z = randn_input(SEED, "eb:%s:z" % name, shape, 3.0)
        bar = max(BAR, 10 * float(g["edge.%s.dev" % name]))
        _inputs[("eb", name)] = (z, torch.from_numpy(g["edge.%s.target" % name]), float(g["edge.%s.value" % name]),
                                 torch.from_numpy(g["edge.%s.grad" % name]), bar)
    return _inputs[("eb", name)]


# ---------------------------------------------------------------------------------------------------- no GPU needed

@pytest.mark.parametrize("name", sorted(GM_CASES))
def test_grad_mag_closed_form_reproduces_the_reference(name):
    want = torch.from_numpy(_golden()["gradmag.%s.out" % name]).double()
    got = grad_mag_closed(_gm_case(name))
    rel = float(((got - want).abs() / want.abs()).max())
    print("%s: worst relative deviation %.2e" % (name, rel))
    assert tuple(want.shape) == GM_CASES[name] and rel <= 1e-6


@pytest.mark.parametrize("name", sorted(EB_CASES))
def test_edge_closed_form_reproduces_the_reference(name):
    z, t, want, wgrad, _ = _eb_case(name)
    value, grad = edge_closed(z, t)
    gmax = float(wgrad.abs().max())
    err = float((grad - wgrad.double()).abs().max())
    print("%s: value %.8e vs %.8e, grad err %.2e of max %.3e" % (name, value, want, err, gmax))
    assert abs(value - want) <= 1e-6 * abs(want)
    assert err <= 1e-6 * gmax


def test_fixture_covers_what_it_claims():
    g = _golden()
    assert [list(c) for c in g["cases"]["gradmag"]] == [[k] + list(v) for k, v in GM_CASES.items()]
    assert sorted(c[0] for c in g["cases"]["edge"]) == sorted(EB_CASES)
    assert float(g["gradmag.dev"]) == max(float(g["gradmag.%s.dev" % k]) for k in GM_CASES)
    assert 0 < float(g["gradmag.dev"]) <= 2.0 ** -23            # values below 1: one ulp of the reference's f32 result
    for name in EB_CASES:
        assert float(g["edge.%s.dev" % name]) <= BAR / 10
    for name in ("nopos", "allpos"):
        assert float(g["edge.%s.value" % name]) == 0.0 and not g["edge.%s.grad" % name].any()
    assert not g["edge.nopos.target"].any() and bool((g["edge.allpos.target"] == 1).all())
    t = g["edge.p10.target"]
    assert 0.05 < float((t == 1).mean()) < 0.15 and bool(((t == 0) | (t == 1)).all())
    t = g["edge.mixed.target"]
    assert all(bool((t == v).any()) for v in (0.0, 1.0, 0.5, 2.0))
    assert not g["edge.mixed.grad"][(t != 0) & (t != 1)].any() and g["edge.mixed.grad"].any()
    assert bool(np.isfinite(g["edge.big80.grad"]).all()) and np.isfinite(float(g["edge.big80.value"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ext_small.npz")) < 1 << 20


def test_symbols_are_declared_exported_and_bound():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    text = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    want = {"sdhip_grad_mag": [p, l, l, l, i, p, i, i, i, i, i, i, p],
            "sdhip_edge_bce_workspace_bytes": [l],
            "sdhip_edge_bce": [p, l, i, p, p, p, l, p, l, p],
            "sdhip_gate_pair_fwd": [p, i, p, i, p, i, p, i, l, i, i, p],
            "sdhip_gate_pair_bwd": [p, i, p, i, p, i, p, i, p, i, p, i, p, i, l, i, i, p]}
    for name, sig in want.items():
        assert " %s(" % name in text and hasattr(_lib._lib, name), name
        assert _lib.SIGNATURES[name] == sig, name
        assert getattr(_lib._lib, name).restype is (ctypes.c_long if name.endswith("_bytes") else ctypes.c_int)
    # one pair of integer counts and one f64 partial per 4096-element tile, 1024 tiles at most
    assert _lib.edge_bce_workspace_bytes(1) == 24 and _lib.edge_bce_workspace_bytes(4096) == 24
    assert _lib.edge_bce_workspace_bytes(4097) == 48 and _lib.edge_bce_workspace_bytes(1 << 30) == 1024 * 24
    assert _lib._lib.sdhip_edge_bce_workspace_bytes(0) < 0 and _lib._lib.sdhip_edge_bce_workspace_bytes((1 << 40) + 1) < 0


def _refused(fn, ok, changes):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    for change, word in changes:
        k = dict(ok, **change)
        rc = fn(*k.values(), None)
        assert rc == _lib.ERR_ARG and word in _lib._lib.sdhip_last_error(), (change, rc, _lib._lib.sdhip_last_error())


def test_error_codes_without_a_gpu():
    """Argument validation happens before any GPU work: error code and message, nothing aborts."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    L = _lib._lib
    _refused(L.sdhip_grad_mag, dict(img=a, bs=48, cs=16, ps=1, idt=_lib.F32, out=a, ldy=3, odt=_lib.F32, B=1, H=4, W=4, C=3),
             ((dict(img=None), b"null"), (dict(out=None), b"null"), (dict(C=0), b"C 0"), (dict(C=5, ldy=8), b"C 5"), (dict(H=1), b"H 1"),
              (dict(W=1), b"W 1"), (dict(B=0), b"B 0"), (dict(ps=0), b"strides"), (dict(cs=0), b"strides"), (dict(bs=-1), b"strides"),
              (dict(ldy=2), b"stride"), (dict(idt=7), b"dtype"), (dict(odt=7), b"dtype")))
    _refused(L.sdhip_edge_bce, dict(z=a, ldz=1, dt=_lib.F32, t=a, g=a, loss=a, n=16, ws=a, wsb=24),
             ((dict(z=None), b"null"), (dict(t=None), b"null"), (dict(g=None), b"null"), (dict(loss=None), b"null"), (dict(ws=None), b"null"),
              (dict(n=0), b"n 0"), (dict(ldz=0), b"stride"), (dict(dt=7), b"dtype"), (dict(wsb=23), b"workspace"),
              (dict(n=4097, wsb=24), b"workspace"), (dict(ws=a + 4), b"workspace")))
    _refused(L.sdhip_gate_pair_fwd, dict(a=a, lda=8, b=a, ldb=8, g=a, ldg=1, y=a, ldy=16, npix=2, C=8, dt=_lib.F32),
             ((dict(a=None), b"null"), (dict(b=None), b"null"), (dict(g=None), b"null"), (dict(y=None), b"null"), (dict(C=0), b"C 0"),
              (dict(npix=0), b"npix 0"), (dict(lda=7), b"strides"), (dict(ldb=7), b"strides"), (dict(ldg=0), b"strides"),
              (dict(ldy=15), b"strides"), (dict(dt=7), b"dtype")))
    _refused(L.sdhip_gate_pair_bwd, dict(gy=a, ldgy=16, a=a, lda=8, b=a, ldb=8, g=a, ldg=1, ga=a, ldga=8, gb=a, ldgb=8, gg=a, ldgg=1,
                                         npix=2, C=8, dt=_lib.F32),
             ((dict(gy=None), b"null"), (dict(ga=None), b"null"), (dict(gb=None), b"null"), (dict(gg=None), b"null"), (dict(C=0), b"C 0"),
              (dict(npix=0), b"npix 0"), (dict(ldgy=15), b"strides"), (dict(ldga=7), b"strides"), (dict(ldgg=0), b"strides"),
              (dict(dt=7), b"dtype")))


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, SdhipError
    img = torch.zeros(1, 3, 4, 5)
    for a in ((img,), (img[0],), (torch.zeros(1, 5, 4, 5),), (torch.zeros(1, 3, 1, 5),), (torch.zeros(1, 3, 4, 1),), (img, torch.float16)):
        with pytest.raises(SdhipError):
            ops.grad_mag(*a)
    z, t = torch.zeros(2, 1, 4, 5), torch.zeros(2, 1, 4, 5)
    for a in ((z, t), (torch.zeros(2, 2, 4, 5), torch.zeros(2, 2, 4, 5)), (z, t[:, :, :3]), (z[0], t[0]), (z, t.double()),
              (z, torch.zeros(2, 1, 5, 4).transpose(2, 3))):
        with pytest.raises(SdhipError):
            ops.edge_loss(*a)
    x, g = torch.zeros(2, 8, 4, 5), torch.zeros(2, 1, 4, 5)
    for a in ((x, x, g), (x, x[:, :4], g), (x, x, x), (x, x, g[:1]), (x[0], x[0], g[0]), (x, x.bfloat16(), g)):
        with pytest.raises(SdhipError):
            ops.gate_pair(*a)
    seg, d = torch.zeros(2, 3, 4, 5), torch.zeros(2, 1, 4, 5)
    for a in ((z, d, seg, seg, d), (z, d, seg, seg[:, :2], d), (z, seg, seg, seg, d), (z, d, seg, seg, d[:, :, :2]),
              (z, d, seg, seg, d, t[:, :, :2]), (z[:, :, :2], d, seg, seg, d, t)):
        with pytest.raises(SdhipError):
            ops.edge_step_loss(*a)


# ---------------------------------------------------------------------------------------------------- on the GPU

def _layouts(E):
    """The same image as NCHW, channels-last and (three channels) a slice of a 4-channel image of either layout."""
    x = E.cuda()
    outs = [("nchw", x), ("channels_last", x.contiguous(memory_format=torch.channels_last))]
    if E.shape[1] == 3:
        four = torch.cat([x, torch.full_like(x[:, :1], 7.0)], 1)
        outs += [("slice of nchw", four[:, :3]), ("slice of channels_last", four.contiguous(memory_format=torch.channels_last)[:, :3])]
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GM_CASES))
def test_grad_mag_f32(name):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    g = _golden()
    E = _gm_case(name)
    want = grad_mag_closed(E)
    bar = 10 * float(g["gradmag.dev"])
    base = None
    for tag, x in _layouts(E):
        out = ops.grad_mag(x)
        B, C, H, W = E.shape
        ld = (C + 7) & ~7
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, C, H, W) and out.stride() == (H * W * ld, 1, W * ld, ld)
        got = out.cpu()
        err = float((got.double() - want).abs().max())
        print("%s %s: worst error %.2e (bar %.2e), against the reference's own run %.2e"
              % (name, tag, err, bar, float((got - torch.from_numpy(g["gradmag.%s.out" % name])).abs().max())))
        assert err <= bar
        base = got if base is None else base
        assert torch.equal(got, base), tag
    # a bf16 image: the differences of bf16 values are exact in f32, the closed form on the rounded image is the reference
    Eb = E.bfloat16()
    got = ops.grad_mag(Eb.cuda(), dtype=torch.float32).cpu()
    err = float((got.double() - grad_mag_closed(Eb.float())).abs().max())
    print("%s bf16 image: worst error %.2e" % (name, err))
    assert err <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GM_CASES))
def test_grad_mag_bf16_output(name):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    E = _gm_case(name)
    want = grad_mag_closed(E)
    bar = 10 * float(_golden()["gradmag.dev"])
    base = None
    for tag, x in _layouts(E):
        out = ops.grad_mag(x, dtype=torch.bfloat16)
        assert out.dtype == torch.bfloat16 and out.stride(1) == 1 and out.stride(3) == 8
        got = out.cpu()
        err = (got.double() - want).abs()
        print("%s %s bf16: worst error %.2e" % (name, tag, float(err.max())))
        assert bool((err <= 2.0 ** -8 * want.abs() + bar).all())
        base = got if base is None else base
        assert torch.equal(got, base), tag
    with pytest.raises(Exception):
        ops.grad_mag(E.cuda().requires_grad_(True))


def _padded(z, ld=8):
    """The logits as channel 0 of a (B,H,W,ld) buffer whose other channels hold junk: a head's output in a padded pixel."""
    B, _, H, W = z.shape
    buf = torch.full((B, H, W, ld), 7.0, dtype=z.dtype, device="cuda")
    buf[..., 0] = z.cuda()[:, 0]
    return buf[..., :1].permute(0, 3, 1, 2)


def _run_edge(z, t):
    """(value as a Python float of the f32 scalar, gradient w.r.t. z on the CPU) of ops.edge_loss on the GPU."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    zz = (z if z.is_cuda else z.cuda()).detach().requires_grad_(True)
    loss = ops.edge_loss(zz, t.cuda())
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    assert zz.grad.dtype == zz.dtype and zz.grad.shape == zz.shape
    return float(loss.detach()), zz.grad.detach().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EB_CASES))
def test_edge_loss_f32(name):
    z, t, want, wgrad, bar = _eb_case(name)
    got, grad = _run_edge(z, t)
    gmax = float(wgrad.abs().max())
    err = float((grad - wgrad).abs().max())
    print("%s: value %.8e vs %.8e (rel %.2e), grad err %.2e of max %.3e" % (name, got, want, abs(got - want) / max(abs(want), 1e-300), err, gmax))
    assert abs(got - want) <= bar * abs(want) + 1e-12
    assert err <= bar * gmax
    assert np.isfinite(got) and bool(torch.isfinite(grad).all())
    if name in ("nopos", "allpos"):
        assert got == 0.0 and not grad.any()
    if name == "mixed":
        assert not grad[(t != 0) & (t != 1)].any()
    # the same bits from a second call and from logits that sit in a padded pixel stride
    again = _run_edge(z, t)
    assert again[0] == got and torch.equal(again[1], grad)
    pad = _run_edge(_padded(z), t)
    assert pad[0] == got and torch.equal(pad[1], grad)


@pytest.mark.gpu
def test_edge_loss_single_element():
    """(1,1,1,1): the reference's numpy indexing fails on this shape, the closed form says 0 for a lone class and the kernel
    must not read past its one element."""
    for tv in (1.0, 0.0, 0.5):
        z, t = torch.tensor([[[[1.5]]]]), torch.tensor([[[[tv]]]])
        want, wgrad = edge_closed(z, t)
        for zz in (z, _padded(z)):
            got, grad = _run_edge(zz, t)
            assert want == 0.0 and got == 0.0 and not grad.any() and not wgrad.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "p10", "mixed", "big80"])
def test_edge_loss_bf16_logits(name):
    z, t, _, _, bar = _eb_case(name)
    zb = z.bfloat16()
    want, wgrad = edge_closed(zb.float(), t)
    for zz in (zb, _padded(zb)):
        got, grad = _run_edge(zz, t)
        assert grad.dtype == torch.bfloat16
        gmax = float(wgrad.abs().max())
        err = (grad.double() - wgrad).abs()
        print("%s bf16: value %.8e vs %.8e, worst grad err %.2e of max %.3e" % (name, got, want, float(err.max()), gmax))
        assert abs(got - want) <= bar * abs(want) + 1e-12
        assert bool((err <= 2.0 ** -8 * wgrad.abs() + 1e-5 * gmax).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (1, 19, 3, 5)])
def test_gate_pair_matches_autograd(shape):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(11)
    a, b = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    g = torch.rand((B, 1, H, W), generator=gen)
    gy = torch.randn((B, 2 * C, H, W), generator=gen)

    def compose(dt):
        xs = [v.to(dt).clone().requires_grad_(True) for v in (a, b, g)]
        y = torch.cat((xs[0] * xs[2], xs[1] * (1 - xs[2])), 1)
        y.backward(gy.to(dt))
        return [y.detach()] + [v.grad for v in xs]
    want, f32 = compose(torch.float64), compose(torch.float32)
    dev = max(float((s.double() - w).abs().max() / w.abs().max()) for s, w in zip(f32, want))
    xs = [v.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for v in (a, b, g)]
    y = ops.gate_pair(*xs)
    assert tuple(y.shape) == (B, 2 * C, H, W) and y.stride(1) == 1
    if C % 4 == 0:
        assert y.is_contiguous(memory_format=torch.channels_last)
    lo, hi = y[:, :C], y[:, C:]
    assert lo.untyped_storage().data_ptr() == hi.untyped_storage().data_ptr() == y.untyped_storage().data_ptr()   # one buffer, two halves
    y.backward(gy.cuda())
    got = [y.detach().cpu()] + [v.grad.cpu() for v in xs]
    for name, s, w in zip(("y", "ga", "gb", "gg"), got, want):
        err = float((s.double() - w).abs().max() / w.abs().max())
        print("%s %s: error %.2e of the largest element (f32 composition on the CPU: %.2e)" % (shape, name, err, dev))
        assert s.shape == w.shape and err <= 10 * dev


@pytest.mark.gpu
def test_gate_pair_bf16_and_strided_inputs():
    """bf16 takes the 16-byte path at C = 64 and the element path at C = 19; inputs that are channel slices of wider slabs."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    gen = torch.Generator().manual_seed(12)
    for C in (64, 19):
        B, H, W = 2, 5, 7
        slab = torch.randn((B, H, W, 2 * C + 8), generator=gen).bfloat16().cuda()
        a, b = slab[..., :C].permute(0, 3, 1, 2), slab[..., C:2 * C].permute(0, 3, 1, 2)
        g = torch.rand((B, 1, H, W), generator=gen).bfloat16().cuda()
        gy = torch.randn((B, 2 * C, H, W), generator=gen).bfloat16().cuda()
        xs = [v.detach().requires_grad_(True) for v in (a, b, g)]
        y = ops.gate_pair(*xs)
        y.backward(gy)
        ref = [v.detach().double().cpu().requires_grad_(True) for v in (a, b, g)]
        yr = torch.cat((ref[0] * ref[2], ref[1] * (1 - ref[2])), 1)
        yr.backward(gy.double().cpu())
        for name, s, w in zip(("y", "ga", "gb", "gg"), [y.detach()] + [v.grad for v in xs], [yr.detach()] + [v.grad for v in ref]):
            err = (s.double().cpu() - w).abs()
            # one rounding of an f32 result to bf16, plus the f32 sum's own error on gg
            assert s.dtype == torch.bfloat16 and bool((err <= 2.0 ** -8 * w.abs() + 1e-5 * float(w.abs().max())).all()), (C, name, float(err.max()))
