"""SGD with momentum (`-optimType sgd`, torch_implementation.py:715-716), its device-resident learning rate, the poly
schedule (torch_implementation.py:599-608), `TrainStep.flush` and the torch.optim.SGD checkpoint layout.

No test compares a training trajectory through the network: the kernel is checked against torch.optim.SGD in f64 on its own
buffers, and the step's plumbing against that formula applied to the gradient the step itself left in `flat_g`.

The tolerance of every comparison with the formula is derived, not tuned: after step s, elementwise on p and on buf,
16 * s * 2^-24 * max(1, max|p_ref|, max|buf_ref|) - six f32 roundings per step (g*scale, wd*p, their sum, momentum*buf, its
sum, lr*buf and the subtraction, some of them fused) with a margin; torch.optim.SGD in f32 stays 35x or more inside it.
The learning rate and the weight decay of these tests are large on purpose: every term of the update then moves p far more
than the tolerance, so a dropped term cannot hide (with the reference's 1e-4 it could).
"""
import ctypes
import json
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from oracle import ref_models as R
from oracle.detweights import fill_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pmt_learning_for_semantic_segmentation_and_disparity_amd")
ULP = 2.0 ** -24
MOMENTUM, WD = 0.9, 0.05


def _tol(s, *refs):
    return 16 * s * ULP * max(1.0, *[float(r.abs().max()) for r in refs])


def _formula(p, buf, g, lr, grad_scale, momentum=MOMENTUM, wd=WD):
    """torch.optim.SGD's update (dampening 0, no Nesterov) in f64; returns (p, buf)."""
    d = g.double() * grad_scale + wd * p.double()
    buf = momentum * buf.double() + d
    return p.double() - lr * buf, buf


def _close(got, want, tol):
    err = float((got.double().cpu() - want.cpu()).abs().max())
    assert err <= tol, (err, tol)
    return err


# ------------------------------------------------------------------ CPU
def test_poly_lr_pins():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import poly_lr
    assert poly_lr(3, 0, 40) == 0.00499375
    assert abs(poly_lr(3, 1, 40) - 0.004993697916666667) <= 1e-18
    assert abs(poly_lr(2400, 5, 40) - 0.005 / 96000) <= 1e-18 and abs(poly_lr(3000, 0, 40) - 0.005 / 96000) <= 1e-18
    assert poly_lr(0, 0, 40) == 0.005 and poly_lr(1, 0, 10, base_lr=1.0, epoch_total=2) == 0.5


class _Tiny(torch.nn.Module):
    """Shapes with numel not divisible by 4 exercise the 16-byte aligned slices of the flat buffer."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 5, 3)
        self.bn = torch.nn.BatchNorm2d(5)
        self.b = torch.nn.Linear(7, 3)


def _fake_step(model, optimizer="sgd"):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import flatten_parameters
    flat_p, flat_g = flatten_parameters(model)
    if optimizer == "sgd":
        return types.SimpleNamespace(model=model, flat_p=flat_p, flat_g=flat_g, optimizer="sgd", momentum_buf=torch.zeros_like(flat_p),
                                     steps_done=0, lr=0.005, momentum=0.9, weight_decay=1e-4)
    return types.SimpleNamespace(model=model, flat_p=flat_p, flat_g=flat_g, exp_avg=torch.zeros_like(flat_p),
                                 exp_avg_sq=torch.zeros_like(flat_p), beta_pow=torch.ones(2), steps_done=0,
                                 lr=0.0015, betas=(0.9, 0.999), eps=1e-7)


def _torch_sgd_run(steps=3, idle=(), **kw):
    """A net torch.optim.SGD has stepped `steps` times; the parameters at the positions `idle` never had a gradient."""
    torch.manual_seed(1)
    net = _Tiny()
    opt = torch.optim.SGD(net.parameters(), **dict(dict(lr=0.005, momentum=0.9, weight_decay=1e-4), **kw))
    for _ in range(steps):
        for i, p in enumerate(net.parameters()):
            p.grad = None if i in idle else torch.randn_like(p)
        opt.step()
    return net, opt


def test_saved_state_loads_in_torch_sgd():
    """make_state of an SGD step is what torch.optim.SGD.load_state_dict accepts, and the optimizer that loaded it continues
    bit-identically to the one that produced the buffers."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as C
    net, opt = _torch_sgd_run()
    step = _fake_step(_Tiny())
    C.load_model_state(step.model, net.state_dict())
    C.load_optimizer_state(step, opt.state_dict())
    assert step.steps_done == 0                                        # torch.optim.SGD's state holds no step count
    step.steps_done = 3
    state = C.make_state(step, epoch=1)
    group = state["optimizer"]["param_groups"][0]
    assert group == {"lr": 0.005, "momentum": 0.9, "dampening": 0, "weight_decay": 1e-4, "nesterov": False, "maximize": False,
                     "foreach": None, "differentiable": False, "fused": None, "params": list(range(6))}
    assert all(set(v) == {"momentum_buffer"} for v in state["optimizer"]["state"].values()) and len(state["optimizer"]["state"]) == 6
    wrapped = torch.nn.Sequential()
    wrapped.add_module("module", _Tiny())                              # the DDP wrapper's naming
    wrapped.load_state_dict(state["state_dict"])
    opt2 = torch.optim.SGD(wrapped.parameters(), lr=1.0)
    opt2.load_state_dict(state["optimizer"])
    assert opt2.param_groups[0]["lr"] == 0.005 and opt2.param_groups[0]["momentum"] == 0.9 and opt2.param_groups[0]["weight_decay"] == 1e-4
    for p, q in zip(net.parameters(), wrapped.parameters()):
        g = torch.randn_like(p)
        p.grad, q.grad = g, g.clone()
    opt.step()
    opt2.step()
    for p, q in zip(net.parameters(), wrapped.parameters()):
        assert torch.equal(p, q)


def test_torch_sgd_state_loads_into_the_flat_buffer():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as C
    idle = 4                                                           # b.weight: never had a gradient
    net, opt = _torch_sgd_run(idle=(idle,))
    sd = opt.state_dict()
    assert idle not in sd["state"] and len(sd["state"]) == 5
    step = _fake_step(_Tiny())
    step.momentum_buf.fill_(7.0)                                       # whatever was there is replaced
    C.load_optimizer_state(step, sd)
    off = 0
    for i, p in enumerate(step.model.parameters()):
        n = p.numel()
        pad = ((n + 3) // 4) * 4
        if i == idle:
            assert not step.momentum_buf[off:off + pad].any()
        else:
            assert torch.equal(step.momentum_buf[off:off + n].view(p.shape), sd["state"][i]["momentum_buffer"])
            assert not step.momentum_buf[off + n:off + pad].any()      # the padding of the slice
        off += pad
    assert (step.lr, step.momentum, step.weight_decay) == (0.005, 0.9, 1e-4)
    step.steps_done, step.grad_free = 3, [idle]
    again = C.optimizer_state_dict(step)
    assert sorted(again["state"]) == [0, 1, 2, 3, 5]
    for i in again["state"]:
        assert torch.equal(again["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    step.steps_done = 0
    assert C.optimizer_state_dict(step)["state"] == {}                 # torch: no state before the first step
    # a None buffer (torch writes one for a parameter group with momentum 0) reads as zeros
    sd["state"][0]["momentum_buffer"] = None
    C.load_optimizer_state(step, sd)
    assert not step.momentum_buf[:((step.model.a.weight.numel() + 3) // 4) * 4].any()


def test_optimizer_kinds_do_not_mix():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as C
    _, sgd = _torch_sgd_run()
    net = _Tiny()
    adam = torch.optim.Adam(net.parameters(), lr=0.0015, eps=1e-7)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    adam.step()
    with pytest.raises(ValueError, match="Adam"):
        C.load_optimizer_state(_fake_step(_Tiny(), "sgd"), adam.state_dict())
    with pytest.raises(ValueError, match="SGD"):
        C.load_optimizer_state(_fake_step(_Tiny(), "adam"), sgd.state_dict())
    C.load_optimizer_state(_fake_step(_Tiny(), "adam"), adam.state_dict())     # a step without `optimizer` is an Adam step
    for kw in (dict(nesterov=True), dict(dampening=0.1), dict(maximize=True)):
        _, opt = _torch_sgd_run(steps=1, **kw)
        with pytest.raises(ValueError, match="nesterov"):
            C.load_optimizer_state(_fake_step(_Tiny(), "sgd"), opt.state_dict())


def test_sgd_step_signature():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    table = {"p": ctypes.c_void_p, "l": ctypes.c_long, "f": ctypes.c_float}
    assert _lib.SIGNATURES["sdhip_sgd_step"] == [table[c] for c in "p p p p l f f f p l p".split()]
    assert _lib._lib.sdhip_sgd_step.restype is ctypes.c_int


def test_live_ranges_are_the_complement_of_the_idle_slices():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import live_ranges
    m = _Tiny()                       # numel 135, 5, 5, 5, 21, 3 -> slices of 136, 8, 8, 8, 24, 4
    assert live_ranges(m, []) == [[0, 188]]
    assert live_ranges(m, [0]) == [[136, 188]] and live_ranges(m, [5]) == [[0, 184]]
    assert live_ranges(m, [1, 2, 4]) == [[0, 136], [152, 160], [184, 188]]
    assert live_ranges(m, range(6)) == []


def test_argument_checks_under_host_sanitizers(tmp_path):
    """sdhip_sgd_step refuses NULL pointers, misaligned buffers and n_live < 0 with SDHIP_ERR_ARG and a message before it
    launches anything: a stand-alone program (tests/host_sgd_args.cpp, its own main) linked with the two translation units
    it needs, host code under AddressSanitizer + UBSan.  It runs without a GPU."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "host_sgd_args")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
           os.path.join(PKG, "csrc", "optim_loss.hip"), os.path.join(PKG, "csrc", "runtime.hip"),
           "-x", "hip", os.path.join(ROOT, "tests", "host_sgd_args.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
    assert r.stdout.count("rc -1") == 11


# ------------------------------------------------------------------ GPU: the kernel
def _sgd_call(p, g, buf, lr_dev, grad_scale, live=None):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    call("sdhip_sgd_step", ptr(p), ptr(g), ptr(buf), ptr(lr_dev), p.numel(), MOMENTUM, WD, grad_scale,
         ptr(live), 0 if live is None else live.shape[0], stream_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4099, 3])
def test_sgd_kernel_matches_torch_sgd_in_f64(n):
    """5 steps, fresh gradients 3*randn, a different rate in the device scalar before each step; the reference is
    torch.optim.SGD on f64 CPU tensors (checked here to be the written-out formula)."""
    gen = torch.Generator().manual_seed(11 + n)
    p0 = torch.randn(n, generator=gen)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=0.1, momentum=MOMENTUM, weight_decay=WD)
    fp, fbuf = p0.double(), torch.zeros(n, dtype=torch.float64)
    p, buf = p0.cuda(), torch.zeros(n, device="cuda")
    lr_dev = torch.zeros(1, device="cuda")
    for s in range(1, 6):
        lr = 0.1 * 0.7 ** (s - 1)
        g = 3 * torch.randn(n, generator=gen)
        opt.param_groups[0]["lr"] = lr
        ref.grad = g.double() * 0.5
        opt.step()
        fp, fbuf = _formula(fp, fbuf, g, lr, 0.5)
        p_ref, buf_ref = ref.detach(), opt.state[ref]["momentum_buffer"]
        assert float((fp - p_ref).abs().max()) <= 1e-12 and float((fbuf - buf_ref).abs().max()) <= 1e-12
        lr_dev.fill_(lr)
        _sgd_call(p, g.cuda(), buf, lr_dev, 0.5)
        tol = _tol(s, p_ref, buf_ref)
        e = (_close(p, p_ref, tol), _close(buf, buf_ref, tol))
        print("n %d step %d: |p err| %.3g |buf err| %.3g tol %.3g" % (n, s, e[0], e[1], tol))


def _rows(case):
    if case == "four":
        return [[0, 8], [12, 1028], [2048, 2052], [4096, 8200]]
    return [[8 * k, 8 * k + 4] for k in range(300)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["four", "stride8"])
def test_sgd_kernel_steps_only_the_live_rows(case):
    n, rows = 8200, _rows(case)
    gen = torch.Generator().manual_seed(5)
    p0, b0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)      # a non-zero buffer: an untouched one must keep it
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e in rows:
        inside[b:e] = True
    live = torch.tensor(rows, dtype=torch.int64, device="cuda")
    lr_dev = torch.zeros(1, device="cuda")
    for table in (live, None):
        p, buf = p0.cuda(), b0.cuda()
        fp, fbuf = p0.double(), b0.double()
        for s in (1, 2):
            lr = 0.1 / s
            g = 3 * torch.randn(n, generator=gen)
            lr_dev.fill_(lr)
            _sgd_call(p, g.cuda(), buf, lr_dev, 0.5, table)
            np_, nb_ = _formula(fp, fbuf, g, lr, 0.5)
            if table is not None:
                np_, nb_ = torch.where(inside, np_, fp), torch.where(inside, nb_, fbuf)
            fp, fbuf = np_, nb_
            tol = _tol(s, fp, fbuf)
            _close(p, fp, tol)
            _close(buf, fbuf, tol)
        if table is not None:
            assert torch.equal(p.cpu()[~inside], p0[~inside]) and torch.equal(buf.cpu()[~inside], b0[~inside])
            assert not torch.equal(p.cpu()[inside], p0[inside])
        else:
            assert bool(((p.cpu() != p0) | (buf.cpu() != b0)).all())                 # a NULL table updates everything


# ------------------------------------------------------------------ GPU: TrainStep
def _model():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    torch.manual_seed(0)
    return fill_state_dict(N.minidsnetExt(R.CFG(), labels=2, patch_type='1dcorr'), 5).cuda().train()


def _warp_model():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N, warp
    k = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "warp.npz"))["keys"]))["div_1d"]
    torch.manual_seed(0)
    m = getattr(warp, k["cls"])(N.CFG(**k["cfg"]), labels=k["labels"], pretrained=False, patch_type=k["patch"],
                                include_edges=k["edges"], backbone=k["backbone"])
    return fill_state_dict(m, 5).cuda().train()


def _sgd_step(model=None, **kw):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    kw = dict(dict(dtype=torch.float32, use_graph=False, optimizer="sgd", lr=0.05, weight_decay=WD), **kw)
    return TrainStep(model if model is not None else _model(), **kw)


def _live_mask(ts):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import live_ranges
    mask = torch.zeros(ts.flat_p.numel(), dtype=torch.bool, device=ts.flat_p.device)
    for b, e in live_ranges(ts.model, ts.grad_free or ()):
        mask[b:e] = True
    return mask


@pytest.mark.gpu
def test_constructor_defaults_and_refusals():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import SdhipError
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep
    mk = lambda: torch.nn.Conv2d(3, 5, 3).cuda()
    a = TrainStep(mk(), use_graph=False)
    assert (a.optimizer, a.lr, a.weight_decay) == ("adam", 0.0015, 0) and a.momentum_buf is None and a.lr_dev is None
    s = TrainStep(mk(), use_graph=False, optimizer="sgd")
    assert (s.optimizer, s.lr, s.momentum, s.weight_decay) == ("sgd", 0.005, 0.9, 1e-4)
    assert s.exp_avg is None and s.exp_avg_sq is None and s.beta_pow is None
    assert s.momentum_buf.shape == s.flat_p.shape and s.momentum_buf.dtype == torch.float32 and not s.momentum_buf.any()
    assert s.lr_dev.shape == (1,) and s.lr_dev.dtype == torch.float32 and float(s.lr_dev) == float(np.float32(0.005))
    s.set_lr(0.25)
    assert s.lr == 0.25 and float(s.lr_dev) == 0.25
    a.set_lr(0.5)                                                      # Adam, nothing captured yet
    assert a.lr == 0.5
    with pytest.raises(SdhipError, match="rmsprop"):
        TrainStep(mk(), use_graph=False, optimizer="rmsprop")
    with pytest.raises(SdhipError, match="weight_decay"):
        TrainStep(mk(), use_graph=False, weight_decay=1e-4)


@pytest.mark.gpu
def test_eager_steps_apply_the_formula_to_their_own_gradient():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    ts = _sgd_step()
    lr = 0.05
    for s in range(3):
        if s == 2:
            lr = 0.02
            ts.set_lr(lr)
        p0, b0 = ts.flat_p.clone(), ts.momentum_buf.clone()
        ts(*batch)
        g = ts.flat_g                                                  # still this step's gradient
        assert float(g.abs().max()) > 0
        p_ref, b_ref = _formula(p0, b0, g, float(np.float32(lr)), 1.0)
        mask = _live_mask(ts)
        p_ref, b_ref = torch.where(mask, p_ref, p0.double()), torch.where(mask, b_ref, b0.double())
        tol = _tol(1, p_ref, b_ref)
        e = (_close(ts.flat_p, p_ref, tol), _close(ts.momentum_buf, b_ref, tol))
        print("step %d: |p err| %.3g |buf err| %.3g tol %.3g; max |lr*buf| %.3g" % (s, e[0], e[1], tol, lr * float(b_ref.abs().max())))
    assert ts.steps_done == 3 and ts.grad_free is not None
    ops.set_step_context(None)


@pytest.mark.gpu
def test_replay_reads_the_rate_from_the_device():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import SdhipError, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    ts = _sgd_step(use_graph=True)
    ts.capture(*batch, warmup=2)
    assert ts.steps_done == 2
    ts.set_lr(0.0)
    p0, b0 = ts.flat_p.clone(), ts.momentum_buf.clone()
    ts(*batch)
    assert torch.equal(ts.flat_p, p0) and not torch.equal(ts.momentum_buf, b0)
    ts.set_lr(0.01)
    p1 = ts.flat_p.clone()
    ts(*batch)
    b2 = ts.momentum_buf.double()
    want = -float(np.float32(0.01)) * b2
    _close(ts.flat_p.double() - p1.double(), want, _tol(1, ts.flat_p, b2))
    assert float(want.abs().max()) > 100 * _tol(1, ts.flat_p, b2)       # the step is far above what the tolerance would hide
    assert ts.steps_done == 4
    ops.set_step_context(None)
    # Adam's rate is part of its graph
    ad = TrainStep(_model(), dtype=torch.float32, use_graph=True, lr=1e-4)
    ad.set_lr(2e-4)
    ad.capture(*batch, warmup=2)
    with pytest.raises(SdhipError, match="captured"):
        ad.set_lr(1e-4)
    assert ad.lr == 2e-4
    ops.set_step_context(None)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_decay_leaves_unreached_parameters_alone(graph):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as C, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import synthetic_batch, live_ranges
    batch = synthetic_batch(2, 256, 256)
    ts = _sgd_step(_warp_model(), use_graph=graph)
    before = {k: v.detach().clone() for k, v in ts.model.named_parameters()}
    if graph:
        ts.capture(*batch, warmup=2)
    for _ in range(2):
        ts(*batch)
    ops.set_step_context(None)
    assert ts.grad_free and ts.live is not None and ts.live.tolist() == live_ranges(ts.model, ts.grad_free)
    names = [k for k, _ in ts.model.named_parameters()]
    idle = {names[i] for i in ts.grad_free}
    for k, v in ts.model.named_parameters():
        if k in idle:
            assert torch.equal(v.detach(), before[k]), k
    assert not torch.equal(ts.model.segNet.conv1d_1[0].c2d.weight.detach(), before["segNet.conv1d_1.0.c2d.weight"])
    assert not ts.momentum_buf[~_live_mask(ts)].any()
    state = C.optimizer_state_dict(ts)["state"]
    assert set(state) == set(range(len(names))) - set(ts.grad_free)


@pytest.mark.gpu
def test_flush_closes_an_open_cycle():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batches = [synthetic_batch(2, 256, 256, seed=100 + i) for i in range(2)]
    ts = _sgd_step(accumulate=3)
    assert ts.flush() is False
    p0 = ts.flat_p.clone()
    for b in batches:
        ts(*b)
    assert ts.steps_done == 0 and torch.equal(ts.flat_p, p0)
    g = ts.flat_g.clone()                                              # the sum of two micro-batch gradients
    assert ts.flush() is True
    p_ref, b_ref = _formula(p0, torch.zeros_like(p0), g, float(np.float32(0.05)), 1.0 / 3)
    mask = _live_mask(ts)
    p_ref, b_ref = torch.where(mask, p_ref, p0.double()), torch.where(mask, b_ref, torch.zeros_like(b_ref))
    tol = _tol(1, p_ref, b_ref)
    _close(ts.flat_p, p_ref, tol)
    _close(ts.momentum_buf, b_ref, tol)
    assert ts.steps_done == 1 and not torch.equal(ts.flat_p, p0)
    p1, b1 = ts.flat_p.clone(), ts.momentum_buf.clone()
    assert ts.flush() is False
    assert ts.steps_done == 1 and torch.equal(ts.flat_p, p1) and torch.equal(ts.momentum_buf, b1)
    ts(*batches[0])                                                    # opens a new cycle: the buffer is cleared first
    assert ts.steps_done == 1 and ts._micro == 1
    ops.set_step_context(None)
    fresh = _sgd_step(lr=0.0, weight_decay=0.0)                        # the same weights, one plain call
    fresh.flat_p.copy_(p1)
    ops.invalidate_packed_weights()
    fresh(*batches[0])
    ops.set_step_context(None)
    rel = float((ts.flat_g - fresh.flat_g).norm() / fresh.flat_g.norm())
    print("gradient after flush vs a fresh call: rel %.3g" % rel)
    assert rel < 1e-3, rel
    # Adam
    ad = TrainStep(_model(), dtype=torch.float32, use_graph=False, lr=1e-3, accumulate=3)
    q0 = ad.flat_p.clone()
    ad(*batches[0])
    assert ad.flush() is True and ad.steps_done == 1 and not torch.equal(ad.flat_p, q0)
    assert ad.flush() is False
    ops.set_step_context(None)


@pytest.mark.gpu
def test_sgd_checkpoint_round_trip_on_the_device(tmp_path):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import checkpoint as C, nn as N, ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    mk = lambda seed: fill_state_dict(N.minidsnetExt(R.CFG(), labels=2, patch_type='1dcorr'), seed).cuda().train()
    a = _sgd_step(mk(5))
    for _ in range(2):
        a(*batch)
    ops.set_step_context(None)
    a.set_lr(0.02)
    base = str(tmp_path / "sgd")
    C.save_checkpoint(C.make_state(a, epoch=1), 0.0, 0.5, 1.0, 0.5, base)
    b = _sgd_step(mk(6), lr=0.3, momentum=0.5, weight_decay=0.0)
    C.load_checkpoint_and_params(base + ".pth.tar", b, map_location="cuda:0")
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.momentum_buf, b.momentum_buf) and bool(b.momentum_buf.any())
    assert float(b.lr_dev) == float(np.float32(0.02)) and (b.lr, b.momentum, b.weight_decay) == (0.02, 0.9, WD)
    assert b.steps_done == 0
    ad = TrainStep(mk(6), dtype=torch.float32, use_graph=False)
    with pytest.raises(ValueError, match="SGD"):
        C.load_optimizer_state(ad, torch.load(base + ".pth.tar", weights_only=False)["optimizer"])
