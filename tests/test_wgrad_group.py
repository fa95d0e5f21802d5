"""Grouped weight gradients (sdhip_conv2d_wgrad_group, include/sdhip.h): the weight gradients of many layers in one grid per
kernel instantiation.  The reference computes them layer by layer inside loss.backward() (torch_implementation.py:389;
layers: models/densenet.py:25-93, models/dsnet_t2.py:80-117, models_psmnet/stackhourglass.py:31-50); nothing reads them
before the optimizer step (:724), which is what allows the regrouping.  Results must equal the per-layer launches up to
the order of the f32 atomic adds."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rowops_ref import diag_switches  # noqa: E402


def _layer(dev, B, H, W, Cin, Cout, k, ldx=None, pro=False, groups=1, stride=1, dil=1, D=1, kd=1, bias=False, seed=0):
    """One layer's operands + geometry ('same'-style padding), as the arguments of sdhip_conv2d_wgrad."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(seed)
    ldx = ldx or ((Cin + 7) & ~7)
    pad = dil * (k - 1) // 2
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    pd = (kd - 1) // 2
    Do = D                                   # depth stride 1, 'same' depth padding
    x = torch.randn(B * D, H, W, ldx, generator=g).to(torch.bfloat16).to(dev)
    ldy = (Cout + 7) & ~7
    dy = (torch.randn(B * Do, Ho, Wo, ldy, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    sc = (torch.rand(groups, Cin, generator=g) + 0.5).to(dev) if pro else None
    sh = (torch.rand(groups, Cin, generator=g) - 0.5).to(dev) if pro else None
    per = _lib.packed_elems(Cout, Cin, k * k, _lib.BF16) * kd
    return dict(x=x, dy=dy, sc=sc, sh=sh, per=per, bias=bias,
                geo=(B, H, W, Cin, ldx, Ho, Wo, Cout, ldy, k, k, stride, dil, pad, pad, D, Do, kd, 1, pd, int(pro), groups))


def _run_single(L, dev):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, ptr, stream_ptr
    acc = torch.zeros(L["per"], dtype=torch.float32, device=dev)
    db = torch.zeros(L["geo"][7], dtype=torch.float32, device=dev) if L["bias"] else None
    g = L["geo"]
    call("sdhip_conv2d_wgrad", ptr(L["x"]), ptr(L["dy"]), ptr(acc), ptr(db), ptr(L["sc"]), ptr(L["sh"]), *g, 1, _lib.BF16, stream_ptr())
    return acc, db


def _run_group(layers, dev, max_wg=0):
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    from pmt_learning_for_semantic_segmentation_and_disparity_amd._lib import call, stream_ptr
    items = (_lib.WgradItem * len(layers))()
    outs = []
    names = [f[0] for f in _lib.WgradItem._fields_]
    for it, L in zip(items, layers):
        acc = torch.zeros(L["per"], dtype=torch.float32, device=dev)
        db = torch.zeros(L["geo"][7], dtype=torch.float32, device=dev) if L["bias"] else None
        dp = lambda t: t.data_ptr() if t is not None else None
        vals = (dp(L["x"]), dp(L["dy"]), dp(acc), dp(db), dp(L["sc"]), dp(L["sh"])) + tuple(L["geo"])
        for n, v in zip(names, vals):
            setattr(it, n, v)
        outs.append((acc, db))
    call("sdhip_conv2d_wgrad_group", ctypes.cast(items, ctypes.c_void_p), len(layers), max_wg, _lib.BF16, stream_ptr())
    return outs


@pytest.mark.gpu
def test_group_equals_per_layer_launches():
    """A step's worth of shapes in one call: 20 DenseNet 1x1 bottlenecks of growing width on one map (prologue, slab prefix:
    > 16 layers of one instantiation -> two grids), their 3x3 partners, DMA-path 3x3 / 5x5 decoder layers on several map
    sizes, a 32-channel (two input-channel tiles) layer, a strided layer, a 3-D layer, a chunk-packed wide 1x1, a thin
    8 -> 1 layer and a 7x7 layer (both launched on their own inside the call)."""
    dev = torch.device("cuda:0")
    layers = []
    for i in range(20):
        layers.append(_layer(dev, 4, 16, 32, 64 + 32 * i, 128, 1, ldx=704, pro=True, groups=2, seed=i))
        layers.append(_layer(dev, 4, 16, 32, 128, 32, 3, pro=True, groups=2, seed=100 + i))
    layers += [
        _layer(dev, 2, 64, 128, 64, 64, 3, seed=201), _layer(dev, 2, 32, 64, 64, 64, 3, seed=202), _layer(dev, 2, 33, 47, 64, 64, 3, seed=203),
        _layer(dev, 2, 64, 128, 64, 64, 5, seed=204), _layer(dev, 1, 40, 72, 64, 64, 5, bias=True, seed=205),
        _layer(dev, 2, 64, 128, 32, 32, 3, seed=206), _layer(dev, 2, 64, 128, 32, 64, 3, seed=207),
        _layer(dev, 2, 64, 128, 64, 64, 3, stride=2, seed=208),
        _layer(dev, 1, 16, 32, 32, 32, 3, D=6, kd=3, seed=209),
        _layer(dev, 2, 32, 64, 512, 256, 1, pro=True, seed=210),
        _layer(dev, 2, 128, 256, 8, 1, 5, dil=2, bias=True, seed=211),
        _layer(dev, 2, 32, 64, 16, 64, 7, seed=212),
        _layer(dev, 2, 24, 40, 65, 64, 1, ldx=72, bias=True, seed=213),
    ]
    want = [_run_single(L, dev) for L in layers]
    for max_wg in (0, 96):                                       # 96: grids limited to a part of the chip (overlap mode)
        got = _run_group(layers, dev, max_wg)
        torch.cuda.synchronize()
        for i, ((wa, wb), (ga, gb)) in enumerate(zip(want, got)):
            n = float(wa.norm())
            assert n > 0, i
            err = float((ga - wa).norm()) / n
            assert err < 2e-5, (i, max_wg, layers[i]["geo"], err)          # f32 atomics in another order
            if wb is not None:
                assert float((gb - wb).abs().max()) <= 1e-4 * max(1.0, float(wb.abs().max())), i


@pytest.mark.gpu
def test_group_of_one_and_argument_errors():
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    dev = torch.device("cuda:0")
    L = _layer(dev, 2, 32, 64, 64, 64, 3, seed=5)
    (wa, _), ((ga, _),) = _run_single(L, dev), _run_group([L], dev)
    assert float((ga - wa).norm()) <= 2e-5 * float(wa.norm())
    rc = _lib._lib.sdhip_conv2d_wgrad_group(None, 3, 0, _lib.BF16, None)
    assert rc == _lib.ERR_ARG and b"bad arguments" in _lib._lib.sdhip_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(2, 1, 37, 70, 32, 32), (1, 1, 8, 32, 8, 16), (2, 1, 64, 128, 24, 32),
                                              (1, 5, 9, 40, 32, 32), (2, 3, 6, 33, 16, 24), (1, 2, 4, 24, 32, 8),
                                              (1, 4, 10, 50, 64, 32), (2, 2, 5, 24, 64, 16)])
def test_half_row_kernel_matches_f32_contraction(B, D, H, W, Cin, Cout):
    """conv_wgrad_half.h (64-byte LDS rows, all depth taps per workgroup; <= 32 channels on both sides, 3x3 / 3x3x3, stride 1,
    padding 1): the weight gradient against ATen's f32 contraction of the same bf16-rounded operands — ragged tiles, channel
    counts below 32, depth taps that leave the volume, 64 input channels as two half layers (dres0[0] of PSMNet: wgrad_layer in
    conv_wgrad.hip), and the same layer through the general kernel (SDHIP_WGRAD_NO_HALF32)."""
    import os
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    torch.manual_seed(B * 100 + D * 10 + Cin)
    dev = torch.device("cuda:0")
    three = D > 1
    x = torch.randn(B, Cin, D, H, W, device=dev).to(torch.bfloat16)
    g = (torch.randn(B, Cout, D, H, W, device=dev) * 0.1).to(torch.bfloat16)
    if three:
        w = torch.zeros(Cout, Cin, 3, 3, 3, device=dev)
        want = torch.nn.grad.conv3d_weight(x.float(), w.shape, g.float(), stride=1, padding=1)
    else:
        w = torch.zeros(Cout, Cin, 3, 3, device=dev)
        want = torch.nn.grad.conv2d_weight(x[:, :, 0].float(), w.shape, g[:, :, 0].float(), stride=1, padding=1)
    to_img = lambda t: t.permute(0, 2, 1, 3, 4).reshape(B * D, t.shape[1], H, W).contiguous(memory_format=torch.channels_last)
    xi, gi = ops.aligned_view(to_img(x)), ops.aligned_view(to_img(g))
    spec = ops.conv3d_spec(xi[0], D, w, 1, 1) if three else ops.conv_spec(xi[0], w, 'conv', 1, 1, 1)
    ops.set_step_context(None)
    got = {}
    for sw in ("", "1"):
        with diag_switches(SDHIP_WGRAD_NO_HALF32=sw or None):
            got[sw], _ = ops._wgrad_impl(xi[0], xi[1], gi[0], gi[1], w, None, spec, None, None, False, 1)
    n = float(want.norm())
    assert n > 0
    assert float((got[""] - want).norm()) / n < 2e-3, float((got[""] - want).norm()) / n
    assert float((got["1"] - want).norm()) / n < 2e-3
    assert float((got[""] - got["1"]).norm()) / n < 1e-4          # same products, another summation order


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,H,W,Cin,k", [(2, 1, 37, 70, 32, 5), (1, 1, 16, 40, 24, 3), (2, 5, 9, 45, 32, 3), (1, 11, 8, 32, 16, 3),
                                          (1, 20, 24, 64, 32, 3)])
def test_single_map_wgrad_matches_f32_contraction(B, D, H, W, Cin, k):
    """conv_wgrad_single.h (ONE output map, 9..32 input channels, <= 32 taps: taps as the MFMA row axis, dy gathered from a
    scalar halo; classif1-3 of PSMNet end in such a layer) against ATen's f32 contraction of the same bf16-rounded operands,
    and against the same layer through the general kernels (SDHIP_CONV_NO_THIN): ragged tiles, depth taps that leave the
    volume, several slices per workgroup."""
    import os
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops, _lib
    torch.manual_seed(B * 100 + D * 10 + Cin)
    dev = torch.device("cuda:0")
    three = D > 1
    pad = k // 2
    x = torch.randn(B, Cin, D, H, W, device=dev).to(torch.bfloat16)
    g = (torch.randn(B, 1, D, H, W, device=dev) * 0.1).to(torch.bfloat16)
    if three:
        w = torch.zeros(1, Cin, k, k, k, device=dev)
        want = torch.nn.grad.conv3d_weight(x.float(), w.shape, g.float(), stride=1, padding=pad)
    else:
        w = torch.zeros(1, Cin, k, k, device=dev)
        want = torch.nn.grad.conv2d_weight(x[:, :, 0].float(), w.shape, g[:, :, 0].float(), stride=1, padding=pad)
    to_img = lambda t: t.permute(0, 2, 1, 3, 4).reshape(B * D, t.shape[1], H, W).contiguous(memory_format=torch.channels_last)
    xi, gi = ops.aligned_view(to_img(x)), ops.aligned_view(to_img(g))
    spec = ops.conv3d_spec(xi[0], D, w, 1, pad) if three else ops.conv_spec(xi[0], w, 'conv', 1, 1, pad)
    ops.set_step_context(None)
    got = {}
    for sw in ("", "1"):
        with diag_switches(SDHIP_CONV_NO_THIN=sw or None):
            got[sw], _ = ops._wgrad_impl(xi[0], xi[1], gi[0], gi[1], w, None, spec, None, None, False, 1)
    n = float(want.norm())
    assert n > 0 and got[""].shape == want.shape
    assert float((got[""] - want).norm()) / n < 2e-3, float((got[""] - want).norm()) / n
    assert float((got["1"] - want).norm()) / n < 2e-3
    assert float((got[""] - got["1"]).norm()) / n < 1e-4          # same products, another summation order


def _model():
    from oracle import ref_models as R
    from oracle.detweights import fill_state_dict
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import nn as N
    return fill_state_dict(N.minidsnetExt(R.CFG(aspp=0), labels=2, patch_type='1dcorr'), 31).cuda().train()


@pytest.mark.gpu
def test_step_with_grouped_wgrads_equals_per_layer_step():
    """The whole training step with queued + grouped weight gradients against the same step with per-layer launches
    (bf16, same kernels: the gradients differ by f32 summation order only), and the captured step's node count."""
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import ops
    from pmt_learning_for_semantic_segmentation_and_disparity_amd.train import TrainStep, synthetic_batch
    batch = synthetic_batch(2, 256, 256)
    grads, losses = [], []
    for defer in (False, False, True):
        ts = TrainStep(_model(), dtype=torch.bfloat16, use_graph=False, lr=0.0)
        ts.ctx.defer_wgrad = defer
        for _ in range(3):                               # measuring step, arming step, a steady-state step
            loss = ts(*batch)
        losses.append(float(loss))
        grads.append(ts.flat_g.clone())
        ops.set_step_context(None)
    assert abs(losses[0] - losses[2]) <= 1e-6 * max(1.0, abs(losses[0]))
    # The backward pass of this network is not reproducible bit for bit: its BatchNorm reductions are f32 atomics, and the
    # train-mode BatchNorm chain amplifies their summation order to ~2 % of the gradient norm between two IDENTICAL runs
    # (tests/diag/gpu_wgroup_noise.py: 0.0236 / 0.0239 / 0.0234).  Grouping may cost no more than that noise.
    n = float(grads[0].norm())
    noise = float((grads[0] - grads[1]).norm()) / n
    diff = float((grads[0] - grads[2]).norm()) / n
    assert n > 0 and diff <= 1.5 * noise + 1e-4, (diff, noise)
    # per parameter, on the large-gradient convolution weights: a dropped or misrouted layer scores ~1
    ts = TrainStep(_model(), dtype=torch.bfloat16, use_graph=True, lr=0.0)
    ts.debug_graph = True
    ts(*batch)
    ops.set_step_context(None)
    off, checked = 0, 0
    for p in ts.model.parameters():
        k = p.numel()
        a, b, c = (g[off:off + k] for g in grads)
        off += ((k + 3) // 4) * 4
        na = float(a.norm())
        if p.dim() == 4 and na > 1e-3 * n:
            pn = float((a - b).norm()) / na
            assert float((a - c).norm()) / na <= 3.0 * pn + 0.02, (tuple(p.shape), na, pn)
            checked += 1
    assert checked > 50, checked
    from pmt_learning_for_semantic_segmentation_and_disparity_amd import _lib
    nodes = _lib.graph_node_counts(ts.graph)
    assert nodes["kernel"] < 1100 and nodes["total"] < 1150, nodes      # round 2: 1248 kernel nodes
