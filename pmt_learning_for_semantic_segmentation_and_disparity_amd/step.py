"""What a captured step (train.TrainStep, evalstep.EvalStep; a new step class starts here) is built from: the recorder that turns
a body into a hipGraph and brings the process back when that fails, the two device tables at the head of a step with the check
that they read only memory the step owns, and the call of the model with its default loss."""
import gc
import sys

import torch

from . import _lib, multitask, ops
from ._lib import ptr, stream_ptr


def close_broken_capture(graph, streams, device, who):
    """Best-effort return to a launchable process after an exception inside a capture: the capture is ended on every stream
    it spans and the allocator's pool redirection closed."""
    try:
        graph.capture_end()                  # ends the allocator's pool redirection when the capture itself is intact
    except BaseException:
        pass
    for st in streams:
        try:
            _lib.abort_capture(st)
        except _lib.SdhipError as e:
            sys.stderr.write("[%s] %s\n" % (who, e))
    try:
        torch._C._cuda_endAllocateToPool(device.index or 0, graph.pool())
    except BaseException:
        pass


def _default_generator(device):
    return torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]


def capture_generator_state(device):
    """State of torch's default CUDA generator, taken before a capture begins (reset_capture_generator)."""
    try:
        return _default_generator(device).get_state()
    except BaseException:
        return None


def reset_capture_generator(device, state, who):
    """capture_begin put torch's default CUDA generator into capture mode and only a completed capture_end takes it out
    again ("Offset increment outside graph capture" on the next torch.randn(device='cuda')): give the generator a fresh,
    non-capturing state object carrying EXACTLY the seed and offset it had before the capture began - later torch CUDA draws
    continue the stream instead of replaying it from its start."""
    try:
        gen = _default_generator(device)
        fresh = torch.Generator(device=device)
        if state is not None:
            fresh.set_state(state)
        else:
            fresh.manual_seed(gen.initial_seed())
        gen.graphsafe_set_state(fresh.graphsafe_get_state())
    except BaseException as e:
        sys.stderr.write("[%s] could not reset the capture state of torch's CUDA generator: %s\n" % (who, str(e).splitlines()[0]))


class Recording:
    """`with Recording(...) as rec: graph, result = rec.record(body)`: hipGraphs recorded on `stream` (the one the warm-up ran
    on), one per record() call.  No device memory may be released while a stream records (what `torch.cuda.graph` guards
    against the same way): garbage is collected on entry and the cyclic collector stays off until the section ends - a discarded
    model collected in the middle of a recording pass frees tensors, fires the weight-cache callbacks and took the process down.
    The capture is driven by hand: `torch.cuda.graph` re-raises out of its __exit__ when the capture was invalidated and then
    neither restores the current stream nor ends the capture, after which nothing in the process can launch (ROCm 7.2).
    After ANY exception out of record() the capture is ended on `stream` and on the streams of `also_close()` (those the body
    forks to), the allocator is out of the graph's pool, the collector is as it was, and the exception propagates; nothing of
    the body has run.  With reset_generator torch's CUDA generator has its state of entry (`gen_state`) back as well; without,
    it is still in capture mode until the caller hands `gen_state` to reset_capture_generator (once the device has answered).
    Host-side bookkeeping of the half-recorded body is the caller's to reset in either case."""

    def __init__(self, stream, device, who, error_mode="global", keep_graph=False, also_close=lambda: (), reset_generator=True):
        self.stream, self.device, self.who, self.error_mode, self.keep_graph = stream, device, who, error_mode, keep_graph
        self.also_close, self.reset_generator = also_close, reset_generator

    def __enter__(self):
        gc.collect()
        torch.cuda.empty_cache()
        self.gc_was_on = gc.isenabled()
        gc.disable()
        self.gen_state = capture_generator_state(self.device)
        return self

    def __exit__(self, *exc):
        if self.gc_was_on:
            gc.enable()

    def record(self, body, fault=None):
        """(graph, body()); fault: a callable run inside the capture, behind the body (tests make a capture fail with it)."""
        graph = torch.cuda.CUDAGraph(keep_graph=self.keep_graph)    # kept: _lib.graph_node_counts (node inventory tests)
        with torch.cuda.stream(self.stream):
            graph.capture_begin(capture_error_mode=self.error_mode)
            try:
                result = body()
                if fault is not None:
                    fault()
                graph.capture_end()
            except BaseException:
                close_broken_capture(graph, [self.stream] + list(self.also_close()), self.device, self.who)
                del graph
                if self.reset_generator:
                    reset_capture_generator(self.device, self.gen_state, self.who)
                raise
        return graph, result


class Tables:
    """fold_desc (sdhip_conv_pack_fold_batch: folded packs, biases, scale / shift tables) and pack_desc (sdhip_conv_pack_batch:
    every other pack) of one step, int64 device tables or None, and the two launches that open every pass of the step."""

    def __init__(self, dtype, device, sources, required, fold_error, pack_error):
        """sources: the names of ops.row_sources checked in a fold row (0 = absent passes, except for those in `required`)."""
        self.dt, self.device = _lib.code_of(dtype), device
        self.sources, self.required, self.fold_error, self.pack_error = sources, required, fold_error, pack_error
        self.fold_desc = self.pack_desc = None

    def build(self, fold_rows, pack_rows, owned):
        """Both tables are replayed for the lifetime of the step: every source must lie in `owned` (ops.ByteSpans) - any other
        is freed memory once its owner is gone (tests/test_train.py::test_pack_table_holds_only_the_steps_own_weights)."""
        for r in fold_rows:
            src = ops.row_sources(r)
            if not all(src[k] is None or (src[k] == 0 and k not in self.required) or owned.contains(src[k]) for k in self.sources):
                raise _lib.SdhipError(self.fold_error)
        for r in pack_rows:
            if not owned.contains(r[0]):
                raise _lib.SdhipError(self.pack_error)
        self.fold_desc = torch.tensor(fold_rows, dtype=torch.int64, device=self.device) if fold_rows else None
        self.pack_desc = torch.tensor(pack_rows, dtype=torch.int64, device=self.device) if pack_rows else None
        return self

    def launch(self):       # through ops.call, like every other launch of a pass: the launch-inventory tests watch that name
        if self.fold_desc is not None:      # first: folded packs + biases + tables from the weights and statistics of now
            ops.call("sdhip_conv_pack_fold_batch", ptr(self.fold_desc), self.fold_desc.shape[0], self.dt, stream_ptr())
        if self.pack_desc is not None:      # one launch packs every other weight
            ops.call("sdhip_conv_pack_batch", ptr(self.pack_desc), self.pack_desc.shape[0], self.dt, stream_ptr())


def model_outputs(model, dtype, left, right, seg, disp, extra=()):
    """What the model returns for one batch in `dtype`.  A multitask model gets the reference harness's call
    (torch_implementation.py:146-149): the targets, labels from the full one-hot (ATen argmax)."""
    x, y = left.to(dtype), right.to(dtype)
    if getattr(model, "multiTaskLoss", 0) and seg is not None and disp is not None:
        return model(x, y, None, disp, seg.argmax(1))
    if getattr(model, "disp_input", False):
        # `ThreeOutPutsDisp` (warp.minidsnetDivideDisp; torch_implementation.py:133-134): the network reads the f32 disparity target
        if disp is None:
            raise _lib.SdhipError("model_outputs: a disp_input model (%s) is called as model(left, right, disp) and needs the "
                                  "disparity target, in training and in evaluation" % type(model).__name__)
        return model(x, y, disp.float(), *extra)
    return model(x, y, *extra)


def edge_loss(model, outs, seg, disp, edges, *, smooth_grad=0.0, use_lovasz=False, loss=None, class_weights=None,
              mask_invalid_disp=False, **other):
    """The loss of the reference step for an `edgeOut` network (`edge_outputs`: ext_small.Ext_small / Ext_smallv2), whose
    outputs are `edge_ds, disp1, seg1, _` (torch_implementation.py:170-171): CE(outs[2]) + L1(outs[1]), plus
    lossEdge_fn(edges, outs[0]) when the edge target is given (:320-323).  Upstream gives this output type one
    ['cross_entropy'] head and never consults `-loss` (:279,286-288): Lovasz, a `loss=` list and smooth_grad are refused."""
    if use_lovasz or loss is not None:
        raise _lib.SdhipError("default_loss: an edge_outputs model has ONE cross-entropy head (the reference's edgeOut step does not "
                              "consult -loss); use_lovasz / loss do not apply: pass use_lovasz=False and no loss list")
    if smooth_grad or other.get("ignore_void") or other.get("seg3") is not None:
        raise _lib.SdhipError("default_loss: smooth_grad / ignore_void / seg3 do not apply to an edge_outputs model")
    return ops.edge_step_loss(outs[0], outs[1], outs[2], seg, disp, edges=edges, mask_invalid_disp=mask_invalid_disp,
                              class_weights=class_weights)


def photo_step_loss(model, outs, seg, left, *, use_lovasz=True, loss=None, class_weights=None, ignore_void=False, **other):
    """The loss of the reference step for a `ThreeOutPutsDispConsist` network (`photo_outputs`: warp.minidsnetDivideDisp2;
    torch_implementation.py:157-158,279-317): CE(outs[0]) + [-loss list](outs[2]) + CE(outs[4]) + MSE(outs[5], left).  The
    disparity has NO target term: upstream multiplies its L1 by 0 (dropped here) and trains the head through the warped image."""
    if left is None:
        raise _lib.SdhipError("default_loss: a photo_outputs model (%s) compares its warped right image with the left image: "
                              "pass left=..." % type(model).__name__)
    if left.dim() != 4 or left.shape[1] != 3:
        raise _lib.SdhipError("default_loss: the photometric term needs the 3-channel left image, got %s (upstream's MSELoss "
                              "fails on a 4-channel include_edges input too)" % (tuple(left.shape),))
    if other.get("seg3") is not None:
        raise _lib.SdhipError("default_loss: seg3 is outs[4] of a photo_outputs model, not an argument")
    plan = loss if loss is not None else (("cross_entropy", "lovasz_loss") if use_lovasz else ("cross_entropy",))
    total = ops.seg_loss(outs[0], seg, ("cross_entropy",), class_weights)
    total = total + ops.seg_loss(outs[2], seg, plan, class_weights, ignore_void)
    total = total + ops.seg_loss(outs[4], seg, ("cross_entropy",), class_weights)
    return total + ops.photo_loss(outs[5], left)


def default_loss(model, outs, seg, disp, *, left=None, smooth_grad=0.0, **train_loss_kwargs):
    """The loss of the reference step on the outputs of model_outputs.  Multitask: the sum of the three maps' means
    (torch_implementation.py:173-176,285-325), from the loss kernels' own sums.
    smooth_grad (non-zero): the weight of the `smooth_grad` disparity regulariser of lossDisp_fn (losses/multiLosses.py:143-146),
    ops.disp_smooth_loss(left, outs[1], seg, smooth_grad), added to the rest; `left` is the f32 left image of the batch.
    An `edge_outputs` model (ext_small.Ext_small / Ext_smallv2) gets edge_loss above without the edge term, CE + L1: the
    edge target is no input of a step (train.EdgeStepLoss carries it).
    A `photo_outputs` model (warp.minidsnetDivideDisp2) gets photo_step_loss above: it needs `left`, 3 channels."""
    if smooth_grad:
        if getattr(model, "multiTaskLoss", 0):
            raise _lib.SdhipError("default_loss: the multitask loss is the three maps' means; smooth_grad has no place in it")
        if left is None:
            raise _lib.SdhipError("default_loss: smooth_grad needs the left image (left=...)")
    if getattr(model, "multiTaskLoss", 0):
        return multitask.step_loss(outs[4], outs[5], outs[6])
    if getattr(model, "edge_outputs", False):
        return edge_loss(model, outs, seg, disp, None, smooth_grad=smooth_grad, **train_loss_kwargs)
    if getattr(model, "photo_outputs", False):
        loss = photo_step_loss(model, outs, seg, left, **train_loss_kwargs)
        return loss + ops.disp_smooth_loss(left, outs[1], seg, smooth_grad) if smooth_grad else loss
    # the `ThreeOutPuts` networks (warp.minidsnetDivide*) add the cross-entropy of their third segmentation map, outs[4]
    # (torch_implementation.py:157-158,298); Lovasz stays on outs[2], which the metrics score as well
    seg3 = outs[4] if getattr(model, "three_outputs", False) else None
    loss = ops.train_loss(outs[0], outs[1], outs[2], seg, disp, seg3=seg3, **train_loss_kwargs)
    if smooth_grad:
        loss = loss + ops.disp_smooth_loss(left, outs[1], seg, smooth_grad)
    return loss
