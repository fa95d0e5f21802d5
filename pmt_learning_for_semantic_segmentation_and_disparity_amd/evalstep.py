"""Evaluation step: the forward pass of test_model (torch_implementation.py:450-582: model.eval(), torch.no_grad(),
networkOutput per batch), optionally captured as ONE hipGraph, with eval-mode BatchNorm folded into the weight packs.

With running statistics, conv -> BatchNorm -> activation is one convolution with pre-scaled weights, a bias and the activation
epilogue every forward kernel already has: the convbn / deconvbn layers (Conv2DownUp, pyramids, ASPP, heads) run as ONE launch
instead of three.  Every other eval-mode BatchNorm (DenseNet norm1 / norm2 / transitions / norm5, depthwise and 3-D nodes) reads
its scale / shift from a table instead of launching a per-channel finalize for constants.  Folded packs, biases and tables are
written by one batched launch (sdhip_conv_pack_fold_batch) at the head of every step, the plain packs of every other weight by a
second one (sdhip_conv_pack_batch): a step always sees the current weights and running statistics, whoever changed them (a
TrainStep's fused optimizer, load_state_dict, an in-place edit) - there is nothing to refresh by hand.
The plain table names the cached forward packs of the model's parameters and of cached views that lie inside them (HANet
packs a (Cout, Cin, k, 1) view of its Conv1d weights); a cached pack that no row rewrites is not trusted but repacked, in
place, wherever it is used (ops.packed_weight).  Single rank: the reference evaluates on rank 0.
"""
import torch

from . import _lib, ops, step


def _clone(t):
    """A static copy of a step input: a tensor, None, or a tuple of them (HANet's `pos`)."""
    if t is None:
        return None
    return tuple(_clone(u) for u in t) if isinstance(t, (tuple, list)) else t.clone()


def _refill(dst, src):
    if dst is None:
        return
    if isinstance(dst, tuple):
        for d, s in zip(dst, src):
            _refill(d, s)
    elif dst.data_ptr() != src.data_ptr():
        dst.copy_(src, non_blocking=True)


class EvalStep:
    def __init__(self, model, dtype=torch.bfloat16, use_graph=True, fold_bn=True, metrics=None, with_loss=False, loss_kwargs=None):
        params = list(model.parameters())
        if model.training:
            raise _lib.SdhipError("EvalStep: the model is in training mode; call model.eval() first, as test_model does")
        if not params or not params[0].is_cuda:
            raise _lib.SdhipError("EvalStep: the model must live on the GPU; there is no CPU path")
        if dtype not in (torch.bfloat16, torch.float32):
            raise _lib.SdhipError("EvalStep: dtype %s (f32 and bf16 only)" % dtype)
        if ops.parallel.world_size() != 1:
            # the reference evaluates on rank 0 alone (torch_implementation.py:450-582); nothing here exchanges statistics
            raise _lib.SdhipError("EvalStep: single rank only (a data-parallel process group of %d ranks is configured)"
                                  % ops.parallel.world_size())
        self.model, self.dtype, self.use_graph, self.fold_bn = model, dtype, use_graph, fold_bn
        # metrics.StepMetrics (or None): scored on the second segmentation head and the disparity, as TrainStep does
        self.metrics, self.with_loss = metrics, with_loss
        self.loss_kwargs = dict(loss_kwargs or {})
        self.device = params[0].device
        self.ctx = ops.StepContext(self.device)
        self.ctx.fold = ops.FoldState(dtype, self.device) if fold_bn else None   # off: today's eval arithmetic, captured
        # every source of the two tables lies inside a parameter or buffer of THIS model, and the running statistics exist
        self.tables = step.Tables(dtype, self.device, ("weight", "gamma", "beta", "mean", "var", "conv_bias"), ("mean", "var"),
                                  "EvalStep: fold table holds a source outside this model's parameters and buffers",
                                  "EvalStep: weight-pack table holds a source outside this model's parameters")
        self.keep = []               # every buffer the two tables (and so the graph) read or write
        self.graph = self.static = self.outs = None
        self.folded_calls = 0        # folded layer calls of one step
        self.debug_graph = False     # tests: keep the captured hipGraph inspectable (_lib.graph_node_counts)
        self._capture_fault = None   # tests: a callable invoked inside the capture to make it fail
        self._armed = False
        self._homes = None

    # -- pieces ---------------------------------------------------------------------------------
    pack_desc = property(lambda self: self.tables.pack_desc)
    fold_desc = property(lambda self: self.tables.fold_desc)

    def _tensors(self):
        return list(self.model.parameters()) + list(self.model.buffers())

    def _refresh_cached(self):
        """The already-cached packs of this model's parameters, repacked IN PLACE: a cached buffer may be one optimizer step
        stale (the fused optimizer does not move weight._version), and its address may sit in a TrainStep's replayed table -
        so it is rewritten, never replaced."""
        self.tables.build([], self._pack_rows(), ops.ByteSpans.of(self._tensors())).launch()     # _arm builds the step's own
        self.ctx.frozen_bufs = {id(b) for b in self._packs()}

    def _pack_rows(self):
        """Rows of the cached forward packs of this model's weights: of the parameters themselves and of cached views that lie
        inside them (HANet's (Cout, Cin, k, 1) views of its Conv1d weights).  An eval forward reads no other orientation."""
        params = list(self.model.parameters())
        return ops.pack_descriptors(self.dtype, owners=params, spans=ops.ByteSpans.of(params), modes=('fwd',))

    def _packs(self):
        params = list(self.model.parameters())
        return ops.cached_packs(self.dtype, params, spans=ops.ByteSpans.of(params), modes=('fwd',))

    def _arm(self):
        """After the measuring pass: the two device tables."""
        fold = self.ctx.fold
        if fold is not None:
            fold.finish()
        self.tables.build(fold.rows() if fold is not None else [], self._pack_rows(), ops.ByteSpans.of(self._tensors()))
        self.keep = self._packs()
        # a cached pack outside the table (none is expected) is repacked at every use instead of being trusted (ops.packed_weight)
        self.ctx.frozen_bufs = {id(b) for b in self.keep}
        if fold is not None:
            self.keep += [fold.table_buf] + [t for r in fold.layers.values() for t in (r.pack, r.bias_out)]
        self._homes = [t.data_ptr() for t in self._tensors()]
        self._armed = True

    def _forward(self, left, right, seg, disp, extra):
        outs = step.model_outputs(self.model, self.dtype, left, right, seg, disp, extra)
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        if self.metrics is not None:
            self.metrics.update(outs[2], seg, outs[1], disp)
        if self.with_loss:
            if seg is None or disp is None:
                raise _lib.SdhipError("EvalStep: with_loss needs seg and disp")
            if len(outs) < 3 and not getattr(self.model, "multiTaskLoss", 0):
                raise _lib.SdhipError("EvalStep: with_loss needs a model with two segmentation heads and a disparity")
            wants_left = self.loss_kwargs.get("smooth_grad") or getattr(self.model, "photo_outputs", False)
            kw = dict(self.loss_kwargs, left=left) if wants_left else self.loss_kwargs
            outs = outs + (step.default_loss(self.model, outs, seg, disp, **kw),)
        return outs

    def _step(self, left, right, seg, disp, extra):
        """One step under this step's own context; the context that was installed before is put back on the way out."""
        prev = ops._ctx[0]
        ops.set_step_context(self.ctx)
        try:
            with torch.no_grad():
                if self.ctx.fold is not None:
                    self.ctx.fold.calls = 0
                if not self._armed:
                    self._refresh_cached()
                    self.ctx.frozen_pack = True       # cached packs are handed out as they are (just refreshed), never replaced
                    outs = self._forward(left, right, seg, disp, extra)
                    self._arm()
                else:
                    self.tables.launch()      # folded packs + biases + tables, then every other pack of this model
                    outs = self._forward(left, right, seg, disp, extra)
                self.folded_calls = self.ctx.fold.calls if self.ctx.fold is not None else 0
                return outs
        finally:
            ops.set_step_context(prev)

    def _check_homes(self):
        if self._homes != [t.data_ptr() for t in self._tensors()]:
            raise _lib.SdhipError("EvalStep: a parameter or buffer of the model moved after the step was built (a TrainStep "
                                  "created later re-homes the parameters): build the EvalStep after the TrainStep")

    # -- capture --------------------------------------------------------------------------------
    def capture(self, left, right, seg=None, disp=None, *extra):
        self.static = [_clone(t) for t in (left, right, seg, disp) + tuple(extra)]
        a, b, s, d, ex = self.static[0], self.static[1], self.static[2], self.static[3], tuple(self.static[4:])
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            # the eager passes must not count: a batch is scored once, by the replay that follows the capture
            saved = None if self.metrics is None else (self.metrics.counts.clone(), self.metrics.sums.clone())
            for _ in range(2):         # the measuring pass, then one pass on the tables
                self._step(a, b, s, d, ex)
            if saved is not None:
                self.metrics.counts.copy_(saved[0])
                self.metrics.sums.copy_(saved[1])
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        # nothing of a failed recording pass has run: the recorder gives torch's CUDA generator its state back itself
        with step.Recording(cap, self.device, "EvalStep", keep_graph=self.debug_graph) as rec:
            self.graph, self.outs = rec.record(lambda: self._step(a, b, s, d, ex), self._capture_fault)
        torch.cuda.current_stream().wait_stream(cap)
        return self

    # -- public ---------------------------------------------------------------------------------
    def __call__(self, left, right, seg=None, disp=None, *extra):
        if (self.metrics is not None or self.with_loss) and (seg is None or disp is None):
            raise _lib.SdhipError("EvalStep: metrics / with_loss need seg and disp")
        if self.model.training:
            raise _lib.SdhipError("EvalStep: the model was switched to training mode; call model.eval() before evaluating")
        if self._armed:
            self._check_homes()
        if not self.use_graph:
            return self._step(left, right, seg, disp, extra)
        if self.graph is None:
            self.capture(left, right, seg, disp, *extra)    # a failed capture is closed (sdhip_abort_capture) and raises
        for dst, src in zip(self.static, (left, right, seg, disp) + tuple(extra)):
            _refill(dst, src)
        self.graph.replay()
        return self.outs
