"""Training step of the hot path: forward + loss + backward + optimizer, optionally captured as ONE hipGraph.

Counterpart of train_model's inner loop (torch_implementation.py:350-397) without its host-side metric /
JPEG work: model(left, right) -> CE(seg1) + CE(seg2) + Lovasz(seg2) + L1(disp) [+ CE(seg3)] -> backward -> Adam or SGD.
Parameters live in one flat f32 buffer (one fused optimizer launch, one gradient all-reduce over RCCL when
data-parallel); activations run in `dtype` (bf16 MFMA path or exact f32 path).

The optimizer is the reference's `-optimType` (torch_implementation.py:715-724): Adam (lr 0.0015, eps 1e-7), or SGD with
momentum (lr 0.005, momentum 0.9, weight decay 1e-4).  Adam's rate is a by-value kernel argument, fixed once the step is a
hipGraph.  SGD's rate lives in device memory (`lr_dev`), which the kernel reads at every launch: `set_lr` between replays is
what the reference's per-iteration `adjust_learning_rate` (`poly_lr` here) needs.  `flush` closes an accumulation cycle
early, as the reference does at the last batch of an epoch (torch_implementation.py:390).
"""
import torch

from . import _lib, densenet, ops, parallel, step
from ._lib import call, ptr, stream_ptr


def poly_lr(epoch, itr, total_iter, base_lr=0.005, epoch_total=2400):
    """The rate adjust_learning_rate sets before every iteration of an SGD run (torch_implementation.py:352-353,599-608):
    base_lr * (1 - T/N) with T iterations done of N, held at its last value once `epoch_total` epochs have passed.  Host
    arithmetic in double precision, like the reference's; a loop calls `ts.set_lr(poly_lr(epoch, i, len(loader)))`."""
    T = epoch * total_iter + itr
    N = epoch_total * total_iter
    if epoch >= epoch_total:
        T = N - 1
    return base_lr * (1 - T / float(N))


def freeze_bn(model):
    """`-freeze_bn 1` (torch_implementation.py:235-241): every nn.BatchNorm2d goes into eval mode and its weight and bias stop
    requiring a gradient; returns those modules.  BatchNorm3d (PSMNet's volume stack) is left alone, as upstream.  Unlike
    upstream this holds under data parallelism too: the reference converts to SyncBatchNorm first (:739), which is not a
    BatchNorm2d, so its flag freezes nothing there; here the norms are nn.BatchNorm2d on every world size."""
    mods = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in mods:
        m.eval()
        if m.weight is not None:
            m.weight.requires_grad_(False)
        if m.bias is not None:
            m.bias.requires_grad_(False)
    return mods


_freeze_bn = freeze_bn      # TrainStep.__init__ has a keyword of the same name


def live_ranges(model, idle):
    """Rows (begin, end) of the flat buffer that cover every parameter whose position in `model.parameters()` is not in
    `idle`: the complement of the idle parameters' slices, adjacent slices merged.  Every bound is a multiple of 4, as the
    slices of flatten_parameters are (the `live` table of sdhip_sgd_step)."""
    rows, off, idle = [], 0, set(idle)
    for i, p in enumerate(model.parameters()):
        end = off + ((p.numel() + 3) // 4) * 4
        if i not in idle:
            if rows and rows[-1][1] == off:
                rows[-1][1] = end
            else:
                rows.append([off, end])
        off = end
    return rows


def flatten_parameters(model):
    """Re-home every parameter into one contiguous f32 buffer (and its .grad into a second one)."""
    params = [p for p in model.parameters()]
    n = sum(((p.numel() + 3) // 4) * 4 for p in params)     # 16-byte aligned slices
    dev = params[0].device
    flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
    flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
    off = 0
    with torch.no_grad():
        for p in params:
            k = p.numel()
            flat_p[off:off + k].copy_(p.detach().reshape(-1))
            p.data = flat_p[off:off + k].view(p.shape)
            p.grad = flat_g[off:off + k].view(p.shape)
            off += ((k + 3) // 4) * 4
    return flat_p, flat_g


class StepLoss:
    """`TrainStep(model, loss_fn=StepLoss(model, smooth_grad=w, ...))`: the default loss of the step (step.default_loss) with the
    options TrainStep.__init__ has no keyword for.  smooth_grad: the weight of the reference's `smooth_grad` disparity
    regulariser (ops.disp_smooth_loss; 1 is the reference's value) on the disparity output, the f32 left image and the full
    one-hot target of the batch.  use_lovasz, loss and class_weights are TrainStep's keywords of the same names: the list is
    checked and the table uploaded here, once, so that the step captures into the hipGraph.  `wants_images` makes TrainStep
    hand over the input images; `metrics=` is scored as with the default loss, the heads being the same."""
    wants_images = True

    def __init__(self, model, smooth_grad=1.0, use_lovasz=True, loss=None, class_weights=None):
        if getattr(model, "multiTaskLoss", 0) and (smooth_grad or loss is not None or class_weights is not None):
            raise _lib.SdhipError("StepLoss: the multitask modes have their own loss; smooth_grad / loss / class_weights do not apply to them")
        self.model, self.smooth_grad, self.use_lovasz = model, float(smooth_grad), use_lovasz
        self.seg_loss = None if loss is None else tuple([loss] if isinstance(loss, str) else loss)
        if self.seg_loss is not None:
            ops.seg_loss_plan(self.seg_loss)
        self.class_weights = ops.seg_class_weights(class_weights, device=next(model.parameters()).device)

    def __call__(self, outs, seg, disp, left=None, right=None):
        return step.default_loss(self.model, outs, seg, disp, left=left, smooth_grad=self.smooth_grad, use_lovasz=self.use_lovasz,
                                 loss=self.seg_loss, class_weights=self.class_weights)


class EdgeStepLoss:
    """`TrainStep(model, loss_fn=EdgeStepLoss(model))`: the loss of the reference's `edgeOut` step (step.edge_loss) WITH its edge
    term, CE(outs[2]) + L1(outs[1]) + lossEdge_fn(data['edges'], outs[0]), for the `edge_outputs` networks (ext_small.Ext_small,
    Ext_smallv2).  A step takes four tensors; the edge target, dense f32 (B,1,H,W), lives in a device buffer of this object:
    `set_edges(t)` copies the batch's target into it before the step is called.  The buffer is allocated on first use and keeps
    its address, so a captured step reads it at every replay and sees the current target; a target of another shape or dtype
    raises once the buffer exists.  Calling the loss before set_edges raises."""

    def __init__(self, model, class_weights=None):
        if not getattr(model, "edge_outputs", False):
            raise _lib.SdhipError("EdgeStepLoss: the model has no edge head (edge_outputs); use StepLoss or the default loss")
        self.model = model
        self.class_weights = ops.seg_class_weights(class_weights, device=next(model.parameters()).device)
        self.edges = None

    def set_edges(self, t):
        if t.dim() != 4 or t.shape[1] != 1 or t.dtype != torch.float32:
            raise _lib.SdhipError("EdgeStepLoss.set_edges: the edge target must be f32 (B,1,H,W), got %s %s" % (t.dtype, tuple(t.shape)))
        if self.edges is None:
            device = next(self.model.parameters()).device
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise _lib.SdhipError("EdgeStepLoss.set_edges: the buffer cannot be allocated while a stream is capturing")
            self.edges = torch.empty(tuple(t.shape), dtype=torch.float32, device=device)
        elif tuple(t.shape) != tuple(self.edges.shape):
            raise _lib.SdhipError("EdgeStepLoss.set_edges: the edge target changed shape, %s after %s: the buffer a captured step "
                                  "reads cannot move" % (tuple(t.shape), tuple(self.edges.shape)))
        self.edges.copy_(t, non_blocking=True)
        return self

    def __call__(self, outs, seg, disp):
        if self.edges is None:
            raise _lib.SdhipError("EdgeStepLoss: call set_edges(data['edges']) before the step")
        return step.edge_loss(self.model, outs, seg, disp, self.edges, class_weights=self.class_weights)


class TrainStep:
    def __init__(self, model, dtype=torch.bfloat16, lr=None, betas=(0.9, 0.999), eps=1e-7, use_lovasz=True,
                 use_graph=True, world_size=1, process_group=None, use_side_stream=None, loss_fn=None, metrics=None, accumulate=1,
                 optimizer='adam', momentum=0.9, weight_decay=None, freeze_bn=False, fold_bn=True, loss=None, class_weights=None):
        self.model, self.dtype, self.use_lovasz = model, dtype, use_lovasz
        # `-optimType` (torch_implementation.py:715-724): the defaults of lr and weight_decay are those of the reference's optimizer
        if optimizer not in ("adam", "sgd"):
            raise _lib.SdhipError("TrainStep: optimizer %r is not one of 'adam', 'sgd'" % (optimizer,))
        self.optimizer = optimizer
        sgd = optimizer == "sgd"
        if lr is None:
            lr = 0.005 if sgd else 0.0015
        if weight_decay is None:
            weight_decay = 1e-4 if sgd else 0
        if not sgd and weight_decay != 0:
            # the fused Adam runs over the whole flat buffer: it would decay the parameters that never receive a gradient, which
            # torch.optim.Adam skips (sdhip_sgd_step has the `live` table for that; sdhip_adam_step has not)
            raise _lib.SdhipError("TrainStep: weight_decay is only supported with optimizer='sgd'")
        self.momentum, self.weight_decay = momentum, weight_decay
        # `-loss` list of the second segmentation head and the `-segWeight 1` class table (ops.train_loss); both None: the
        # default step.  The list is checked and the table uploaded here, once, so that the step captures into the hipGraph
        if loss_fn is not None and (loss is not None or class_weights is not None):
            raise _lib.SdhipError("TrainStep: a custom loss_fn computes the whole loss; loss / class_weights do not apply to it")
        if getattr(model, "multiTaskLoss", 0) and (loss is not None or class_weights is not None):
            raise _lib.SdhipError("TrainStep: the multitask modes have their own loss; loss / class_weights do not apply to them")
        self.seg_loss = None if loss is None else tuple([loss] if isinstance(loss, str) else loss)
        if self.seg_loss is not None:
            ops.seg_loss_plan(self.seg_loss)
        self.class_weights = ops.seg_class_weights(class_weights, device=next(model.parameters()).device)
        # metrics.StepMetrics (or None): scored inside the step on the second segmentation head and the disparity, as the
        # reference's lossSeg_fn(seg2) / lossDisp_fn calls do (torch_implementation.py:293,304) — one extra launch, graph-safe
        self.metrics = metrics
        self.loss_fn = loss_fn      # (outputs, seg, disp) -> scalar; default: the joint seg+disp loss of the reference step
        self.lr, self.betas, self.eps = lr, betas, eps
        # gradient accumulation (`-acmt_grad K`, torch_implementation.py:335,362,390-397): K calls form one optimizer step — the
        # gradients of K micro-batches add up in the flat buffer, the K-th call all-reduces, steps with their mean and clears
        self.accumulate = max(1, int(accumulate))
        self._micro = 0
        # `-freeze_bn 1`: the state is established here and again before every pass that runs Python modules (the reference's
        # epoch loop calls model.train(), which would silently unfreeze); "frozen" itself is a property of the modules
        # (ops.bn_frozen), so a model frozen by hand computes the same.  fold_bn False: frozen arithmetic, never folded
        self.freeze_bn, self.fold_bn = bool(freeze_bn), bool(fold_bn)
        if self.freeze_bn:
            _freeze_bn(model)
        self._dense_blocks = densenet.dense_blocks(model)
        self.graphs = {}            # (first, last) call of an accumulation cycle -> (hipGraph, its loss tensor)
        self.world_size, self.pg = world_size, process_group
        parallel.configure(process_group, world_size)     # sync-BN statistics exchange + gradient all-reduce
        self.flat_p, self.flat_g = flatten_parameters(model)
        self.exp_avg = self.exp_avg_sq = self.beta_pow = None
        self.momentum_buf = self.lr_dev = None
        if sgd:
            self.momentum_buf = torch.zeros_like(self.flat_p)
            # the rate the kernel reads at every launch (set_lr): a captured step follows a schedule
            self.lr_dev = torch.full((1,), lr, dtype=torch.float32, device=self.flat_p.device)
        else:
            self.exp_avg = torch.zeros_like(self.flat_p)
            self.exp_avg_sq = torch.zeros_like(self.flat_p)
            self.beta_pow = torch.ones(2, dtype=torch.float32, device=self.flat_p.device)
        # SGD with weight decay: device table of the flat buffer's rows that belong to parameters the loss reaches, built
        # before the first optimizer step when there are others (grad_free below); None: every element is stepped
        self.live = None
        self.use_graph = use_graph
        if use_graph and world_size > 1 and _backend_of(process_group) != "nccl":
            # host-staged collectives (gloo: rehearsals and tests on fewer GPUs than ranks) cannot be part of a hipGraph
            import sys
            sys.stderr.write("[TrainStep] process group backend %r cannot be captured: running WITHOUT a graph\n" % _backend_of(process_group))
            self.use_graph = False
        # Weight gradients on a second captured stream: on one GPU every kernel fills the chip and the overlap buys nothing
        # (measured 31.8 ms without vs 32.5 ms with), but under data parallelism the main stream sits in ~400 latency-bound
        # sync-BN all-reduces per step — the weight gradients then run inside those waits.
        # Single GPU, opt-in (SDHIP_TUNE_WGRAD_OVERLAP=1): the side stream carries the decoder's grouped weight gradients, in
        # grids limited to part of the chip, beside the DenseNet backward chain (StepContext.overlap_point).  Measured on
        # one box (ms/step): off 21.29 / 21.31; grids of 64 / 128 / 192 / 256 workgroups 27.5 / 21.9 / 21.5 / 21.7 — the chain's
        # small latency-bound kernels lose what the overlap hides (~2.8 ms slower beside the streaming grids), as in round 2.
        self.overlap_wgrad = world_size == 1 and use_side_stream is None and _lib.TUNE_WGRAD_OVERLAP and not _lib.DIAG_NO_WGRAD_GROUP
        if use_side_stream is None:
            use_side_stream = world_size > 1 or self.overlap_wgrad
        self.use_side_stream = use_side_stream and not _lib.DIAG_NO_SIDE   # timing diagnostics only
        self.graph = None
        self.static = None
        self.loss = None
        # per-step services (ops.StepContext): the first eager step measures / records, later steps use them
        self.ctx = ops.StepContext(self.flat_p.device)
        self.ctx.nbt = []
        if self.freeze_bn:
            # frozen norms are constants of a step: one batched launch at its head writes every folded pack, bias and
            # scale / shift table from the live parameters (recorded during the measuring step)
            self.ctx.fold = ops.FoldState(dtype, self.flat_p.device, train=True, fold=self.fold_bn)
        # built by _arm: every pack source, and weight, gamma and beta of every fold row, is a slice of THIS step's flat buffer
        self.tables = step.Tables(dtype, self.flat_p.device, ("weight", "gamma", "beta"), (),
                                  "fold table holds a source outside this step's parameter buffer",
                                  "weight-pack table holds a source outside this step's parameter buffer")
        self.steps_done = 0       # optimizer steps actually EXECUTED (eager steps + graph replays; the recording pass of a capture runs nothing)
        self._capture_fault = None   # tests: a callable invoked inside the capture to make it fail
        self.debug_graph = False     # tests: keep the captured hipGraph inspectable (_lib.graph_node_counts)
        # multitask and warp models: positions (in model.parameters() order) of the parameters the loss never reaches (mode
        # 2's unused decoder; the warp networks' key-only members), found on the first step.  torch.optim.Adam keeps no
        # state for them (their .grad stays None), so a saved optimizer state omits them as well
        # (checkpoint.optimizer_state_dict); here their gradient slice stays 0, their moments stay 0 and the fused Adam
        # leaves them bit-identical (update 0 / (0 + eps)).  SGD with weight decay would move them (d = wd * p), so it looks
        # for them in every model and steps only the rows of the others (self.live)
        self.grad_free = None
        # dropout streams differ per rank (the reference's ranks draw from independently seeded generators) and advance
        # once per step on the device, so that graph replays see new masks (ops.rng_seed_tensor)
        # (the tensor belongs to this step's context: creating a second TrainStep does not restart the first one's stream)
        self.ctx.seed = torch.full((1,), ops.rng_seed_value(_rank_of(process_group) if world_size > 1 else 0), dtype=torch.int64,
                                   device=self.flat_p.device)

    # -- pieces ---------------------------------------------------------------------------------
    def _arm(self):
        """After the first (measuring) step: allocate the zero arena, freeze the weight packs into one batched
        launch, switch parameter gradients to direct accumulation into the flat buffer."""
        self.ctx.allocate_arena()
        rows = ops.pack_descriptors(self.dtype, owners=self.model.parameters())   # this model's weights only
        fold = self.ctx.fold
        if fold is not None:
            fold.finish()
        self.tables.build(fold.rows() if fold is not None else [], rows, ops.ByteSpans.of([self.flat_p]))
        self.ctx.frozen_pack = self.pack_desc is not None
        self.ctx.direct_grads = True
        if self.use_side_stream:
            self.ctx.side = torch.cuda.Stream()
            self.ctx.overlap = self.overlap_wgrad
        self.nbt_tensors = [t for t, _ in self.ctx.nbt]
        self.nbt_incs = [int(i) for _, i in self.ctx.nbt]

    pack_desc = property(lambda self: self.tables.pack_desc)
    fold_desc = property(lambda self: self.tables.fold_desc)

    def forward_backward(self, left, right, seg, disp, first=True):
        """first: this call opens an accumulation cycle — the flat gradient buffer is cleared; later calls of the cycle add."""
        if self.freeze_bn:
            freeze_bn(self.model)           # a model.train() since the last pass must not unfreeze
        for name, blk in self._dense_blocks:
            densenet.block_training(blk, name)      # a half-frozen dense block raises here, before any launch
        ops.set_step_context(self.ctx)
        self.ctx.begin_step()       # one memset clears every zero-initialised workspace of the step
        if first:
            self.flat_g.zero_()
        self.tables.launch()        # weights change every step: folds and packs (forward and data-grad orientation) are rewritten
        if self.ctx.fold is not None:
            self.ctx.fold.live = True       # packs and tables hold this step's weights until the optimizer moves them
        try:
            return self._forward_backward(left, right, seg, disp)
        finally:
            if self.ctx.fold is not None:
                self.ctx.fold.live = False

    def _forward_backward(self, left, right, seg, disp):
        mt, three = getattr(self.model, "multiTaskLoss", 0), getattr(self.model, "three_outputs", False)
        outs = step.model_outputs(self.model, self.dtype, left, right, seg, disp)
        if self.loss_fn is not None and getattr(self.loss_fn, "wants_images", False):
            loss = self.loss_fn(outs, seg, disp, left=left, right=right)      # StepLoss: terms that read the input images
        elif self.loss_fn is not None:
            loss = self.loss_fn(outs, seg, disp)
        else:
            # a photo_outputs model (warp.minidsnetDivideDisp2) compares its warped right image with the f32 left image
            images = dict(left=left) if getattr(self.model, "photo_outputs", False) else {}
            loss = step.default_loss(self.model, outs, seg, disp, use_lovasz=self.use_lovasz, loss=self.seg_loss,
                                     class_weights=self.class_weights, **images)
        if self.grad_free is None and (mt or three or self.freeze_bn or (self.optimizer == "sgd" and self.weight_decay != 0)):
            self.grad_free = _unreached_parameters(self.model, loss)
        if self.metrics is not None and (self.loss_fn is None or isinstance(self.loss_fn, (StepLoss, EdgeStepLoss))):    # the default heads
            self.metrics.update(outs[2].detach(), seg, outs[1].detach(), disp)
        loss.backward()
        self.ctx.join()             # weight gradients ran on the side stream
        return loss.detach()

    def all_reduce(self):
        parallel.all_reduce_sum_(self.flat_g)   # one RCCL sum over xGMI per step; Adam divides by world_size

    def optimizer_step(self):
        grad_scale = 1.0 / (self.world_size * self.accumulate)
        if self.optimizer == "sgd":
            if self.live is None and self.weight_decay != 0 and self.grad_free:
                # once, on the first (eager) step: the table exists before any capture
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.SdhipError("TrainStep: the live table of the SGD step cannot be built inside a capture")
                self.live = torch.tensor(live_ranges(self.model, self.grad_free), dtype=torch.int64, device=self.flat_p.device)
            live = self.live if self.weight_decay != 0 else None
            call("sdhip_sgd_step", ptr(self.flat_p), ptr(self.flat_g), ptr(self.momentum_buf), ptr(self.lr_dev), self.flat_p.numel(),
                 self.momentum, self.weight_decay, grad_scale, ptr(live), 0 if live is None else live.shape[0], stream_ptr())
        else:
            call("sdhip_adam_step", ptr(self.flat_p), ptr(self.flat_g), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.beta_pow),
                 self.flat_p.numel(), self.lr, self.betas[0], self.betas[1], self.eps, 0.0, grad_scale, stream_ptr())
        ops.invalidate_packed_weights()

    def set_lr(self, lr):
        """Learning rate of the following steps.  SGD: also written to `lr_dev` on the current stream, so it reaches eager
        steps and replays of a captured step alike - legal before and after the capture and between replays.  Adam's rate
        is a by-value argument of its kernel, fixed in the hipGraph: after a capture this raises."""
        if torch.cuda.is_current_stream_capturing():
            raise _lib.SdhipError("TrainStep.set_lr: called while a stream is capturing")
        if self.optimizer != "sgd" and self.graph is not None:
            raise _lib.SdhipError("TrainStep.set_lr: Adam's learning rate is part of the captured hipGraph; use optimizer='sgd' "
                                  "for a schedule, or set the rate before the capture")
        self.lr = float(lr)
        if self.optimizer == "sgd":
            self.lr_dev.fill_(self.lr)

    def flush(self):
        """Close an open accumulation cycle now: all-reduce and step, eagerly, on what has accumulated - the reference also
        steps at the last batch of an epoch (torch_implementation.py:390).  The scale stays 1 / (world_size * accumulate): the
        reference divides every micro-loss by K whatever the length of the tail.  (The loss a call of TrainStep returns is
        NOT divided by K; the reference logs loss / K.)  Returns True if a step was taken; the next call then opens a
        cycle, eagerly or by replay.  False, and nothing done, if no cycle was open."""
        if self._micro == 0:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise _lib.SdhipError("TrainStep.flush: called while a stream is capturing")
        self.all_reduce()
        self.optimizer_step()
        self._micro = 0
        self.steps_done += 1
        return True

    def _phase(self):
        """(first, last) of the call about to run within its accumulation cycle; advances the cycle counter."""
        first = self._micro == 0
        self._micro += 1
        last = self._micro >= self.accumulate
        if last:
            self._micro = 0
        return first, last

    def _eager(self, left, right, seg, disp, phase=None):
        """One (micro-)step.  phase = (first, last) of the accumulation cycle (None: decided by the call counter)."""
        first, last = phase if phase is not None else self._phase()
        loss = self.forward_backward(left, right, seg, disp, first)
        if last:
            self.all_reduce()
            self.optimizer_step()
        if self.ctx.arena is None:
            self._arm()
        elif self.nbt_tensors:
            torch._foreach_add_(self.nbt_tensors, self.nbt_incs)   # BatchNorm.num_batches_tracked, one launch
        # next step draws new dropout masks.  A device-side add AFTER the backward pass (which regenerates this step's
        # masks from the same seed): captured into the graph, so every replay advances it too.
        self.ctx.seed.add_(1)
        if last and not torch.cuda.is_current_stream_capturing():
            self.steps_done += 1
        return loss

    # -- public ---------------------------------------------------------------------------------
    def capture(self, left, right, seg, disp, warmup=2):
        """Warm up eagerly on a side stream, then record forward+backward(+all-reduce)+Adam as one hipGraph."""
        self.static = [t.clone() for t in (left, right, seg, disp)]
        # warm-up and capture share ONE side stream: autograd's AccumulateGrad nodes remember the stream they were created
        # on (the first forward), and a different capture stream would make every parameter gradient cross streams
        cap = torch.cuda.Stream()
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            for _ in range(warmup * self.accumulate - self._micro):      # whole accumulation cycles: the capture starts at a cycle boundary
                self._eager(*self.static)
        torch.cuda.current_stream().wait_stream(cap)
        torch.cuda.synchronize()
        # data parallel: the RCCL watchdog thread polls events while we capture; thread-local capture errors keep its
        # (legal) calls from invalidating the capture of this thread
        mode = "thread_local" if self.world_size > 1 else "global"
        K = self.accumulate
        phases = [(True, True)] if K == 1 else ([(True, False), (False, True)] if K == 2 else [(True, False), (False, False), (False, True)])
        with step.Recording(cap, self.flat_p.device, "TrainStep", error_mode=mode, keep_graph=self.debug_graph, reset_generator=False,
                            also_close=lambda: [self.ctx.side] if self.ctx.side is not None else []) as rec:
            self._gen_state = rec.gen_state
            # one graph per kind of call of an accumulation cycle: the opening one clears the gradient buffer, the closing one
            # holds the all-reduce and Adam (accumulate = 1: one graph that does both).  The side stream is part of every
            # capture; after a failure the generator is reset by _abandon_capture, once the device has answered
            self.graphs = {ph: rec.record(lambda: self._eager(*self.static, phase=ph), self._capture_fault) for ph in phases}
        torch.cuda.current_stream().wait_stream(cap)
        self.graph, self.loss = self.graphs[phases[-1]]      # the closing call's graph (accumulate = 1: the only one)
        return self

    def _abandon_capture(self):
        """A capture that raised recorded launches but executed none: device state (parameters, moments, running
        statistics, dropout seed) is that of the last eager warm-up step.  Only host-side bookkeeping of the half-recorded
        step has to be reset before eager steps continue."""
        self.graph, self.graphs, self.use_graph, self.loss = None, {}, False, None
        torch.cuda.synchronize()               # raises if the process could not be brought back: nothing can run then
        step.reset_capture_generator(self.flat_p.device, getattr(self, "_gen_state", None), "TrainStep")
        self.ctx.unpacks = []
        self.ctx.wq = []
        self.ctx.wq_keep.clear()
        self.ctx.keep.clear()
        ops.invalidate_packed_weights()

    def __call__(self, left, right, seg, disp):
        if not self.use_graph:
            return self._eager(left, right, seg, disp)
        if self.graph is None:
            try:
                self.capture(left, right, seg, disp)
            except RuntimeError as e:   # e.g. a collective that cannot be captured on this RCCL build: run eagerly, loudly
                import sys
                sys.stderr.write("[TrainStep] hipGraph capture failed (%s); continuing WITHOUT a graph\n" % str(e).splitlines()[0])
                self._abandon_capture()
                return self._eager(left, right, seg, disp)
        for dst, src in zip(self.static, (left, right, seg, disp)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        ph = self._phase()
        graph, loss = self.graphs[ph]
        graph.replay()
        if ph[1]:
            self.steps_done += 1
        return loss


def _unreached_parameters(model, loss):
    """Positions of the parameters whose AccumulateGrad node the autograd graph of `loss` does not contain."""
    reached, seen, keep, stack = set(), set(), [], [loss.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        keep.append(fn)            # visited nodes stay alive during the walk, so their ids stay unique
        v = getattr(fn, "variable", None)
        if v is not None:
            reached.add(id(v))
        stack.extend(f for f, _ in fn.next_functions)
    return [i for i, p in enumerate(model.parameters()) if id(p) not in reached]


def _backend_of(pg):
    import torch.distributed as dist
    try:
        return dist.get_backend(pg)
    except Exception:
        return None


def _rank_of(pg):
    import torch.distributed as dist
    return dist.get_rank(pg) if dist.is_available() and dist.is_initialized() else 0


def synthetic_batch(B, H, W, labels=2, device="cuda", seed=1234):
    """S-ROSeS-shaped synthetic batch (tensor contract of util/utilTorchDataLoader.py:176-258,608-630)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    left = torch.rand((B, 3, H, W), generator=g)
    right = torch.rand((B, 3, H, W), generator=g)
    lab = torch.randint(0, labels, (B, H, W), generator=g)
    seg = torch.nn.functional.one_hot(lab, labels).permute(0, 3, 1, 2).float().contiguous()
    disp = (torch.rand((B, 1, H, W), generator=g) * 8.0 * seg[:, 1:2] + 0.1).contiguous()
    return [t.to(device) for t in (left, right, seg, disp)]
