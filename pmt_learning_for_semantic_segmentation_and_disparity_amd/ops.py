"""Autograd bindings of the libsdhip.so kernels.

Tensors keep the reference's logical NCHW shapes but live in channels-last
(NHWC) memory, possibly as a channel slice of a wider slab; `nhwc_view`
returns the pixel stride the C ABI wants.  Nothing in this file computes on the
CPU or through ATen kernels: a non-GPU tensor is an error.
"""
import torch

from . import _lib
from ._lib import call, dtype_code, ptr, stream_ptr, try_call


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SdhipError("sdhip ops need GPU tensors (got %s); there is no CPU path" % t.device)


def nhwc_view(x):
    """Return (tensor, ld): x itself if its memory is NHWC with a uniform pixel stride, else a channels-last copy."""
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    ld = sw
    ok = (sc == 1 or C == 1) and ld >= C and (sh == W * ld or H == 1) and (sb == H * W * ld or B == 1)
    if W == 1:
        ok = False if (sc != 1 and C != 1) else (sh >= C and (sb == H * sh or B == 1))
        ld = sh if ok else ld
    if not ok:
        x = x.contiguous(memory_format=torch.channels_last)
        if x.stride(1) != 1 and C != 1:  # degenerate shapes: force an explicit NHWC buffer
            x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        ld = C
    return x, ld


def empty_nhwc(B, C, H, W, dtype, device):
    return torch.empty((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


def alloc_nhwc(B, C, H, W, dtype, device):
    """(tensor, ld): NHWC tensor whose pixel stride is rounded up to 8 elements (16 bytes of bf16), so that tensors
    with odd channel counts (the 65-channel concats, 1-channel maps of models/dsnet_t2.py:1128-1170) still take the
    16-byte vector / LDS-DMA paths of the conv kernels.  The pad channels are never read as data (the kernels mask
    the channel tail) and never written."""
    ld = (C + 7) & ~7
    if ld == C:
        return empty_nhwc(B, C, H, W, dtype, device), C
    return torch.empty((B, H, W, ld), dtype=dtype, device=device)[..., :C].permute(0, 3, 1, 2), ld


def aligned_view(x):
    """nhwc_view + 16-byte-aligned pixels: a tensor whose pixel stride is not a multiple of 8 elements (1- or 2-channel
    maps coming from outside the conv stack, e.g. the loss gradients) is copied once into a padded buffer, so that the
    conv kernels read it with 16-byte vectors instead of element by element."""
    xv, ld = nhwc_view(x)
    if ld % 8 == 0:
        return xv, ld
    B, C, H, W = xv.shape
    y, ldy = alloc_nhwc(B, C, H, W, xv.dtype, xv.device)
    call("sdhip_affine_act", ptr(xv), ld, ptr(y), ldy, None, 0, None, None, B * H * W, C, 1, 0, dtype_code(xv), stream_ptr())
    return y, ldy


class _CorrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in1, in2, PH, PW, dil):
        _require_gpu(in1, in2)
        if in1.shape != in2.shape or in1.dtype != in2.dtype:
            raise _lib.SdhipError("correlation inputs must have the same shape and dtype")
        B, C, H, W = in1.shape
        a, lda = nhwc_view(in1)
        b, ldb = nhwc_view(in2)
        if lda != ldb:
            a = a.contiguous(memory_format=torch.channels_last); b = b.contiguous(memory_format=torch.channels_last)
            lda = ldb = C
        out = torch.empty((B, H, W, PH, PW), dtype=in1.dtype, device=in1.device)
        call("sdhip_corr_fwd", ptr(a), ptr(b), ptr(out), B, H, W, C, lda, PH, PW, dil, PH * PW,
             dtype_code(in1), stream_ptr())
        ctx.save_for_backward(a, b)
        ctx.cfg = (PH, PW, dil, lda)
        # (B,PH,PW,H,W) view of NHWC memory, displacement fastest
        return out.permute(0, 3, 4, 1, 2)

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        PH, PW, dil, ld = ctx.cfg
        B, C, H, W = a.shape
        g = gout.permute(0, 3, 4, 1, 2)  # (B,H,W,PH,PW)
        if not g.is_contiguous():
            g = g.contiguous()
        if ld != C:
            a = a.contiguous(memory_format=torch.channels_last); b = b.contiguous(memory_format=torch.channels_last)
            ld = C
        ga = empty_nhwc(B, C, H, W, a.dtype, a.device)
        gb = empty_nhwc(B, C, H, W, a.dtype, a.device)
        call("sdhip_corr_bwd", ptr(a), ptr(b), ptr(g), ptr(ga), ptr(gb), B, H, W, C, ld, PH, PW, dil,
             PH * PW, dtype_code(a), stream_ptr())
        return ga, gb, None, None, None


def correlation(in1, in2, patch_h, patch_w, dilation_patch=1):
    return _CorrFn.apply(in1, in2, patch_h, patch_w, dilation_patch)


# ============================================================================ convolution
import weakref

class StepContext:
    """Per-step services (all optional; ops work without one).  A step installs its own context (set_step_context) before each
    pass: train.TrainStep leaves it installed, evalstep.EvalStep puts the previously installed one back on its way out.
      * zero arena: every small zero-initialised workspace of the step (statistics replicas, packed f32 weight-gradient
        accumulators, dscale/dshift replicas) is bump-allocated from ONE buffer that a single memset clears per step;
      * frozen weight packs: all weights are packed by one batched launch at step start;
      * direct gradients: parameter gradients are written (accumulated) straight into the flat gradient buffer;
      * deferred num_batches_tracked increments (one multi-tensor add per step).
    """

    def __init__(self, device):
        self.device = device
        self.arena = None
        self.offset = 0
        self.measured = 0
        self.frozen_pack = False
        self.frozen_bufs = None  # ids of the pack buffers the step's table rewrites (None: every cached pack counts as packed)
        self.direct_grads = False
        self.nbt = None          # list of (tensor, increment) recorded while measuring
        self.side = None         # second HIP stream: weight gradients run beside the data-gradient chain
        self.keep = []           # tensors the side stream still reads (kept alive until join())
        self.unpacks = []        # deferred weight-gradient unpack descriptors of the running step (direct_grads)
        self.unpack_key = None   # the descriptor rows the cached device table was built from
        self.unpack_desc = None
        self.seed = None         # device-resident dropout seed of the owning TrainStep (rng_seed_tensor)
        # Deferred weight gradients: nothing reads a weight gradient before the optimizer, so every layer's launch is queued
        # (with its operands kept alive) and join() issues them grouped by kernel instantiation — one grid per bucket instead
        # of ~200 per-layer launches that fill a quarter of the chip each (sdhip_conv2d_wgrad_group)
        self.defer_wgrad = not _lib.DIAG_NO_WGRAD_GROUP
        self.wq = []             # [(WgradItem fields...)] of the running step
        self.wq_keep = []        # operands of the queued launches
        self.wq_dt = None
        # single GPU: the queue is flushed onto the side stream, with grids limited to part of the chip, when the backward pass
        # reaches the DenseNet towers (overlap_point) — their ~400 small dependent kernels leave most CUs idle
        self.overlap = False
        # a FoldState switches conv_bn_act / _bn_finalize to the folded path: every eval-mode BatchNorm of an eval step
        # (evalstep.EvalStep), the frozen BatchNorms of a training step (train.TrainStep(freeze_bn=True))
        self.fold = None

    def flush_wgrads(self, max_wg=0):
        """Issue the queued weight-gradient launches (grouped) on the current stream; max_wg > 0 limits every grid."""
        if not self.wq:
            return
        import ctypes
        items = (_lib.WgradItem * len(self.wq))()
        for it, row in zip(items, self.wq):
            (it.x, it.dy, it.dw_packed, it.dbias, it.in_scale, it.in_shift, it.B, it.H, it.W, it.Cin, it.ldx, it.Ho, it.Wo, it.Cout,
             it.lddy, it.kh, it.kw, it.stride, it.dil, it.pad_t, it.pad_l, it.D, it.Do, it.kd, it.sd, it.pad_d, it.in_relu, it.groups) = row
        n, dt = len(self.wq), self.wq_dt
        self.wq = []
        try:
            call("sdhip_conv2d_wgrad_group", ctypes.cast(items, ctypes.c_void_p), n, int(max_wg), dt, stream_ptr())
        finally:
            self.wq_keep.clear()

    def flush_to_side(self, min_items=12, max_wg=0):
        """Data parallel: the main stream spends most of the backward pass in latency-bound sync-BN exchanges — buckets of
        queued weight gradients run beside it on the side stream as soon as they are worth a grid."""
        if self.side is None or len(self.wq) < min_items:
            return
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)                  # the queued operands were produced on the main stream
        self.keep.extend(self.wq_keep)               # the caching allocator must not recycle them before join()
        with torch.cuda.stream(self.side):
            self.flush_wgrads(max_wg)

    def overlap_point(self):
        """Called where the backward pass enters a long chain of small dependent kernels (a DenseNet block): what is queued
        so far goes to the side stream in grids of at most TUNE_OVERLAP_WG workgroups, which leave the other CUs to the chain."""
        if self.overlap:
            self.flush_to_side(min_items=1, max_wg=_lib.TUNE_OVERLAP_WG)

    def join(self):
        """Call after backward, before the optimizer: the queued weight gradients are launched (grouped), the main stream
        waits for the side stream, then ONE launch adds every packed weight-gradient accumulator of the step into the flat
        gradient buffer."""
        self.flush_wgrads()
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
        if self.unpacks:
            key = tuple(self.unpacks)
            if key != self.unpack_key:   # arena offsets and gradient slices repeat step after step: built once
                if torch.cuda.is_current_stream_capturing():
                    raise _lib.SdhipError("weight-gradient layout changed between the warm-up step and graph capture")
                self.unpack_desc = torch.tensor(self.unpacks, dtype=torch.int64, device=self.device)
                self.unpack_key = key
            call("sdhip_conv_unpack_batch", ptr(self.unpack_desc), len(self.unpacks), self.unpack_dt, stream_ptr())
            self.unpacks = []
        self.keep.clear()

    def begin_step(self):
        self.unpacks = []
        self.wq = []
        self.wq_keep.clear()
        if self.arena is not None:
            self.offset = 0
            self.arena.zero_()

    def zeros(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        nbytes = ((n * torch.empty((), dtype=dtype).element_size() + 255) // 256) * 256
        if self.arena is None:
            self.measured += nbytes
            return torch.zeros(shape, dtype=dtype, device=self.device), False
        if self.offset + nbytes > self.arena.numel():
            raise _lib.SdhipError("zero arena exhausted (%d + %d > %d)" % (self.offset, nbytes, self.arena.numel()))
        t = self.arena[self.offset:self.offset + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)
        self.offset += nbytes
        return t, True

    def allocate_arena(self):
        self.arena = torch.zeros(int(self.measured * 1.05) + 4096, dtype=torch.uint8, device=self.device)


_ctx = [None]


def set_step_context(ctx):
    _ctx[0] = ctx


def overlap_point():
    c = _ctx[0]
    if c is not None:
        c.overlap_point()


def _zeros(shape, dtype, device):
    """(tensor of zeros, prezeroed flag for the C ABI)."""
    c = _ctx[0]
    if c is not None:
        return c.zeros(shape, dtype)
    return torch.zeros(shape, dtype=dtype, device=device), False


def _grad_target(param):
    """The flat-gradient slice to accumulate a parameter gradient into, or None (then the Function returns the gradient)."""
    c = _ctx[0]
    if c is not None and c.direct_grads and param is not None and param.is_leaf and param.grad is not None:
        return param.grad
    return None


_pack_cache = {}   # id(weight parameter) -> (weakref, {(mode, dtype): (version, packed)})
_pack_generation = [0]


def invalidate_packed_weights():
    """Call after parameters were changed outside autograd's version tracking (the fused Adam kernel)."""
    _pack_generation[0] += 1


def _cache_entry(weight):
    k = id(weight)
    hit = _pack_cache.get(k)
    if hit is None or hit[0]() is not weight:
        hit = (weakref.ref(weight, lambda _r, k=k: _pack_cache.pop(k, None)), {})
        _pack_cache[k] = hit
    return hit[1]


def _pack_params(kind, mode, Cout, Cin, T):
    """(M, K, stride_m, stride_k, flip) of include/sdhip.h for a Conv2d / stride-1 ConvTranspose2d weight."""
    if kind == 'conv':       # weight (Cout, Cin, kh, kw)
        return (Cout, Cin, Cin * T, T, 0) if mode == 'fwd' else (Cin, Cout, T, Cin * T, 1)
    if kind == 'deconv':     # weight (Cin, Cout, kh, kw), run as a correlation with flipped taps
        return (Cout, Cin, T, Cout * T, 1) if mode == 'fwd' else (Cin, Cout, Cout * T, T, 0)
    raise _lib.SdhipError("unknown conv kind %r" % kind)


def packed_weight(weight, kind, mode, dtype):
    """Pack an f32 parameter for the kernels (cached per parameter version, repacked after each optimizer step)."""
    Cout, Cin = (weight.shape[0], weight.shape[1]) if kind == 'conv' else (weight.shape[1], weight.shape[0])
    kd = weight.shape[2] if weight.dim() == 5 else 1
    T = weight.shape[-2] * weight.shape[-1]
    ent = _cache_entry(weight)
    key = (kind, mode, dtype)
    hit = ent.get(key)
    c = _ctx[0]
    frozen = hit is not None and c is not None and c.frozen_pack
    if frozen and (c.frozen_bufs is None or id(hit[1]) in c.frozen_bufs):
        return hit[1]           # packed by the batched launch at step start (step.Tables.launch)
    ver = (weight._version, _pack_generation[0])
    if not frozen and hit is not None and hit[0] == ver and not torch.cuda.is_current_stream_capturing():
        return hit[1]
    dt = _lib.code_of(dtype)
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    rows = _pack_rows(w, kind, mode, dt)
    per = _lib.packed_elems(rows[0][2], rows[0][3], T, dt)
    # frozen, but no row of the step's table rewrites this pack: it is repacked here, at every use, INTO the cached buffer
    # (another step's replayed table or graph may hold its address: a cached buffer is rewritten, never replaced)
    buf = hit[1] if frozen else torch.empty(per * kd, dtype=dtype, device=weight.device)
    es = buf.element_size()
    for src_off, dst_blk, M, K, T_, sm, sk, flip in rows:   # one launch per depth tap (3-D) / one in all (2-D)
        call("sdhip_conv_pack_weights", ctypes_ptr(w.data_ptr() + 4 * src_off), ctypes_ptr(buf.data_ptr() + es * per * dst_blk),
             M, K, T_, sm, sk, flip, dt, stream_ptr())
    ent[key] = (ver, buf)
    return buf


def ctypes_ptr(addr):
    import ctypes
    return ctypes.c_void_p(addr)


def _pack_rows(w, kind, mode, dt):
    """[(src element offset, destination depth block, M, K, T, stride_m, stride_k, flip)] — one row per depth tap.
    A 3-D weight (.., kd, kh, kw) is packed [kd][q][t][m][c]; with flip (data-grad / transposed orientation) the depth
    taps are reversed as well as the in-plane taps."""
    Cout, Cin = (w.shape[0], w.shape[1]) if kind == 'conv' else (w.shape[1], w.shape[0])
    kd = w.shape[2] if w.dim() == 5 else 1
    T = w.shape[-2] * w.shape[-1]
    M, K, sm, sk, flip = _pack_params(kind, mode, Cout, Cin, T * kd)
    # _pack_params' strides are in units of "taps per (m,k) pair" = kd*T for volumes; the tap index inside one depth tap is < T
    rows = []
    for kdi in range(kd):
        rows.append((kdi * T, (kd - 1 - kdi) if flip else kdi, M, K, T, sm, sk, flip))
    return rows


class ByteSpans:
    """[begin, end) byte ranges of device memory, in any order: what a step owns.  Not merged: a range across a seam lies in neither."""

    def __init__(self, spans=()):
        self.spans = sorted((int(b), int(e)) for b, e in spans)

    @classmethod
    def of(cls, tensors):
        return cls((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in tensors if t.numel())

    def contains(self, addr, nbytes=1):
        import bisect
        i = bisect.bisect_right(self.spans, (addr, float("inf"))) - 1
        return i >= 0 and self.spans[i][0] <= addr and addr + nbytes <= self.spans[i][1]


def _pack_owned(w, own, spans):
    """Does the cached weight `w` belong to a step: it is one of the step's tensors (`own`: ids; None: everything does), or -
    `spans`: the ByteSpans of the step's parameters - a dense f32 view that lies inside one of them (HANet hands the kernels a
    (Cout, Cin, k, 1) view of its Conv1d weights: same memory, another tensor)."""
    if own is None or id(w) in own:
        return True
    if spans is None or not w.is_contiguous() or w.dtype != torch.float32 or not w.numel():
        return False
    return spans.contains(w.data_ptr(), 4 * w.numel())


def pack_descriptors(dtype, owners=None, spans=None, modes=None):
    """int64 [n][8] descriptor table {src, dst, M, K, T, stride_m, stride_k, flip} of the cached packs of `dtype` that belong
    to the parameters in `owners` (an iterable of tensors; None: every cached pack).  A training step must pass ITS model's
    parameters: the table is replayed step after step (inside a hipGraph), so a row of another model's weight — or of a
    per-step temporary such as the space-to-depth stem weight — would keep reading and writing that tensor's memory after
    it has been freed (a GPU memory fault once the allocator has returned the block: found by the full test suite, where
    several models are alive at once).  spans: also the cached views inside those byte ranges (_pack_owned).  modes: only the
    packs of these orientations (an eval forward reads 'fwd' packs only)."""
    own = None if owners is None else {id(t) for t in owners}
    rows = []
    # (a snapshot: the weak-reference callbacks of parameters that die meanwhile — a discarded model being collected — pop
    #  their entries, which must not happen under a live dictionary iterator)
    for ref, ent in list(_pack_cache.values()):
        w = ref()
        if w is None or not _pack_owned(w, own, spans):
            continue
        for (kind, mode, dt), (_, buf) in list(ent.items()):
            if dt != dtype or (modes is not None and mode not in modes):
                continue
            dtc = _lib.code_of(dt)
            if kind == 'phase':     # the eight sub-pixel sub-kernels of a 3x3x3 stride-2 weight: one single-tap row per tap
                for src_off, dst_off, M, K, T, sm, sk, flip in _phase_rows(w, dtc)[0]:
                    rows.append([w.data_ptr() + 4 * src_off, buf.data_ptr() + buf.element_size() * dst_off, M, K, T, sm, sk, flip])
                continue
            prow = _pack_rows(w, kind, mode, dtc)
            per = _lib.packed_elems(prow[0][2], prow[0][3], prow[0][4], dtc)
            for src_off, dst_blk, M, K, T, sm, sk, flip in prow:
                rows.append([w.data_ptr() + 4 * src_off, buf.data_ptr() + buf.element_size() * per * dst_blk, M, K, T, sm, sk, flip])
    return rows


def cached_packs(dtype, owners, spans=None, modes=None):
    """The cached pack buffers that pack_descriptors(dtype, owners, spans, modes) names: whoever replays such a table keeps them."""
    own = {id(t) for t in owners}
    return [buf for ref, ent in list(_pack_cache.values()) if ref() is not None and _pack_owned(ref(), own, spans)
            for (kind, mode, dt), (_, buf) in list(ent.items()) if dt == dtype and (modes is None or mode in modes)]


# ---- eval step: BatchNorm folded into the packs (sdhip_conv_pack_fold_batch) ------------------------------------------------
FOLD_COLS = 16      # int64 columns of a row of sdhip_conv_pack_fold_batch (include/sdhip.h)
FOLD_ACTS = (0, 1, 2)   # activations the epilogue of sdhip_conv2d_fwd takes


def _eps_bits(eps):
    import struct
    return struct.unpack("<I", struct.pack("<f", float(eps)))[0]


def _addr(t):
    return 0 if t is None else t.data_ptr()


def fold_row(weight, kind, bn, conv_bias, pack, bias_out):
    """One "fold" row of sdhip_conv_pack_fold_batch: the forward pack of a 2-D (Cout,Cin,kh,kw) / (Cin,Cout,kh,kw) weight
    (M, K, T, strides and flip exactly those of _pack_rows) scaled by `bn`'s eval-mode scale; bias_out receives the shift."""
    if weight.dim() != 4:
        raise _lib.SdhipError("fold_row: only 2-D convolution weights fold")
    (src_off, _, M, K, T, sm, sk, flip), = _pack_rows(weight, kind, 'fwd', None)
    return [0, weight.data_ptr() + 4 * src_off, _addr(pack), _addr(bias_out), M, K, T, sm, sk, flip, _addr(bn.weight), _addr(bn.bias),
            _addr(bn.running_mean), _addr(bn.running_var), _eps_bits(bn.eps), _addr(conv_bias)]


def table_row(bn, groups, scale, shift):
    """One "table" row: scale / shift [groups][C] of a BatchNorm that is not folded."""
    return [1, 0, _addr(scale), _addr(shift), bn.num_features, groups, 0, 0, 0, 0, _addr(bn.weight), _addr(bn.bias),
            _addr(bn.running_mean), _addr(bn.running_var), _eps_bits(bn.eps), 0]


def row_sources(row):
    """The addresses a fold_row / table_row makes sdhip_conv_pack_fold_batch READ, by name (0: absent): whoever replays the
    row checks them against the memory it owns.  `weight` is None for a table row, which has none."""
    return {"weight": row[1] if row[0] == 0 else None, "gamma": row[10], "beta": row[11], "mean": row[12], "var": row[13], "conv_bias": row[15]}


class FoldLayer:
    __slots__ = ("weight", "bn", "kind", "pack", "bias_out", "ok")


class FoldState:
    """What an eval step (evalstep.EvalStep) knows about its model's BatchNorms.  While `measuring` (one eager pass) every
    eligible conv + BatchNorm layer gets a private folded pack and bias, and every other eval-mode BatchNorm a slot in the
    scale / shift tables; afterwards the records are fixed: a layer or BatchNorm the pass did not meet runs as it does without
    an eval step."""

    def __init__(self, dtype, device, train=False, fold=True):
        self.dtype, self.device = dtype, device
        # train: the state of a training step (train.TrainStep).  It serves FROZEN BatchNorms (bn_frozen) of grad-enabled passes,
        # and only while `live`: between the batched launch at the head of a step and the end of its backward pass, when packs
        # and tables hold the current weights.  fold False: tables only (TrainStep(fold_bn=False))
        self.train, self.fold, self.live = train, fold, not train
        self.measuring = True
        self.layers = {}       # (id(weight), id(bn), kind) -> FoldLayer
        self.tables = {}       # (id(bn), groups) -> [bn, groups, scale view, shift view]
        self.table_buf = None
        self.calls = 0         # folded layer calls of the running step

    def _launch(self, rows):
        desc = torch.tensor(rows, dtype=torch.int64, device=self.device)
        call("sdhip_conv_pack_fold_batch", ptr(desc), len(rows), _lib.code_of(self.dtype), stream_ptr())

    def layer(self, weight, bn, kind):
        if not self.fold:
            return None
        key = (id(weight), id(bn), kind)
        rec = self.layers.get(key)
        if rec is None and self.measuring:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.SdhipError("FoldState: a layer cannot be recorded inside a capture")
            rec = FoldLayer()
            rec.weight, rec.bn, rec.kind, rec.ok = weight, bn, kind, True
            (_, _, M, K, T, _, _, _), = _pack_rows(weight, kind, 'fwd', None)
            dt = _lib.code_of(self.dtype)
            rec.pack = torch.empty(_lib.packed_elems(M, K, T, dt), dtype=self.dtype, device=self.device)
            rec.bias_out = torch.empty(M, dtype=torch.float32, device=self.device)
            self._launch([fold_row(weight.detach(), kind, bn, None, rec.pack, rec.bias_out)])
            self.layers[key] = rec
        return rec

    def table(self, bn, groups):
        """(scale, shift) views [groups][C] of the precomputed tables, or None (measuring: the slot is recorded)."""
        key = (id(bn), groups)
        rec = self.tables.get(key)
        if rec is None:
            if self.measuring:
                self.tables[key] = [bn, groups, None, None]
            return None
        return (rec[2], rec[3]) if rec[2] is not None else None

    def finish(self):
        """End of the measuring pass: allocate the tables; rows() then describes every record."""
        self.measuring = False
        slot = lambda bn, g: (g * bn.num_features + 3) & ~3      # 16-byte aligned tables: the consumers read them as f32x4
        n = sum(2 * slot(bn, g) for bn, g, _, _ in self.tables.values())
        self.table_buf = torch.empty(max(n, 4), dtype=torch.float32, device=self.device)
        off = 0
        for rec in self.tables.values():
            bn, g = rec[0], rec[1]
            k, step = g * bn.num_features, slot(bn, g)
            rec[2] = self.table_buf[off:off + k].view(g, bn.num_features)
            rec[3] = self.table_buf[off + step:off + step + k].view(g, bn.num_features)
            off += 2 * step

    def rows(self):
        rows = [fold_row(r.weight.detach(), r.kind, r.bn, None, r.pack, r.bias_out) for r in self.layers.values() if r.ok]
        rows += [table_row(bn, g, sc, sh) for bn, g, sc, sh in self.tables.values()]
        return rows


def bn_frozen(bn):
    """`-freeze_bn 1` (torch_implementation.py:235-241) as a property of the module: eval mode and neither affine parameter
    requires a gradient.  Such a norm is a constant per-channel scale / shift of the step."""
    return not bn.training and not _wants_grad(bn.weight, bn.bias)


def _wants_grad(gamma, beta):
    return (gamma is not None and gamma.requires_grad) or (beta is not None and beta.requires_grad)


def _fold_state(bn=None):
    """The FoldState of the installed context when a folded path applies: an eval step's for an eval-mode BatchNorm without
    autograd, a training step's for a frozen BatchNorm while that step's pass runs (`live`; the grad mode says nothing
    there: it is off inside every autograd node's forward)."""
    c = _ctx[0]
    if c is None or c.fold is None or (bn is not None and bn.training):
        return None
    if c.fold.train:
        return c.fold if c.fold.live and bn is not None and bn_frozen(bn) else None
    return None if torch.is_grad_enabled() else c.fold


def _folded_conv_bn_act(fold, x, weight, bn, spec, act, residual, groups, views=None):
    """act(BatchNorm_eval(conv(x))) (+ residual) as ONE sdhip_conv2d_fwd over the folded pack (+ one copy that seeds the output
    with the residual: never more launches than the unfolded path's three).  None: this layer does not fold (the caller runs
    the unfolded path).  views: a list that receives (xv, ldx, ldy) of the launch (the training node saves them)."""
    if act not in FOLD_ACTS or spec.D != 1 or spec.Do != 1 or weight.dim() != 4 or bn.running_mean is None or x.dtype != fold.dtype:
        return None
    rec = fold.layer(weight, bn, spec.kind)
    if rec is None or not rec.ok:
        return None
    _require_gpu(x, weight)
    B, Cin, H, W = x.shape
    xv, ldx = aligned_view(x)
    Cout = spec.cout(weight)
    y, ldy = alloc_nhwc(B, Cout, spec.Ho, spec.Wo, x.dtype, x.device)
    if residual is not None:
        # the skip of d3 / d4 (Conv2DownUp): y starts as the residual and the convolution accumulates onto it - the epilogue sums
        # act(conv + bias) and the skip in f32 and rounds once, where an add pass behind the convolution would round twice
        if residual.shape != y.shape or residual.dtype != y.dtype:
            raise _lib.SdhipError("conv_bn_act: residual does not match the output")
        rv, ldres = nhwc_view(residual)
        call("sdhip_affine_act", ptr(rv), ldres, ptr(y), ldy, None, 0, None, None, B * spec.Ho * spec.Wo, Cout, 1, 0, dtype_code(x),
             stream_ptr())
    ran = try_call("sdhip_conv2d_fwd", ptr(xv), ptr(rec.pack), ptr(y), ptr(rec.bias_out), None, None, None, 0, 1,
                   B, H, W, Cin, ldx, spec.Ho, spec.Wo, Cout, ldy, spec.kh, spec.kw, spec.stride, spec.dil, spec.pad_t, spec.pad_l,
                   *spec.depth(), 0, groups, act, int(residual is not None), dtype_code(x), stream_ptr())
    if not ran:
        rec.ok = False      # no kernel with this epilogue for the shape: the layer stays on the unfolded path for good
        return None
    fold.calls += 1
    if views is not None:
        views.append((xv, ldx, ldy))
    return y


class _NoFold(Exception):
    """The folded kernel does not take this layer's shape: conv_bn_act runs the table form instead (once; the record remembers)."""


class _FoldedConvBNActFn(torch.autograd.Function):
    """y = act(BatchNorm(conv(x))) with a FROZEN BatchNorm (bn_frozen) inside a training step: ONE sdhip_conv2d_fwd over the
    pack the step's batched launch folded the norm into, with the shift as bias and the activation in the epilogue.  The node
    keeps x and the activated y; the raw convolution output never exists.  Backward: sdhip_act_out_bwd turns gy into the
    gradient of the raw output, g * act'(y) * scale, and the data and weight gradients run on that with the RAW weight
    (dW_raw = wgrad(x, g act' s) exactly: the fold scales whole output channels).  No residual: with a skip the epilogue
    rounds act(.) + skip once and the activated value the backward needs is never stored (conv_bn_act keeps the table form)."""

    @staticmethod
    def forward(ctx, x, weight, fold, spec, bn, act, groups, in_slot, in_bn):
        views = []
        y = _folded_conv_bn_act(fold, x, weight, bn, spec, act, None, groups, views)
        if y is None:
            raise _NoFold()
        (xv, ldx, ldy), = views
        # scale [1][Cout] of the same norm: a row of the step's table once the step is armed (no launch)
        scale = _bn_finalize(None, 1, bn, 0, 1)[0]
        ctx.spec, ctx.act, ctx.ldx, ctx.ldy, ctx.in_slot, ctx.in_bn = spec, act, ldx, ldy, in_slot, in_bn
        ctx.save_for_backward(xv, weight, y, scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, y, scale = ctx.saved_tensors
        spec = ctx.spec
        B, Cout = y.shape[0], y.shape[1]
        g, ldg = nhwc_view(gy)
        graw, ldgr = alloc_nhwc(B, Cout, spec.Ho, spec.Wo, y.dtype, y.device)
        call("sdhip_act_out_bwd", ptr(g), ldg, ptr(y), ctx.ldy, ptr(graw), ldgr, ptr(scale), B * spec.Ho * spec.Wo, Cout, 1, ctx.act,
             dtype_code(y), stream_ptr())
        acc, addend = _take_parked(ctx.in_slot, xv, ctx.needs_input_grad[0])
        gx, gw, _ = _conv_backward(spec, xv, ctx.ldx, weight, graw, ldgr, None, None, False, 1, ctx.needs_input_grad[0],
                                   ctx.needs_input_grad[1], acc_into=acc, addend=addend, bn_slot=ctx.in_bn)
        return gx, gw, None, None, None, None, None, None, None


class ConvSpec:
    """Geometry of one convolution in correlation form (what the kernels take)."""
    __slots__ = ("kind", "kh", "kw", "stride", "dil", "pad_t", "pad_l", "Ho", "Wo", "D", "Do", "kd", "sd", "pad_d")

    def __init__(self, kind, kh, kw, stride, dil, pad_t, pad_l, Ho, Wo, D=1, Do=1, kd=1, sd=1, pad_d=0):
        self.kind, self.kh, self.kw, self.stride, self.dil = kind, kh, kw, stride, dil
        self.pad_t, self.pad_l, self.Ho, self.Wo = pad_t, pad_l, Ho, Wo
        # depth axis of 3-D convolutions over [B][D][H][W][C] volumes (tensors of B*D "images"); 2-D: all ones / zero
        self.D, self.Do, self.kd, self.sd, self.pad_d = D, Do, kd, sd, pad_d

    def depth(self):
        return (self.D, self.Do, self.kd, self.sd, self.pad_d)

    def cout(self, weight):
        """Output channels of `weight`: (Cout, Cin, ..) for a convolution, (Cin, Cout, ..) for a transposed one."""
        return weight.shape[0 if self.kind == 'conv' else 1]


def _conv_launch(x, ldx, wp, y, ldy, bias, in_scale, in_shift, stats, B, H, W, Cin, Ho, Wo, Cout,
                 kh, kw, stride, dil, pad_t, pad_l, in_relu, groups, act, accumulate, nrep=1, depth=(1, 1, 1, 1, 0)):
    """stats: None, or f64 [nrep][groups][2][>=Cout] (or a [groups][2][C] slice of a slab with nrep=1).
    B is the true batch; depth = (D, Do, kd, sd, pad_d) for volumes."""
    sld = stats.stride(-2) if stats is not None else 0
    call("sdhip_conv2d_fwd", ptr(x), ptr(wp), ptr(y), ptr(bias), ptr(in_scale), ptr(in_shift), ptr(stats), sld, nrep,
         B, H, W, Cin, ldx, Ho, Wo, Cout, ldy, kh, kw, stride, dil, pad_t, pad_l, *depth,
         int(in_relu), groups, act, int(accumulate), dtype_code(x), stream_ptr())


NREP = _lib.NREP

from . import parallel  # noqa: E402


def _sync_stats(stats, nrep):
    """Data parallel: all-reduce the f64 (sum, sum of squares) over ranks (sync-BN) — in place on the replica buffer when it
    is dense (the replicas are folded by whoever consumes the buffer, as on one GPU); a strided view is folded into a
    compact copy first."""
    if stats is None or parallel.world_size() == 1:
        return stats, nrep
    if stats.is_contiguous():
        parallel.all_reduce_sum_(stats)
        return stats, nrep
    G, _, C = stats.shape[-3:]
    compact, pz = _zeros((G, 2, C), torch.float64, stats.device)   # zero arena of the step: no fill launch per layer
    if not pz:
        compact.zero_()
    call("sdhip_stats_replica_sum", ptr(stats), ptr(compact), nrep, G, C, stats.stride(-2), C, stream_ptr())
    parallel.all_reduce_sum_(compact)
    return compact, 1


def _bn_finalize(stats, nrep, bn, count, groups, synced=False):
    """(scale, shift, mean, invstd), each f32 [groups][C]; stats None => eval mode (running statistics).
    `count` is the LOCAL element count per group; under data parallelism statistics and count become global."""
    C = bn.num_features
    dev = bn.weight.device
    if stats is None:
        fold = _fold_state(bn)
        t = fold.table(bn, groups) if fold is not None else None
        if t is not None:   # eval step: constants, written by the step's batched launch (mean / invstd serve a backward only)
            return [t[0], t[1], None, None]
    if not synced:      # `synced`: the statistics were already summed over ranks (slab statistics of a dense block)
        stats, nrep = _sync_stats(stats, nrep)
    count = parallel.global_count(count)
    out = [torch.empty((groups, C), dtype=torch.float32, device=dev) for _ in range(4)]
    if stats is not None:
        _bn_track(bn, groups)
        call("sdhip_bn_finalize", ptr(stats), stats.stride(-2), nrep, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
             ptr(bn.running_var), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), C, groups, float(count),
             float(bn.eps), float(_bn_momentum(bn)), stream_ptr())
    else:
        call("sdhip_bn_finalize", None, 0, 1, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
             ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), C, groups, float(count), float(bn.eps), 0.0, stream_ptr())
    return out


def _fused_bn():
    """Consumer-side finalize kernels.  They also serve under data parallelism: the sync-BN exchange all-reduces the
    producer's replica buffer in place, between the launch that fills it and the launch that consumes it."""
    return not _lib.DIAG_NO_FUSED_BN


def _bn_momentum(bn):
    return 0.1 if bn.momentum is None else bn.momentum


def _bn_track(bn, groups):
    """BatchNorm.num_batches_tracked bookkeeping of one train-mode normalisation."""
    if bn.num_batches_tracked is None:
        return
    c = _ctx[0]
    if c is not None and c.nbt is not None and c.arena is not None:
        return                                                    # applied by one multi-tensor add per step (train.TrainStep)
    if c is not None and c.nbt is not None:
        c.nbt.append((bn.num_batches_tracked, groups))           # recorded during the measuring step
    bn.num_batches_tracked += groups


def _bn_param_grads(gamma, beta, C, device):
    """Where a BatchNorm backward kernel puts dgamma / dbeta: (dgamma, dbeta, direct, returned).  direct: the two buffers
    are the parameters' slices of the flat gradient buffer and the kernel accumulates into them — the autograd node then
    returns `returned` = (None, None); otherwise they are fresh f32 [C] tensors and `returned` is the pair itself."""
    tg, tb = _grad_target(gamma), _grad_target(beta)
    if tg is not None and tb is not None:
        return tg, tb, True, (None, None)
    dgamma, dbeta = (torch.empty(C, dtype=torch.float32, device=device) for _ in range(2))
    return dgamma, dbeta, False, (dgamma, dbeta)


def bn_backward_two_phase(gy, ldg, x, ldx, gx, ldgx, scale, shift, mean, invstd, gamma, beta, npix, C, groups, act, count, dt):
    """Train-mode backward of y = act(BatchNorm(x)): (1) reductions only, [data parallel: the replica sums are all-reduced
    in place], (2) ONE pass that derives the statistics gradient from the replica sums itself and writes the complete
    gradient of x (+ dgamma / dbeta).  `count`: the global element count per group.
    Returns (dgamma, dbeta), each None when accumulated straight into the flat gradient buffer."""
    dev = scale.device
    both, pz = _zeros((2, NREP, groups, C), torch.float32, dev)
    dsc, dsh = both[0], both[1]
    call("sdhip_affine_act_bwd", ptr(gy), ldg, ptr(x), ldx, None, 0, ptr(scale), ptr(shift), ptr(dsc), ptr(dsh), NREP,
         npix, C, groups, act, 0, int(pz), dt, stream_ptr())
    parallel.all_reduce_sum_(both)            # sync-BN: the replica sums become global in place (`count` is the global count)
    dgamma, dbeta, direct, returned = _bn_param_grads(gamma, beta, C, dev)
    call("sdhip_bn_bwd_apply_fin", ptr(gy), ldg, ptr(x), ldx, ptr(gx), ldgx, ptr(scale), ptr(shift), ptr(dsc), ptr(dsh), NREP,
         ptr(gamma), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), int(direct), parallel.param_scale(), npix, C, groups,
         float(count), act, dt, stream_ptr())
    return returned


def _bn_backward(gy, ldg, x, ldx, gx, ldgx, scale, shift, mean, invstd, gamma, npix, C, groups, act, count, train,
                 dt, accumulate_gx=False, dstats=None, accumulate_dstats=False, beta=None):
    """Backward of y = act(x*scale + shift) with scale/shift from batch statistics.
    Writes gx (+)= gy*act'*scale and returns (dgamma, dbeta, dstats[groups][2][C]); the caller still has to add the
    statistics path dstats[0] + 2*x*dstats[1] (sdhip_stats_fix) to the gradient of whatever produced x."""
    dev = scale.device
    if not train and not _wants_grad(gamma, beta):
        # frozen BatchNorm: a constant scale / shift.  No reductions, no replica buffers, no finalize, and the parameters'
        # slices of the flat gradient buffer are not touched (torch: their .grad stays None)
        call("sdhip_affine_act_bwd", ptr(gy), ldg, ptr(x), ldx, ptr(gx), ldgx, ptr(scale), ptr(shift), None, None, 1,
             npix, C, groups, act, int(accumulate_gx), 0, dt, stream_ptr())
        return None, None, None
    both, pz = _zeros((2, NREP, groups, C), torch.float32, dev)
    dsc, dsh = both[0], both[1]
    call("sdhip_affine_act_bwd", ptr(gy), ldg, ptr(x), ldx, ptr(gx), ldgx, ptr(scale), ptr(shift), ptr(dsc), ptr(dsh), NREP,
         npix, C, groups, act, int(accumulate_gx), int(pz), dt, stream_ptr())
    dgamma, dbeta, direct, returned = _bn_param_grads(gamma, beta, C, dev)
    par_flag = 2 if direct else 0
    if dstats is None:
        dstats = torch.empty((groups, 2, C), dtype=torch.float64, device=dev)
        accumulate_dstats = False
    if parallel.world_size() > 1 and train:
        # sync-BN backward: dgamma/dbeta from the LOCAL sums, the statistics gradient from the GLOBAL sums
        call("sdhip_bn_finalize_bwd", ptr(dsc), ptr(dsh), NREP, ptr(gamma), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta),
             None, C, par_flag, C, groups, float(count), 1, stream_ptr())
        parallel.all_reduce_sum_(both)                         # [2][NREP][groups][C] in place: the finalize folds the replicas
        call("sdhip_bn_finalize_bwd", ptr(dsc), ptr(dsh), NREP, ptr(gamma), ptr(mean), ptr(invstd), None, None,
             ptr(dstats), dstats.stride(-2), int(accumulate_dstats), C, groups, float(parallel.global_count(count)), 1,
             stream_ptr())
    else:
        call("sdhip_bn_finalize_bwd", ptr(dsc), ptr(dsh), NREP, ptr(gamma), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta),
             ptr(dstats), dstats.stride(-2), int(accumulate_dstats) | par_flag, C, groups, float(count), int(train), stream_ptr())
    return (*returned, dstats)


_BN_ACTS = (0, 1, 2, _lib.ACT_HSWISH, _lib.ACT_HSIGMOID)   # activations the two-phase BatchNorm backward kernels take


def _bn_act_forward(yraw, ldr, bn, ws, count, groups, act, residual=None):
    """The tail of a convolution-like node: y = act(BatchNorm(yraw)) (+ residual) from the raw output and the statistics
    replicas `ws` (f64 [NREP][groups][2][C]) its epilogue summed; ws None => eval mode (running statistics).  `count`: the
    LOCAL element count per group.  Returns (y, scale, shift, mean, invstd)."""
    B, C, Ho, Wo = yraw.shape
    npix, dt = B * Ho * Wo, dtype_code(yraw)
    rv, ldres = nhwc_view(residual) if residual is not None else (None, 0)
    y, ldy = alloc_nhwc(B, C, Ho, Wo, yraw.dtype, yraw.device)
    if ws is not None and _fused_bn():
        # one launch: every workgroup derives scale/shift of its channels from the statistics the conv just wrote
        scale, shift, mean, invstd = [torch.empty((groups, C), dtype=torch.float32, device=yraw.device) for _ in range(4)]
        _bn_track(bn, groups)
        parallel.all_reduce_sum_(ws)         # sync-BN: the epilogue's replica sums become global, in place
        call("sdhip_affine_act_bn", ptr(yraw), ldr, ptr(y), ldy, ptr(rv), ldres, ptr(ws), ws.stride(-2), NREP, ptr(bn.weight),
             ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
             npix, C, groups, float(parallel.global_count(count)), float(bn.eps), float(_bn_momentum(bn)), act, dt, stream_ptr())
    else:
        scale, shift, mean, invstd = _bn_finalize(ws, NREP, bn, count, groups)
        call("sdhip_affine_act", ptr(yraw), ldr, ptr(y), ldy, ptr(rv), ldres, ptr(scale), ptr(shift), npix, C, groups, act, dt,
             stream_ptr())
    return y, scale, shift, mean, invstd


def _bn_act_backward(g, ldg, yraw, ldraw, scale, shift, mean, invstd, gamma, beta, groups, act, count, train, presummed=None,
                     out=None):
    """Backward of _bn_act_forward w.r.t. yraw, the statistics path included: (graw, ldgr, dgamma, dbeta), dgamma / dbeta
    None when accumulated straight into the flat gradient buffer.  `count`: the LOCAL element count per group.
    presummed: f64 [NREP][groups][2][C] sums the producer of g already took against yraw (BNSlot, the DenseNet block's
    conv2 data gradient) — the reduction pass is skipped.  out: (tensor, ld) to write graw into (may be g itself: the
    kernels are elementwise) instead of a fresh tensor."""
    B, C, Ho, Wo = yraw.shape
    npix, dt = B * Ho * Wo, dtype_code(yraw)
    graw, ldgr = out if out is not None else alloc_nhwc(B, C, Ho, Wo, yraw.dtype, yraw.device)
    if presummed is not None:
        dgamma, dbeta, direct, returned = _bn_param_grads(gamma, beta, C, yraw.device)
        parallel.all_reduce_sum_(presummed)
        call("sdhip_bn_bwd_apply_fin_d", ptr(g), ldg, ptr(yraw), ldraw, ptr(graw), ldgr, ptr(scale), ptr(shift), ptr(presummed), NREP,
             ptr(gamma), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), int(direct), parallel.param_scale(), npix, C, groups,
             float(parallel.global_count(count)), act, dt, stream_ptr())
        return graw, ldgr, *returned
    if train and act not in _BN_ACTS:
        # the one-pass form below leaves the statistics path to its caller, and there is no kernel for it here
        raise _lib.SdhipError("train-mode BatchNorm backward: activation %d is not one the two-phase kernels take" % act)
    if train and _fused_bn():
        dgamma, dbeta = bn_backward_two_phase(g, ldg, yraw, ldraw, graw, ldgr, scale, shift, mean, invstd, gamma, beta, npix, C,
                                              groups, act, parallel.global_count(count), dt)
    elif train:
        # two-phase: reductions only (no gradient written), per-channel finalize, then ONE pass writes the complete
        # gradient of the conv output — 10 bytes per element instead of 12
        dgamma, dbeta, dS = _bn_backward(g, ldg, yraw, ldraw, None, 0, scale, shift, mean, invstd, gamma, npix, C, groups, act,
                                         count, True, dt, beta=beta)
        call("sdhip_bn_bwd_apply", ptr(g), ldg, ptr(yraw), ldraw, ptr(graw), ldgr, ptr(scale), ptr(shift), ptr(dS), C, npix, C,
             groups, act, dt, stream_ptr())
    else:
        dgamma, dbeta, _ = _bn_backward(g, ldg, yraw, ldraw, graw, ldgr, scale, shift, mean, invstd, gamma, npix, C, groups, act,
                                        count, False, dt, beta=beta)
    return graw, ldgr, dgamma, dbeta


class GradSlot:
    """Carries one gradient contribution from the autograd node that produces it FIRST in the backward pass to the node
    whose data-gradient launch can add to it in place.  Conv2DownUp (models/dsnet_t2.py:80-117): x1 feeds c2 and, as a skip,
    d4 — d4's backward runs before c2's (it was created later), parks the skip gradient here instead of handing it to
    autograd, and c2's data gradient is launched with accumulate = 1 on that buffer: the sum of the two contributions
    costs no pass of its own (autograd would run an elementwise add over the full-resolution map)."""
    __slots__ = ("g", "exclusive")

    def __init__(self, exclusive):
        # exclusive: the parked tensor is referenced by nobody else (it is the fresh data gradient of the node behind the
        # parking one), so the sum may be formed IN it; otherwise it is only read (sdhip_conv2d_fwd_add) — an incoming
        # gradient from outside the block may be shared with another branch of the graph
        self.g = None
        self.exclusive = exclusive


def _take_parked(slot, xv, need_x):
    """(acc_into, addend) of _conv_backward: the gradient the skip consumer of xv parked in `slot` (a GradSlot or None), taken out."""
    if slot is None or slot.g is None or not need_x:
        return None, None
    parked, slot.g = slot.g, None
    if parked.shape != xv.shape or parked.dtype != xv.dtype:
        raise _lib.SdhipError("GradSlot: parked gradient does not match the input it belongs to")
    return (parked, None) if slot.exclusive else (None, parked)


BN_SLOT_MAX_BYTES = _lib.TUNE_BN_SLOT_MAX_MB << 20
BAND_BX_FORMS = tuple(f for f in _lib.TUNE_BAND_BX_FORMS.split(",") if f)   # forms of the persistent kernel that fuse at any size


class BNSlot:
    """Links a convbn + ReLU node to the ONE node that consumes its output, so that the consumer's data-gradient launch —
    which holds every value of dL/d relu(bn(u)) once — also takes the two reductions the BatchNorm backward starts with
    (sdhip_conv2d_fwd_bnbwd) and the producer's backward skips its reduction pass over that gradient and u.
    The producer fills (u, scale, shift) in its forward; the consumer's backward fills (sums, gptr); the producer uses the
    sums only if the gradient it is handed IS the tensor the consumer wrote (gptr) — any other gradient route (an extra
    consumer, autograd summing contributions) silently falls back to the two-pass form."""
    __slots__ = ("u", "ldu", "scale", "shift", "groups", "C", "sums", "gptr")

    def __init__(self):
        self.u = self.scale = self.shift = self.sums = None
        self.ldu = self.groups = self.C = 0
        self.gptr = 0


_BAND_BX_NAMES = {"band(5x5, bx)": "5x5", "band(3x3, bx)": "3x3"}     # sdhip_last_path -> the form's word in BAND_BX_FORMS
_DRY_Y = ctypes_ptr(1 << 20)                # stand-ins for tensors that do not exist yet when the dispatch is asked: it
_DRY_SUMS = ctypes_ptr(2 << 20)             # reads their alignment only, and the allocator's is 256 bytes


def _bnbwd_band_form(args):
    """'5x5' / '3x3' if the library runs the sdhip_conv2d_fwd_bnbwd call with these arguments on the persistent whole-CU
    kernel with the BatchNorm-backward sums in its epilogue (conv_band_bx_kernel), else None.  The library's own dispatch
    answers, in dry mode: nothing is launched, no operand is read.  A call the entry point refuses outright (channel counts or
    pixel strides that are no multiple of 4: SDHIP_ERR_ARG) runs on no kernel: None, and the caller never makes it."""
    with _lib.dispatch_dry():
        rc = _lib._lib.sdhip_conv2d_fwd_bnbwd(*args)
    return _BAND_BX_NAMES.get(_lib.last_path()) if rc == 0 else None


def _conv_backward(ctx_spec, xv, ldx, weight, g, ldg, in_scale, in_shift, in_relu, groups, need_x, need_w, bias=None, acc_into=None,
                   addend=None, bn_slot=None):
    """dgrad (w.r.t. the post-prologue input) and wgrad of one conv; returns (g_post, gw, gb)."""
    spec = ctx_spec
    Bimg, Cin, H, W = xv.shape
    B = Bimg // spec.D
    Cout = spec.cout(weight)
    dt = dtype_code(xv)
    gpost = gw = gb = None
    if need_x:
        wd = packed_weight(weight, spec.kind, 'dgrad', xv.dtype)
        fused_bn = False
        # On the halo-tile kernels the epilogue's reads of u sit exposed behind the MFMA loop, so on maps of more than ~40 MB
        # it costs more than the streaming pass it replaces (profiles/r02_step_summary.txt: full resolution, 32 channels,
        # +33 us against a 27 us pass); below that the pass is launch- and latency-bound and the fusion wins (64 channels
        # at 128x256: +3.5 against 18).  The persistent kernel (conv_band.h) has an epilogue of its own that issues u in
        # the layout of its stores, in one batch per tile — a stage ahead where the registers allow it: shapes on that
        # kernel fuse whatever their size, each form behind its own switch (BAND_BX_FORMS; DESIGN.md section 7 has the table)
        # — which kernel the call would run on is the library's to say: it is asked, in dry mode, with the call's own arguments
        if (bn_slot is not None and bn_slot.u is not None and bn_slot.C == Cin and xv.dtype == torch.bfloat16 and spec.stride == 1
                and spec.sd == 1 and spec.kd == 1 and spec.D == 1 and tuple(bn_slot.u.shape) == (Bimg, Cin, H, W)):
            # the input of this convolution was relu(bn(u)): the launch that writes its gradient also takes that
            # BatchNorm's two backward reductions (and adds a parked skip gradient on the way)
            other = acc_into if acc_into is not None else addend
            ov, ldo = nhwc_view(other) if other is not None else (None, 0)

            def bnbwd_args(y, ldy, sums):
                return (ptr(g), ptr(wd), y, sums, Cin, NREP, ptr(bn_slot.u), bn_slot.ldu, ptr(bn_slot.scale), ptr(bn_slot.shift), ptr(ov), ldo,
                        B, spec.Ho, spec.Wo, Cout, ldg, H, W, Cin, ldy, spec.kh, spec.kw, spec.dil, spec.dil * (spec.kh - 1) - spec.pad_t,
                        spec.dil * (spec.kw - 1) - spec.pad_l, bn_slot.groups, 0, dt, stream_ptr())
            if ((spec.kh * spec.kw <= 9 and Bimg * H * W * Cin * 2 <= BN_SLOT_MAX_BYTES)
                    or _bnbwd_band_form(bnbwd_args(_DRY_Y, (Cin + 7) & ~7, _DRY_SUMS)) in BAND_BX_FORMS):     # (the pixel stride alloc_nhwc gives)
                gpost, ldgp = alloc_nhwc(Bimg, Cin, H, W, xv.dtype, xv.device)
                sums = _zeros((NREP, bn_slot.groups, 2, Cin), torch.float64, xv.device)[0]
                fused_bn = try_call("sdhip_conv2d_fwd_bnbwd", *bnbwd_args(ptr(gpost), ldgp, ptr(sums)))
                if fused_bn:
                    bn_slot.sums, bn_slot.gptr = sums, gpost.data_ptr()
        # Conv3d(k=3, stride 2, padding 1) over even extents (hourglass conv1 / conv3, stackhourglass.py:13-19): its data gradient is
        # the transposed convolution that doubles every extent — eight sub-pixel phases of 1..8 taps over dY itself (27 taps per dY
        # voxel), not a stride-1 correlation over the zero-stuffed dY (8 x 27: seven of eight products are zeros)
        if (not fused_bn and acc_into is None and addend is None and spec.kind == 'conv' and spec.stride == 2 and spec.sd == 2
                and spec.kd == 3 and spec.kh == 3 and spec.kw == 3 and spec.dil == 1 and spec.pad_t == 1 and spec.pad_l == 1
                and spec.pad_d == 1 and spec.D == 2 * spec.Do and H == 2 * spec.Ho and W == 2 * spec.Wo and not _lib.DIAG_NO_PHASE_DGRAD):
            gpost, ldgp = alloc_nhwc(Bimg, Cin, H, W, xv.dtype, xv.device)
            packs, _keep = _phase_packs(weight, xv.dtype)       # (Cout, Cin, 3,3,3) IS the transposed convolution's (in, out, ...) layout
            for (pd, ph, pw), wpk in zip(_PHASES, packs):
                call("sdhip_conv2d_fwd_phase", ptr(g), ptr(wpk), ptr(gpost), None, 0, 1, B, spec.Ho, spec.Wo, Cout, ldg, Cin, ldgp,
                     1 + ph, 1 + pw, spec.Do, 1 + pd, 1, pd, ph, pw, dt, stream_ptr())
            if need_w:
                gw, gb = wgrad(xv, ldx, g, ldg, weight, bias, spec, in_scale, in_shift, in_relu, groups)
            return gpost, gw, gb
        if fused_bn:
            pass
        elif acc_into is not None:
            gpost, ldgp = nhwc_view(acc_into)     # holds the other contribution: this launch adds to it
        else:
            gpost, ldgp = alloc_nhwc(Bimg, Cin, H, W, xv.dtype, xv.device)
        pt = spec.dil * (spec.kh - 1) - spec.pad_t
        pl = spec.dil * (spec.kw - 1) - spec.pad_l
        pd = (spec.kd - 1) - spec.pad_d
        gsrc, ldsrc, Dg, Hg, Wg = g, ldg, spec.Do, spec.Ho, spec.Wo
        if spec.stride != 1 or spec.sd != 1:
            # strided convolution: its data gradient is a stride-1 correlation (flipped weights) over the zero-stuffed dY
            Dg, Hg, Wg = (spec.Do - 1) * spec.sd + 1, (spec.Ho - 1) * spec.stride + 1, (spec.Wo - 1) * spec.stride + 1
            gsrc = empty_nhwc(B * Dg, Cout, Hg, Wg, xv.dtype, xv.device)
            call("sdhip_stuff", ptr(g), ldg, ptr(gsrc), Cout, B, spec.Do, spec.Ho, spec.Wo, Cout, spec.sd, spec.stride, 1, dt,
                 stream_ptr())
            ldsrc = Cout
        fused_add = fused_bn
        if not fused_bn and addend is not None and spec.kd == 1 and spec.D == 1 and spec.dil == 1 and gsrc is g:
            av, lda = nhwc_view(addend)
            fused_add = try_call("sdhip_conv2d_fwd_add", ptr(gsrc), ptr(wd), ptr(gpost), ptr(av), lda, B, Hg, Wg, Cout, ldsrc, H, W, Cin,
                                 ldgp, spec.kh, spec.kw, pt, pl, dt, stream_ptr())
        if not fused_add:
            _conv_launch(gsrc, ldsrc, wd, gpost, ldgp, None, None, None, None, B, Hg, Wg, Cout, H, W, Cin,
                         spec.kh, spec.kw, 1, spec.dil, pt, pl, False, 1, 0, acc_into is not None, 1, (Dg, spec.D, spec.kd, 1, pd))
            if addend is not None:            # no kernel on this shape's path adds a second tensor: one elementwise pass
                gpost = add(gpost, addend)

    if need_w:
        gw, gb = wgrad(xv, ldx, g, ldg, weight, bias, spec, in_scale, in_shift, in_relu, groups)
    return gpost, gw, gb


def wgrad(xv, ldx, g, ldg, weight, bias, spec, in_scale=None, in_shift=None, in_relu=False, groups=1):
    """Weight (and bias) gradient of one conv.  Returns (gw, gb), each None when it was accumulated straight into the
    flat gradient buffer (StepContext.direct_grads).  With a StepContext side stream the launches go there: nothing
    downstream of a weight gradient runs before the optimizer, so it overlaps the latency-bound data-gradient chain."""
    c = _ctx[0]
    if c is not None and c.side is not None and c.direct_grads and not c.defer_wgrad:
        main = torch.cuda.current_stream()
        c.side.wait_stream(main)                     # g and x are produced on the main stream
        c.keep.append((xv, g, in_scale, in_shift))   # the caching allocator must not recycle them before join()
        with torch.cuda.stream(c.side):
            return _wgrad_impl(xv, ldx, g, ldg, weight, bias, spec, in_scale, in_shift, in_relu, groups)
    return _wgrad_impl(xv, ldx, g, ldg, weight, bias, spec, in_scale, in_shift, in_relu, groups)


def _wgrad_impl(xv, ldx, g, ldg, weight, bias, spec, in_scale, in_shift, in_relu, groups):
    Bimg, Cin, H, W = xv.shape
    B = Bimg // spec.D
    Cout = spec.cout(weight)
    dt = dtype_code(xv)
    T = spec.kh * spec.kw
    per = _lib.packed_elems(Cout, Cin, T, dt)
    acc, pz = _zeros((per * spec.kd,), torch.float32, xv.device)
    tw = _grad_target(weight)
    tb = _grad_target(bias) if bias is not None else None
    gb = None
    if bias is not None:
        if tb is not None:
            dbias, dbias_pz = tb, True       # the flat gradient buffer is zeroed once per step; the kernel adds
        else:
            dbias, dbias_pz = _zeros((Cout,), torch.float32, xv.device)
            gb = dbias
    else:
        dbias, dbias_pz = None, True
    if bias is not None and pz != dbias_pz:   # one flag covers both buffers: zero the not-yet-zeroed one here
        if not pz:
            acc.zero_()
        elif tb is None:
            dbias.zero_()
        pz = True
    c = _ctx[0]
    if (c is not None and c.defer_wgrad and c.direct_grads and c.arena is not None and tw is not None and pz
            and (bias is None or tb is not None)):
        # queued: launched by StepContext.join() in one grid per kernel instantiation; the operands stay alive until then
        dpt = lambda t: t.data_ptr() if t is not None else None
        c.wq.append((dpt(xv), dpt(g), dpt(acc), dpt(dbias), dpt(in_scale), dpt(in_shift), B, H, W, Cin, ldx, spec.Ho, spec.Wo, Cout, ldg,
                     spec.kh, spec.kw, spec.stride, spec.dil, spec.pad_t, spec.pad_l) + tuple(spec.depth()) + (int(in_relu), groups))
        c.wq_keep.append((xv, g, in_scale, in_shift))
        c.wq_dt = dt
        if not c.overlap:
            c.flush_to_side()
    else:
        call("sdhip_conv2d_wgrad", ptr(xv), ptr(g), ptr(acc), ptr(dbias), ptr(in_scale), ptr(in_shift),
             B, H, W, Cin, ldx, spec.Ho, spec.Wo, Cout, ldg, spec.kh, spec.kw, spec.stride, spec.dil,
             spec.pad_t, spec.pad_l, *spec.depth(), int(in_relu), groups, int(pz), dt, stream_ptr())
    # unpack by the WEIGHT's own channel count (the activation may carry zero-padded extra channels: 8-channel images),
    # depth tap by depth tap for 3-D weights
    gw = None
    target = tw
    if target is None:
        gw = target = torch.empty_like(weight, memory_format=torch.contiguous_format)
    c = _ctx[0]
    defer = c is not None and c.direct_grads and tw is not None and pz and c.arena is not None
    for src_off, blk, M, K, T_, sm, sk, flip in _pack_rows(weight, spec.kind, 'fwd', dt):
        if defer:   # accumulators live in the step's zero arena until join(): unpack all of them in one launch there
            c.unpacks.append((acc.data_ptr() + 4 * per * blk, target.data_ptr() + 4 * src_off, M, K, T_, sm, sk, flip))
            c.unpack_dt = dt
        else:
            call("sdhip_conv_unpack_wgrad", ctypes_ptr(acc.data_ptr() + 4 * per * blk), ctypes_ptr(target.data_ptr() + 4 * src_off),
                 M, K, T_, sm, sk, flip, 1 if tw is not None else 0, dt, stream_ptr())
    return gw, gb


class _ConvFn(torch.autograd.Function):
    """y = act(conv(x) + bias)   (conv2dSame / ConvTranspose2dSame / nn.Conv2d without a BatchNorm behind it)."""

    @staticmethod
    def forward(ctx, x, weight, bias, spec, act):
        _require_gpu(x, weight)
        Bimg, Cin, H, W = x.shape
        B = Bimg // spec.D
        xv, ldx = aligned_view(x)
        Cout = spec.cout(weight)
        wp = packed_weight(weight, spec.kind, 'fwd', x.dtype)
        y, ldy = alloc_nhwc(B * spec.Do, Cout, spec.Ho, spec.Wo, x.dtype, x.device)
        _conv_launch(xv, ldx, wp, y, ldy, bias.detach() if bias is not None else None, None, None, None, B, H, W, Cin,
                     spec.Ho, spec.Wo, Cout, spec.kh, spec.kw, spec.stride, spec.dil, spec.pad_t, spec.pad_l, False, 1, act, False,
                     1, spec.depth())
        ctx.spec, ctx.act, ctx.ldx = spec, act, ldx
        ctx.save_for_backward(xv, weight, bias, y if act else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, bias, ysaved = ctx.saved_tensors
        spec, act = ctx.spec, ctx.act
        B = xv.shape[0] // spec.D * spec.Do      # output images
        Cout = spec.cout(weight)
        g, ldg = aligned_view(gy)
        if act:   # activation fused in the epilogue: derivative from the stored output
            g2, ldg2 = alloc_nhwc(B, Cout, spec.Ho, spec.Wo, xv.dtype, xv.device)
            call("sdhip_affine_act_bwd", ptr(g), ldg, ptr(ysaved), nhwc_view(ysaved)[1], ptr(g2), ldg2, None, None, None, None, 1,
                 B * spec.Ho * spec.Wo, Cout, 1, 1 if act == 1 else 4, 0, 0, dtype_code(xv), stream_ptr())
            g, ldg = g2, ldg2
        gx, gw, gb = _conv_backward(spec, xv, ctx.ldx, weight, g, ldg, None, None, False, 1, ctx.needs_input_grad[0],
                                    ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]), bias)
        return gx, gw, gb, None, None


class _ConvBNActFn(torch.autograd.Function):
    """y = act(BatchNorm(conv(x))) (+ residual) as ONE autograd node: the conv epilogue sums the batch statistics,
    a per-channel kernel turns them into scale/shift (and updates the running statistics), one elementwise pass
    normalises, activates and adds the skip.  convbn / deconvbn (+ReLU, + skip add) of models/dsnet_t2.py:16-117."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, spec, bn, act, groups, in_slot=None, res_slot=None, in_bn=None, out_bn=None):
        _require_gpu(x, weight)
        ctx.in_slot, ctx.res_slot, ctx.in_bn, ctx.out_bn = in_slot, res_slot, in_bn, out_bn
        Bimg, Cin, H, W = x.shape
        Btrue = Bimg // spec.D
        B = Btrue * spec.Do                      # output images
        xv, ldx = aligned_view(x)
        Cout = spec.cout(weight)
        wp = packed_weight(weight, spec.kind, 'fwd', x.dtype)
        yraw, ldr_ = alloc_nhwc(B, Cout, spec.Ho, spec.Wo, x.dtype, x.device)
        train = bn.training
        ws = _zeros((NREP, groups, 2, Cout), torch.float64, x.device)[0] if train else None
        _conv_launch(xv, ldx, wp, yraw, ldr_, None, None, None, ws, Btrue, H, W, Cin, spec.Ho, spec.Wo, Cout,
                     spec.kh, spec.kw, spec.stride, spec.dil, spec.pad_t, spec.pad_l, False, groups, 0, False, NREP, spec.depth())
        count = (B // groups) * spec.Ho * spec.Wo
        y, scale, shift, mean, invstd = _bn_act_forward(yraw, ldr_, bn, ws, count, groups, act, residual)
        ctx.spec, ctx.act, ctx.groups, ctx.ldx, ctx.count, ctx.train = spec, act, groups, ldx, count, train
        ctx.ldraw = ldr_
        ctx.has_res = residual is not None
        if out_bn is not None and train and act == 1 and _fused_bn() and spec.D == 1 and spec.Do == 1:
            out_bn.u, out_bn.ldu, out_bn.scale, out_bn.shift, out_bn.groups, out_bn.C = yraw, ldr_, scale, shift, groups, Cout
        ctx.save_for_backward(xv, weight, gamma, beta, yraw, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, gamma, beta, yraw, scale, shift, mean, invstd = ctx.saved_tensors
        spec, groups = ctx.spec, ctx.groups
        g, ldg = nhwc_view(gy)
        ob, sums = ctx.out_bn, None
        if ob is not None and ob.sums is not None and ob.gptr == g.data_ptr() and ctx.train and _fused_bn():
            # the node that produced gy already summed it against yraw (BNSlot): straight to the second phase
            sums, ob.sums, ob.gptr = ob.sums, None, 0
        graw, ldgr, dgamma, dbeta = _bn_act_backward(g, ldg, yraw, ctx.ldraw, scale, shift, mean, invstd, gamma, beta, groups,
                                                     ctx.act, ctx.count, ctx.train, presummed=sums)
        acc, addend = _take_parked(ctx.in_slot, xv, ctx.needs_input_grad[0])
        gx, gw, _ = _conv_backward(spec, xv, ctx.ldx, weight, graw, ldgr, None, None, False, 1, ctx.needs_input_grad[0],
                                   ctx.needs_input_grad[1], acc_into=acc, addend=addend, bn_slot=ctx.in_bn)
        gres = gy if ctx.has_res else None
        if gres is not None and ctx.res_slot is not None:
            ctx.res_slot.g, gres = gy, None                   # handed to the producer-side consumer of the skip tensor instead
        return gx, gw, dgamma, dbeta, gres, None, None, None, None, None, None, None, None


class _BNConvFn(torch.autograd.Function):
    """y = conv(relu(BatchNorm(x))) with the statistics of x given (DenseNet transition, models/densenet.py:119-128):
    norm + relu are the conv's fused input prologue.  Returns gradients for x and for its statistics."""

    @staticmethod
    def forward(ctx, x, stats, weight, gamma, beta, spec, bn, groups):
        _require_gpu(x, weight)
        B, Cin, H, W = x.shape
        xv, ldx = nhwc_view(x)
        Cout = weight.shape[0]
        train = bn.training
        count = (B // groups) * H * W
        scale, shift, mean, invstd = _bn_finalize(stats if train else None, 1, bn, count, groups, synced=True)
        wp = packed_weight(weight, spec.kind, 'fwd', x.dtype)
        y = empty_nhwc(B, Cout, spec.Ho, spec.Wo, x.dtype, x.device)
        _conv_launch(xv, ldx, wp, y, Cout, None, scale, shift, None, B, H, W, Cin, spec.Ho, spec.Wo, Cout,
                     spec.kh, spec.kw, spec.stride, spec.dil, spec.pad_t, spec.pad_l, True, groups, 0, False)
        ctx.spec, ctx.groups, ctx.ldx, ctx.count, ctx.train = spec, groups, ldx, count, train
        ctx.save_for_backward(xv, weight, gamma, beta, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, gamma, beta, scale, shift, mean, invstd = ctx.saved_tensors
        spec, groups = ctx.spec, ctx.groups
        B, Cin, H, W = xv.shape
        dt = dtype_code(xv)
        g, ldg = nhwc_view(gy)
        gpost, gw, _ = _conv_backward(spec, xv, ctx.ldx, weight, g, ldg, scale, shift, True, groups, True, True)
        gx = empty_nhwc(B, Cin, H, W, xv.dtype, xv.device)
        dgamma, dbeta, dS = _bn_backward(gpost, nhwc_view(gpost)[1], xv, ctx.ldx, gx, Cin, scale, shift, mean, invstd, gamma,
                                         B * H * W, Cin, groups, 1, ctx.count, ctx.train, dt, beta=beta)
        return gx, (dS if ctx.train else None), gw, dgamma, dbeta, None, None, None


class _BNActFn(torch.autograd.Function):
    """y = act(BatchNorm(x)) with the statistics of x given (norm5 of the DenseNet, models/densenet.py:239-241)."""

    @staticmethod
    def forward(ctx, x, stats, gamma, beta, bn, act, groups):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        train = bn.training
        count = (B // groups) * H * W
        scale, shift, mean, invstd = _bn_finalize(stats if train else None, 1, bn, count, groups, synced=True)
        y = empty_nhwc(B, C, H, W, x.dtype, x.device)
        call("sdhip_affine_act", ptr(xv), ldx, ptr(y), C, None, 0, ptr(scale), ptr(shift), B * H * W, C, groups, act,
             dtype_code(x), stream_ptr())
        ctx.cfg = (ldx, act, groups, count, train)
        ctx.save_for_backward(xv, gamma, beta, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, gamma, beta, scale, shift, mean, invstd = ctx.saved_tensors
        ldx, act, groups, count, train = ctx.cfg
        B, C, H, W = xv.shape
        g, ldg = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, xv.dtype, xv.device)
        dgamma, dbeta, dS = _bn_backward(g, ldg, xv, ldx, gx, C, scale, shift, mean, invstd, gamma, B * H * W, C, groups, act,
                                         count, train, dtype_code(xv), beta=beta)
        return gx, (dS if train else None), dgamma, dbeta, None, None, None


def conv1x1_cat_forward(segs, weight, bias, act):
    """act(conv1x1(cat([upsample_nearest(x_i, 2^us_i)], dim=1)) + bias) without building the concatenation or the
    upsampled maps (sdhip_conv1x1_cat_fwd).  segs: [(tensor (B, c_i, H >> us_i, W >> us_i), us_i)], at most two; bf16."""
    (x0, us0) = segs[0]
    x1, us1 = segs[1] if len(segs) > 1 else (None, 0)
    B, c0 = x0.shape[0], x0.shape[1]
    H, W = x0.shape[2] << us0, x0.shape[3] << us0
    v0, ld0 = aligned_view(x0)
    v1, ld1 = aligned_view(x1) if x1 is not None else (None, 0)
    c1 = x1.shape[1] if x1 is not None else 0
    Cout = weight.shape[0]
    wp = packed_weight(weight, 'conv', 'fwd', x0.dtype)
    y, ldy = alloc_nhwc(B, Cout, H, W, x0.dtype, x0.device)
    call("sdhip_conv1x1_cat_fwd", ptr(v0), ld0, c0, us0, ptr(v1), ld1, c1, us1, ptr(wp), ptr(y), ldy,
         ptr(bias.detach()) if bias is not None else None, B, H, W, Cout, act, dtype_code(x0), stream_ptr())
    return y


class _UpCatConv1x1Fn(torch.autograd.Function):
    """y = act(conv1x1(cat([nearest_upsample(xs, 2^us), xf], dim=1))) — `conv1d_2(torch.cat((F.interpolate(y, scale_factor=8),
    xleft2), 1))` and its siblings (models/dsnet_t2.py:1211-1216,1262-1291,927-933) as one kernel: neither the upsampled
    map nor the concatenation is ever written.  The backward pass never touches the upsampled form either:
      grad(xs)      = dgrad1x1(sum-pool_{2^us}(g), W)[:, :c0]        (pooling and the 1x1 contraction commute)
      grad(xf)      = conv1x1(g, W[:, c0:]^T)
      dW[:, :c0]    = wgrad(xs, sum-pool(g)),   dW[:, c0:] = wgrad(xf, g)."""

    @staticmethod
    def forward(ctx, xs, xf, weight, us, act):
        _require_gpu(xs, xf, weight)
        y = conv1x1_cat_forward([(xs, us), (xf, 0)], weight, None, act)
        ctx.save_for_backward(xs, xf, weight, y if act else None)
        ctx.cfg = (us, act)
        return y

    @staticmethod
    def backward(ctx, gy):
        xs, xf, weight, ysaved = ctx.saved_tensors
        us, act = ctx.cfg
        B, Cout, H, W = gy.shape
        c0, c1 = xs.shape[1], xf.shape[1]
        h, w = xs.shape[2], xs.shape[3]
        dt = dtype_code(gy)
        g, ldg = aligned_view(gy)
        if act:
            g2, ldg2 = alloc_nhwc(B, Cout, H, W, gy.dtype, gy.device)
            call("sdhip_affine_act_bwd", ptr(g), ldg, ptr(ysaved), nhwc_view(ysaved)[1], ptr(g2), ldg2, None, None, None, None, 1,
                 B * H * W, Cout, 1, 1 if act == 1 else 4, 0, 0, dt, stream_ptr())
            g, ldg = g2, ldg2
        k = 1 << us
        gp = avgpool(g, k)                                   # mean over the 2^us x 2^us block; the sum is k*k times that
        gpv, ldgp = aligned_view(gp)
        # gradient of the small map
        wd = packed_weight(weight, 'conv', 'dgrad', gy.dtype)
        gsm, ldgs = alloc_nhwc(B, c0 + c1, h, w, gy.dtype, gy.device)
        _conv_launch(gpv, ldgp, wd, gsm, ldgs, None, None, None, None, B, h, w, Cout, h, w, c0 + c1, 1, 1, 1, 1, 0, 0, False, 1, 0, False)
        gxs = affine_act(gsm[:, :c0], _const_vec(float(k * k), c0, gy.device), None, None, 0)
        # gradient of the full-resolution segment: a Cout -> c1 1x1 convolution with W[:, c0:]^T
        w_f = weight.detach()[:, c0:].transpose(0, 1).contiguous()
        gxf, ldgf = alloc_nhwc(B, c1, H, W, gy.dtype, gy.device)
        _conv_launch(g, ldg, packed_weight(w_f, 'conv', 'fwd', gy.dtype), gxf, ldgf, None, None, None, None, B, H, W, Cout, H, W, c1,
                     1, 1, 1, 1, 0, 0, False, 1, 0, False)
        # weight gradient, segment by segment
        xsv, ldxs = aligned_view(xs)
        xfv, ldxf = aligned_view(xf)
        gw_s, _ = wgrad(xsv, ldxs, gpv, ldgp, weight.detach()[:, :c0], None, ConvSpec('conv', 1, 1, 1, 1, 0, 0, h, w))
        gw_f, _ = wgrad(xfv, ldxf, g, ldg, weight.detach()[:, c0:], None, ConvSpec('conv', 1, 1, 1, 1, 0, 0, H, W))
        gw = torch.cat([gw_s * float(k * k), gw_f], 1)
        return gxs, gxf, gw, None, None


def upcat_conv1x1(xs, xf, weight, act=0):
    """act(conv1x1(cat([nearest_upsample(xs to xf's size), xf], 1))); None when the fused kernel does not apply (f32 parity
    path, sizes that are not a power-of-two multiple): the caller then composes interpolate + concat + conv."""
    if xs.dtype != torch.bfloat16 or xf.dtype != torch.bfloat16 or weight.dim() != 4 or weight.shape[2:] != (1, 1):
        return None
    H, W, h, w = xf.shape[2], xf.shape[3], xs.shape[2], xs.shape[3]
    if h == 0 or H % h or W % w or H // h != W // w:
        return None
    k = H // h
    if k < 1 or k & (k - 1) or k > 64 or xs.shape[1] % 8:
        return None
    return _UpCatConv1x1Fn.apply(xs, xf, weight, k.bit_length() - 1, act)


def conv_same_geometry(H, W, k, stride, dil):
    """TF-'same' padding of conv2dSame (models/torch_model.py:276-281): output ceil(size/stride), extra pad bottom/right."""
    def one(size):
        out = -(-size // stride)
        total = max((out - 1) * stride - size + dil * (k - 1) + 1, 0)
        return out, total // 2
    Ho, pt = one(H)
    Wo, pl = one(W)
    return Ho, Wo, pt, pl


def deconv_same_geometry(H, W, k, dil):
    """Stride-1 ConvTranspose2dSame (models/torch_model.py:320-346): full transposed conv of size H+dil*(k-1),
    cropped from start = full//2 - H//2; as a correlation with flipped taps the top/left padding is dil*(k-1) - start."""
    D = dil * (k - 1)
    def one(size):
        start = (size + D) // 2 - size // 2
        return D - start
    return one(H), one(W)


def conv_spec(x, weight, kind='conv', stride=1, dilation=1, padding=0):
    """padding: int (symmetric, nn.Conv2d), 'same' (conv2dSame) or 'ctsame' (stride-1 ConvTranspose2dSame)."""
    B, C, H, W = x.shape
    kh, kw = weight.shape[2], weight.shape[3]
    if kind == 'deconv':
        if stride != 1 or padding != 'ctsame' or kh != kw:
            raise _lib.SdhipError("ConvTranspose2d is implemented for stride 1 with 'same' cropping only")
        pt, pl = deconv_same_geometry(H, W, kh, dilation)
        Ho, Wo = H, W
    elif padding == 'same':
        if kh != kw:
            raise _lib.SdhipError("'same' padding needs a square kernel")
        Ho, Wo, pt, pl = conv_same_geometry(H, W, kh, stride, dilation)
    else:
        pt, pl = (int(padding[0]), int(padding[1])) if isinstance(padding, (tuple, list)) else (int(padding), int(padding))
        Ho = (H + 2 * pt - dilation * (kh - 1) - 1) // stride + 1
        Wo = (W + 2 * pl - dilation * (kw - 1) - 1) // stride + 1
    return ConvSpec(kind, kh, kw, stride, dilation, pt, pl, Ho, Wo)


def conv2d(x, weight, bias=None, *, kind='conv', stride=1, dilation=1, padding=0, act=0):
    return _ConvFn.apply(x, weight, bias, conv_spec(x, weight, kind, stride, dilation, padding), act)


def conv_bn_act(x, weight, bn, *, kind='conv', stride=1, dilation=1, padding=0, act=0, residual=None, groups=1,
                in_slot=None, res_slot=None, in_bn=None, out_bn=None):
    """in_slot / res_slot (GradSlot, optional): the gradient of `residual` is parked in res_slot instead of being returned
    to autograd, and a gradient parked in in_slot is summed into this node's data gradient by its own launch.
    in_bn / out_bn (BNSlot, optional): x is the output of the convbn + ReLU node that owns in_bn / this node's output has
    exactly one consumer, which holds out_bn as its in_bn."""
    fold = _fold_state(bn)
    if fold is not None and fold.train:
        # training step, frozen BatchNorm: the folded node when the layer has no skip, else the table form of _ConvBNActFn
        if fold.fold and residual is None and act in FOLD_ACTS and weight.dim() == 4 and x.dtype == fold.dtype:
            try:
                return _FoldedConvBNActFn.apply(x, weight, fold, conv_spec(x, weight, kind, stride, dilation, padding), bn, act,
                                                groups, in_slot, in_bn)
            except _NoFold:
                pass
    elif fold is not None:   # eval step: conv with the folded pack, bias and activation epilogue (FoldState)
        y = _folded_conv_bn_act(fold, x, weight, bn, conv_spec(x, weight, kind, stride, dilation, padding), act, residual, groups)
        if y is not None:
            return y
    return _ConvBNActFn.apply(x, weight, bn.weight, bn.bias, residual, conv_spec(x, weight, kind, stride, dilation, padding),
                              bn, act, groups, in_slot, res_slot, in_bn, out_bn)


def bn_conv(x, stats, bn, weight, *, padding=0, groups=1):
    """conv(relu(bn(x))) with x's batch statistics `stats` ([groups][2][C] f64) supplied by the producer of x."""
    return _BNConvFn.apply(x, stats, weight, bn.weight, bn.bias, conv_spec(x, weight, 'conv', 1, 1, padding), bn, groups)


def bn_act(x, stats, bn, act=1, groups=1):
    return _BNActFn.apply(x, stats, bn.weight, bn.bias, bn, act, groups)


class _AffineActFn(torch.autograd.Function):
    """y = act(x*scale + shift) (+ residual) with CONSTANT scale/shift (no gradient to them)."""

    @staticmethod
    def forward(ctx, x, scale, shift, residual, act):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        rv, ldr = nhwc_view(residual) if residual is not None else (None, 0)
        y = empty_nhwc(B, C, H, W, x.dtype, x.device)
        call("sdhip_affine_act", ptr(xv), ldx, ptr(y), C, ptr(rv), ldr, ptr(scale), ptr(shift), B * H * W, C, 1, act,
             dtype_code(x), stream_ptr())
        ctx.save_for_backward(xv, scale, shift)
        ctx.cfg = (ldx, act, residual is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, scale, shift = ctx.saved_tensors
        ldx, act, has_res = ctx.cfg
        B, C, H, W = xv.shape
        g, ldg = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, xv.dtype, xv.device)
        call("sdhip_affine_act_bwd", ptr(g), ldg, ptr(xv), ldx, ptr(gx), C, ptr(scale), ptr(shift), None, None, 1,
             B * H * W, C, 1, act, 0, 0, dtype_code(xv), stream_ptr())
        return gx, None, None, (gy if has_res else None), None


def affine_act(x, scale=None, shift=None, residual=None, act=0):
    return _AffineActFn.apply(x, scale, shift, residual, act)


# ============================================================================ pooling / resize / concat / broadcast product
class _MaxPool3s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = empty_nhwc(B, C, Ho, Wo, x.dtype, x.device)
        idx = torch.empty((B * Ho * Wo, C), dtype=torch.uint8, device=x.device)
        call("sdhip_maxpool3s2_fwd", ptr(xv), ldx, ptr(y), C, ptr(idx), B, H, W, C, dtype_code(x), stream_ptr())
        ctx.save_for_backward(idx)
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        g, ldg = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, gy.dtype, gy.device)
        call("sdhip_maxpool3s2_bwd", ptr(g), ldg, ptr(idx), ptr(gx), C, B, H, W, C, dtype_code(gy), stream_ptr())
        return gx


def maxpool3s2(x):
    return _MaxPool3s2Fn.apply(x)


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        y = empty_nhwc(B, C, H // k, W // k, x.dtype, x.device)
        call("sdhip_avgpool_fwd", ptr(xv), ldx, ptr(y), C, B, H, W, C, k, dtype_code(x), stream_ptr())
        ctx.cfg = (B, C, H, W, k)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, C, H, W, k = ctx.cfg
        g, ldg = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, gy.dtype, gy.device)
        call("sdhip_avgpool_bwd", ptr(g), ldg, ptr(gx), C, B, H, W, C, k, dtype_code(gy), stream_ptr())
        return gx, None


def avgpool(x, k):
    """k x k / stride k average pool.  Large windows are built as a chain of <= 8 x 8 pools (mean of equal-size
    means), which keeps every launch wide; nn.AvgPool2d(128) of a 128x256 map would otherwise be 2 serial threads."""
    while k > 8 and k % 2 == 0:
        step = 8 if k % 8 == 0 else 2
        x = _AvgPoolFn.apply(x, step)
        k //= step
    return _AvgPoolFn.apply(x, k) if k > 1 else x


_MODES = {'nearest': 0, 'bilinear': 1, 'bilinear_ac': 2}


class _ResizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Ho, Wo, mode, scale_h, scale_w, out):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        if out is None:
            y, ldy = empty_nhwc(B, C, Ho, Wo, x.dtype, x.device), C
        else:
            y, ldy = out, out.stride(3)
        call("sdhip_resize_fwd", ptr(xv), ldx, ptr(y), ldy, B, H, W, C, Ho, Wo, mode, scale_h, scale_w, dtype_code(x), stream_ptr())
        ctx.cfg = (B, C, H, W, Ho, Wo, mode, scale_h, scale_w)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, C, H, W, Ho, Wo, mode, scale_h, scale_w = ctx.cfg
        g, ldg = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, gy.dtype, gy.device)
        tmp = torch.empty(B * Ho * W * C, dtype=torch.float32, device=gy.device)
        call("sdhip_resize_bwd", ptr(g), ldg, ptr(gx), C, ptr(tmp), B, H, W, C, Ho, Wo, mode, scale_h, scale_w,
             dtype_code(gy), stream_ptr())
        return gx, None, None, None, None, None, None


def interpolate(x, size=None, scale_factor=None, mode='nearest', align_corners=None):
    """F.interpolate for the modes on the hot path.  A same-size nearest / bilinear(align_corners=False) resize is the
    identity (source index == destination index, lambda == 0) and is skipped."""
    B, C, H, W = x.shape
    if size is not None:
        Ho, Wo = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
        sh = sw = 0.0
    else:
        Ho, Wo = int(H * scale_factor), int(W * scale_factor)
        sh = sw = 1.0 / float(scale_factor)   # ATen uses the user scale when recompute_scale_factor is unset
    if mode == 'bilinear' and align_corners:
        m = 2
    elif mode in ('nearest', 'bilinear'):
        m = _MODES[mode]
    else:
        raise _lib.SdhipError("interpolate mode %r is not on the hot path" % mode)
    if (Ho, Wo) == (H, W) and m != 2:
        return x
    return _ResizeFn.apply(x, Ho, Wo, m, sh, sw, None)


class _SplitBatchFn(torch.autograd.Function):
    """x -> (x[:B], x[B:]) for the two tower halves of a batched pass.  The forward is free (views); the backward writes the
    two incoming gradients into the halves of ONE NHWC buffer (autograd's own slice backward builds two zero-filled NCHW
    tensors, adds them and leaves the consumer a layout conversion: ~1 ms per step)."""

    @staticmethod
    def forward(ctx, x, B):
        ctx.set_materialize_grads(False)          # an unused half arrives as None (zeroed below), not as an NCHW zero tensor
        ctx.B = B
        ctx.meta = (tuple(x.shape), x.dtype, x.device)
        return x[:B], x[B:]

    @staticmethod
    def backward(ctx, ga, gb):
        (N, C, H, W), dtype, dev = ctx.meta
        B = ctx.B
        if ga is None and gb is None:
            return None, None
        g, ld = alloc_nhwc(N, C, H, W, dtype, dev)
        for part, lo, hi in ((ga, 0, B), (gb, B, N)):
            dst = g[lo:hi]
            if part is None:
                dst.zero_()
                continue
            pv, ldp = nhwc_view(part)
            call("sdhip_affine_act", ptr(pv), ldp, ptr(dst), ld, None, 0, None, None, (hi - lo) * H * W, C, 1, 0, dtype_code(pv),
                 stream_ptr())
        return g, None


def split_batch(x, B):
    return _SplitBatchFn.apply(x, B)


class _ConcatFn(torch.autograd.Function):
    """torch.cat(dim=1) as copies into channel slices of one NHWC slab; the backward is free (views)."""

    @staticmethod
    def forward(ctx, *xs):
        _require_gpu(*xs)
        B, _, H, W = xs[0].shape
        Ct = sum(t.shape[1] for t in xs)
        out, ldo = alloc_nhwc(B, Ct, H, W, xs[0].dtype, xs[0].device)
        off, offs = 0, []
        for t in xs:
            C = t.shape[1]
            tv, ld = nhwc_view(t)
            dst = out[:, off:off + C]
            call("sdhip_affine_act", ptr(tv), ld, ptr(dst), ldo, None, 0, None, None, B * H * W, C, 1, 0, dtype_code(t), stream_ptr())
            offs.append((off, C))
            off += C
        ctx.offs = offs
        return out

    @staticmethod
    def backward(ctx, g):
        return tuple(g[:, o:o + c] for o, c in ctx.offs)


def concat(xs):
    return _ConcatFn.apply(*xs)


# ============================================================================ pooled pyramids (csrc/pyramid.hip)
class _Unfused(Exception):
    """An entry point of csrc/pyramid.hip declined its arguments in a forward pass (nothing was launched by it): the caller
    composes the single-tensor nodes instead."""


class _PyramidUpcatFn(torch.autograd.Function):
    """cat([x] + [bilinear(m -> x's size) for m in maps], 1) as ONE launch that writes whole rows of the slab, and the
    gradients of all maps in two; the x-part of the gradient stays a view of the slab's gradient, as in _ConcatFn."""

    @staticmethod
    def forward(ctx, x, *maps):
        _require_gpu(x, *maps)
        B, C, H, W = x.shape
        n, Cb = len(maps), maps[0].shape[1]
        if any(m.shape[0] != B or m.shape[1] != Cb or m.dtype != x.dtype for m in maps):
            raise _lib.SdhipError("pyramid_upcat: the branch maps must share x's batch and dtype and one channel count")
        xv, ldx = nhwc_view(x)
        mv = [nhwc_view(m) for m in maps]
        out, ldo = alloc_nhwc(B, C + n * Cb, H, W, x.dtype, x.device)
        arg, keep = _lib.pyr_maps([(v, v.shape[2], v.shape[3], ld) for v, ld in mv])
        if not try_call("sdhip_pyramid_upcat_fwd", ptr(xv), ldx, arg, n, ptr(out), ldo, B, H, W, C, Cb, dtype_code(x), stream_ptr()):
            raise _Unfused()
        ctx.cfg = (B, C, H, W, Cb, [(m.shape[2], m.shape[3]) for m in maps])
        return out

    @staticmethod
    def backward(ctx, gy):
        B, C, H, W, Cb, sizes = ctx.cfg
        n = len(sizes)
        need_x, need_m = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:])
        g, ldg = nhwc_view(gy)
        gms = [None] * n
        if need_m:
            gms = [empty_nhwc(B, Cb, h, w, g.dtype, g.device) for h, w in sizes]
            tmp = torch.empty(B * H * Cb * sum(w for _, w in sizes), dtype=torch.float32, device=g.device)
            arg, keep = _lib.pyr_maps([(t, h, w, Cb) for t, (h, w) in zip(gms, sizes)])
            if not try_call("sdhip_pyramid_upcat_bwd", ptr(g), ldg, arg, n, ptr(tmp), B, H, W, C, Cb, dtype_code(g), stream_ptr()):
                for j, (h, w) in enumerate(sizes):
                    call("sdhip_resize_bwd", ptr(g[:, C + j * Cb:C + (j + 1) * Cb]), ldg, ptr(gms[j]), Cb, ptr(tmp), B, h, w, Cb, H, W,
                         1, 0.0, 0.0, dtype_code(g), stream_ptr())
        return (g[:, :C] if need_x else None,) + tuple(gms)


def pyramid_upcat(x, maps):
    """cat([x] + [bilinear upsample of each map to x's size], 1); None where the fused kernel does not apply (the caller
    then composes interpolate + concat)."""
    try:
        return _PyramidUpcatFn.apply(x, *maps)
    except _Unfused:
        return None


class _RepeatBatchFn(torch.autograd.Function):
    """x -> [x | x] along the batch (one tower's map fed to both halves of a batched pass): two copies into one NHWC
    buffer; the backward adds the two halves of the incoming gradient."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        out, ldo = alloc_nhwc(2 * B, C, H, W, x.dtype, x.device)
        for lo in (0, B):
            call("sdhip_affine_act", ptr(xv), ldx, ptr(out[lo:lo + B]), ldo, None, 0, None, None, B * H * W, C, 1, 0, dtype_code(x),
                 stream_ptr())
        ctx.B = B
        return out

    @staticmethod
    def backward(ctx, g):
        with torch.no_grad():
            return add(g[:ctx.B], g[ctx.B:])


def repeat_batch(x):
    return _RepeatBatchFn.apply(x)


class _MulBcastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, m):
        _require_gpu(a, m)
        B, C, H, W = a.shape
        av, lda = nhwc_view(a)
        mv, ldm = nhwc_view(m)
        y = empty_nhwc(B, C, H, W, a.dtype, a.device)
        call("sdhip_mul_bcast_fwd", ptr(av), lda, ptr(mv), ldm, ptr(y), C, B * H * W, C, dtype_code(a), stream_ptr())
        ctx.save_for_backward(av, mv)
        ctx.cfg = (lda, ldm)
        return y

    @staticmethod
    def backward(ctx, g):
        av, mv = ctx.saved_tensors
        lda, ldm = ctx.cfg
        B, C, H, W = av.shape
        gv, ldg = nhwc_view(g)
        ga = empty_nhwc(B, C, H, W, av.dtype, av.device)
        gm = empty_nhwc(B, 1, H, W, av.dtype, av.device)
        call("sdhip_mul_bcast_bwd", ptr(gv), ldg, ptr(av), lda, ptr(mv), ldm, ptr(ga), C, ptr(gm), 1, B * H * W, C,
             dtype_code(av), stream_ptr())
        return ga, gm


def mul_bcast(a, m):
    """a (B,C,H,W) * m (B,1,H,W)."""
    return _MulBcastFn.apply(a, m)


# ============================================================================ disparity warp and gated blend
def _warp_check(right, disp, left=None, gate=None, softmax_gate=False):
    _require_gpu(right, disp, left, gate)
    if right.dim() != 4 or disp.dim() != 4:
        raise _lib.SdhipError("warp: maps must be (B,C,H,W), got %s and %s" % (tuple(right.shape), tuple(disp.shape)))
    B, C, H, W = right.shape
    if tuple(disp.shape) != (B, 1, H, W):
        raise _lib.SdhipError("warp: the offset must be (B,1,H,W) = %s, got %s" % ((B, 1, H, W), tuple(disp.shape)))
    if disp.dtype != right.dtype:
        raise _lib.SdhipError("warp: the offset's dtype %s differs from the map's %s" % (disp.dtype, right.dtype))
    if gate is not None:
        if tuple(left.shape) != (B, C, H, W) or left.dtype != right.dtype or gate.dtype != right.dtype:
            raise _lib.SdhipError("warp_blend: seg_left %s / seg_right %s / gate differ in shape or dtype" % (tuple(left.shape), (B, C, H, W)))
        if tuple(gate.shape) not in ((B, 1, H, W), (B, C, H, W)) or (softmax_gate and gate.shape[1] != C):
            raise _lib.SdhipError("warp_blend: the gate must be (B,1,H,W) or (B,C,H,W) (softmax: C channels), got %s" % (tuple(gate.shape),))


class _WarpBlendFn(torch.autograd.Function):
    """sdhip_warp_blend_fwd / _bwd.  gate None: (warped,) = apply_disparity(right, sign * disp).  Otherwise
    (both, warped[, prob]) with both = (1 - a) * left + a * warped; prob (softmax gate only) is not differentiable."""

    @staticmethod
    def forward(ctx, left, right, disp, gate, sign, softmax_gate):
        _warp_check(right, disp, left, gate, softmax_gate)
        B, C, H, W = right.shape
        rv, ldr = nhwc_view(right)
        dv, ldd = nhwc_view(disp)
        warped = empty_nhwc(B, C, H, W, right.dtype, right.device)
        lv = gv = both = prob = None
        ldl = ldgt = gch = 0
        if gate is not None:
            lv, ldl = nhwc_view(left)
            gv, ldgt = nhwc_view(gate)
            gch = gate.shape[1]
            both = empty_nhwc(B, C, H, W, right.dtype, right.device)
            if softmax_gate:
                prob = empty_nhwc(B, C, H, W, right.dtype, right.device)
        call("sdhip_warp_blend_fwd", ptr(lv), ldl, ptr(rv), ldr, ptr(dv), ldd, float(sign), ptr(gv), ldgt, gch, int(softmax_gate),
             ptr(warped), C, ptr(both), C, ptr(prob), C, B, H, W, C, dtype_code(right), stream_ptr())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(lv, rv, dv, prob if softmax_gate else gv)
        ctx.cfg = (ldl, ldr, ldd, C if softmax_gate else ldgt, gch, float(sign), bool(softmax_gate))
        if gate is None:
            return warped
        if softmax_gate:
            ctx.mark_non_differentiable(prob)
            return both, warped, prob
        return both, warped

    @staticmethod
    def backward(ctx, *gs):
        lv, rv, dv, av = ctx.saved_tensors
        ldl, ldr, ldd, lda, gch, sign, softmax_gate = ctx.cfg
        B, C, H, W = rv.shape
        g_both, g_warped = (None, gs[0]) if av is None else (gs[0], gs[1])
        if g_both is None and g_warped is None:
            return None, None, None, None, None, None
        gb, ldgb = nhwc_view(g_both) if g_both is not None else (None, 0)
        gw, ldgw = nhwc_view(g_warped) if g_warped is not None else (None, 0)
        need = ctx.needs_input_grad
        dev, dt = rv.device, rv.dtype
        g_left = empty_nhwc(B, C, H, W, dt, dev) if av is not None and need[0] else None
        g_right = empty_nhwc(B, C, H, W, dt, dev) if need[1] else None
        g_disp = torch.empty((B, 1, H, W), dtype=dt, device=dev) if need[2] else None
        g_gate = empty_nhwc(B, gch, H, W, dt, dev) if av is not None and need[3] else None
        call("sdhip_warp_blend_bwd", ptr(gb), ldgb, ptr(gw), ldgw, ptr(lv), ldl, ptr(rv), ldr, ptr(dv), ldd, sign, ptr(av), lda, gch,
             int(softmax_gate), ptr(g_left), C, ptr(g_right), C, ptr(g_disp), 1, ptr(g_gate), gch, B, H, W, C, dtype_code(rv),
             stream_ptr())
        return g_left, g_right, g_disp, g_gate, None, None


def apply_disparity(img, x_offset, sign=1.0):
    """models/torch_dsnet.py apply_disparity(img, x_offset) with wrap_mode='edge': img (B,C,H,W) sampled at column
    j + x_offset[b,0,y,j] with linear interpolation, differentiable in both arguments.  The reference's edge rules hold:
    a sample at or beyond the right edge is 0, one beyond the left edge copies column 0, and a clamped offset gets no gradient.
    sign=-1.0 is apply_disparity(img, -x_offset) without a pass that negates the map (the networks warp with -disp)."""
    if sign not in (1.0, -1.0):
        raise _lib.SdhipError("apply_disparity: sign must be 1.0 or -1.0, got %r" % (sign,))
    return _WarpBlendFn.apply(None, img, x_offset, None, float(sign), False)


def warp_blend(seg_left, seg_right, disp, gate, softmax_gate=False):
    """(both, warped_right[, gate_probabilities]): warped_right = apply_disparity(seg_right, -disp) and
    both = (1 - a) * seg_left + a * warped_right in one pass.  gate: (B,1,H,W) or (B,C,H,W) blend weights a; with
    softmax_gate the gate holds raw (B,C,H,W) scores, a is their softmax over the channels and is returned third."""
    if gate is None:
        raise _lib.SdhipError("warp_blend needs a gate; the plain warp is apply_disparity")
    return _WarpBlendFn.apply(seg_left, seg_right, disp, gate, -1.0, softmax_gate)


# ---------------------------------------------------------------------------- the *_disp networks (warp.minidsnetDivideDisp / Disp2)
def _nhwc_ld(x):
    """Pixel stride of x if its memory is NHWC with a uniform pixel stride (nhwc_view would return x itself), else None."""
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if W == 1:
        sw = sh
    ok = (sc == 1 or C == 1) and sw >= C and (sh == W * sw or H == 1) and (sb == H * W * sw or B == 1)
    return sw if ok else None


def warp_image_masked(right, gt_disp, out=None):
    """apply_disparity(right, -gt_disp) * (gt_disp > 0): the image the third tower pass of minidsnetDivideDisp reads
    (models/dsnet_t2_warp.py:811), one launch, no gradient (the ground truth is a constant).
      right   — (B, 1 <= C <= 4, H, W) f32 or bf16; NCHW, channels-last or a channel slice of either, no copy is made
      gt_disp — dense f32 (B,1,H,W)
      out     — optional (B,C,H,W) f32 / bf16 tensor in NHWC memory (pixel stride >= C); default: right's dtype at the padded
                pixel stride the conv nodes read.  Pad lanes are not written.
    The edge rules of apply_disparity hold: a sample at or beyond the right edge is 0, one clamped on the left copies column 0."""
    if right.dim() != 4 or gt_disp.dim() != 4:
        raise _lib.SdhipError("warp_image_masked: image and disparity must be 4-D, got %s and %s" % (tuple(right.shape), tuple(gt_disp.shape)))
    B, C, H, W = right.shape
    if min(B, H, W) < 1 or not 1 <= C <= 4:
        raise _lib.SdhipError("warp_image_masked: need B, H, W >= 1 and 1 <= C <= 4, got %s" % (tuple(right.shape),))
    if tuple(gt_disp.shape) != (B, 1, H, W) or gt_disp.dtype != torch.float32 or not gt_disp.is_contiguous():
        raise _lib.SdhipError("warp_image_masked: the disparity must be a dense f32 (B,1,H,W) = %s tensor, got %s %s"
                              % ((B, 1, H, W), gt_disp.dtype, tuple(gt_disp.shape)))
    dt_in = dtype_code(right)
    if right.requires_grad or gt_disp.requires_grad:
        raise _lib.SdhipError("warp_image_masked has no backward pass: its inputs must not require a gradient (ops.apply_disparity has one)")
    if out is not None:
        if tuple(out.shape) != (B, C, H, W) or out.dtype not in (torch.float32, torch.bfloat16) or _nhwc_ld(out) is None:
            raise _lib.SdhipError("warp_image_masked: `out` must be a (B,C,H,W) = %s f32 / bf16 tensor in NHWC memory" % ((B, C, H, W),))
    _require_gpu(right, gt_disp, out)
    right, strides = _strided_image(right)
    if out is None:
        out, ldy = alloc_nhwc(B, C, H, W, right.dtype, right.device)
    else:
        ldy = _nhwc_ld(out)
    call("sdhip_warp_image_masked", ptr(right), strides[0], strides[1], strides[2], dt_in, ptr(gt_disp), ptr(out), ldy, dtype_code(out),
         B, H, W, C, stream_ptr())
    return out


class _GateFn(torch.autograd.Function):
    """A one-channel gate g on two C-channel maps, `pair` choosing between the two operators (csrc/edge.hip, csrc/warp.hip):
      pair:  cat(a * g, b * (1 - g), dim=1) written straight into one 2C-channel NHWC slab at the padded pixel stride
      blend: (1 - g) * a + g * b, C channels
    ga, gb and gg come out of one backward launch."""

    @staticmethod
    def forward(ctx, a, b, g, pair):
        B, C, H, W = a.shape
        av, lda = nhwc_view(a)
        bv, ldb = nhwc_view(b)
        gv, ldg = nhwc_view(g)
        y, ldy = alloc_nhwc(B, 2 * C, H, W, a.dtype, a.device) if pair else (empty_nhwc(B, C, H, W, a.dtype, a.device), C)
        call("sdhip_gate_pair_fwd" if pair else "sdhip_gate_blend_fwd", ptr(av), lda, ptr(bv), ldb, ptr(gv), ldg, ptr(y), ldy,
             B * H * W, C, dtype_code(a), stream_ptr())
        ctx.save_for_backward(av, bv, gv)
        ctx.cfg = (lda, ldb, ldg, pair)
        return y

    @staticmethod
    def backward(ctx, gy):
        av, bv, gv = ctx.saved_tensors
        lda, ldb, ldg, pair = ctx.cfg
        B, C, H, W = av.shape
        gyv, ldgy = nhwc_view(gy)
        ga = empty_nhwc(B, C, H, W, av.dtype, av.device)
        gb = empty_nhwc(B, C, H, W, av.dtype, av.device)
        gg = empty_nhwc(B, 1, H, W, av.dtype, av.device)
        call("sdhip_gate_pair_bwd" if pair else "sdhip_gate_blend_bwd", ptr(gyv), ldgy, ptr(av), lda, ptr(bv), ldb, ptr(gv), ldg,
             ptr(ga), C, ptr(gb), C, ptr(gg), 1, B * H * W, C, dtype_code(av), stream_ptr())
        return ga, gb, gg, None


def _check_gate_args(who, a, b, g):
    if a.dim() != 4 or tuple(b.shape) != tuple(a.shape) or tuple(g.shape) != (a.shape[0], 1) + tuple(a.shape[2:]):
        raise _lib.SdhipError("%s: need a, b (B,C,H,W) and g (B,1,H,W), got %s, %s and %s"
                              % (who, tuple(a.shape), tuple(b.shape), tuple(g.shape)))
    if a.numel() < 1:
        raise _lib.SdhipError("%s of an empty tensor" % who)
    if not a.dtype == b.dtype == g.dtype:
        raise _lib.SdhipError("%s: a, b and g must share one dtype, got %s, %s and %s" % (who, a.dtype, b.dtype, g.dtype))
    dtype_code(a)
    _require_gpu(a, b, g)


def gate_blend(a, b, g):
    """(1 - g) * a + g * b for a, b (B,C,H,W) and a one-channel gate g (B,1,H,W), all of one dtype (f32 / bf16): the unwarped blend
    `seg_branch_both` of the *_disp networks (models/dsnet_t2_warp.py:834) as one launch, and one backward launch for all three
    gradients.  (warp_blend with a zero disparity is NOT this: the warp's right-edge rule zeroes the last column.)"""
    _check_gate_args("gate_blend", a, b, g)
    return _GateFn.apply(a, b, g, False)


# ---------------------------------------------------------------------------- plumbing of the scalar loss terms
_loss_ws = {}


def _loss_workspace(term, key, nbytes, device):
    """The scratch buffer the kernels of loss term `term` fold their slots in (csrc/loss_common.h), for the problem `key` on
    `device`: uint8, at least nbytes, a whole number of 8-byte slots.  Cached, so a captured step finds it allocated; the
    term is part of the key, so two terms of one step never share a buffer."""
    key = (term,) + tuple(key) + (str(device),)
    ws = _loss_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((nbytes + 7) // 8 * 8, dtype=torch.uint8, device=device)
        _loss_ws[key] = ws
    return ws


class _ValueGradFn(torch.autograd.Function):
    """A scalar loss term whose kernels produce value and gradient in one pass: photo_loss, seg_loss, disp_smooth_loss,
    edge_loss.  `launch(x, loss, *args)` adds the term onto the f64 `loss` and returns its gradient w.r.t. x, the one input
    that gets one."""

    @staticmethod
    def forward(ctx, x, launch, *args):
        loss = torch.zeros(1, dtype=torch.float64, device=x.device)
        ctx.save_for_backward(launch(x, loss, *args))
        ctx.nargs = 2 + len(args)
        return loss.float().reshape(())

    @staticmethod
    def backward(ctx, gout):
        g, = ctx.saved_tensors
        return (g * gout.to(g.dtype),) + (None,) * (ctx.nargs - 1)


def _dense_disp(disp):
    """A (B,1,H,W) map as the loss kernels read it, pixel after pixel: disp itself, or a dense copy of a 1-channel map that
    sits inside a padded pixel stride (a direct conv output)."""
    dv, ldd = nhwc_view(disp)
    return dv if ldd == 1 else disp.contiguous()


def _photo_term(warped, loss, left, weight):
    """loss += weight * MSELoss(warped, left); returns the gradient w.r.t. warped: the two launches of sdhip_photo_mse."""
    B, C, H, W = warped.shape
    wv, ldw = nhwc_view(warped)
    left, strides = _strided_image(left)
    npix = B * H * W
    ws = _loss_workspace("photo", (npix,), _lib.photo_mse_workspace_bytes(npix), warped.device)
    g = empty_nhwc(B, C, H, W, warped.dtype, warped.device)
    call("sdhip_photo_mse", ptr(wv), ldw, dtype_code(wv), ptr(left), strides[0], strides[1], strides[2], ptr(g), ptr(loss), weight,
         B, H, W, C, ptr(ws), ws.numel(), stream_ptr())
    return g


def photo_loss(warped, left, weight=1.0):
    """weight * torch.nn.MSELoss()(warped, left): the photometric term of the reference's `ThreeOutPutsDispConsist` step
    (torch_implementation.py:314-317), the mean over batch, channels and pixels of the squared difference.
      warped — (B, 1 <= C <= 4, H, W) f32 or bf16 (the warped right image, a network output); the only input that gets a
               gradient, 2 * weight * (warped - left) / (B*C*H*W) in its dtype
      left   — f32 image of the same shape; NCHW, channels-last or a channel slice of either, no copy is made
    Returns an f32 scalar; value and gradient are reproducible bit for bit and do not depend on the operands' strides."""
    if warped.dim() != 4 or left.dim() != 4:
        raise _lib.SdhipError("photo_loss: warped and left must be 4-D (B,C,H,W), got %s and %s" % (tuple(warped.shape), tuple(left.shape)))
    if tuple(warped.shape) != tuple(left.shape):
        raise _lib.SdhipError("photo_loss: warped %s and left %s differ in shape (MSELoss of a 3-channel warp needs the 3-channel "
                              "image)" % (tuple(warped.shape), tuple(left.shape)))
    if warped.numel() < 1 or not 1 <= warped.shape[1] <= 4:
        raise _lib.SdhipError("photo_loss: need B, H, W >= 1 and 1 <= C <= 4, got %s" % (tuple(warped.shape),))
    if left.dtype != torch.float32:
        raise _lib.SdhipError("photo_loss: the left image must be f32, the input a step is fed (got %s)" % left.dtype)
    dtype_code(warped)
    _require_gpu(warped, left)
    if warped.device != left.device:
        raise _lib.SdhipError("photo_loss: warped and left live on different devices")
    return _ValueGradFn.apply(warped, _photo_term, left, float(weight))


# ============================================================================ losses of the timed step
# entries of the reference's `-loss` list (losses/multiLosses.py:8-128) built here / defined upstream but not built
SEG_LOSS_TERMS = ("cross_entropy", "lovasz_loss", "tversky_loss2", "dice_loss", "diceEntropy")
SEG_LOSS_NOT_BUILT = ("tversky_loss", "area_ce", "area_hinge", "binary_ce", "categoricalNlll", "ohm_loss", "dual_edge_reg")
SEG_MAX_CLASSES = 32


def seg_loss_plan(loss):
    """(ce_weight, lovasz_weight, term bits) of a `-loss` list as lossSeg_fn reads it: cross-entropy and the Lovasz term that
    follows it are halved when the list has more than two entries (losses/multiLosses.py:64-72), Lovasz without
    cross-entropy has factor 1 (:80-81), diceEntropy counts only when dice_loss is absent (:107-115).  A name the reference
    defines but this package does not build raises NotImplementedError; any other string raises ValueError (the reference
    ignores it silently)."""
    names = [loss] if isinstance(loss, str) else list(loss)
    for n in names:
        if n in SEG_LOSS_NOT_BUILT:
            raise NotImplementedError("segmentation loss term %r is not built (built: %s)" % (n, ", ".join(SEG_LOSS_TERMS)))
        if n not in SEG_LOSS_TERMS:
            raise ValueError("unknown segmentation loss term %r (known: %s)" % (n, ", ".join(SEG_LOSS_TERMS + SEG_LOSS_NOT_BUILT)))
    ce = "cross_entropy" in names
    w1 = 0.5 if ce and len(names) > 2 else 1.0
    terms = 0
    if "tversky_loss2" in names:
        terms |= _lib.SEG_TVERSKY
    if "dice_loss" in names:
        terms |= _lib.SEG_DICE
    elif "diceEntropy" in names:
        terms |= _lib.SEG_DICE_ENTROPY
    return (w1 if ce else 0.0), (w1 if "lovasz_loss" in names else 0.0), terms


def seg_class_weights(class_weights, C=None, device=None):
    """The `-segWeight` table as the kernels read it: C f32 on the GPU (None stays None = no weights).  A sequence is uploaded
    (do this once, before a step is captured); a tensor must already be f32 on the GPU."""
    if class_weights is None:
        return None
    n = class_weights.numel() if isinstance(class_weights, torch.Tensor) else len(class_weights)
    if C is not None and n != C:
        raise _lib.SdhipError("class_weights has %d entries for %d classes" % (n, C))
    if isinstance(class_weights, torch.Tensor):
        _require_gpu(class_weights)
        if class_weights.dtype != torch.float32 or class_weights.dim() != 1 or not class_weights.is_contiguous():
            raise _lib.SdhipError("class_weights must be a contiguous 1-D f32 tensor")
        return class_weights
    if device is None or torch.device(device).type != "cuda":
        raise _lib.SdhipError("sdhip ops need a GPU (got %s for class_weights); there is no CPU path" % device)
    return torch.tensor([float(v) for v in class_weights], dtype=torch.float32, device=device)


def _seg_terms(s, tv, ldt, grad, loss, ce_weight, terms, cw):
    """loss += the sum-based terms of one segmentation head, grad = their gradient: the three launches of csrc/segloss.hip.
    (tv, ldt): nhwc_view of the one-hot target."""
    B, C, H, W = s.shape
    sv, ld = nhwc_view(s)
    ws = _loss_workspace("seg", (B, H * W, C), _lib.seg_terms_workspace_bytes(B, H * W, C), s.device)
    dt, st = dtype_code(s), stream_ptr()
    call("sdhip_seg_sums", ptr(sv), ld, ptr(tv), ldt, B, H * W, C, ptr(ws), ws.numel(), dt, st)
    call("sdhip_seg_finish", ptr(ws), ws.numel(), ptr(cw), ptr(loss), B, H * W, C, ce_weight, terms, st)
    call("sdhip_seg_terms_bwd", ptr(sv), ld, ptr(tv), ldt, ptr(grad), C, ptr(ws), ws.numel(), B, H * W, C, dt, st)


def _lovasz_term(s, tv, ldt, grad, loss, weight, ignore_void):
    """loss += weight * Lovasz-softmax, grad += its gradient (in place, onto what the other terms left there)."""
    B, C, H, W = s.shape
    npix = B * H * W
    sv, ld = nhwc_view(s)
    ws = _loss_workspace("lovasz", (npix, C), _lib.lovasz_workspace_bytes(npix, C), s.device)
    call("sdhip_lovasz_softmax", ptr(sv), ld, ptr(tv), ldt, ptr(grad), C, ptr(loss), npix, C, weight, ptr(ws),
         ws.numel(), int(ignore_void), dtype_code(s), stream_ptr())


def _check_seg_args(logits, seg_t, class_weights):
    if logits.dim() != 4 or tuple(seg_t.shape) != tuple(logits.shape):
        raise _lib.SdhipError("segmentation logits and one-hot target must both be (B,C,H,W), got %s and %s"
                              % (tuple(logits.shape), tuple(seg_t.shape)))
    C = logits.shape[1]
    if C > SEG_MAX_CLASSES:
        raise _lib.SdhipError("the segmentation loss terms serve at most %d classes (got %d)" % (SEG_MAX_CLASSES, C))
    if seg_t.dtype != torch.float32:
        raise _lib.SdhipError("the one-hot segmentation target must be f32 (got %s)" % seg_t.dtype)
    if class_weights is not None:
        n = class_weights.numel() if isinstance(class_weights, torch.Tensor) else len(class_weights)
        if n != C:
            raise _lib.SdhipError("class_weights has %d entries for %d classes" % (n, C))


def _seg_loss_term(logits, loss, seg_t, plan, cw, ignore_void):
    """loss += lossSeg_fn(loss list, ...)[2] on one segmentation head (losses/multiLosses.py:8-128); returns the gradient."""
    ce_weight, lovasz_weight, terms = plan
    B, C, H, W = logits.shape
    g = empty_nhwc(B, C, H, W, logits.dtype, logits.device)
    tv, ldt = nhwc_view(seg_t)
    _seg_terms(logits, tv, ldt, g, loss, ce_weight, terms, cw)
    if lovasz_weight:
        _lovasz_term(logits, tv, ldt, g, loss, lovasz_weight, ignore_void)
    return g


def seg_loss(logits, seg_target, loss=("cross_entropy",), class_weights=None, ignore_void=False):
    """The segmentation loss of one head as the reference's lossSeg_fn(loss, seg_target, logits, CFG, ...)[2] adds it up.
    logits (B,C,H,W) f32 / bf16, C <= 32; seg_target: one-hot f32 (B,C,H,W), a void pixel is an all-zero row (cityscapes /
    kitti: the 20th channel already dropped).
      loss          — the `-loss` list: cross_entropy, lovasz_loss, tversky_loss2, dice_loss, diceEntropy (seg_loss_plan)
      class_weights — the `-segWeight 1` table of the dataset, supplied by the caller (length C): multiplies the
                      cross-entropy and the Tversky term per class; never the dice terms or Lovasz
      ignore_void   — the Lovasz term's rule for void pixels (train_loss)
    Returns an f32 scalar; value and gradient are reproducible bit for bit except for the Lovasz term."""
    plan = seg_loss_plan(loss)
    _check_seg_args(logits, seg_target, class_weights)
    _require_gpu(logits, seg_target)
    cw = seg_class_weights(class_weights, logits.shape[1], logits.device)
    return _ValueGradFn.apply(logits, _seg_loss_term, seg_target, plan, cw, bool(ignore_void))


class _TrainLossFn(torch.autograd.Function):
    """total = CE(seg1) + CE(seg2) [+ Lovasz(seg2)] + L1(disp) [+ CE(seg3)]  — the loss of the reference's training step
    (torch_implementation.py:279,293,304,325 with `-loss cross_entropy lovasz_loss`; seg3: the third segmentation output of
    the `ThreeOutPuts` networks, :157-158,298).  The gradients w.r.t. the network outputs are produced in the same pass."""

    @staticmethod
    def forward(ctx, seg1, disp, seg2, seg_t, disp_t, use_lovasz, mask_invalid_disp=False, ignore_void=False, seg3=None,
                plan=None, cw=None):
        _require_gpu(seg1, disp, seg2, seg_t, disp_t, seg3)
        B, C, H, W = seg1.shape
        npix = B * H * W
        dt = dtype_code(seg1)
        loss = torch.zeros(1, dtype=torch.float64, device=seg1.device)
        tv, ldt = nhwc_view(seg_t)
        grads = []
        lovasz_weight = 1.0
        for i, s in enumerate((seg1, seg2) if seg3 is None else (seg1, seg2, seg3)):
            sv, ld = nhwc_view(s)
            g = empty_nhwc(B, C, H, W, s.dtype, s.device)
            if plan is None:
                call("sdhip_ce_loss", ptr(sv), ld, ptr(tv), ldt, ptr(g), C, ptr(loss), npix, C, 1.0, dt, stream_ptr())
            elif i == 1 and plan is not None:      # seg2 takes the `-loss` list (torch_implementation.py:293)
                ce_weight, lovasz_weight, terms = plan
                use_lovasz = lovasz_weight != 0.0
                _seg_terms(s, tv, ldt, g, loss, ce_weight, terms, cw)
            else:                                   # seg1 / seg3: ['cross_entropy'] with the class weights (:279,297)
                _seg_terms(s, tv, ldt, g, loss, 1.0, 0, cw)
            grads.append(g)
        dv = _dense_disp(disp)
        if not disp_t.is_contiguous():
            raise _lib.SdhipError("disparity target must be a dense (B,1,H,W) tensor")
        gd = torch.empty_like(dv)
        call("sdhip_l1_loss", ptr(dv), ptr(disp_t), ptr(gd), ptr(loss), npix, 1.0, int(mask_invalid_disp), dt, stream_ptr())
        if use_lovasz:   # added onto the gradient of seg2's other terms in place
            _lovasz_term(seg2, tv, ldt, grads[1], loss, lovasz_weight, ignore_void)
        total = loss
        ctx.save_for_backward(grads[0], gd, grads[1], grads[2] if seg3 is not None else None)
        return total.float()

    @staticmethod
    def backward(ctx, g):
        g1, gd, g2, g3 = ctx.saved_tensors
        return g1, gd, g2, None, None, None, None, None, g3, None, None   # d(total)/d(total) is 1 in the training step


MT_IGNORE_INDEX = 19     # F.cross_entropy(..., ignore_index=19) of util/utilTorchLoss.py:533,535, whatever the class count


def _map_grad(g):
    """(f32 tensor, g_stride) of the upstream gradient of a per-pixel loss map: an expanded scalar (every stride 0, what
    autograd hands over for `.sum()`) is read in place; anything else as a dense map."""
    if g is None:
        return None, 0
    if all(s == 0 for s in g.stride()):
        return g.float(), 0
    return g.float().contiguous(), 1


def _log_var_grad(log_var):
    """(pointer target the kernel accumulates d/d log_var into, gradient to hand back to autograd or None)."""
    t = _grad_target(log_var)
    if t is not None:
        return t, None
    g, _ = _zeros((1,), torch.float32, log_var.device)
    return g, g.view(log_var.shape)


def _check_log_var(log_var):
    if log_var.numel() != 1 or log_var.dtype != torch.float32 or not log_var.is_contiguous():
        raise _lib.SdhipError("log-variance must be one contiguous f32 element (got %s %s)" % (tuple(log_var.shape), log_var.dtype))


class _MTSegFn(torch.autograd.Function):
    """(map, mean): map = exp(-lv) * CE(logits, labels, ignore_index, reduction='none') + lv, (B,H,W) f32, and its mean from
    the f64 sum the same pass accumulates (util/utilTorchLoss.py:533-536)."""

    @staticmethod
    def forward(ctx, logits, labels, log_var, ignore_index):
        _require_gpu(logits, labels, log_var)
        _check_log_var(log_var)
        B, C, H, W = logits.shape
        if tuple(labels.shape) != (B, H, W):
            raise _lib.SdhipError("labels must be (B,H,W) = %s, got %s" % ((B, H, W), tuple(labels.shape)))
        npix = B * H * W
        yv, ld = nhwc_view(logits)
        lab = labels.long().contiguous()
        m = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
        lse = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
        mean = torch.empty((), dtype=torch.float32, device=logits.device)
        s, _ = _zeros((1,), torch.float64, logits.device)
        call("sdhip_mt_seg_fwd", ptr(yv), ld, ptr(lab), ptr(log_var), ptr(m), ptr(lse), ptr(s), ptr(mean), npix, C, int(ignore_index),
             1.0 / npix, dtype_code(logits), stream_ptr())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(yv, lab, lse, log_var)
        ctx.cfg = (ld, B, C, H, W, int(ignore_index))
        return m, mean

    @staticmethod
    def backward(ctx, gmap, gmean):
        yv, lab, lse, log_var = ctx.saved_tensors
        ld, B, C, H, W, ign = ctx.cfg
        npix = B * H * W
        if gmap is None and gmean is None:
            return None, None, None, None
        g, gs = _map_grad(gmap)
        gm = gmean.float().contiguous() if gmean is not None else None
        gx = empty_nhwc(B, C, H, W, yv.dtype, yv.device) if ctx.needs_input_grad[0] else None
        tlv, glv = _log_var_grad(log_var) if ctx.needs_input_grad[2] else (None, None)
        call("sdhip_mt_seg_bwd", ptr(yv), ld, ptr(lab), ptr(lse), ptr(log_var), ptr(g), gs, ptr(gm), 1.0 / npix, ptr(gx), C,
             ptr(tlv), npix, C, ign, dtype_code(yv), stream_ptr())
        return gx, None, glv, None


class _MTL1Fn(torch.autograd.Function):
    """(map, mean): map = exp(-lv) * |pred - target| + lv, (B,1,H,W) f32 (util/utilTorchLoss.py:532; no disp > 0 mask)."""

    @staticmethod
    def forward(ctx, pred, target, log_var):
        _require_gpu(pred, target, log_var)
        _check_log_var(log_var)
        B, C, H, W = pred.shape
        if C != 1 or tuple(target.shape) != (B, 1, H, W):
            raise _lib.SdhipError("disparity and its target must be (B,1,H,W), got %s and %s" % (tuple(pred.shape), tuple(target.shape)))
        n = B * H * W
        pv, ldp = nhwc_view(pred)
        t = target.float().contiguous()
        m = torch.empty((B, 1, H, W), dtype=torch.float32, device=pred.device)
        mean = torch.empty((), dtype=torch.float32, device=pred.device)
        s, _ = _zeros((1,), torch.float64, pred.device)
        call("sdhip_mt_l1_fwd", ptr(pv), ldp, ptr(t), ptr(log_var), ptr(m), ptr(s), ptr(mean), n, 1.0 / n, dtype_code(pred), stream_ptr())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(pv, t, log_var)
        ctx.cfg = (ldp, B, H, W)
        return m, mean

    @staticmethod
    def backward(ctx, gmap, gmean):
        pv, t, log_var = ctx.saved_tensors
        ldp, B, H, W = ctx.cfg
        n = B * H * W
        if gmap is None and gmean is None:
            return None, None, None
        g, gs = _map_grad(gmap)
        gm = gmean.float().contiguous() if gmean is not None else None
        gp = torch.empty((B, 1, H, W), dtype=pv.dtype, device=pv.device) if ctx.needs_input_grad[0] else None
        tlv, glv = _log_var_grad(log_var) if ctx.needs_input_grad[2] else (None, None)
        call("sdhip_mt_l1_bwd", ptr(pv), ldp, ptr(t), ptr(log_var), ptr(g), gs, ptr(gm), 1.0 / n, ptr(gp), 1, ptr(tlv), n,
             dtype_code(pv), stream_ptr())
        return gp, None, glv


def multitask_seg_loss(logits, labels, log_var, ignore_index=MT_IGNORE_INDEX):
    """exp(-lv) * F.cross_entropy(logits, labels, ignore_index=ignore_index, reduction='none') + lv, (B,H,W) f32.  A label
    outside [0, C) counts as ignored (the reference raises).  The returned map carries its mean, computed by the same
    pass, as `map.sdhip_mean` (loss_map_mean)."""
    m, mean = _MTSegFn.apply(logits, labels, log_var, ignore_index)
    m.sdhip_mean = mean
    return m


def multitask_l1_loss(pred, target, log_var):
    """exp(-lv) * F.l1_loss(pred, target, reduction='none') + lv, (B,1,H,W) f32; `map.sdhip_mean` as multitask_seg_loss."""
    m, mean = _MTL1Fn.apply(pred, target, log_var)
    m.sdhip_mean = mean
    return m


def loss_map_mean(m):
    """mean(m) of a map returned by multitask_seg_loss / multitask_l1_loss: the f32 scalar their forward pass produced from
    its f64 sum (no reduction kernel); its gradient reaches the map's backward kernel as one uniform term."""
    mean = getattr(m, "sdhip_mean", None)
    if mean is None:
        raise _lib.SdhipError("loss_map_mean: the map was not produced by a multitask loss operator")
    return mean


def train_loss(seg1, disp, seg2, seg_target, disp_target, use_lovasz=True, mask_invalid_disp=False, ignore_void=False, seg3=None,
               loss=None, class_weights=None):
    """seg_target: one-hot f32 (B,C,H,W); disp_target: f32 (B,1,H,W); seg3 (optional): a third segmentation output that adds
    its cross-entropy (the warp networks).  The two dataset rules of losses/multiLosses.py are
    opt-in, both off by default (roses / garden, `ignore=None`, :11-17):
      ignore_void       — cityscapes / kitti (:19-21, the 20th one-hot channel dropped, `ignore=19`): an all-zero target row
                          marks a void pixel, removed from the Lovasz term.  Off: its label is argmax = class 0 and it counts.
                          (Its cross-entropy term is zero under either rule: sum(-t * log_softmax) over a zero row.)
      mask_invalid_disp — disparities <= 0 are invalid (:134-141).
    loss (the reference's `-loss` list, seg_loss_plan) replaces `CE(seg2) [+ Lovasz(seg2)]` by the list's terms on seg2 and
    then decides about Lovasz instead of use_lovasz; class_weights (`-segWeight 1`: the dataset's table, length C, from the
    caller) multiplies the cross-entropy of seg1, seg2 and seg3 and the Tversky term.  With one of them given and the other
    None, the list is what use_lovasz says and the weights are 1.  Both None: the step's original launches."""
    if loss is None and class_weights is None:
        return _TrainLossFn.apply(seg1, disp, seg2, seg_target, disp_target, use_lovasz, mask_invalid_disp, ignore_void, seg3)
    plan = seg_loss_plan(loss if loss is not None else (("cross_entropy", "lovasz_loss") if use_lovasz else ("cross_entropy",)))
    _check_seg_args(seg2, seg_target, class_weights)
    _require_gpu(seg1, disp, seg2, seg_target, disp_target, seg3)
    cw = seg_class_weights(class_weights, seg2.shape[1], seg2.device)
    return _TrainLossFn.apply(seg1, disp, seg2, seg_target, disp_target, use_lovasz, mask_invalid_disp, ignore_void, seg3, plan, cw)


def _image_strides(left):
    """(batch, channel, pixel) strides of a (B,>=3,H,W) image whose rows follow one another pixel by pixel (NCHW, channels-last
    or a channel slice of either), or None."""
    B, C, H, W = left.shape
    sb, sc, sh, sw = left.stride()
    if W == 1:
        sw = sh
    if min(sb, sc, sw) < 1 or (H > 1 and sh != W * sw):
        return None
    return sb, sc, sw


def _strided_image(img):
    """(img, its (batch, channel, pixel) strides); a layout _image_strides does not serve is copied to NCHW first."""
    strides = _image_strides(img)
    if strides is None:
        img = img.contiguous()
        strides = _image_strides(img)
    return img, strides


def _disp_smooth_term(disp, loss, left, seg_t, weight):
    """loss += weight * smoothing_gradients (util/utilTorchLoss.py:41-101) on one disparity map; returns the gradient w.r.t.
    disp: value and gradient in one stencil pass."""
    B, _, H, W = disp.shape
    C = seg_t.shape[1]
    left, strides = _strided_image(left)
    tv, ldt = nhwc_view(seg_t)
    dv = _dense_disp(disp)
    ws = _loss_workspace("disp_smooth", (B, H, W), _lib.disp_smooth_workspace_bytes(B, H, W), disp.device)
    g = torch.empty((B, 1, H, W), dtype=dv.dtype, device=dv.device)
    call("sdhip_disp_smooth", ptr(left), strides[0], strides[1], strides[2], ptr(tv), ldt, ptr(dv), dtype_code(dv), ptr(g),
         ptr(loss), B, H, W, C, weight, ptr(ws), ws.numel(), stream_ptr())
    return g


def disp_smooth_loss(left, disp_pred, seg_target, weight=1.0):
    """The reference's smoothing_gradients(left, disp_pred, seg_target) (util/utilTorchLoss.py:41-101; `smooth_grad` of
    lossDisp_fn, losses/multiLosses.py:143-146) times `weight`: an edge-aware smoothness penalty on the predicted disparity
    that acts where a pixel's whole 3x3 neighbourhood has the pixel's own class, weighted by exp(1 - |grad of the smoothed
    luma|) of the left image (include/sdhip.h has the closed form).  weight = 1 is the reference's value, its 0.7 inside.
      left       — (B,>=3,H,W) f32 image (channels 0..2 are read); NCHW or channels-last, no copy is made of either
      disp_pred  — (B,1,H,W) f32 or bf16; the only input that gets a gradient (in its dtype)
      seg_target — one-hot f32 (B,C,H,W), C <= 32; an all-zero row has no class and gets no term.  Upstream passes the full
                   one-hot including the void channel, so void regions smooth as a class of their own; a caller who dropped
                   that channel gets no term there.
    Returns an f32 scalar; value and gradient are reproducible bit for bit."""
    if left.dim() != 4 or disp_pred.dim() != 4 or seg_target.dim() != 4:
        raise _lib.SdhipError("disp_smooth_loss: image, disparity and target must be 4-D (B,C,H,W), got %s, %s and %s"
                              % (tuple(left.shape), tuple(disp_pred.shape), tuple(seg_target.shape)))
    B, C1, H, W = disp_pred.shape
    if C1 != 1 or left.shape[1] < 3 or (left.shape[0],) + tuple(left.shape[2:]) != (B, H, W) or \
            (seg_target.shape[0],) + tuple(seg_target.shape[2:]) != (B, H, W):
        raise _lib.SdhipError("disp_smooth_loss: need a (B,>=3,H,W) image, a (B,1,H,W) disparity and a (B,C,H,W) target, got %s, %s "
                              "and %s" % (tuple(left.shape), tuple(disp_pred.shape), tuple(seg_target.shape)))
    if min(B, H, W) < 1 or not 1 <= seg_target.shape[1] <= SEG_MAX_CLASSES:
        raise _lib.SdhipError("disp_smooth_loss: empty tensor, or a target of %d channels (1 to %d are served)"
                              % (seg_target.shape[1], SEG_MAX_CLASSES))
    _require_gpu(left, disp_pred, seg_target)
    if not left.device == disp_pred.device == seg_target.device:
        raise _lib.SdhipError("disp_smooth_loss: image, disparity and target live on different devices")
    if left.dtype != torch.float32:
        raise _lib.SdhipError("disp_smooth_loss: the image must be f32, the input a step is fed (got %s)" % left.dtype)
    if seg_target.dtype != torch.float32:
        raise _lib.SdhipError("disp_smooth_loss: the one-hot segmentation target must be f32 (got %s)" % seg_target.dtype)
    dtype_code(disp_pred)
    return _ValueGradFn.apply(disp_pred, _disp_smooth_term, left, seg_target, float(weight))


# ============================================================================ Ext_small edge networks (csrc/edge.hip)
def grad_mag(img, dtype=None):
    """The edge map the reference harness feeds the `edgeOut` networks, utilTorchGate.compute_grad_mag(img, True, False)
    (torch_implementation.py:136) as upstream computes it (include/sdhip.h has the closed form): per channel
    sqrt(Ox^2 + Oy^2 + 1e-6) of the central differences with zero padding.  img: (B, C <= 4, H >= 2, W >= 2) f32 or bf16, NCHW,
    channels-last or a channel slice of either (no copy is made); the result, `dtype` (default: img's), lives in NHWC memory at
    the padded pixel stride the conv nodes read.  One launch, f32 arithmetic, no gradient: an image never requires one."""
    if img.dim() != 4:
        raise _lib.SdhipError("grad_mag: the image must be 4-D (B,C,H,W), got %s" % (tuple(img.shape),))
    B, C, H, W = img.shape
    if B < 1 or not 1 <= C <= 4 or H < 2 or W < 2:
        raise _lib.SdhipError("grad_mag: need B >= 1, 1 <= C <= 4 and H, W >= 2, got %s" % (tuple(img.shape),))
    _require_gpu(img)
    dt_in = dtype_code(img)
    dtype = img.dtype if dtype is None else dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise _lib.SdhipError("grad_mag: output dtype %s (f32 and bf16 only)" % dtype)
    if img.requires_grad:
        raise _lib.SdhipError("grad_mag has no backward pass: the image must not require a gradient")
    img, strides = _strided_image(img)
    out, ldy = alloc_nhwc(B, C, H, W, dtype, img.device)
    call("sdhip_grad_mag", ptr(img), strides[0], strides[1], strides[2], dt_in, ptr(out), ldy, _lib.code_of(dtype), B, H, W, C, stream_ptr())
    return out


def _check_edge_args(edge_logits, edges):
    if edge_logits.dim() != 4 or edge_logits.shape[1] != 1 or tuple(edges.shape) != tuple(edge_logits.shape):
        raise _lib.SdhipError("edge logits and edge target must both be (B,1,H,W), got %s and %s"
                              % (tuple(edge_logits.shape), tuple(edges.shape)))
    if edge_logits.numel() < 1:
        raise _lib.SdhipError("edge loss of an empty tensor")
    if edges.dtype != torch.float32:
        raise _lib.SdhipError("the edge target must be f32 (got %s)" % edges.dtype)
    if not edges.is_contiguous():
        raise _lib.SdhipError("the edge target must be a dense (B,1,H,W) tensor")
    dtype_code(edge_logits)


def _edge_term(z, loss, edges):
    """loss += lossEdge_fn(edges, z) (losses/multiLosses.py:166-182); returns the gradient w.r.t. z (dense, z's dtype): the
    three launches of sdhip_edge_bce."""
    n = z.numel()
    zv, ldz = nhwc_view(z)
    ws = _loss_workspace("edge", (n,), _lib.edge_bce_workspace_bytes(n), z.device)
    g = torch.empty(tuple(z.shape), dtype=z.dtype, device=z.device)
    call("sdhip_edge_bce", ptr(zv), ldz, dtype_code(zv), ptr(edges), ptr(g), ptr(loss), n, ptr(ws), ws.numel(), stream_ptr())
    return g


def edge_loss(edge_logits, edges):
    """The reference's lossEdge_fn(edges, edge_logits): mean(w * BCEWithLogits(edge_logits, edges)) with the class-balancing
    weight w = N/(P+N) on the pixels where edges == 1, P/(P+N) where edges == 0 and 0 on any other value, P and N the counts of
    ones and zeros over the whole batch.  No positives or no negatives: value and gradient are exactly 0.
      edge_logits — (B,1,H,W) f32 or bf16, dense or a 1-channel map inside a padded pixel stride (a head's output); the only
                    input that gets a gradient (dense, in its dtype)
      edges       — dense f32 (B,1,H,W)
    Returns an f32 scalar; value and gradient are reproducible bit for bit."""
    _check_edge_args(edge_logits, edges)
    _require_gpu(edge_logits, edges)
    return _ValueGradFn.apply(edge_logits, _edge_term, edges)


class _EdgeStepLossFn(torch.autograd.Function):
    """total = CE(seg) + L1(disp) [+ lossEdge_fn(edges, edge logits)] — the loss of the reference's step for the `edgeOut`
    networks (torch_implementation.py:170-171,279,304,320-325: one cross-entropy, `CFG.loss` is not consulted).  The gradients
    w.r.t. the network outputs are produced in the same pass, as in _TrainLossFn."""

    @staticmethod
    def forward(ctx, edge_logits, disp, seg, seg_t, disp_t, edges, mask_invalid_disp, cw):
        B, C, H, W = seg.shape
        npix = B * H * W
        dt = dtype_code(seg)
        loss = torch.zeros(1, dtype=torch.float64, device=seg.device)
        tv, ldt = nhwc_view(seg_t)
        sv, ld = nhwc_view(seg)
        gs = empty_nhwc(B, C, H, W, seg.dtype, seg.device)
        if cw is None:
            call("sdhip_ce_loss", ptr(sv), ld, ptr(tv), ldt, ptr(gs), C, ptr(loss), npix, C, 1.0, dt, stream_ptr())
        else:
            _seg_terms(seg, tv, ldt, gs, loss, 1.0, 0, cw)
        dv = _dense_disp(disp)
        gd = torch.empty_like(dv)
        call("sdhip_l1_loss", ptr(dv), ptr(disp_t), ptr(gd), ptr(loss), npix, 1.0, int(mask_invalid_disp), dt, stream_ptr())
        ge = _edge_term(edge_logits, loss, edges) if edges is not None else None
        ctx.save_for_backward(ge, gd, gs)
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        ge, gd, gs = ctx.saved_tensors
        return ge, gd, gs, None, None, None, None, None      # d(total)/d(total) is 1 in the training step


def edge_step_loss(edge_logits, disp, seg_logits, seg_target, disp_target, edges=None, mask_invalid_disp=False, class_weights=None):
    """The loss of the reference step on the outputs `edge_ds, disp1, seg1, _` of an `edgeOut` network (Ext_small, Ext_smallv2):
    cross-entropy of the ONE segmentation head + L1 of the disparity + lossEdge_fn(edges, edge_logits) as one node.
      edges             — dense f32 (B,1,H,W) edge target, or None: the edge term is left out and the edge head gets no gradient
      mask_invalid_disp — disparities <= 0 are invalid (train_loss)
      class_weights     — the `-segWeight 1` table (length C) on the cross-entropy
    Returns an f32 tensor of one element."""
    _check_seg_args(seg_logits, seg_target, class_weights)
    if tuple(disp.shape) != (seg_logits.shape[0], 1) + tuple(seg_logits.shape[2:]) or tuple(disp_target.shape) != tuple(disp.shape):
        raise _lib.SdhipError("disparity and its target must be (B,1,H,W) of the segmentation's size, got %s and %s"
                              % (tuple(disp.shape), tuple(disp_target.shape)))
    if not disp_target.is_contiguous():
        raise _lib.SdhipError("disparity target must be a dense (B,1,H,W) tensor")
    if edges is not None:
        _check_edge_args(edge_logits, edges)
        if tuple(edges.shape) != tuple(disp.shape):
            raise _lib.SdhipError("the edge target %s does not match the outputs %s" % (tuple(edges.shape), tuple(disp.shape)))
    _require_gpu(edge_logits, disp, seg_logits, seg_target, disp_target, edges)
    cw = seg_class_weights(class_weights, seg_logits.shape[1], seg_logits.device)
    return _EdgeStepLossFn.apply(edge_logits, disp, seg_logits, seg_target, disp_target, edges, bool(mask_invalid_disp), cw)


def gate_pair(a, b, g):
    """torch.cat((a * g, b * (1 - g)), 1) for a, b (B,C,H,W) and a one-channel gate g (B,1,H,W), all of one dtype (f32 / bf16):
    the `s2_d*s2_at | s2_s*(1-s2_at)` line of the Ext_small networks (models/dsnet_t2_ext_small.py:361) as one launch that writes
    both halves into one 2C-channel NHWC buffer, and one backward launch for all three gradients."""
    _check_gate_args("gate_pair", a, b, g)
    return _GateFn.apply(a, b, g, True)


# ============================================================================ dropout / global average pool
_rng = {"seed": None, "layers": 0}


_RNG_BASE, _RNG_RANK_STRIDE = 0x5DEECE66D, 0x9E3779B97F4A7C15 >> 1


def rng_seed_tensor(device):
    """Device-resident dropout seed.  train.TrainStep advances it once per step with a device-side add (captured into the
    step's hipGraph, so replays draw new masks); forward and backward of one step read the same value."""
    c = _ctx[0]
    if c is not None and c.seed is not None:                  # a TrainStep's own stream (steps must not reset each other)
        return c.seed
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:       # "cuda" and "cuda:0" must name the same tensor: a captured step
        device = torch.device("cuda", torch.cuda.current_device())   # keeps adding to the one it was recorded with
    if _rng["seed"] is None or _rng["seed"].device != device:
        _rng["seed"] = torch.full((1,), _RNG_BASE, dtype=torch.int64, device=device)
    return _rng["seed"]


def rng_seed_value(rank=0, base=_RNG_BASE):
    return (base + rank * _RNG_RANK_STRIDE) & 0x7FFFFFFFFFFFFFFF


def rng_reseed(device, rank=0, base=_RNG_BASE):
    """Restart the dropout stream (the module-level one, or the installed TrainStep's); ranks of a data-parallel job get
    disjoint streams (in place: a captured graph keeps reading the same tensor)."""
    rng_seed_tensor(device).fill_(rng_seed_value(rank, base))


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, layer_id):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ld = nhwc_view(x)
        if ld != C:
            xv = xv.contiguous(memory_format=torch.channels_last)
        y = empty_nhwc(B, C, H, W, x.dtype, x.device)
        seed = rng_seed_tensor(x.device)
        call("sdhip_dropout", ptr(xv), ptr(y), ptr(seed), layer_id, x.numel(), p, dtype_code(x), stream_ptr())
        ctx.cfg = (p, layer_id)
        return y

    @staticmethod
    def backward(ctx, gy):
        p, layer_id = ctx.cfg
        B, C, H, W = gy.shape
        g, ld = nhwc_view(gy)
        if ld != C:
            g = g.contiguous(memory_format=torch.channels_last)
        gx = empty_nhwc(B, C, H, W, gy.dtype, gy.device)
        call("sdhip_dropout", ptr(g), ptr(gx), ptr(rng_seed_tensor(gy.device)), layer_id, gy.numel(), p, dtype_code(gy), stream_ptr())
        return gx, None, None


def dropout(x, p, training, layer_id):
    if not training or p == 0.0:
        return x
    return _DropoutFn.apply(x, float(p), int(layer_id))


# ============================================================================ HANet pieces (models_hanet/HANet.py:74-128)
class _RowPoolMaxFn(torch.autograd.Function):
    """nn.AdaptiveMaxPool2d((OH, 1)): (B,C,H,W) -> (B,C,OH,1)."""

    @staticmethod
    def forward(ctx, x, OH):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ldx = nhwc_view(x)
        y, ldy = alloc_nhwc(B, C, OH, 1, x.dtype, x.device)
        idx = torch.empty((B, OH, C), dtype=torch.int32, device=x.device)
        call("sdhip_rowpool_max_fwd", ptr(xv), ldx, ptr(y), ldy, ptr(idx), B, H, W, C, OH, dtype_code(x), stream_ptr())
        ctx.save_for_backward(idx)
        ctx.cfg = (B, C, H, W, OH)
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        B, C, H, W, OH = ctx.cfg
        g, ldg = nhwc_view(gy)
        gx, ldgx = alloc_nhwc(B, C, H, W, gy.dtype, gy.device)
        call("sdhip_rowpool_max_bwd", ptr(g), ldg, ptr(idx), ptr(gx), ldgx, B, H, W, C, OH, dtype_code(gy), stream_ptr())
        return gx, None


def rowpool_max(x, OH):
    return _RowPoolMaxFn.apply(x, int(OH))


class _MulRowsFn(torch.autograd.Function):
    """a (B,C,H,W) * att (B,C,H,1): torch.mul(out, x1d.unsqueeze(3)) of models_hanet/HANet.py:112."""

    @staticmethod
    def forward(ctx, a, att):
        _require_gpu(a, att)
        B, C, H, W = a.shape
        if tuple(att.shape) != (B, C, H, 1):
            raise _lib.SdhipError("mul_rows: attention must be (B,C,H,1), got %s for %s" % (tuple(att.shape), tuple(a.shape)))
        av, lda = nhwc_view(a)
        tv, ldt = nhwc_view(att)
        y, ldy = alloc_nhwc(B, C, H, W, a.dtype, a.device)
        call("sdhip_mul_rows_fwd", ptr(av), lda, ptr(tv), ldt, ptr(y), ldy, B, H, W, C, dtype_code(a), stream_ptr())
        ctx.save_for_backward(av, tv)
        ctx.cfg = (lda, ldt)
        return y

    @staticmethod
    def backward(ctx, g):
        av, tv = ctx.saved_tensors
        lda, ldt = ctx.cfg
        B, C, H, W = av.shape
        gv, ldg = nhwc_view(g)
        ga, ldga = alloc_nhwc(B, C, H, W, av.dtype, av.device)
        gt, ldgt = alloc_nhwc(B, C, H, 1, av.dtype, av.device)
        call("sdhip_mul_rows_bwd", ptr(gv), ldg, ptr(av), lda, ptr(tv), ldt, ptr(ga), ldga, ptr(gt), ldgt, B, H, W, C,
             dtype_code(av), stream_ptr())
        return ga, gt


def mul_rows(a, att):
    return _MulRowsFn.apply(a, att)


class _DropoutChannelsFn(torch.autograd.Function):
    """nn.Dropout2d on a (B,C,L[,1]) row descriptor: whole (sample, channel) rows are dropped."""

    @staticmethod
    def forward(ctx, x, p, layer_id):
        _require_gpu(x)
        B, C, L, W = x.shape
        xv, ldx = nhwc_view(x)
        y, ldy = alloc_nhwc(B, C, L, W, x.dtype, x.device)
        call("sdhip_dropout_channels", ptr(xv), ldx, ptr(y), ldy, ptr(rng_seed_tensor(x.device)), layer_id, B, L * W, C, p,
             dtype_code(x), stream_ptr())
        ctx.cfg = (p, layer_id)
        return y

    @staticmethod
    def backward(ctx, gy):
        p, layer_id = ctx.cfg
        B, C, L, W = gy.shape
        g, ldg = nhwc_view(gy)
        gx, ldgx = alloc_nhwc(B, C, L, W, gy.dtype, gy.device)
        call("sdhip_dropout_channels", ptr(g), ldg, ptr(gx), ldgx, ptr(rng_seed_tensor(gy.device)), layer_id, B, L * W, C, p,
             dtype_code(gy), stream_ptr())
        return gx, None, None


def dropout_channels(x, p, training, layer_id):
    if not training or p == 0.0:
        return x
    return _DropoutChannelsFn.apply(x, float(p), int(layer_id))


def global_avg_pool(x):
    """nn.AdaptiveAvgPool2d((1,1)): gcd(H,W)-sized square average pools (equal windows, so the mean of the window means is
    the global mean), then the mean of the few remaining cells (a (B,C,h,w) tensor with h*w tiny)."""
    import math
    B, C, H, W = x.shape
    k = math.gcd(H, W)
    y = avgpool(x, k) if k > 1 else x
    return y.mean((2, 3), keepdim=True) if y.shape[2] * y.shape[3] > 1 else y


# ============================================================================ 3-D convolutions and PSMNet ops
def conv3d_spec(x, D, weight, stride=1, padding=1):
    """nn.Conv3d(k, stride, padding) over a volume held as (B*D, C, H, W) NHWC images."""
    Bimg, C, H, W = x.shape
    kd, kh, kw = weight.shape[2:]
    Do = (D + 2 * padding - kd) // stride + 1
    Ho = (H + 2 * padding - kh) // stride + 1
    Wo = (W + 2 * padding - kw) // stride + 1
    return ConvSpec('conv', kh, kw, stride, 1, padding, padding, Ho, Wo, D, Do, kd, stride, padding)


def conv3d_bn_act(x, D, weight, bn, stride=1, padding=1, act=0, residual=None, groups=1, in_slot=None, res_slot=None):
    """in_slot / res_slot: see conv_bn_act (GradSlot)."""
    spec = conv3d_spec(x, D, weight, stride, padding)
    return _ConvBNActFn.apply(x, weight, bn.weight, bn.bias, residual, spec, bn, act, groups, in_slot, res_slot), spec.Do


def conv3d(x, D, weight, stride=1, padding=1):
    spec = conv3d_spec(x, D, weight, stride, padding)
    return _ConvFn.apply(x, weight, None, spec, 0), spec.Do


class _StuffFn(torch.autograd.Function):
    """Zero insertion: y[n, d*sd, h*s, w*s] = x[n,d,h,w] (extent (D-1)*sd+1 ...); backward is the strided gather."""

    @staticmethod
    def forward(ctx, x, D, sd, s):
        _require_gpu(x)
        Bimg, C, H, W = x.shape
        B = Bimg // D
        xv, ld = nhwc_view(x)
        Ds, Hs, Ws = (D - 1) * sd + 1, (H - 1) * s + 1, (W - 1) * s + 1
        y = empty_nhwc(B * Ds, C, Hs, Ws, x.dtype, x.device)
        call("sdhip_stuff", ptr(xv), ld, ptr(y), C, B, D, H, W, C, sd, s, 1, dtype_code(x), stream_ptr())
        ctx.cfg = (B, D, H, W, C, sd, s)
        return y

    @staticmethod
    def backward(ctx, gy):
        B, D, H, W, C, sd, s = ctx.cfg
        g, ld = nhwc_view(gy)
        gx = empty_nhwc(B * D, C, H, W, gy.dtype, gy.device)
        call("sdhip_stuff", ptr(g), ld, ptr(gx), C, B, D, H, W, C, sd, s, 0, dtype_code(gy), stream_ptr())
        return gx, None, None, None


# Sub-pixel decomposition of ConvTranspose3d(k=3, s=2, p=1, output_padding=1): per axis, output 2m takes input m with tap 1;
# output 2m+1 takes inputs m, m+1 with taps 2, 0.  Phase (pd, ph, pw) is a stride-1 correlation with a (1+pd)x(1+ph)x(1+pw)
# sub-kernel; the 27 taps, ordered phase by phase (input offset major), index the flat 3x3x3 kernel as follows.
_PHASE_TAPS = ([1], [2, 0])
_PHASES = [(pd, ph, pw) for pd in (0, 1) for ph in (0, 1) for pw in (0, 1)]
_PHASE_INDEX = [a * 9 + b * 3 + c for (pd, ph, pw) in _PHASES for a in _PHASE_TAPS[pd] for b in _PHASE_TAPS[ph] for c in _PHASE_TAPS[pw]]
_phase_index_dev = {}


def _phase_rows(weight, dt):
    """Single-tap pack rows (src element offset, dst element offset, M, K, 1, stride_m, stride_k, 0) that build the eight packed
    sub-kernels of a (Cin, Cout, 3, 3, 3) transposed-convolution weight straight from the parameter, one buffer behind the
    other, and [(element offset, elements)] of the eight sub-kernels.  Needs one channel chunk (Cin <= 64 bf16 / 32 f32): a
    tap's [Mpad][CK] block is then contiguous in the packed [kd][q][t][m][c] layout."""
    Cin, Cout = weight.shape[0], weight.shape[1]
    rows, spans, base = [], [], 0
    for (pd, ph, pw) in _PHASES:
        nd, T = 1 + pd, (1 + ph) * (1 + pw)
        per = _lib.packed_elems(Cout, Cin, T, dt)
        blk = per // T                                   # one tap's [Mpad][CK] block (single channel chunk)
        for kdi, a in enumerate(_PHASE_TAPS[pd]):
            t = 0
            for b_ in _PHASE_TAPS[ph]:
                for c_ in _PHASE_TAPS[pw]:
                    rows.append((a * 9 + b_ * 3 + c_, base + kdi * per + t * blk, Cout, Cin, 1, 27, Cout * 27, 0))
                    t += 1
        spans.append((base, per * nd))
        base += per * nd
    return rows, spans


def _phase_packs(weight, dtype):
    """The eight packed sub-kernels of a (Cin, Cout, 3, 3, 3) ConvTranspose3d weight (equally: of a stride-2 Conv3d weight
    (Cout', Cin', 3, 3, 3) read as its adjoint), taps ordered phase by phase, input offset major.  One channel chunk: cached
    per parameter like ops.packed_weight and, inside a training step, packed by the step's ONE batched launch (27 single-tap
    rows per weight in the descriptor table).  Wider weights: a gather reorders the taps into a (Cout, Cin, 27) buffer, from
    which every (phase, depth tap) is packed with its own strides."""
    Cin, Cout = weight.shape[0], weight.shape[1]
    dev = weight.device
    dt = _lib.code_of(dtype)
    if Cin <= (64 if dtype == torch.bfloat16 else 32) and weight.is_contiguous():
        ent = _cache_entry(weight)
        key = ('phase', 'fwd', dtype)
        hit = ent.get(key)
        c = _ctx[0]
        rows, spans = _phase_rows(weight, dt)
        ver = (weight._version, _pack_generation[0])
        fresh = hit is not None and ((c is not None and c.frozen_pack) or (hit[0] == ver and not torch.cuda.is_current_stream_capturing()))
        if fresh:
            buf = hit[1]
        else:
            buf = torch.empty(spans[-1][0] + spans[-1][1], dtype=dtype, device=dev)
            es = buf.element_size()
            w = weight.detach()
            for src_off, dst_off, M, K, T, sm, sk, flip in rows:
                call("sdhip_conv_pack_weights", ctypes_ptr(w.data_ptr() + 4 * src_off), ctypes_ptr(buf.data_ptr() + es * dst_off),
                     M, K, T, sm, sk, flip, dt, stream_ptr())
            ent[key] = (ver, buf)
        return [buf[o:o + n] for o, n in spans], buf
    idx = _phase_index_dev.get(str(dev))
    if idx is None:
        idx = _phase_index_dev[str(dev)] = torch.tensor(_PHASE_INDEX, dtype=torch.int64, device=dev)
    wre = weight.detach().reshape(Cin, Cout, 27).index_select(2, idx).transpose(0, 1).contiguous()      # (Cout, Cin, 27)
    packs, off = [], 0
    for (pd, ph, pw) in _PHASES:
        nd, T = 1 + pd, (1 + ph) * (1 + pw)
        per = _lib.packed_elems(Cout, Cin, T, dt)
        buf = torch.empty(per * nd, dtype=dtype, device=dev)
        es = buf.element_size()
        for kdi in range(nd):
            call("sdhip_conv_pack_weights", ctypes_ptr(wre.data_ptr() + 4 * (off + kdi * T)), ctypes_ptr(buf.data_ptr() + es * per * kdi),
                 Cout, Cin, T, Cin * 27, 27, 0, dt, stream_ptr())
        packs.append(buf)
        off += nd * T
    return packs, wre


class _Deconv3dS2BNActFn(torch.autograd.Function):
    """y = act(BatchNorm3d(ConvTranspose3d(k=3, s=2, p=1, op=1)(x))) (+ residual), models_psmnet/stackhourglass.py:25-29,42-48.
    Forward: eight sub-pixel phases over the un-stuffed volume (27 taps per input voxel, not 8 x 27 over a zero-stuffed
    one), their statistics summed by the conv epilogues.  Backward: the adjoint of a transposed convolution is the
    stride-2 convolution with the same weight, so the data gradient is a strided forward convolution of dy and the weight
    gradient the strided weight-gradient kernel with the roles of x and dy exchanged — no stuffing either."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, residual, D, bn, act, groups):
        _require_gpu(x, weight)
        Bimg, Cin, H, W = x.shape
        Btrue = Bimg // D
        Cout = weight.shape[1]
        xv, ldx = aligned_view(x)
        Bo = Btrue * 2 * D
        yraw, ldr_ = alloc_nhwc(Bo, Cout, 2 * H, 2 * W, x.dtype, x.device)
        train = bn.training
        ws = _zeros((NREP, groups, 2, Cout), torch.float64, x.device)[0] if train else None
        packs, keep = _phase_packs(weight, x.dtype)
        for (pd, ph, pw), wp in zip(_PHASES, packs):
            call("sdhip_conv2d_fwd_phase", ptr(xv), ptr(wp), ptr(yraw), ptr(ws), ws.stride(-2) if ws is not None else 0, NREP if ws is not None else 1,
                 Btrue, H, W, Cin, ldx, Cout, ldr_, 1 + ph, 1 + pw, D, 1 + pd, groups, pd, ph, pw, dtype_code(x), stream_ptr())
        count = (Bo // groups) * 4 * H * W
        y, scale, shift, mean, invstd = _bn_act_forward(yraw, ldr_, bn, ws, count, groups, act, residual)
        ctx.cfg = (D, act, groups, ldx, ldr_, count, train, residual is not None)
        ctx.save_for_backward(xv, weight, gamma, beta, yraw, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, gamma, beta, yraw, scale, shift, mean, invstd = ctx.saved_tensors
        D, act, groups, ldx, ldraw, count, train, has_res = ctx.cfg
        Bimg, Cin, H, W = xv.shape
        Btrue = Bimg // D
        Cout = yraw.shape[1]
        Ho, Wo = 2 * H, 2 * W
        g, ldg = nhwc_view(gy)
        graw, ldgr, dgamma, dbeta = _bn_act_backward(g, ldg, yraw, ldraw, scale, shift, mean, invstd, gamma, beta, groups, act,
                                                     count, train)
        # adjoint of the transposed convolution: Conv3d(weight viewed as (out = Cin, in = Cout), stride 2, padding 1) of graw
        spec = ConvSpec('conv', 3, 3, 2, 1, 1, 1, H, W, 2 * D, D, 3, 2, 1)
        gx = None
        if ctx.needs_input_grad[0]:
            gx, ldgx = alloc_nhwc(Bimg, Cin, H, W, xv.dtype, xv.device)
            _conv_launch(graw, ldgr, packed_weight(weight, 'conv', 'fwd', xv.dtype), gx, ldgx, None, None, None, None, Btrue, Ho, Wo, Cout,
                         H, W, Cin, 3, 3, 2, 1, 1, 1, False, 1, 0, False, 1, spec.depth())
        gw = None
        if ctx.needs_input_grad[1]:
            gw, _ = wgrad(graw, ldgr, xv, ldx, weight, None, spec)       # "input" = dy, "output gradient" = x: same (Cin, Cout, 3,3,3) layout
        return gx, gw, dgamma, dbeta, (gy if has_res else None), None, None, None, None


def deconv3d_s2_bn_act(x, D, weight, bn, act=0, residual=None, groups=1):
    """nn.ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1) + BatchNorm3d (models_psmnet/stackhourglass.py:25-29):
    output extent exactly 2x; sub-pixel phases forward, strided convolution kernels backward (_Deconv3dS2BNActFn)."""
    return _Deconv3dS2BNActFn.apply(x, weight, bn.weight, bn.bias, residual, D, bn, act, groups), 2 * D


class _CostVolumeFn(torch.autograd.Function):
    """Concatenation cost volume of PSMNet (models_psmnet/stackhourglass.py:110-119) as (B*D, 2C, H, W) images."""

    @staticmethod
    def forward(ctx, left, right, D):
        _require_gpu(left, right)
        B, C, H, W = left.shape
        lv, ldl = nhwc_view(left)
        rv, ldr = nhwc_view(right)
        if ldl != ldr:
            lv = lv.contiguous(memory_format=torch.channels_last); rv = rv.contiguous(memory_format=torch.channels_last)
            ldl = C
        vol = empty_nhwc(B * D, 2 * C, H, W, left.dtype, left.device)
        call("sdhip_cost_volume_fwd", ptr(lv), ptr(rv), ldl, ptr(vol), B, D, H, W, C, dtype_code(left), stream_ptr())
        ctx.cfg = (B, C, H, W, D)
        return vol

    @staticmethod
    def backward(ctx, g):
        B, C, H, W, D = ctx.cfg
        gv, ld = nhwc_view(g)
        if ld != 2 * C:
            gv = gv.contiguous(memory_format=torch.channels_last)
        gl = empty_nhwc(B, C, H, W, g.dtype, g.device)
        gr = empty_nhwc(B, C, H, W, g.dtype, g.device)
        call("sdhip_cost_volume_bwd", ptr(gv), ptr(gl), ptr(gr), C, B, D, H, W, C, dtype_code(g), stream_ptr())
        return gl, gr, None


def cost_volume(left, right, D):
    return _CostVolumeFn.apply(left, right, D)


class _SoftArgminFn(torch.autograd.Function):
    """trilinear upsample -> softmax over disparity -> expectation (stackhourglass.py:138-155, submodule.py:56-64)."""

    @staticmethod
    def forward(ctx, cost, D4, maxdisp, H, W):
        _require_gpu(cost)
        Bimg, C, H4, W4 = cost.shape
        if C != 1:
            raise _lib.SdhipError("soft-argmin expects a 1-channel cost volume")
        B = Bimg // D4
        c = cost.contiguous()
        pred = torch.empty((B, H, W), dtype=cost.dtype, device=cost.device)
        # (log-sum-exp, pred) per pixel: the backward pass starts from them instead of repeating the two softmax passes
        stats = torch.empty((B * H * W, 2), dtype=torch.float32, device=cost.device) if (maxdisp == 4 * D4 and ctx.needs_input_grad[0]) else None
        call("sdhip_softargmin_fwd", ptr(c), ptr(pred), ptr(stats), B, D4, H4, W4, maxdisp, H, W, dtype_code(cost), stream_ptr())
        ctx.save_for_backward(c, stats)
        ctx.cfg = (B, D4, H4, W4, maxdisp, H, W)
        return pred

    @staticmethod
    def backward(ctx, g):
        c, stats = ctx.saved_tensors
        B, D4, H4, W4, maxdisp, H, W = ctx.cfg
        gc = torch.empty_like(c)
        nws = _lib._lib.sdhip_softargmin_bwd_workspace_floats(B, D4, H4, W4, maxdisp, H, W)
        tmp = torch.empty(nws, dtype=torch.float32, device=c.device)
        call("sdhip_softargmin_bwd", ptr(c), ptr(g.contiguous()), ptr(stats), ptr(gc), ptr(tmp), nws, B, D4, H4, W4, maxdisp, H, W,
             dtype_code(c), stream_ptr())
        return gc, None, None, None, None


def soft_argmin(cost, D4, maxdisp, H, W):
    return _SoftArgminFn.apply(cost, D4, maxdisp, H, W)


def relu(x):
    return affine_act(x, None, None, None, 1)


def add(x, y):
    return affine_act(x, None, None, y, 0)


class _MeanL1Fn(torch.autograd.Function):
    """mean over the predictions of mean |pred - target| — the (build-defined) PSMNet training loss: the reference has no
    PSMNet training harness; value and gradients in one pass per prediction."""

    @staticmethod
    def forward(ctx, target, *preds):
        _require_gpu(target, *preds)
        loss = torch.zeros(1, dtype=torch.float64, device=target.device)
        t = target.contiguous().float()
        grads = []
        for p in preds:
            pv = p.contiguous()
            g = torch.empty_like(pv)
            call("sdhip_l1_loss", ptr(pv), ptr(t), ptr(g), ptr(loss), pv.numel(), 1.0 / len(preds), 0, dtype_code(pv), stream_ptr())
            grads.append(g)
        ctx.save_for_backward(*grads)
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        return (None,) + tuple(ctx.saved_tensors)


def mean_l1_loss(preds, target):
    return _MeanL1Fn.apply(target, *preds)


# ============================================================================ dsnet extras
class _LogSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        B, C, H, W = x.shape
        xv, ld = nhwc_view(x)
        y = empty_nhwc(B, C, H, W, x.dtype, x.device)
        call("sdhip_log_softmax_fwd", ptr(xv), ld, ptr(y), C, B * H * W, C, dtype_code(x), stream_ptr())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        B, C, H, W = y.shape
        g, ld = nhwc_view(gy)
        gx = empty_nhwc(B, C, H, W, y.dtype, y.device)
        call("sdhip_log_softmax_bwd", ptr(g), ld, ptr(y), C, ptr(gx), C, B * H * W, C, dtype_code(y), stream_ptr())
        return gx


def log_softmax(x):
    return _LogSoftmaxFn.apply(x)


_consts = {}


def _const_vec(v, n, device):
    key = (float(v), n, str(device))
    if key not in _consts:
        _consts[key] = torch.full((1, n), float(v), dtype=torch.float32, device=device)
    return _consts[key]


def axpby(a, x, b, y):
    """a*x + b*y (the 0.9/0.1 and 0.8/0.2 head blends of models/dsnet_t2.py:272,308)."""
    C = x.shape[1]
    t = affine_act(y, _const_vec(b, C, x.device), None, None, 0)
    return affine_act(x, _const_vec(a, C, x.device), None, t, 0)


def deconv_same_strided_spec(x, weight, stride):
    """ConvTranspose2dSame with stride > 1 (models/torch_model.py:320-346): full transposed conv of extent (H-1)*s+k,
    cropped from start = full//2 - (s*H)//2 to s*H.  Run as a stride-1 correlation with flipped taps over the
    zero-stuffed input: top/left padding (k-1) - start."""
    B, C, H, W = x.shape
    k = weight.shape[2]

    def one(size):
        full, target = (size - 1) * stride + k, size * stride
        h, oh = full // 2, target // 2
        start = h - (oh if h - oh >= 0 else h)
        return (k - 1) - start, target
    pt, Ho = one(H)
    pl, Wo = one(W)
    return ConvSpec('deconv', k, k, 1, 1, pt, pl, Ho, Wo)


def deconv2d_strided(x, weight, bias, stride, bn=None, act=0, residual=None, groups=1):
    xs = _StuffFn.apply(x, 1, 1, stride)
    spec = deconv_same_strided_spec(x, weight, stride)
    if bn is None:
        return _ConvFn.apply(xs, weight, bias, spec, act)
    return _ConvBNActFn.apply(xs, weight, bn.weight, bn.bias, residual, spec, bn, act, groups)


# ============================================================================ MobileNetV3: depthwise conv, squeeze-excite
ACT_HSWISH, ACT_HSIGMOID = _lib.ACT_HSWISH, _lib.ACT_HSIGMOID


def dw_out_size(n, k, stride):
    return (n + 2 * ((k - 1) // 2) - k) // stride + 1


class SESide:
    """What the depthwise node hands to the SELayer behind it: the per-image channel sums of the raw convolution output
    (its epilogue's average pool) and the BatchNorm's (scale, shift) — the pooled BatchNorm output is scale*mean + shift."""
    __slots__ = ("pool", "scale", "shift", "groups")

    def __init__(self):
        self.pool = self.scale = self.shift = None
        self.groups = 1


class _DWConvBNActFn(torch.autograd.Function):
    """y = act(BatchNorm(depthwise_conv(x))) as ONE autograd node (InvertedResidual, models/mobilenetv3.py:97-114):
    the depthwise kernel's epilogue sums the batch statistics (and, for an SELayer behind it, the per-image pool), one
    elementwise pass finalizes, normalises and activates.  The weight is the (C, 1, k, k) f32 parameter as stored."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn, k, stride, act, groups, side):
        _require_gpu(x, weight)
        if weight.dtype != torch.float32 or not weight.is_contiguous():
            raise _lib.SdhipError("depthwise weight must be a contiguous f32 (C, 1, k, k) tensor")
        B, C, H, W = x.shape
        Ho, Wo = dw_out_size(H, k, stride), dw_out_size(W, k, stride)
        xv, ldx = nhwc_view(x)
        dt = dtype_code(x)
        yraw, ldr = alloc_nhwc(B, C, Ho, Wo, x.dtype, x.device)
        train = bn.training
        ws = _zeros((NREP, groups, 2, C), torch.float64, x.device)[0] if train else None
        parts = _lib.dw_pool_parts(H, W, C, k, stride, dt) if side is not None else 0
        pool = _zeros((B, parts, C), torch.float32, x.device)[0] if side is not None else None   # per-workgroup slots
        call("sdhip_dw_conv_fwd", ptr(xv), ldx, ptr(weight.detach()), ptr(yraw), ldr, ptr(ws), C, NREP, ptr(pool), parts,
             B, H, W, C, k, stride, groups, dt, stream_ptr())
        count = (B // groups) * Ho * Wo
        y, scale, shift, mean, invstd = _bn_act_forward(yraw, ldr, bn, ws, count, groups, act)
        if side is not None:
            side.pool, side.scale, side.shift, side.groups = pool, scale, shift, groups
        ctx.cfg = (k, stride, act, groups, ldx, ldr, count, train)
        ctx.save_for_backward(xv, weight, gamma, beta, yraw, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, gamma, beta, yraw, scale, shift, mean, invstd = ctx.saved_tensors
        k, stride, act, groups, ldx, ldraw, count, train = ctx.cfg
        B, C, H, W = xv.shape
        dt = dtype_code(xv)
        g, ldg = nhwc_view(gy)
        graw, ldgr, dgamma, dbeta = _bn_act_backward(g, ldg, yraw, ldraw, scale, shift, mean, invstd, gamma, beta, groups, act,
                                                     count, train)
        gx = None
        if ctx.needs_input_grad[0]:
            gx, ldgx = alloc_nhwc(B, C, H, W, xv.dtype, xv.device)
            call("sdhip_dw_conv_dgrad", ptr(graw), ldgr, ptr(weight.detach()), ptr(gx), ldgx, B, H, W, C, k, stride, dt,
                 stream_ptr())
        gw = None
        if ctx.needs_input_grad[1]:
            tw = _grad_target(weight)
            target = tw if tw is not None else _zeros(tuple(weight.shape), torch.float32, weight.device)[0]
            nparts = _lib.dw_wgrad_parts(B, H, W, C, k, stride)
            part = torch.empty((nparts * k * k * C,), dtype=torch.float32, device=weight.device)   # every slot is written
            call("sdhip_dw_conv_wgrad", ptr(xv), ldx, ptr(graw), ldgr, ptr(target), ptr(part), nparts, B, H, W, C, k, stride, dt,
                 stream_ptr())
            gw = None if tw is not None else target
        return gx, gw, dgamma, dbeta, None, None, None, None, None, None


def dw_conv_bn_act(x, weight, bn, stride=1, act=0, groups=1, side=None):
    """act(bn(nn.Conv2d(C, C, k, stride, (k-1)//2, groups=C, bias=False)(x))); `side` (SESide) receives what an SELayer
    behind it needs."""
    k = weight.shape[-1]
    if weight.shape[1] != 1 or weight.shape[0] != x.shape[1] or weight.shape[-2] != k or k not in (3, 5) or stride not in (1, 2):
        raise _lib.SdhipError("depthwise convolution: (C, 1, k, k) weights with k 3 / 5 and stride 1 / 2 only")
    return _DWConvBNActFn.apply(x, weight, bn.weight, bn.bias, bn, k, stride, act, groups, side)


class _SEScaleActFn(torch.autograd.Function):
    """y = act(z * s[b, c]) with s = SELayer's excitation of z (models/mobilenetv3.py:64-77) — one launch for the pooled
    MLP (the pool comes from the depthwise epilogue, SESide), one elementwise pass (sdhip_affine_act with a group per
    image).  Backward: the reductions ds, one launch for the MLP's backward (parameter gradients and the pooled-path term),
    one elementwise pass writing dL/dz."""

    @staticmethod
    def forward(ctx, z, w1, b1, w2, b2, side, act):
        _require_gpu(z, w1)
        B, C, H, W = z.shape
        r = w1.shape[0]
        zv, ldz = nhwc_view(z)
        dev = z.device
        inv_hw = 1.0 / (H * W)
        s = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = torch.empty((B * (2 * C + r),), dtype=torch.float32, device=dev)
        call("sdhip_se_fwd", ptr(side.pool), side.pool.shape[1], inv_hw, ptr(side.scale), ptr(side.shift), side.groups, ptr(w1.detach()),
             ptr(b1.detach()), ptr(w2.detach()), ptr(b2.detach()), ptr(s), ptr(ws), B, C, r, stream_ptr())
        y, ldy = alloc_nhwc(B, C, H, W, z.dtype, dev)
        call("sdhip_affine_act", ptr(zv), ldz, ptr(y), ldy, None, 0, ptr(s), None, B * H * W, C, B, act, dtype_code(z), stream_ptr())
        ctx.cfg = (ldz, act, r, inv_hw)
        ctx.save_for_backward(zv, w1, b1, w2, b2, s, ws)
        return y

    @staticmethod
    def backward(ctx, gy):
        zv, w1, b1, w2, b2, s, ws = ctx.saved_tensors
        ldz, act, r, inv_hw = ctx.cfg
        B, C, H, W = zv.shape
        dev = zv.device
        dt = dtype_code(zv)
        g, ldg = nhwc_view(gy)
        both, pz = _zeros((2, NREP, B, C), torch.float32, dev)
        call("sdhip_affine_act_bwd", ptr(g), ldg, ptr(zv), ldz, None, 0, ptr(s), None, ptr(both[0]), ptr(both[1]), NREP,
             B * H * W, C, B, act, 0, int(pz), dt, stream_ptr())
        outs = []
        for prm in (w1, b1, w2, b2):
            t = _grad_target(prm)
            outs.append((t, False) if t is not None else (_zeros(tuple(prm.shape), torch.float32, dev)[0], True))
        gpool = torch.empty((B, C), dtype=torch.float32, device=dev)
        call("sdhip_se_bwd", ptr(both[0]), NREP, ptr(ws), ptr(w1.detach()), ptr(w2.detach()), ptr(outs[0][0]), ptr(outs[1][0]),
             ptr(outs[2][0]), ptr(outs[3][0]), ptr(gpool), inv_hw, B, C, r, stream_ptr())
        gz, ldgz = alloc_nhwc(B, C, H, W, zv.dtype, dev)
        call("sdhip_se_scale_bwd", ptr(g), ldg, ptr(zv), ldz, ptr(gz), ldgz, ptr(s), ptr(gpool), H * W, B, C, act, dt, stream_ptr())
        grads = [t if ret else None for t, ret in outs]
        return (gz, *grads, None, None)


def se_scale_act(z, fc1, fc2, side, act=0):
    """act(SELayer(z)) given the SESide the depthwise node behind z filled (fc1 / fc2: the two nn.Linear)."""
    if side is None or side.pool is None:
        raise _lib.SdhipError("se_scale_act needs the pool of the depthwise node in front of it (SESide)")
    return _SEScaleActFn.apply(z, fc1.weight, fc1.bias, fc2.weight, fc2.bias, side, act)


# ============================================================================ DeepLabV3+ / Xception-65: dilated depthwise 3x3
def dw_dil_wgrad_parts(B, H, W, C, stride):
    """Partial slots of sdhip_dw_dil_conv_wgrad for this shape (include/sdhip.h)."""
    n = _lib._lib.sdhip_dw_dil_wgrad_parts(B, H, W, C, stride)
    if n <= 0:
        raise _lib.SdhipError("sdhip_dw_dil_wgrad_parts: unsupported depthwise shape")
    return n


class _DWDilConvBNActFn(torch.autograd.Function):
    """y = act(BatchNorm(depthwise_conv3x3(relu?(x), stride, dilation))) as ONE autograd node — depthwise + bn_depth (+ relu1)
    of SeparableConv2d (models_deeplab_mod/common.py:24-50).  relu_first is applied in the kernel's load: x itself is saved
    un-rectified (the 'sum' skip of XceptionBlock reads it), the data gradient masks with [x > 0] in its own launch and the
    weight gradient rectifies in its load."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn, stride, dil, in_relu, act, groups):
        _require_gpu(x, weight)
        if weight.dtype != torch.float32 or not weight.is_contiguous():
            raise _lib.SdhipError("depthwise weight must be a contiguous f32 (C, 1, 3, 3) tensor")
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        xv, ldx = nhwc_view(x)
        dt = dtype_code(x)
        yraw, ldr = alloc_nhwc(B, C, Ho, Wo, x.dtype, x.device)
        train = bn.training
        ws = _zeros((NREP, groups, 2, C), torch.float64, x.device)[0] if train else None
        call("sdhip_dw_dil_conv_fwd", ptr(xv), ldx, ptr(weight.detach()), ptr(yraw), ldr, ptr(ws), C, NREP, B, H, W, C, stride, dil,
             int(in_relu), groups, dt, stream_ptr())
        count = (B // groups) * Ho * Wo
        y, scale, shift, mean, invstd = _bn_act_forward(yraw, ldr, bn, ws, count, groups, act)
        ctx.cfg = (stride, dil, in_relu, act, groups, ldx, ldr, count, train)
        ctx.save_for_backward(xv, weight, gamma, beta, yraw, scale, shift, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xv, weight, gamma, beta, yraw, scale, shift, mean, invstd = ctx.saved_tensors
        stride, dil, in_relu, act, groups, ldx, ldraw, count, train = ctx.cfg
        B, C, H, W = xv.shape
        dt = dtype_code(xv)
        g, ldg = nhwc_view(gy)
        graw, ldgr, dgamma, dbeta = _bn_act_backward(g, ldg, yraw, ldraw, scale, shift, mean, invstd, gamma, beta, groups, act,
                                                     count, train)
        gx = None
        if ctx.needs_input_grad[0]:
            gx, ldgx = alloc_nhwc(B, C, H, W, xv.dtype, xv.device)
            call("sdhip_dw_dil_conv_dgrad", ptr(graw), ldgr, ptr(weight.detach()), ptr(xv) if in_relu else None, ldx, ptr(gx), ldgx,
                 B, H, W, C, stride, dil, dt, stream_ptr())
        gw = None
        if ctx.needs_input_grad[1]:
            tw = _grad_target(weight)
            target = tw if tw is not None else _zeros(tuple(weight.shape), torch.float32, weight.device)[0]
            nparts = dw_dil_wgrad_parts(B, H, W, C, stride)
            part = torch.empty((nparts * 9 * C,), dtype=torch.float32, device=weight.device)   # every slot is written
            call("sdhip_dw_dil_conv_wgrad", ptr(xv), ldx, ptr(graw), ldgr, ptr(target), ptr(part), nparts, B, H, W, C, stride, dil,
                 int(in_relu), dt, stream_ptr())
            gw = None if tw is not None else target
        return gx, gw, dgamma, dbeta, None, None, None, None, None, None


def dw_dil_conv_bn_act(x, weight, bn, stride=1, dilation=1, in_relu=False, act=0, groups=1):
    """act(bn(nn.Conv2d(C, C, 3, stride, padding=dilation, dilation=dilation, groups=C, bias=False)(relu(x) if in_relu else x)))."""
    if tuple(weight.shape) != (x.shape[1], 1, 3, 3) or stride not in (1, 2) or dilation < 1:
        raise _lib.SdhipError("dilated depthwise convolution: (C, 1, 3, 3) weights, stride 1 / 2, dilation >= 1 only")
    return _DWDilConvBNActFn.apply(x, weight, bn.weight, bn.bias, bn, stride, int(dilation), bool(in_relu), act, groups)
