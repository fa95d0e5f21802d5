/*
 * sdhip.h — C ABI of libsdhip.so, the MI355X (gfx950) hot path of the joint
 * segmentation + disparity network of
 * cuevhv/PMT_learning_for_semantic_segmentation_and_disparity.
 *
 * Conventions (every entry point):
 *   - plain C, no C++ / torch types; all pointers are BORROWED device pointers;
 *     the callee never allocates or frees caller-visible memory;
 *   - activations are NHWC ("channels last"): element (b,h,w,c) of a tensor with
 *     pixel stride ld (in elements, ld >= C) lives at ((b*H + h)*W + w)*ld + c;
 *     a tensor may therefore be a channel slice of a wider slab;
 *   - dtype: SDHIP_F32 (exact f32 path, f32-input MFMA / f32 FMA) or
 *     SDHIP_BF16 (bf16 storage, f32 accumulate, bf16 MFMA); statistics and loss
 *     values are always f32/f64;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; the
 *     caller passes torch.cuda.current_stream().cuda_stream) and capturable in a
 *     hipGraph: no allocation, no synchronisation, no host read-back inside;
 *   - returns 0 on success or a negative SDHIP_ERR_* code; sdhip_last_error()
 *     returns a thread-local message; nothing ever aborts the process.
 *
 * Each function cites the reference interface (file:line under the upstream
 * repository root) it replaces.
 */
#ifndef SDHIP_H_
#define SDHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDHIP_F32 0
#define SDHIP_BF16 1

#define SDHIP_OK 0
#define SDHIP_ERR_ARG (-1)     /* bad shape / dtype / alignment */
#define SDHIP_ERR_LAUNCH (-2)  /* hip launch failure */
#define SDHIP_ERR_UNSUPPORTED (-3)

/* Activation codes of the elementwise / BatchNorm kernels beyond 0 none, 1 ReLU, 2 sigmoid (4: sigmoid given its output,
 * backward only): the hard activations of MobileNetV3 (models/mobilenetv3.py:44-61), h_swish = x*relu6(x+3)/6 and
 * h_sigmoid = relu6(x+3)/6, with torch's gradient of that composite (0 weight on relu6's kinks). */
#define SDHIP_ACT_HSWISH 5
#define SDHIP_ACT_HSIGMOID 6

/* ABI version of this header; bumped on any signature change. */
int sdhip_abi_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* sdhip_last_error(void);
/* Diagnostic / tuning environment switches (SDHIP_CONV_GENERIC, SDHIP_TUNE_*, ... — DESIGN.md 7b) are read once when
 * the library is loaded (a set switch is announced on stderr) and never per launch; a test or tool that changes the
 * environment for an A/B run inside one process calls this to re-read them.  No reference counterpart. */
void sdhip_diag_reload(void);
/* Which kernel the convolution dispatch chooses.  sdhip_last_path() names the kernel that the last call of
 * sdhip_conv2d_fwd / _fwd_add / _fwd_bnbwd / _fwd_bnpro / _fwd_phase / sdhip_conv2d_wgrad / sdhip_conv2d_wgrad_group (the
 * last item's) on this thread chose: the family word first, details in parentheses — "thin", "band(5x5, bx)", "mid",
 * "fast(4x16, ks 1, single-stage, dma, tail)", "generic(8x32, per_tap)", "gemm1x1", "fast(taps 9, mb 64, cit 4, 4x32, register)",
 * ...; "unsupported" after an SDHIP_ERR_UNSUPPORTED exit, "" before any call and after a call
 * that was refused for its arguments (SDHIP_ERR_ARG).  The string is thread-local and valid
 * until the next call of this function.  While sdhip_dispatch_dry(1) is in force on a thread, those entry points
 * validate and dispatch exactly as usual and launch NOTHING: no operand is dereferenced and the HIP runtime is not
 * touched, so the question can be asked with made-up (suitably aligned) addresses and without a GPU.  The callers and
 * the tests ask the library instead of copying its predicates.  No reference counterpart. */
void sdhip_dispatch_dry(int on);
const char* sdhip_last_path(void);
/* End a stream capture that failed half way (an uncapturable call invalidated it and the caller left its capture block
 * by an exception): hipStreamEndCapture on `stream`, the partial graph destroyed, the sticky error cleared.  Returns 1 if a
 * capture was still open, 0 if none was, < 0 if the stream cannot be brought back.  Host-side recovery for the training
 * step's hipGraph (the reference has no graph capture; its counterpart is simply running the step eagerly). */
int sdhip_abort_capture(void* stream);
/* Node inventory of a captured step: graph = hipGraph_t; counts[0..3] = kernel, memset, memcpy, other nodes.  Returns the
 * total node count (< 0: error).  The library keeps a captured step to kernel nodes (sdhip_zero_async); tests assert it. */
int sdhip_graph_node_counts(void* graph, int* counts);

/* ---------------------------------------------------------------------------
 * Spatial correlation sampler  (third-party op `SpatialCorrelationSampler`,
 * constructed at models/dsnet_t2.py:1078-1087,129-133 and called at
 * models/dsnet_t2.py:1188-1193,1233-1234,221-223 with kernel_size=1, stride=1,
 * padding=0).
 *
 *   out[b,h,w,ph*PW+pw] = sum_c in1[b,h,w,c] * in2[b, h+(ph-PH/2)*dil, w+(pw-PW/2)*dil, c]
 *   (zero where the displaced pixel leaves the image; no normalisation).
 *
 * in1,in2: NHWC (B,H,W,C) with pixel stride ld_in; out: NHWC (B,H,W,PH*PW) with
 * pixel stride ld_out — i.e. the reference's (B,PH,PW,H,W) result stored with
 * the displacement as the fastest dimension.
 * ------------------------------------------------------------------------- */
int sdhip_corr_fwd(const void* in1, const void* in2, void* out,
                   int B, int H, int W, int C, int ld_in,
                   int PH, int PW, int dil_patch, int ld_out,
                   int dtype, void* stream);
/* Gradients w.r.t. both inputs given gout = dL/dout (same layout as out). */
int sdhip_corr_bwd(const void* in1, const void* in2, const void* gout,
                   void* gin1, void* gin2,
                   int B, int H, int W, int C, int ld_in,
                   int PH, int PW, int dil_patch, int ld_out,
                   int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Direct 2-D convolution (im2col-free, LDS-staged halo tiles, MFMA contraction).
 *
 * Replaces ATen/cuDNN under conv2dSame.forward (models/torch_model.py:268-281),
 * the stride-1 ConvTranspose2dSame.forward (models/torch_model.py:320-349), the
 * DenseNet nn.Conv2d layers (models/densenet.py:25-93,131-245) and ASPP
 * (models/aspp.py:7-32).  Weights are consumed in a packed layout produced by
 * sdhip_conv_pack_weights from the module's f32 parameter:
 *     packed[q][t][m][c] = W(m, k = q*CK + c, tap t or T-1-t),  zero padded,
 *     CK = 64 (bf16) / 32 (f32), m < roundup(M,16)
 * with (stride_m, stride_k, flip) selecting which parameter axis is the output
 * ("m") and which the reduction ("k") axis:
 *     Conv2d        weight (Cout,Cin,kh,kw): forward   M=Cout K=Cin sm=Cin*T sk=T    flip=0
 *                                            data grad M=Cin  K=Cout sm=T     sk=Cin*T flip=1
 *     ConvTranspose2d weight (Cin,Cout,kh,kw) (stride 1, run as a correlation):
 *                                            forward   M=Cout K=Cin sm=T     sk=Cout*T flip=1
 *                                            data grad M=Cin  K=Cout sm=Cout*T sk=T    flip=0
 * ------------------------------------------------------------------------- */
long sdhip_conv_packed_elems(int M, int K, int T, int dtype);
int sdhip_conv_pack_weights(const float* src, void* dst, int M, int K, int T,
                            long stride_m, long stride_k, int flip, int dtype, void* stream);
/* Inverse of the packing for the f32 gradient buffer written by sdhip_conv2d_wgrad:
 * grad(m,k,t) (+)= acc[k/CK][flip ? T-1-t : t][m][k%CK]. */
int sdhip_conv_unpack_wgrad(const float* acc, float* grad, int M, int K, int T,
                            long stride_m, long stride_k, int flip, int accumulate, int dtype, void* stream);

/* y[b,oh,ow,m] = act( bias[m] + sum_{t,k} W[m,k,t] * pro(x)[b, oh*stride + kh*dil - pad_t, ow*stride + kw*dil - pad_l, k] )
 *   pro(x) = x, or relu?(x*in_scale[g][k] + in_shift[g][k]) when in_scale != NULL (the BatchNorm+ReLU
 *            that precedes the conv, models/densenet.py:41-45,75-93); zero padding is applied AFTER pro;
 *            in_scale / in_shift are f32 [groups][Cin] for ANY Cin (a channel count that is no multiple
 *            of the 16-byte vector is supported): nothing outside those groups*Cin entries is read, and the elements
 *            [Cin, ldx) of a pixel of x never reach the result, whatever they hold (NaN included);
 *   g      = b / (B/groups): statistics group of image b (left/right tower passes share a launch);
 *   stats  : if non-NULL, f64 [groups][2][stats_ld >= Cout] (stats_ld <= 0 means Cout; a slice of a wider
 *            statistics slab is addressed by offsetting the pointer), replicated stats_nrep times
 *            ([nrep][groups][2][stats_ld]; workgroups spread their atomics over the replicas because thousands
 *            of adds into one 256-byte line serialise; consumers sum the replicas); the kernel ADDS sum(y) and sum(y^2) over pixels
 *            (of the stored, rounded values) — the batch statistics of the BatchNorm that follows;
 *   act    : 0 none, 1 ReLU, 2 sigmoid;  accumulate != 0: y += result.
 * 3-D convolutions (nn.Conv3d / nn.ConvTranspose3d of models_psmnet/submodule.py:16-19, stackhourglass.py:10-50):
 * a volume is [B][D][H][W][C]; (D, Do, kd, sd, pad_d) describe the depth axis and the packed weights gain a leading
 * depth-tap dimension [kd][q][t][m][c] (pack each depth tap with sdhip_conv_pack_weights).  2-D: D=Do=kd=sd=1, pad_d=0.
 * (pad_t, pad_l) is the top/left padding; bottom/right padding is implied by (Ho, Wo)
 * (TF-"same" padding of models/torch_model.py:276-281 is asymmetric for stride 2). */
int sdhip_conv2d_fwd(const void* x, const void* wpacked, void* y,
                     const float* bias, const float* in_scale, const float* in_shift,
                     double* stats, int stats_ld, int stats_nrep,
                     int B, int H, int W, int Cin, int ldx,
                     int Ho, int Wo, int Cout, int ldy,
                     int kh, int kw, int stride, int dil, int pad_t, int pad_l,
                     int D, int Do, int kd, int sd, int pad_d,
                     int in_relu, int groups, int act, int accumulate,
                     int dtype, void* stream);

/* y = conv(relu(BatchNorm_train(x)), wpacked) with the BatchNorm finalized INSIDE the launch — the norm2 -> relu2 -> conv2 of a
 * DenseNet layer (models/densenet.py:41-45,86-93) without a per-channel kernel between conv1's epilogue, which wrote the batch
 * statistics in_stats (f64 [in_stats_nrep <= 4][groups][2][in_stats_ld]: sum, sum of squares), and this launch, whose input
 * prologue needs scale = gamma / sqrt(var + eps), shift = beta - mean * scale: every workgroup derives them for its statistics
 * group (arithmetic of sdhip_bn_finalize), workgroup 0 also writes scale / shift / mean / invstd ([groups][Cin], read by the
 * backward pass) and updates running_mean / running_var (groups in order, momentum as nn.BatchNorm2d; NULL: not tracked).
 * out_stats: as `stats` of sdhip_conv2d_fwd.  Stride 1, no dilation, Cin <= 1024; f32 and bf16.
 * pend_stats (optional): the norm1 -> relu1 -> conv1 of a dense layer (models/densenet.py:41-45,75-85) reads the slab statistics
 * in_stats (one replica) of which the channels [pend_c0, pend_c0 + pend_n) — the previous layer's output — are still spread over
 * the replicas pend_stats (f64 [pend_nrep <= 4][groups][2][pend_ld], channel c - pend_c0): they are taken from there and
 * workgroup 0 folds them into in_stats on the way (what sdhip_bn_fold_finalize does in a launch of its own). */
int sdhip_conv2d_fwd_bnpro(const void* x, const void* wpacked, void* y, double* out_stats, int out_stats_ld, int out_stats_nrep,
                           double* in_stats, int in_stats_ld, int in_stats_nrep,
                           const double* pend_stats, int pend_ld, int pend_nrep, int pend_c0, int pend_n,
                           const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* scale_out, float* shift_out, float* mean_out,
                           float* invstd_out, double count, float eps, float momentum,
                           int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                           int kh, int kw, int pad_t, int pad_l, int groups, int dtype, void* stream);

/* y = conv(x, wpacked) + addend: a data gradient that lands on a tensor with a second consumer — x1 / x2 of Conv2DownUp
 * (models/dsnet_t2.py:80-117) feed the next convolution AND a skip add — written as the SUM of both contributions (addend =
 * the skip's gradient, [B][Ho][Wo] pixels of ldadd elements), summed in f32 and rounded once, instead of autograd running an
 * elementwise add over the map.  Stride 1, no dilation; served by the persistent 5x5 kernel only (bf16, Cin in {8..32, 64},
 * Cout <= 64, at least 192 tiles of 16x32 output pixels, 16-byte aligned pixels): SDHIP_ERR_UNSUPPORTED otherwise. */
int sdhip_conv2d_fwd_add(const void* x, const void* wpacked, void* y, const void* addend, int ldadd,
                         int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                         int kh, int kw, int pad_t, int pad_l, int dtype, void* stream);

/* The data gradient of a stride-1 convolution whose INPUT was relu(BatchNorm_train(u)) — the 3x3 convolution of a DenseNet
 * layer behind norm2 + relu2 (models/densenet.py:41-45,75-93): y = conv(x, wpacked) is dL/d relu(bn(u)) (x = the gradient
 * of the convolution's output, wpacked = its weights packed in data-gradient form), and the epilogue, which holds every
 * value of y once, also takes the two reductions the BatchNorm backward starts with, over the stored (rounded) values:
 *     sums[rep][g][0][c] += sum_pixels gm * u,   sums[rep][g][1][c] += sum_pixels gm,
 *     gm = y where u*scale[g][c] + shift[g][c] > 0, else 0
 * (f64 [sums_nrep][groups][2][sums_ld >= Cout], zeroed by the caller) — what sdhip_affine_act_bwd computes in a pass of its
 * own over y and u.  u: [B][Ho][Wo] pixels of ldu elements, Cout of them used.  addend (optional, as sdhip_conv2d_fwd_add):
 * y = conv + addend, sums taken over that total — the convbn + ReLU layers of Conv2DownUp (models/dsnet_t2.py:80-117), whose
 * output gradient is the next layer's data gradient plus a skip gradient.  bf16, Cout % 4 == 0; consumer:
 * sdhip_bn_bwd_apply_fin_d.  SDHIP_ERR_UNSUPPORTED when the shape has no kernel with this epilogue.
 * mode 1 ("apply", addend required and allowed to be y): the launch is the 1x1 data gradient of a DenseNet layer AND the first
 * phase of norm1's backward over it (models/densenet.py:41-45,75-93: conv1 <- relu1 <- norm1 <- concatenated features):
 *     y = addend + gm * scale[g][c],  gm = conv(x) where u*scale + shift > 0 else 0
 * — the masked, scaled gradient accumulated into the slab's gradient — and the two reductions go, as f32, to
 * ((float*)sums)[which][rep][g][c] (which = 0: sum gm*u, 1: sum gm; [2][sums_nrep][groups][Cout], zeroed by the caller): the
 * dscale / dshift replicas of sdhip_affine_act_bwd, so its consumers (sdhip_stats_fix_fin, sdhip_bn_finalize_bwd) are unchanged. */
int sdhip_conv2d_fwd_bnbwd(const void* x, const void* wpacked, void* y, double* sums, int sums_ld, int sums_nrep,
                           const void* u, int ldu, const float* scale, const float* shift, const void* addend, int ldadd,
                           int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                           int kh, int kw, int dil, int pad_t, int pad_l, int groups, int mode, int dtype, void* stream);

/* One sub-pixel phase of nn.ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1) (models_psmnet/stackhourglass.py:25-29;
 * 2-D: D = kd = 1): output voxel 2m + off of an axis receives input m with kernel tap 1 when off = 0, and inputs m, m+1
 * with taps 2, 0 when off = 1 — so each of the 8 phases (off_d, off_h, off_w) is a stride-1 correlation with a
 * (1+off_d) x (1+off_h) x (1+off_w) sub-kernel over the UN-stuffed input, 27 taps in all instead of 8 x 27 over a
 * zero-stuffed volume.  x: [B][D][H][W][Cin]; y: the [B][2D][2H][2W][Cout] output volume (pixel stride ldy), of which this
 * call writes the voxels (2d + off_d, 2h + off_h, 2w + off_w); wpacked: the phase's sub-kernel packed [kd][q][t][m][c]
 * with taps ordered input-offset-major (sdhip_conv_pack_weights per depth tap); stats: as sdhip_conv2d_fwd (the eight
 * calls add into the same sums).  bf16 / f32, 16-byte aligned pixels.  The depth axis is doubled like the other two also
 * in the 2-D form: with D = kd = 1 and off_d = 0, y is [B][2][2H][2W][Cout] and the four calls fill depth slice 0 of every
 * image; slice 1 is not touched. */
int sdhip_conv2d_fwd_phase(const void* x, const void* wpacked, void* y, double* stats, int stats_ld, int stats_nrep,
                           int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int kh, int kw,
                           int D, int kd, int groups, int off_d, int off_h, int off_w, int dtype, void* stream);
/* prezeroed != 0: the caller already zeroed dw_packed / dbias (one arena memset per step instead of one per call).
 * dW (packed f32, zeroed here) = sum over pixels of dy (x) pro(x); dbias[m] = sum dy (optional).  Only the entries (m < Cout,
 * k < Cin) of dw_packed receive anything: its pad rows [Cout, roundup(Cout,16)) and the channel tail of its last chunk stay
 * exactly zero, whatever the elements [Cin, ldx) of x and [Cout, lddy) of dy hold. */
int sdhip_conv2d_wgrad(const void* x, const void* dy, float* dw_packed, float* dbias,
                       const float* in_scale, const float* in_shift,
                       int B, int H, int W, int Cin, int ldx,
                       int Ho, int Wo, int Cout, int lddy,
                       int kh, int kw, int stride, int dil, int pad_t, int pad_l,
                       int D, int Do, int kd, int sd, int pad_d,
                       int in_relu, int groups, int prezeroed, int dtype, void* stream);
/* The weight gradients of n layers in as few launches as possible: layers that run on the same kernel instantiation share
 * ONE grid (<= 16 layers per grid; the layer table travels in the kernel arguments, so a captured step needs no device
 * table).  items: HOST array, fields as the arguments of sdhip_conv2d_wgrad; every dw_packed / dbias must already be zero
 * (prezeroed semantics).  Results equal n calls of sdhip_conv2d_wgrad up to the order of the f32 atomic adds.  Nothing in
 * a training step reads a weight gradient before the optimizer (torch_implementation.py:389,724), so the step queues its
 * ~200 per-layer launches and issues them here after the backward pass (ops.StepContext.join).
 * max_workgroups > 0: every grid stays within that many workgroups (one round), leaving CUs to the kernels of another
 * stream — the decoder's weight gradients run beside the latency-bound DenseNet backward chain that way; 0: fill the chip. */
typedef struct SdhipWgradItem {
  const void* x; const void* dy; float* dw_packed; float* dbias; const float* in_scale; const float* in_shift;
  int B, H, W, Cin, ldx, Ho, Wo, Cout, lddy, kh, kw, stride, dil, pad_t, pad_l, D, Do, kd, sd, pad_d, in_relu, groups;
} SdhipWgradItem;
int sdhip_conv2d_wgrad_group(const SdhipWgradItem* items, int n, int max_workgroups, int dtype, void* stream);

/* 1x1 convolution (+ bias, + activation) over the channel concatenation [x0 | x1] without materialising it; segment i is
 * read at pixel (h >> us_i, w >> us_i) of a (B, c_i, H >> us_i, W >> us_i) map, i.e. nearest-neighbour upsampled by
 * 2^us_i on the fly.  Replaces `conv1d_2(torch.cat((F.interpolate(y, scale_factor=8), xleft2), 1))` and the other
 * concat -> 1x1 -> ReLU sites of models/dsnet_t2.py:1206-1216,1262-1291,927-933 (the x8 map of :1211 is never written).
 * wpacked: sdhip_conv_pack_weights of the (Cout, c0 + c1, 1, 1) weight; c0 a multiple of 8; bf16 only. */
int sdhip_conv1x1_cat_fwd(const void* x0, int ld0, int c0, int us0, const void* x1, int ld1, int c1, int us1,
                          const void* wpacked, void* y, int ldy, const float* bias,
                          int B, int H, int W, int Cout, int act, int dtype, void* stream);
/* Pack many weights in one launch: desc = ndesc rows of 8 int64 {src ptr, dst ptr, M, K, T, stride_m, stride_k, flip}
 * in device memory (same layout rules as sdhip_conv_pack_weights). */
int sdhip_conv_pack_batch(const long* desc, int ndesc, int dtype, void* stream);
/* The eval counterpart of sdhip_conv_pack_batch (model.eval() + torch.no_grad() of test_model, torch_implementation.py:450-582):
 * with running statistics, conv -> nn.BatchNorm2d -> activation (convbn / deconvbn, models/dsnet_t2.py:16-77) equals one
 * convolution with pre-scaled weights, a bias and the activation epilogue of sdhip_conv2d_fwd.  desc = ndesc rows of 16 int64
 * in device memory, one launch for all of them:
 *   [0] kind: 0 = fold, 1 = table
 *   fold : [1] src weight (f32)  [2] dst pack  [3] bias_out (f32 [M])  [4] M  [5] K  [6] T  [7] stride_m  [8] stride_k  [9] flip
 *          (layout rules of sdhip_conv_pack_weights)
 *   table: [2] scale (f32 [groups][C])  [3] shift (f32 [groups][C])  [4] C  [5] groups            ([1], [6..9] unused)
 *   both : [10] gamma  [11] beta (either 0: 1 / 0)  [12] running_mean  [13] running_var  [14] eps (f32 bits in the low 32)
 *          [15] bias of the convolution (f32 [M]) or 0
 * Per channel m, in the f32 arithmetic of the eval branch of sdhip_bn_finalize:
 *   scale = gamma / sqrt(running_var + eps),  shift = beta - running_mean * scale (+ conv_bias * scale).
 * fold : packed[q][t][m][c] = W(m, k, t) * scale[m] (f32 product, rounded once to the pack dtype), bias_out[m] = shift[m]; the
 *        pad rows m in [M, roundup(M,16)) and the channel tail of the last chunk are written as zeros.
 * table: scale[g][c] / shift[g][c] for every g < groups (a BatchNorm that is not folded: it precedes its convolution, or its
 *        node has no bias epilogue).  Nothing beyond M (C) entries of a per-channel array is read. */
int sdhip_conv_pack_fold_batch(const long* desc, int ndesc, int dtype, void* stream);
/* One launch unpacks (adds) every weight gradient of the step into the flat gradient buffer:
 * desc[i] = {acc ptr (f32, packed as written by sdhip_conv2d_wgrad), grad ptr, M, K, T, stride_m, stride_k, flip};
 * grad(m,k,t) += acc[k/CK][flip ? T-1-t : t][m][k%CK].  Replaces ~200 per-layer sdhip_conv_unpack_wgrad launches of a
 * training step (the optimizer reads the gradients only after the whole backward pass: util/torch_implementation.py:389,724). */
int sdhip_conv_unpack_batch(const long* desc, int ndesc, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * BatchNorm2d in training mode (+ ReLU / sigmoid / skip add), decomposed so the
 * statistics ride on the producing conv and the normalisation on the consumer.
 * Replaces nn.BatchNorm2d as used at models/dsnet_t2.py:16-117,
 * models/densenet.py:25-128, models/aspp.py:7-32; statistics semantics as in
 * sync_batchnorm/batchnorm.py:114-126.  Tensors are [npix][C] row views with a
 * pixel stride; rows of statistics group g are the g-th npix/groups rows.  Statistics tensors are
 * f64 [groups][2][stats_ld] (stats_ld <= 0: = C), so a channel slice of a wider slab can be addressed.
 * ------------------------------------------------------------------------- */
/* stats[g][0][c] += sum x, stats[g][1][c] += sum x^2 (f64). */
int sdhip_channel_stats(const void* x, int ldx, double* stats, int stats_ld, int stats_nrep, long npix, int C, int groups,
                        int zero_first, int dtype, void* stream);
/* Train (stats != NULL): mean = S1/count, var = S2/count - mean^2 (biased), scale = gamma*invstd,
 * shift = beta - mean*scale; running_mean/var updated in place group by group with `momentum`
 * (running_var unbiased).  Eval (stats == NULL): scale/shift from the running statistics. */
int sdhip_bn_finalize(const double* stats, int stats_ld, int stats_nrep, const float* gamma, const float* beta,
                      float* running_mean, float* running_var,
                      float* scale, float* shift, float* mean_out, float* invstd_out,
                      int C, int groups, double count, float eps, float momentum, void* stream);
/* (dscale,dshift)[g][c] -> dgamma[c], dbeta[c] and dstats[g][2][c] (gradient w.r.t. S1, S2; zero in eval). */
int sdhip_bn_finalize_bwd(const float* dscale, const float* dshift, int nrep, const float* gamma,
                          const float* mean, const float* invstd,
                          float* dgamma, float* dbeta, double* dstats, int stats_ld, int accumulate_flags /* bit0: dstats +=, bit1: dgamma/dbeta += */,
                          int C, int groups, double count, int train, void* stream);
/* sdhip_bn_finalize_bwd (train mode, dstats accumulated) of a BatchNorm over the first Cf channels of a DenseNet slab fused
 * with sdhip_stats_fix of the 32 slab channels [cs, cs + 32) that the next layer of the backward walk needs:
 * gout = gin + dS[g][0][c] + 2 x dS[g][1][c] with dS INCLUDING this call's contribution for those channels (which is not
 * written back: nothing reads it again).  dscale/dshift: replicas [nrep][groups][Cf] of sdhip_affine_act_bwd;
 * accumulate_params: dgamma/dbeta += (flat gradient buffer) instead of =.  Rows 16-byte aligned. */
int sdhip_stats_fix_fin(const void* gin, int ldgi, const void* x, int ldx, void* gout, int ldgo, long npix,
                        double* dS, int ldc, int cs, const float* dscale, const float* dshift, int nrep,
                        const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                        int accumulate_params, float param_scale, int Cf, int groups, double count, int dtype, void* stream);
/* y = act(x*scale[g][c] + shift[g][c]) (+ res). scale/shift may be NULL (identity). */
int sdhip_affine_act(const void* x, int ldx, void* y, int ldy, const void* res, int ldr,
                     const float* scale, const float* shift, long npix, int C, int groups, int act,
                     int dtype, void* stream);
/* act: 0 none, 1 ReLU, 2 sigmoid, 4 sigmoid with x holding the sigmoid OUTPUT.
 * dscale/dshift are replicated [nrep][groups][C] (see stats_nrep above; sdhip_bn_finalize_bwd sums them).
 * gx (+)= gy*act'*scale (if gx != NULL; += when accumulate != 0); dscale = sum gy*act'*x, dshift = sum gy*act' (if non-NULL; zeroed here). */
int sdhip_affine_act_bwd(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                         const float* scale, const float* shift, float* dscale, float* dshift, int nrep,
                         long npix, int C, int groups, int act, int accumulate, int prezeroed, int dtype, void* stream);
/* Backward of y = act(conv_folded(x) + bias) through the activation and a FROZEN BatchNorm folded into the weight pack
 * (sdhip_conv_pack_fold_batch; `-freeze_bn 1`, torch_implementation.py:235-241): graw[p][c] = gy[p][c] * act'(y[p][c]) *
 * scale[g][c], the gradient of the RAW convolution output, from which the data and weight gradients run with the raw weight.
 * The derivative is taken from the activation's OUTPUT y: act 0 -> 1, 1 (ReLU) -> y > 0, 2 (sigmoid) -> y (1 - y).
 * scale: f32 [groups][C], group g owns the g-th npix/groups rows.  Only the C logical channels of a row are written.  The
 * 16-byte path is taken when C and the three strides are multiples of 16 bytes of elements and the pointers are aligned. */
int sdhip_act_out_bwd(const void* gy, int ldg, const void* y, int ldy, void* graw, int ldgr, const float* scale,
                      long npix, int C, int groups, int act, int dtype, void* stream);
/* out[row][c] += sum_r ws[r][row][c] over the 2*groups statistics rows (folds conv-epilogue replicas into a slab). */
int sdhip_stats_replica_sum(const double* ws, double* out, int nrep, int groups, int C, int ldw, int ldo, void* stream);
/* sdhip_stats_replica_sum of the Cn newest channels (replicas ws[nrep][groups][2][ldw]) into the statistics slab
 * S[groups][2][ldc] at channel c_new0, followed by sdhip_bn_finalize of the first C >= c_new0 + Cn channels from S — one
 * launch instead of two on the DenseNet's layer-to-layer chain (models/densenet.py:41-45: norm1 of layer l+1 reads every
 * channel up to layer l's output). */
int sdhip_bn_fold_finalize(const double* ws, int nrep, int ldw, int c_new0, int Cn, double* S, int ldc,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           float* scale, float* shift, float* mean_out, float* invstd_out, int C, int groups,
                           double count, float eps, float momentum, void* stream);
/* gout = gin + dstats[g][0][c] + 2*x*dstats[g][1][c]: the gradient that flows through the batch statistics. */
int sdhip_stats_fix(const void* gin, int ldgi, const void* x, int ldx, void* gout, int ldgo,
                    const double* dstats, int stats_ld, long npix, int C, int groups, int dtype, void* stream);
/* Two-phase BatchNorm backward, second phase: gx = gy * act'(x*scale+shift) * scale + dstats[g][0] + 2*x*dstats[g][1] in one
 * pass (first phase: sdhip_affine_act_bwd with gx == NULL, then sdhip_bn_finalize_bwd) — the backward of
 * nn.BatchNorm2d(+ReLU) in train mode, models/dsnet_t2.py:16-117.  act: 0 none, 1 relu, 2 sigmoid. */
int sdhip_bn_bwd_apply(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                       const float* scale, const float* shift, const double* dstats, int stats_ld,
                       long npix, int C, int groups, int act, int dtype, void* stream);
/* Consumer-side finalize (no separate per-channel launch between a reduction and the pass that uses it):
 * affine_act_bn   : y = act(BatchNorm_train(x)) (+ res) straight from the statistics of x (as written by the conv epilogue /
 *                   sdhip_channel_stats); also writes scale/shift/mean/invstd [G][C] for the backward pass and updates
 *                   running_mean / running_var (groups applied in order, momentum as nn.BatchNorm2d) — the forward of
 *                   convbn/deconvbn + ReLU (+ skip add), models/dsnet_t2.py:16-117.
 * bn_bwd_apply_fin: sdhip_bn_bwd_apply with dstats derived in the kernel from the (dscale, dshift) replica sums of
 *                   sdhip_affine_act_bwd; writes (accumulate_params: adds to) dgamma / dbeta summed over groups. */
int sdhip_affine_act_bn(const void* x, int ldx, void* y, int ldy, const void* res, int ldr,
                        const double* stats, int stats_ld, int nrep, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float* scale, float* shift, float* mean_out, float* invstd_out,
                        long npix, int C, int groups, double count, float eps, float momentum, int act, int dtype, void* stream);
int sdhip_bn_bwd_apply_fin(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                           const float* scale, const float* shift, const float* dscale, const float* dshift, int nrep,
                           const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                           int accumulate_params, float param_scale, long npix, int C, int groups, double count, int act, int dtype, void* stream);
/* bn_bwd_apply_fin with the two reductions supplied as f64 [nrep][groups][2][C] = (sum(gm*x), sum(gm)) — the layout in
 * which the epilogue of sdhip_conv2d_fwd_bnbwd adds them. */
int sdhip_bn_bwd_apply_fin_d(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                             const float* scale, const float* shift, const double* sums, int nrep,
                             const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                             int accumulate_params, float param_scale, long npix, int C, int groups, double count, int act, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Pooling / resizing / broadcast product on NHWC tensors (HBM bound).
 * Replace nn.MaxPool2d(3,2,1) (models/densenet.py:158), F.avg_pool2d / nn.AvgPool2d(p,p)
 * (models/densenet.py:232; models/dsnet_t2.py:1983-2022), F.interpolate nearest / bilinear
 * (models/dsnet_t2.py:927-936,1204-1275,2037-2081; models/aspp.py:88) and the attention
 * product s2_d*at_s (models/dsnet_t2.py:1258).  Index maths follow ATen's CPU kernels.
 * ------------------------------------------------------------------------- */
/* 3x3 / stride 2 / pad 1 max pool; idx (u8, [B*Ho*Wo][C]) records the winning tap (first max wins). */
int sdhip_maxpool3s2_fwd(const void* x, int ldx, void* y, int ldy, unsigned char* idx,
                         int B, int H, int W, int C, int dtype, void* stream);
int sdhip_maxpool3s2_bwd(const void* gy, int ldg, const unsigned char* idx, void* gx, int ldgx,
                         int B, int H, int W, int C, int dtype, void* stream);
/* k x k / stride k average pool, no padding, floor mode (output H/k x W/k). */
int sdhip_avgpool_fwd(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, int k,
                      int dtype, void* stream);
int sdhip_avgpool_bwd(const void* gy, int ldg, void* gx, int ldgx, int B, int H, int W, int C, int k,
                      int dtype, void* stream);
/* mode 0 nearest, 1 bilinear align_corners=False, 2 bilinear align_corners=True.
 * scale_h/scale_w > 0 override in/out (F.interpolate(scale_factor=f) uses 1/f). */
int sdhip_resize_fwd(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, int Ho, int Wo,
                     int mode, float scale_h, float scale_w, int dtype, void* stream);
/* tmp: caller-provided f32 workspace of B*Ho*W*C elements. */
int sdhip_resize_bwd(const void* gy, int ldg, void* gx, int ldgx, float* tmp, int B, int H, int W, int C,
                     int Ho, int Wo, int mode, float scale_h, float scale_w, int dtype, void* stream);
/* The pooled pyramids (models/dsnet_t2.py:2037-2081): y = cat([x] + [bilinear(map_j -> (H, W)) for j < n], channels),
 * align_corners=False, written by ONE launch that owns whole rows of the slab y (B, H, W, C + n*Cb; pixel stride ldy).
 * maps: HOST array of n <= 8 branch maps (B, h, w, Cb; pixel stride ld) of any size; the table travels in the kernel
 * arguments.  Every value has the bits sdhip_resize_fwd (mode 1) into the slice and a copy of x would give.
 * SDHIP_ERR_UNSUPPORTED (nothing launched): a pointer, stride or channel count that is not a whole number of 16-byte units. */
typedef struct SdhipPyrMap {
  void* p;
  int h, w, ld, reserved;
} SdhipPyrMap;
int sdhip_pyramid_upcat_fwd(const void* x, int ldx, const SdhipPyrMap* maps, int n, void* y, int ldy,
                            int B, int H, int W, int C, int Cb, int dtype, void* stream);
/* The gradients of all n maps from the slab gradient gy (read in place at channel C + j*Cb, pixel stride ldg) in two
 * launches: the separable gather of sdhip_resize_bwd (W axis into tmp, then H), its window, weights and lanes-per-item
 * rule per branch.  gmaps[j].p receives the gradient of map j (every element written).  tmp: f32 workspace of
 * B*H*Cb*sum(w_j) elements.  The x-part of the gradient is the view gy[:, :C] and is not touched. */
int sdhip_pyramid_upcat_bwd(const void* gy, int ldg, const SdhipPyrMap* gmaps, int n, float* tmp,
                            int B, int H, int W, int C, int Cb, int dtype, void* stream);
/* y[p,c] = a[p,c] * m[p] and its gradients (ga = g*m, gm[p] = sum_c g*a). */
int sdhip_mul_bcast_fwd(const void* a, int lda, const void* m, int ldm, void* y, int ldy, long npix, int C,
                        int dtype, void* stream);
int sdhip_mul_bcast_bwd(const void* g, int ldg, const void* a, int lda, const void* m, int ldm,
                        void* ga, int ldga, void* gm, int ldgm, long npix, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Tail of the training step.
 * ------------------------------------------------------------------------- */
/* Adam over ONE flat f32 buffer (torch.optim.Adam semantics, torch_implementation.py:718-724: lr 0.0015,
 * eps 1e-7).  beta_pow = {beta1^t, beta2^t} lives on the device and is advanced by the call, so the step can
 * be replayed from a hipGraph.  grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int sdhip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* beta_pow,
                    long n, float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                    void* stream);
/* SGD with momentum over ONE flat f32 buffer (torch.optim.SGD semantics with dampening 0 and no Nesterov,
 * torch_implementation.py:715-716: lr 0.005, momentum 0.9, weight_decay 0.0001):
 *   d = g*grad_scale + weight_decay*p;  buf = momentum*buf + d;  p -= (*lr)*buf   (a zero buf gives torch's first step).
 * lr points to one f32 in DEVICE memory that the kernel reads at every launch: a replayed hipGraph steps with whatever
 * the host wrote there last, which is how adjust_learning_rate (torch_implementation.py:352-353,599-608) reaches a
 * captured step.  live: NULL, or a DEVICE table of n_live rows (begin, end) in elements - sorted, disjoint,
 * 0 <= begin < end <= n, every bound a multiple of 4.  Elements outside all rows are neither read-modified nor written,
 * in params and in momentum_buf (torch skips a parameter without a gradient; weight decay must not reach it).  The table
 * is the caller's responsibility: only pointers, 16-byte alignment of the three buffers, n > 0 and n_live >= 0 are checked. */
int sdhip_sgd_step(float* params, const float* grads, float* momentum_buf, const float* lr, long n,
                   float momentum, float weight_decay, float grad_scale,
                   const long* live, long n_live, void* stream);
/* loss += weight * mean_p sum_c -target[p,c]*log_softmax(logits[p,:])_c  and (optionally) its gradient w.r.t. the
 * logits: categoricalCrossEntropy(F.log_softmax(y,1), gt) of util/utilTorchLoss.py:373-378.  target is f32.
 * grad[p,c] = weight/npix * (softmax(logits[p,:])_c * sum_c target[p,c] - target[p,c]) is written, not accumulated.
 * logits, target and grad rows may each be channel slices of a wider slab (ldy, ldt, ldg >= C): nothing past the last
 * pixel's channel C-1 is read or written.  The pad lanes C..ldg-1 of a grad row are unspecified after the call (kept or
 * overwritten with zeros); everything outside the rows is untouched. */
int sdhip_ce_loss(const void* logits, int ldy, const float* target, int ldt, void* grad, int ldg, double* loss,
                  long npix, int C, float weight, int dtype, void* stream);
/* loss += weight * mean |pred - target| (nn.L1Loss, losses/multiLosses.py:141) and its gradient.  mask_nonpositive != 0:
 * elements whose target is <= 0 contribute zero but stay in the mean — L1(pred*zeros, disp*zeros) with zeros = disp > 0,
 * the cityscapes / kitti rule of losses/multiLosses.py:134-141. */
int sdhip_l1_loss(const void* pred, const float* target, void* grad, double* loss, long n, float weight,
                  int mask_nonpositive, int dtype, void* stream);
/* y = x * mask / (1-p), mask from a counter-based hash of (*seed, layer_id, element index): applying the same call to
 * the gradient is the backward pass (nn.Dropout(0.5) of models/aspp.py:79,95).  x/y: dense buffers of n elements. */
int sdhip_dropout(const void* x, void* y, const long* seed, long layer_id, long n, float p, int dtype, void* stream);
/* Lovasz-softmax (util/lovasz_losses.py:153-199: classes='present', per_image=False) on
 * softmax(logits) with labels = argmax(target one-hot), as called at losses/multiLosses.py:70-72.
 * ignore_void != 0 (the cityscapes / kitti rule): a pixel whose target row has no positive entry is void and removed
 * from the loss (`ignore=19` with the 20th one-hot channel dropped, losses/multiLosses.py:19-21; flatten_probas,
 * util/lovasz_losses.py:202-216).  ignore_void == 0 (roses / garden, `ignore=None`, losses/multiLosses.py:11-17): such a
 * pixel has label argmax = class 0 and counts.
 * loss += weight * mean_{present c} dot(sort_desc |fg_c - p_c|, lovasz_grad(fg sorted)); grad (if non-NULL) is
 * ACCUMULATED (+=) with the gradient w.r.t. the logits.  workspace: sdhip_lovasz_workspace_bytes(npix, C) bytes. */
long sdhip_lovasz_workspace_bytes(long npix, int C);
int sdhip_lovasz_softmax(const void* logits, int ldy, const float* target, int ldt, void* grad, int ldg,
                         double* loss, long npix, int C, float weight, void* workspace, long workspace_bytes,
                         int ignore_void, int dtype, void* stream);
/* The other terms lossSeg_fn puts on a segmentation head (`-loss`, `-segWeight`: losses/multiLosses.py:44-115), all of them
 * functions of four sums per (image b, class c) over the image's H*W = hw pixels, with p = softmax(logits), lp = log_softmax,
 * T = target (one-hot f32, a void pixel is an all-zero row): TP = sum T*p, P = sum p, G = sum T, Q = sum T*lp.  N = B*hw.
 *   cross-entropy with class weights w_c   ce_weight * (1/N) sum_b sum_c -w_c*Q            (util/utilTorchLoss.py:373-378)
 *   SDHIP_SEG_TVERSKY       1.5 * mean_c(w_c * mean_b(1 - TP / (TP + (G-TP) + 0.3*(P-TP) + 1e-6)))     (tversky_loss2, :407-426)
 *   SDHIP_SEG_DICE          mean_{b,c}([G > 1] - 2*TP / (P + G + 1))                                   (dice_loss, :429-436)
 *   SDHIP_SEG_DICE_ENTROPY  (1/N) sum_b sum_c -D*Q, D = 10*([G > 1] - 2*TP/(P+G+1)), differentiated through D (diceEntropy, :439-448)
 * Three calls on one stream, sharing a caller-owned workspace of sdhip_seg_terms_workspace_bytes(B, hw, C) bytes (16-byte
 * aligned; < 0 for an unsupported shape; C <= 32), none of whose bytes need initialising:
 *   sdhip_seg_sums       one pass over logits and target; every workgroup STORES its partial sums into a slot of its own;
 *   sdhip_seg_finish     folds the slots in a fixed order in f64, does loss += the value of the active terms (ce_weight = 0:
 *                        no cross-entropy; terms: SDHIP_SEG_* bits; class_weights: C f32 on the device or NULL = all 1) and
 *                        writes the per-(b,c) gradient coefficients into the workspace;
 *   sdhip_seg_terms_bwd  WRITES grad = d(those terms)/d logits (grad != NULL; channels >= C of its pixel stride untouched).
 * No float atomics anywhere: value and gradient are bitwise reproducible. */
#define SDHIP_SEG_TVERSKY 1
#define SDHIP_SEG_DICE 2
#define SDHIP_SEG_DICE_ENTROPY 4
int sdhip_seg_terms_workspace_bytes(int B, long hw, int C);
int sdhip_seg_sums(const void* logits, int ldy, const float* target, int ldt, int B, long hw, int C, void* workspace,
                   long workspace_bytes, int dtype, void* stream);
int sdhip_seg_finish(void* workspace, long workspace_bytes, const float* class_weights, double* loss, int B, long hw, int C,
                     float ce_weight, int terms, void* stream);
int sdhip_seg_terms_bwd(const void* logits, int ldy, const float* target, int ldt, void* grad, int ldg, const void* workspace,
                        long workspace_bytes, int B, long hw, int C, int dtype, void* stream);
/* smoothing_gradients (util/utilTorchLoss.py:41-101), the `smooth_grad` term of lossDisp_fn (losses/multiLosses.py:143-146):
 * an edge-aware smoothness penalty on the predicted disparity d, gated by the one-hot target (values 0 or 1, at most one 1
 * per pixel; an all-zero row has no label).  With Y = 0.2126 R + 0.7152 G + 0.0722 B of the left image, Ys = Y filtered by
 * the 7x7, sigma 2 Gaussian (zero padding 3), M(p) = 1 iff p has a label and its eight neighbours lie inside the image and
 * carry the same label, w_v(p) = M(p) exp(1 - |Ys(y,x) - Ys(y+1,x)|), w_h(p) = M(p) exp(1 - |Ys(y,x) - Ys(y,x+1)|):
 *   loss += s * sum_p [ w_v(p) |d(y,x) - d(y+1,x)| + w_h(p) |d(y,x) - d(y,x+1)| ],   s = weight * 0.7 / (128 B H W)
 *   grad  = d(that)/d d, WRITTEN (not accumulated), with sgn(0) = 0; the image and the target get no gradient.
 * left: f32 ONLY (the image a step is fed, before any cast), channel c of pixel (y, x) of image b at
 *       left[b*left_bs + c*left_cs + (y*W + x)*left_ps]; channels 0..2 are read, later ones ignored.
 * target: f32, pixel stride ldt >= C (may be a channel slice of a wider slab), 1 <= C <= 32.
 * disp, grad: dense (B,1,H,W) of `dtype`.  H < 3 or W < 3: value 0, gradient 0.
 * One stencil launch that stores a f64 partial per workgroup into the workspace (sdhip_disp_smooth_workspace_bytes(B, H, W)
 * bytes, 8-byte aligned, no initialisation needed; < 0 for an unsupported shape) and a one-workgroup launch that folds the
 * partials in a fixed order: no float atomics, value and gradient are bitwise reproducible. */
long sdhip_disp_smooth_workspace_bytes(int B, int H, int W);
int sdhip_disp_smooth(const float* left, long left_bs, long left_cs, int left_ps, const float* target, int ldt,
                      const void* disp, int dtype, void* grad, double* loss, int B, int H, int W, int C, float weight,
                      void* workspace, long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Operators of the Ext_small edge networks (models/dsnet_t2_ext_small.py, output type `edgeOut`): csrc/edge.hip.
 * ------------------------------------------------------------------------- */
/* The edge map compute_grad_mag(img, True, False) (util/utilTorchGate.py:198-204) as upstream actually computes it: convTri
 * returns its input, the one-sided border differences are never recomputed, nothing is normalised.  Per channel, E read as 0
 * outside the image:  Ox = 0.5 (E(y,x+1) - E(y,x-1)),  Oy = 0.5 (E(y+1,x) - E(y-1,x)),  out = sqrt(Ox^2 + Oy^2 + 1e-6).
 * img: f32 or bf16 (in_dtype), channel c of pixel (y, x) of image b at img[b*img_bs + c*img_cs + (y*W + x)*img_ps] (NCHW,
 *      channels-last or a channel slice of either), 1 <= C <= 4, H and W >= 2.
 * out: f32 or bf16 (out_dtype), NHWC with pixel stride ldy >= C; channels C..ldy-1 are not written.  Arithmetic is f32.
 * One launch; the result does not depend on the layout of img.  No backward: the image carries no gradient. */
int sdhip_grad_mag(const void* img, long img_bs, long img_cs, long img_ps, int in_dtype, void* out, int ldy, int out_dtype,
                   int B, int H, int W, int C, void* stream);
/* lossEdge_fn (losses/multiLosses.py:166-182): the class-balanced binary cross-entropy of the edge head,
 *   loss += (1/n) sum_i w_i (max(z_i, 0) - z_i t_i + log1p(exp(-|z_i|))),   grad_i = w_i (sigmoid(z_i) - t_i) / n   (WRITTEN)
 * with w_i = N/(P+N) where t_i == 1, P/(P+N) where t_i == 0 and 0 for any other target value; P and N count the ones and
 * zeros of all n elements (exact integers), the quotients are formed in f32 as the reference forms them.  P = 0 or N = 0:
 * value and gradient are exactly 0.
 * logits: f32 or bf16 (dtype), element i at logits[i*ldz] (the head's output may sit in a padded pixel); target: dense f32;
 * grad: dense, of dtype.  Three launches (count, terms, fold) that keep integer counts and one f64 partial per workgroup in
 * the workspace (sdhip_edge_bce_workspace_bytes(n) bytes, 8-byte aligned, no initialisation needed; < 0 for n outside
 * [1, 2^40]): no float atomics, value and gradient are bitwise reproducible and independent of ldz and of alignment. */
long sdhip_edge_bce_workspace_bytes(long n);
int sdhip_edge_bce(const void* logits, long ldz, int dtype, const float* target, void* grad, double* loss, long n,
                   void* workspace, long workspace_bytes, void* stream);
/* y = cat(a * g, b * (1 - g)) along the channels (models/dsnet_t2_ext_small.py:361): a, b (npix, C), g (npix, 1), y ONE
 * (npix, 2C) buffer with pixel stride ldy >= 2C.  Backward: ga = gy[:, :C] * g, gb = gy[:, C:] * (1 - g),
 * gg[p] = sum_c (gy[p, c] a[p, c] - gy[p, C + c] b[p, c]), all WRITTEN, in one launch. */
int sdhip_gate_pair_fwd(const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* y, int ldy, long npix,
                        int C, int dtype, void* stream);
int sdhip_gate_pair_bwd(const void* gy, int ldgy, const void* a, int lda, const void* b, int ldb, const void* g, int ldg,
                        void* ga, int ldga, void* gb, int ldgb, void* gg, int ldgg, long npix, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Uncertainty-weighted multitask loss (`-multaskloss 1|2`: multiTask_loss, util/utilTorchLoss.py:521-540, called at
 * models/dsnet_t2.py:1167,1296).  Per-pixel maps, reduction='none':
 *   seg:  map[p] = exp(-lv) * CE(logits[p,:], labels[p]) + lv      (F.cross_entropy(..., ignore_index, reduction='none'))
 *   disp: map[p] = exp(-lv) * |pred[p] - target[p]| + lv           (F.l1_loss(..., reduction='none'), no validity mask)
 * log_var: the parameter, ONE f32 in device memory, read at every launch (no host synchronisation: a captured step's
 * replays see the value its Adam launch just wrote).  labels: int64 (B,H,W), dense.  A pixel whose label is
 * ignore_index (the reference passes 19 whatever the class count) has CE 0, so its map value is lv; a label outside
 * [0, C) is invalid input (the reference raises) and is treated here exactly like ignore_index, never read as an index.
 * map, lse, target, gmap: dense f32 per pixel.  The logits / grad rows may be channel slices (ld >= C): nothing past the
 * last pixel's channel C-1 is read, and only the C logical channels of a gradient row are written.
 * ------------------------------------------------------------------------- */
/* map, lse[p] = logsumexp(logits[p,:]) (kept for the backward pass), sum += sum_weight * sum_p map[p] (f64, ONE atomic
 * per workgroup: the caller clears sum, e.g. from the step's zero arena), and mean[0] = (float)*sum if mean != NULL
 * (sum_weight = 1/npix makes it the map's mean). */
int sdhip_mt_seg_fwd(const void* logits, int ldy, const int64_t* labels, const float* log_var, float* map, float* lse,
                     double* sum, float* mean, long npix, int C, int ignore_index, float sum_weight, int dtype, void* stream);
/* Upstream gradient of map[p]: gp = (gmap ? gmap[p * g_stride] : 0) + (gmean ? gmean[0] * gmean_scale : 0) — g_stride = 0
 * reads an expanded scalar without materialising it; gmean is the gradient of the mean the forward produced.
 * grad (optional) = gp * exp(-lv) * (softmax - onehot) for counted pixels, 0 for the others (written, not accumulated).
 * grad_log_var (optional) += sum_p gp * (1 - exp(-lv) * ce_p) (ACCUMULATED: a parameter-gradient slice). */
int sdhip_mt_seg_bwd(const void* logits, int ldy, const int64_t* labels, const float* lse, const float* log_var,
                     const float* gmap, long g_stride, const float* gmean, float gmean_scale, void* grad, int ldg,
                     float* grad_log_var, long npix, int C, int ignore_index, int dtype, void* stream);
/* The disparity term: pred with pixel stride ldp (a 1-channel map), target dense; sum / mean as sdhip_mt_seg_fwd. */
int sdhip_mt_l1_fwd(const void* pred, int ldp, const float* target, const float* log_var, float* map, double* sum,
                    float* mean, long n, float sum_weight, int dtype, void* stream);
/* grad (optional, pixel stride ldg) = gp * exp(-lv) * sign(pred - target), sign(0) = 0 as torch;
 * grad_log_var (optional) += sum_p gp * (1 - exp(-lv) * |pred - target|).  gp as sdhip_mt_seg_bwd. */
int sdhip_mt_l1_bwd(const void* pred, int ldp, const float* target, const float* log_var, const float* gmap, long g_stride,
                    const float* gmean, float gmean_scale, void* grad, int ldg, float* grad_log_var, long n, int dtype,
                    void* stream);

/* ---------------------------------------------------------------------------
 * PSMNet pieces (models_psmnet/stackhourglass.py:110-119,138-155; submodule.py:56-64).
 * ------------------------------------------------------------------------- */
/* scatter != 0: dst[n, d*sd, h*s, w*s, :] = src[n,d,h,w,:] into a zeroed (here) dense tensor of extent
 * ((D-1)*sd+1, (H-1)*s+1, (W-1)*s+1); scatter == 0: the gather back (dst dense-small, src stuffed).
 * Stride-s transposed convolutions and strided data gradients run as stride-1 convolutions over the stuffed tensor. */
int sdhip_stuff(const void* src, int ld_src, void* dst, int ld_dst, int N, int D, int H, int W, int C,
                int sd, int s, int scatter, int dtype, void* stream);
/* vol[b,i,h,w,0:C] = left[b,h,w,:], vol[b,i,h,w,C:2C] = right[b,h,w-i,:] for w >= i, else 0 (vol dense [B][D][H][W][2C]). */
int sdhip_cost_volume_fwd(const void* left, const void* right, int ld, void* vol, int B, int D, int H, int W, int C,
                          int dtype, void* stream);
int sdhip_cost_volume_bwd(const void* gvol, void* gleft, void* gright, int ld, int B, int D, int H, int W, int C,
                          int dtype, void* stream);
/* pred[b,h,w] = sum_d softmax_d(trilinear_upsample(cost)[b,d,h,w]) * d, cost [B][D4][H4][W4] -> (Dout,H,W),
 * align_corners=False (models_psmnet/stackhourglass.py:138-155, submodule.py:56-64); the (B,Dout,H,W) tensor is never
 * materialised.  stats (optional, only with Dout = 4 * D4): f32 [B*H*W][2] = (log-sum-exp, pred) per pixel, which spares the
 * backward pass the two softmax passes.  bwd: workspace of sdhip_softargmin_bwd_workspace_floats() floats; with
 * Dout = 4 * D4 it holds the per-pixel gradients of the D4 levels ([B][D4][H][W]), gathered into gcost without atomics. */
int sdhip_softargmin_fwd(const void* cost, void* pred, float* stats, int B, int D4, int H4, int W4, int Dout, int H, int W,
                         int dtype, void* stream);
long sdhip_softargmin_bwd_workspace_floats(int B, int D4, int H4, int W4, int Dout, int H, int W);
int sdhip_softargmin_bwd(const void* cost, const void* gpred, const float* stats, void* gcost, float* workspace,
                         long workspace_floats, int B, int D4, int H4, int W4, int Dout, int H, int W, int dtype, void* stream);
/* y = log_softmax(x) over the channel axis (F.log_softmax(.., dim=1), models/dsnet_t2.py:216,270) and its backward
 * gx = gy - exp(y) * sum_c gy. */
int sdhip_log_softmax_fwd(const void* x, int ldx, void* y, int ldy, long npix, int C, int dtype, void* stream);
int sdhip_log_softmax_bwd(const void* gy, int ldg, const void* y, int ldy, void* gx, int ldgx, long npix, int C,
                          int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Height-driven attention (HANet_Conv.forward, models_hanet/HANet.py:74-128) — the data-sized pieces; the tiny
 * (B, C, L) convolutions / BatchNorm1d / sigmoid / resize in between run through the conv / BN / resize entry points
 * on (B, C, L, 1) images.
 * rowpool_max: nn.AdaptiveMaxPool2d((OH, 1)) (HANet.py:50-55,84): y[b,i,c] = max over rows [floor(i*H/OH),
 *   ceil((i+1)*H/OH)) and all columns of x[b,:,:,c]; idx[b,i,c] = h*W+w of the first maximum (int32, dense [B][OH][C]).
 *   A NaN wins as in ATen's scan (`v > best || isnan(v)`): the bin's value is NaN and idx its last NaN.  bwd: gx[b,h,w,c] =
 *   sum of gy[b,i,c] over the bins i with idx[b,i,c] = h*W+w, written (only the C logical lanes of each gx pixel are touched).
 * mul_rows: torch.mul(out, attention.unsqueeze(3)) (HANet.py:112): y[b,h,w,c] = a[b,h,w,c] * att[b,h,c].
 * dropout_channels: nn.Dropout2d(p) on a (B, C, L) tensor (HANet.py:27-28,90-91): whole (b,c) rows dropped, rest scaled by
 *   1/(1-p); mask from a counter hash of (*seed, layer_id, b*C+c) — the same call on the gradient is the backward.
 * ------------------------------------------------------------------------- */
int sdhip_rowpool_max_fwd(const void* x, int ldx, void* y, int ldy, int* idx, int B, int H, int W, int C, int OH,
                          int dtype, void* stream);
int sdhip_rowpool_max_bwd(const void* gy, int ldg, const int* idx, void* gx, int ldgx, int B, int H, int W, int C, int OH,
                          int dtype, void* stream);
int sdhip_mul_rows_fwd(const void* a, int lda, const void* att, int ldt, void* y, int ldy, int B, int H, int W, int C,
                       int dtype, void* stream);
int sdhip_mul_rows_bwd(const void* g, int ldg, const void* a, int lda, const void* att, int ldt, void* ga, int ldga,
                       void* gatt, int ldgt, int B, int H, int W, int C, int dtype, void* stream);
int sdhip_dropout_channels(const void* x, int ldx, void* y, int ldy, const long* seed, long layer_id, int B, int L, int C,
                           float p, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * On-device step metrics: one pass over the step's outputs replaces the host-side block
 * of losses/multiLosses.py:116-125,146-154 — SegAccuracyNp (util/utilTorchLoss.py:221-236), GetSegMetricsNp
 * (:251-303), unnormalizedErrorNP (:363-370) and GetDispMetricsNp (:318-343) — which copies three full-resolution
 * maps to the host and runs numpy / sklearn on them every step.
 *   seg         (B*hw pixels, L logits, pixel stride lds) of `dtype`, or NULL
 *   seg_target  one-hot f32, Ct = L or L+1 channels (channel L = "ignore", mask `gt_seg != labels`), pixel stride ldt
 *   disp        dense B*hw disparities of `dtype`, or NULL;  disp_target dense f32
 *   mask_invalid  1: multiply prediction and target by (target > 0) first (`zeros` of lossDisp_fn for kitti/cityscapes)
 * ACCUMULATES (the caller zeroes once per reporting interval) into `nrep` replicas — workgroup g adds into replica
 * g % nrep, so that the closing atomics do not all serialise on one cache line; the caller sums the replicas.  Replica r
 * starts at counts + r*rep_stride (rep_stride >= L*L + SDHIP_METRIC_COUNTS) and sums + r*SDHIP_METRIC_SUM_STRIDE:
 *   counts[0 .. L*L)   confusion matrix, counts[L*gt + pred] over the pixels whose gt class != L
 *   counts[L*L + k], k < SDHIP_METRIC_COUNTS:
 *     0..3  image 0: TP, FP, FN, TN of (logit[1] > 0) against target[1]   (precision / recall / f1, average="micro")
 *     4,5   image 0: matching values and size of the branch mask (target[1] == 1 or raw logit[1] == 1)   (Bf1)
 *     6,7   whole batch: #(|pred - gt| * max_disp > 3 and gt > 0), #(gt > 0)                          (err, val_pxl)
 *     8     image 0: #(target[1] == 1)
 *     9     image 0: pixels scored by the disparity group (denominator of the RMSE / SqRel means)
 *   sums[k], k < SDHIP_METRIC_SUMS (f64): image 0: sum (gt-pred)^2, sum (gt-pred)^2/gt, and the same two over the
 *     pixels with target[1] == 1 (dispRMSE, dispSqRel, branch variants).
 * ------------------------------------------------------------------------- */
#define SDHIP_METRIC_COUNTS 10
#define SDHIP_METRIC_SUMS 4
#define SDHIP_METRIC_SUM_STRIDE 32   /* doubles per replica of `sums` (one 256-byte line) */
int sdhip_step_metrics(const void* seg, int lds, const float* seg_target, int ldt, int Ct, const void* disp,
                       const float* disp_target, long* counts, double* sums, int nrep, int rep_stride, int B, long hw,
                       int L, float max_disp, int mask_invalid, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * On-device sample preparation: everything CustomDataset.__getitem__ does after the PNG
 * containers are decoded (util/utilTorchDataLoader.py:133-274) — PFM decode + flipud (util/utilIOPfm.py:66-101),
 * depth -> disparity (:173-181), output activation (:188-197), one-hot target (:199-211; cityscapes table
 * util/utilCityscape.py:173-186), crop window (RandomCrop :435-463), (x/255 - mean)/std in float64 (:247-248) and the
 * HWC -> tensor conversion of ToTensor (:608-630) — in one launch per sample, writing one batch slot.
 *   left,right  uint8 H x W x img_cs (first 3 channels used), row pitch img_pitch bytes          -> out_left/out_right:
 *               out_h x out_w pixels of `dtype`, pixel stride ld_img (>= 3), value ((v/255 - mean[c]) / std[c])
 *   seg         uint8 H x W x seg_cs; channel seg_channel is classified by seg_mode:
 *               SDHIP_SEG_THRESHOLD (roses: class = v > seg_threshold), SDHIP_SEG_ID_PLUS_ONE (garden: class = v - 1),
 *               SDHIP_SEG_LUT (class = lut[v], a 256-byte device table; 255 there must already be mapped to n_seg - 1)
 *               -> out_seg f32 one-hot, n_seg channels, pixel stride ld_seg
 *   depth       SDHIP_DEPTH_PFM: the PFM payload (f32 rows, bottom row first, depth_pitch bytes apart, byte-swapped when
 *               depth_big_endian): disparity = depth > 0 ? fb / depth : 0;  SDHIP_DEPTH_U16: uint16 rows, disparity = v/256
 *               then activation: LINEAR none; SIGMOID min(d,max_d)/max_d; TANH d' = min(d,max_d), d' != 0 ? 2d'/max_d-1 : -1
 *               -> out_disp f32 dense out_h x out_w
 * row_roll (sliceandSwitch, RandomCrop :455-467): output row r is crop row (r + row_roll) mod out_h; 0 = off.
 * Any of the three groups may be NULL.  All pointers are device pointers; mean/std are HOST float[3].
 * ------------------------------------------------------------------------- */
#define SDHIP_SEG_THRESHOLD 0
#define SDHIP_SEG_ID_PLUS_ONE 1
#define SDHIP_SEG_LUT 2
#define SDHIP_DEPTH_PFM 0
#define SDHIP_DEPTH_U16 1
#define SDHIP_ACT_LINEAR 0
#define SDHIP_ACT_SIGMOID 1
#define SDHIP_ACT_TANH 2
int sdhip_prepare_sample(const unsigned char* left, const unsigned char* right, long img_pitch, int img_cs,
                         const unsigned char* seg, long seg_pitch, int seg_cs, int seg_channel, int seg_mode,
                         int seg_threshold, const unsigned char* lut, const void* depth, long depth_pitch,
                         int depth_mode, int depth_big_endian, int H, int W, int crop_top, int crop_left,
                         int out_h, int out_w, int row_roll, float fb, float max_d, int activation, const float* mean,
                         const float* stdv, void* out_left, void* out_right, int ld_img, float* out_seg,
                         int ld_seg, int n_seg, float* out_disp, int dtype, void* stream);

/* Horizontal flip of ONE prepared stereo sample, in place — RandomCrop(flipHorizontal=True) of
 * util/utilTorchDataLoader.py:476-499 (cityscapes): the two images are swapped and mirrored; every pixel of the disparity
 * and one-hot maps moves to column max(int(c - disp), 0) of its row (the largest source column wins a contested target,
 * untouched targets keep their content), the last 10 / 20 columns are cleared, pixels without disparity go to the void
 * channel (the last of n_seg), then both maps are mirrored.  left/right: H x W pixels of `dtype`, pixel stride ld_img;
 * seg: f32 one-hot, pixel stride ld_seg; disp: dense f32.  workspace: sdhip_flip_sample_workspace_bytes(H, W, n_seg). */
/* augment_DoubleLeftImg of RandomCrop (util/utilTorchDataLoader.py:469-474), in place on ONE prepared sample: left is
 * mirrored, right becomes the mirrored left, the one-hot map is mirrored, the disparity is 0.0001 everywhere. */
int sdhip_double_left_sample(void* left, void* right, int ld_img, float* seg, int ld_seg, int n_seg, float* disp, int H, int W,
                             int dtype, void* stream);
long sdhip_flip_sample_workspace_bytes(int H, int W, int n_seg);
int sdhip_flip_sample(void* left, void* right, int ld_img, float* seg, int ld_seg, int n_seg, float* disp, int H, int W,
                      void* workspace, long workspace_bytes, int dtype, void* stream);


/* ---------------------------------------------------------------------------
 * MobileNetV3-Large backbone (models/mobilenetv3.py, the default backbone of minidsnetExt, models/dsnet_t2.py:942,1935).
 *
 * Depthwise convolution nn.Conv2d(C, C, k, stride, (k-1)/2, groups=C, bias=False) of InvertedResidual
 * (models/mobilenetv3.py:99,110), k in {3, 5}, stride in {1, 2}, any H, W:
 *   y[b,oh,ow,c] = sum_{kh,kw} w[c][kh*k+kw] * x[b, oh*stride - p + kh, ow*stride - p + kw, c],  p = (k-1)/2.
 * w: the f32 parameter as stored, (C, 1, k, k).  x / y: NHWC with pixel strides ldx / ldy (channel slices allowed; the
 * channel tail is masked, pad lanes are never read).  Ho = (H + 2p - k)/stride + 1.
 * stats (optional, f64 [nrep][groups][2][sld], zeroed by the caller): per statistics group (sum, sum of squares) of the
 * stored output, for the BatchNorm behind it (sdhip_affine_act_bn).  pool (optional, f32 [B][pool_parts][C], zeroed by the
 * caller, pool_parts >= sdhip_dw_pool_parts): partial per-image channel sums of the stored output, one slot per workgroup
 * (slots no workgroup writes stay zero) — the global average pool of SELayer (models/mobilenetv3.py:73), since the
 * BatchNorm in between is affine per channel; sdhip_se_fwd adds the slots in a fixed order, so the pool is deterministic. */
int sdhip_dw_conv_fwd(const void* x, int ldx, const float* w, void* y, int ldy, double* stats, int sld, int nrep, float* pool,
                      int pool_parts, int B, int H, int W, int C, int k, int stride, int groups, int dtype, void* stream);
/* Pool slots sdhip_dw_conv_fwd needs for an (H, W, C) input (< 0: unsupported k / stride / shape).  Host only. */
int sdhip_dw_pool_parts(int H, int W, int C, int k, int stride, int dtype);
/* Data gradient of sdhip_dw_conv_fwd: gx[b,ih,iw,c] = sum over the taps that reach (ih, iw) of gy * w (stride 2: at most
 * ceil(k/2)^2 taps per input pixel, gathered; no zero-stuffing, no atomics).  gx is overwritten. */
int sdhip_dw_conv_dgrad(const void* gy, int ldg, const float* w, void* gx, int ldgx,
                        int B, int H, int W, int C, int k, int stride, int dtype, void* stream);
/* Weight gradient of sdhip_dw_conv_fwd, ADDED to dw (C, 1, k, k) f32 — a slice of the flat gradient buffer or a zeroed
 * tensor.  part: f32 workspace of nparts * k*k * C floats (nparts = sdhip_dw_wgrad_parts; no initialisation needed): every
 * workgroup stores its partial sums there, a second launch adds them in a fixed order — no atomics, deterministic. */
int sdhip_dw_conv_wgrad(const void* x, int ldx, const void* gy, int ldg, float* dw, float* part, int nparts,
                        int B, int H, int W, int C, int k, int stride, int dtype, void* stream);
/* Partial slots of sdhip_dw_conv_wgrad for this shape (< 0: unsupported).  Host only. */
int sdhip_dw_wgrad_parts(int B, int H, int W, int C, int k, int stride);
/* Dilated depthwise 3x3 of DeepLabV3+ / Xception-65 (models_deeplab_mod/common.py:24-50 SeparableConv2d):
 * nn.Conv2d(C, C, 3, stride, padding=dil, dilation=dil, groups=C, bias=False), stride in {1, 2}, any dil >= 1, any H, W, C:
 *   y[b,oh,ow,c] = sum_{kh,kw} w[c][kh*3+kw] * f(x[b, oh*stride + (kh-1)*dil, ow*stride + (kw-1)*dil, c]),
 * f = relu when in_relu != 0 (relu_first: rectified in the load, x itself stays as it is), identity otherwise;
 * Ho = (H-1)/stride + 1.  Taps outside the map are skipped, not loaded.  Layout, w, stats as sdhip_dw_conv_fwd; the channel
 * tail is masked on the 16-byte path too (C need not be a multiple of the chunk; pad lanes are never read or written). */
int sdhip_dw_dil_conv_fwd(const void* x, int ldx, const float* w, void* y, int ldy, double* stats, int sld, int nrep,
                          int B, int H, int W, int C, int stride, int dil, int in_relu, int groups, int dtype, void* stream);
/* Data gradient of sdhip_dw_dil_conv_fwd, gathered (no atomics); gx is overwritten.  x (optional): the forward's input when
 * it ran with in_relu — the gradient is multiplied by [x > 0] in the same launch. */
int sdhip_dw_dil_conv_dgrad(const void* gy, int ldg, const float* w, const void* x, int ldx, void* gx, int ldgx,
                            int B, int H, int W, int C, int stride, int dil, int dtype, void* stream);
/* Weight gradient of sdhip_dw_dil_conv_fwd, ADDED to dw (C, 1, 3, 3) f32; it sees relu(x) when in_relu != 0.  part: f32
 * workspace of nparts * 9 * C floats (nparts = sdhip_dw_dil_wgrad_parts; no initialisation needed), folded in a fixed
 * order as in sdhip_dw_conv_wgrad: deterministic. */
int sdhip_dw_dil_conv_wgrad(const void* x, int ldx, const void* gy, int ldg, float* dw, float* part, int nparts,
                            int B, int H, int W, int C, int stride, int dil, int in_relu, int dtype, void* stream);
/* Partial slots of sdhip_dw_dil_conv_wgrad for this shape (< 0: unsupported).  Host only. */
int sdhip_dw_dil_wgrad_parts(int B, int H, int W, int C, int stride);
/* SELayer excitation (models/mobilenetv3.py:64-77): v[b,c] = (sum_p pool[b][p][c])*inv_hw*scale[g][c] + shift[g][c]
 * (pool: the pool_parts slots of sdhip_dw_conv_fwd, added in slot order; scale / shift:
 * the BatchNorm in front, g = b / (B/groups); NULL: identity), h = relu(w1 v + b1), a = w2 h + b2, s = h_sigmoid(a).
 * w1 (r, C), b1 (r), w2 (C, r), b2 (C): the two nn.Linear parameters, f32.  Writes s [B][C] and the saved activations
 * ws = [v (B*C) | h (B*r) | a (B*C)] f32.  One launch; the multiply x * s[b,c] is sdhip_affine_act with groups = B. */
int sdhip_se_fwd(const float* pool, int pool_parts, float inv_hw, const float* scale, const float* shift, int groups,
                 const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* ws,
                 int B, int C, int r, void* stream);
/* Backward of sdhip_se_fwd given ds = dL/ds as the f32 replica sums [nrep][B][C] of sdhip_affine_act_bwd (groups = B):
 * ADDS the four parameter gradients to gw1 / gb1 / gw2 / gb2 (f32 atomics) and writes gpool[b][c] = dL/dv[b,c] * inv_hw,
 * the term every pixel of image b adds to the gradient of the pooled tensor.  One launch. */
int sdhip_se_bwd(const float* ds, int nrep, const float* ws, const float* w1, const float* w2,
                 float* gw1, float* gb1, float* gw2, float* gb2, float* gpool, float inv_hw, int B, int C, int r, void* stream);
/* gx = gy * act'(x * s[b][c]) * s[b][c] + gadd[b][c]: the data gradient of y = act(x * s) (sdhip_affine_act with
 * groups = B) plus the pooled path of SELayer.  act: 0, 1, SDHIP_ACT_HSWISH or SDHIP_ACT_HSIGMOID; B images of npix_img. */
int sdhip_se_scale_bwd(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx, const float* s, const float* gadd,
                       long npix_img, int B, int C, int act, int dtype, void* stream);


/* ---------------------------------------------------------------------------
 * Disparity warp and gated blend of the warp networks (models/torch_dsnet.py:10-86 apply_disparity, wrap_mode='edge';
 * models/dsnet_t2_warp.py minidsnetDivide / minidsnetDivideSoftmax).  For output pixel (b, y, j), all in f32:
 *   x = clamp(j + offset_sign * disp[b,y,j], 0, W-1),  x0 = floor(x),  x1 = min(x0 + 1, W-1)
 *   warped[b,y,j,c] = (x1 - x) * seg_right[b,y,x0,c] + (x - x0) * seg_right[b,y,x1,c]
 *   both[b,y,j,c]   = (1 - a) * seg_left[b,y,j,c] + a * warped[b,y,j,c]
 * As in the reference, x == W-1 makes both weights 0: the right edge (and every pixel clamped to it) is 0; a pixel clamped
 * on the left copies column 0.  All maps are NHWC with a pixel stride ld* >= their channel count (pad lanes are never
 * touched); disp is one channel of `dtype` with pixel stride ldd, widened to f32; offset_sign is +1 (apply_disparity) or
 * -1 (the networks warp with -disp).
 * gate (optional): NULL = plain apply_disparity, seg_left / both / prob must be NULL and gate_ch 0.  Otherwise gate_ch is 1
 * (one blend weight per pixel) or C (one per channel); with gate_softmax != 0 (gate_ch == C) `gate` holds RAW scores, the
 * kernel takes their softmax over the channels, writes it to prob and blends with it.  One launch. */
int sdhip_warp_blend_fwd(const void* seg_left, int ldl, const void* seg_right, int ldr, const void* disp, int ldd,
                         float offset_sign, const void* gate, int ldgt, int gate_ch, int gate_softmax, void* warped, int ldw,
                         void* both, int ldb, void* prob, int ldp, int B, int H, int W, int C, int dtype, void* stream);
/* Backward of sdhip_warp_blend_fwd from g_both and / or g_warped (either may be NULL; g_both needs a gate).  `gate` holds
 * the blend weights the forward pass used: its gate input, or its prob output when gate_softmax != 0.  Outputs, each
 * optional and overwritten:
 *   g_left  = (1 - a) * g_both
 *   g_gate  = g_both * (warped - seg_left), summed over the channels for gate_ch == 1; with gate_softmax the gradient
 *             w.r.t. the raw scores, p_c * (g_c - sum_k g_k p_k)
 *   g_disp  = offset_sign * sum_c gw_c * (seg_right[x1] - seg_right[x0]) where 0 <= j + offset <= W-1 (bounds included),
 *             0 where the clamp is active;  gw = g_warped + a * g_both
 *   g_right = the adjoint of the row gather: gw * (x1 - x) added at x0, gw * (x - x0) added at x1.
 * Two launches: the per-pixel pass, then one workgroup per image row and channel group that accumulates g_right in LDS
 * (float LDS atomics in an 80 KB accumulator, W <= 20480) and stores it once — no global atomics, no workspace.  The order of the LDS adds is not
 * fixed: g_right repeats to f32 rounding, not bit for bit; everything else is deterministic. */
int sdhip_warp_blend_bwd(const void* g_both, int ldgb, const void* g_warped, int ldgw, const void* seg_left, int ldl,
                         const void* seg_right, int ldr, const void* disp, int ldd, float offset_sign, const void* gate, int ldgt,
                         int gate_ch, int gate_softmax, void* g_left, int ldgl, void* g_right, int ldgr, void* g_disp, int ldgd,
                         void* g_gate, int ldgg, int B, int H, int W, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------
 * Operators of minidsnetDivideDisp / minidsnetDivideDisp2 (models/dsnet_t2_warp.py:704-972; `-net dsnet_warp_disp`,
 * `dsnet_warp_disp_consist`).
 *
 * sdhip_warp_image_masked: the image the third tower pass of minidsnetDivideDisp reads (:811),
 *   out[b,y,j,c] = [gt[b,y,j] > 0] * apply_disparity(img, -gt)[b,c,y,j]
 * with the coordinate arithmetic and edge rules of sdhip_warp_blend_fwd (offset_sign -1): a sample at or beyond the right edge
 * is 0, one clamped on the left copies column 0.  img: f32 or bf16 (in_dtype), read through its batch / channel / pixel
 * strides in elements (rows follow one another pixel by pixel: NCHW, channels-last or a channel slice of either; no copy);
 * gt: dense f32 [B][H][W]; out: NHWC of out_dtype with pixel stride ldy >= C, 1 <= C <= 4, pad lanes are not written.
 * One launch, f32 arithmetic, forward only; the result does not depend on the image's layout. */
int sdhip_warp_image_masked(const void* img, long img_bs, long img_cs, long img_ps, int in_dtype, const float* gt, void* out, int ldy,
                            int out_dtype, int B, int H, int W, int C, void* stream);

/* y = (1 - g) * a + g * b for NHWC maps a, b, y of C channels and a one-channel gate g (pixel strides lda, ldb, ldy >= C,
 * ldg >= 1; pad lanes are never touched): the unwarped blend of the *_disp networks (:834).  One launch. */
int sdhip_gate_blend_fwd(const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* y, int ldy, long npix, int C,
                         int dtype, void* stream);
/* ga = (1 - g) * gy, gb = g * gy, gg = sum_c gy_c * (b_c - a_c) (f32 sum); all three are written.  One launch. */
int sdhip_gate_blend_bwd(const void* gy, int ldgy, const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* ga,
                         int ldga, void* gb, int ldgb, void* gg, int ldgg, long npix, int C, int dtype, void* stream);

/* Photometric term of the `ThreeOutPutsDispConsist` step (torch_implementation.py:314-317), MSELoss(warped, left):
 *   loss[0] += weight * mean_{b,c,y,x} (w - l)^2,      grad = 2 * weight * (w - l) / (B*C*H*W)   (WRITTEN, dense NHWC, w's dtype)
 * w: the warped image, NHWC of `dtype` with pixel stride ldw >= C; l: the f32 left image read through its batch / channel / pixel
 * strides (as sdhip_warp_image_masked reads img); 1 <= C <= 4.  Every thread sums its terms in f64, every workgroup stores one f64
 * partial in a slot of its own in the workspace (sdhip_photo_mse_workspace_bytes(npix) bytes, 8-byte aligned, no initialisation
 * needed; < 0 for npix outside 1 .. 2^40) and a one-workgroup launch folds the slots in slot order into loss[0]: no float atomics,
 * value and gradient repeat bit for bit and do not depend on any stride.  Two launches. */
long sdhip_photo_mse_workspace_bytes(long npix);
int sdhip_photo_mse(const void* w, int ldw, int dtype, const float* l, long l_bs, long l_cs, long l_ps, void* grad, double* loss,
                    float weight, int B, int H, int W, int C, void* workspace, long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDHIP_H_ */
