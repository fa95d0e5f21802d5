// Region-overlap and class-weighted terms of the segmentation loss for gfx950: dice_loss, diceEntropy, tversky_loss2
// (util/utilTorchLoss.py:407-448) and categoricalCrossEntropy with a class-weight table (:373-378), as lossSeg_fn adds them
// (losses/multiLosses.py:44-115).  Every one of them is a function of four sums per (image b, class c) over the image's
// pixels, with p = softmax_c(z), lp = log_softmax_c(z), T the one-hot target:
//     TP = sum T*p     P = sum p     G = sum T     Q = sum T*lp
// so the family costs three launches, whatever the list:
//   1. seg_sums_kernel    one pass over logits + target; every workgroup reduces its slab (registers -> wave shuffle -> LDS) and
//                         STORES its 4*C partial sums into a slot of its own (no float atomics: the result is reproducible);
//   2. seg_finish_kernel  one workgroup folds the slots in slot order in f64, adds the active terms' value to the step's f64
//                         loss scalar and writes the coefficient table [B][C][3] = (a = dL/dTP, b = dL/dP, d = factor on -T*lp);
//   3. seg_bwd_kernel     one elementwise pass: with q_c = a_c*T_c + b_c,
//                         g_k = p_k*(q_k - sum_c q_c p_c)  +  p_k * sum_c T_c d_c - T_k d_k.
// Weighted cross-entropy and diceEntropy are the same elementwise form (d = w1*w_c/N and d = D_bc/N), so plain CE with a
// weight table needs no kernel of its own.
//
// Pixel rows travel through LDS as in the many-class cross-entropy (rows_lds.h): 16-byte coalesced global accesses, then one
// lane owns one pixel and keeps its C <= 32 logits / exponentials in registers.
#include "sdhip_common.h"
#include "rows_lds.h"

namespace {

constexpr int SEG_MAX_C = 32;
constexpr int SEG_MAX_SLOTS = 1024;        // slots of all images together: bounds the fold and the workspace
constexpr size_t SEG_LDS_BUDGET = 60 * 1024;

// workgroups (= slots) per image
inline int seg_parts(int B, long hw) {
  const long tiles = (hw + 255) / 256;
  long cap = SEG_MAX_SLOTS / B;
  if (cap < 1) cap = 1;
  return (int)(tiles < cap ? tiles : cap);
}
inline size_t seg_slot_bytes(int B, long hw, int C) { return (((size_t)B * seg_parts(B, hw) * 4 * C * sizeof(double)) + 15) & ~(size_t)15; }
inline size_t seg_ws_bytes(int B, long hw, int C) { return seg_slot_bytes(B, hw, C) + (size_t)B * C * 3 * sizeof(float); }

// one pixel: z - max in zc[], exp(z - max) in e[], returns the sum of the exponentials (channels >= C: zc = 0, e = 0)
template <typename T, int CP>
__device__ __forceinline__ float seg_softmax_row(const T* __restrict__ yp, int C, float (&zc)[CP], float (&e)[CP]) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < CP; ++c) { zc[c] = c < C ? Elem<T>::ld(yp + c) : -INFINITY; mx = fmaxf(mx, zc[c]); }
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    zc[c] = c < C ? zc[c] - mx : 0.f;
    e[c] = c < C ? expf(zc[c]) : 0.f;
    se += e[c];
  }
  return se;
}

// slots[((b*parts + j)*4 + k)*C + c], k = 0 TP, 1 P, 2 G, 3 Q: the sums of workgroup j of image b over its tiles j, j + parts, ...
// Dynamic LDS: [logit rows | target rows | 4 waves x 4*CP floats]; STAGE = false reads the rows from global memory (a row
// stride too wide for LDS, or an image whose first byte is not 4-byte aligned).
template <typename T, int CP, bool STAGE>
__global__ __launch_bounds__(256) void seg_sums_kernel(const T* __restrict__ y, int ldy, const float* __restrict__ t, int ldt,
                                                       double* __restrict__ slots, long hw, int C, int parts, int off_t, int off_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
  T* const ly = reinterpret_cast<T*>(rsm);
  float* const lt = reinterpret_cast<float*>(rsm + off_t);
  float* const red = reinterpret_cast<float*>(rsm + off_r);
  const int tid = threadIdx.x, b = blockIdx.y;
  const long ntiles = (hw + 255) / 256;
  y += (long)b * hw * ldy;
  t += (long)b * hw * ldt;
  float acc[4][CP];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[k][c] = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += parts) {
    const long p0 = tile * 256;
    const int n = (int)min(256L, hw - p0);
    if constexpr (STAGE) {
      // (the tensor's very last row is read up to its last channel only: a channel slice may end with the buffer)
      const bool last = b == (int)gridDim.y - 1 && p0 + n == hw;
      rows_to_lds(y + p0 * ldy, ly, (last ? (n - 1) * ldy + C : n * ldy) * (int)sizeof(T), tid);
      rows_to_lds(t + p0 * ldt, lt, (last ? (n - 1) * ldt + C : n * ldt) * 4, tid);
      __syncthreads();
    }
    if (tid < n) {
      const T* yp = STAGE ? ly + tid * ldy : y + (p0 + tid) * ldy;
      const float* tp = STAGE ? lt + tid * ldt : t + (p0 + tid) * ldt;
      float zc[CP], e[CP];
      const float se = seg_softmax_row<T, CP>(yp, C, zc, e);
      const float inv = 1.f / se, lse = logf(se);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        if (c < C) {
          const float tc = tp[c], p = e[c] * inv;
          acc[0][c] += tc * p;
          acc[1][c] += p;
          acc[2][c] += tc;
          acc[3][c] += tc * (zc[c] - lse);
        }
      }
    }
    if constexpr (STAGE) __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const float s = wave_sum(acc[k][c]);
      if ((tid & 63) == 0) red[(tid >> 6) * 4 * CP + k * CP + c] = s;
    }
  __syncthreads();
  if (tid < 4 * CP) {
    const int k = tid / CP, c = tid % CP;
    if (c < C) {
      double s = 0.0;
      for (int w = 0; w < 4; ++w) s += (double)red[w * 4 * CP + tid];      // wave order: fixed
      slots[(((long)b * parts + blockIdx.x) * 4 + k) * C + c] = s;
    }
  }
}

// One workgroup.  Thread i serves the (b, c) pairs i, i + 256, ...: slot fold in slot order, the terms' values and coefficients
// in f64; the 256 thread sums are added in thread order, so the value is reproducible too.
__global__ __launch_bounds__(256) void seg_finish_kernel(const double* __restrict__ slots, float* __restrict__ coef,
                                                         const float* __restrict__ cw, double* __restrict__ loss, int B, long hw,
                                                         int C, int parts, float ce_weight, int terms) {
  __shared__ double sh[256];
  const double N = (double)B * (double)hw, BC = (double)B * C;
  double acc = 0.0;
  for (int i = threadIdx.x; i < B * C; i += 256) {
    const int b = i / C, c = i % C;
    double TP = 0.0, P = 0.0, G = 0.0, Q = 0.0;
    for (int j = 0; j < parts; ++j) {
      const double* s = slots + ((long)b * parts + j) * 4 * C + c;
      TP += s[0]; P += s[C]; G += s[2 * C]; Q += s[3 * C];
    }
    const double w = cw ? (double)cw[c] : 1.0;
    double a = 0.0, bb = 0.0, d = 0.0, val = 0.0;
    if (ce_weight != 0.f) {                      // w1 * mean_pix sum_c -T*lp*w_c
      const double dc = (double)ce_weight * w / N;
      d += dc;
      val -= dc * Q;
    }
    if (terms & SDHIP_SEG_TVERSKY) {             // 1.5 * mean_c(w_c * mean_b(1 - TP / (TP + FN + 0.3 FP + 1e-6)))
      const double den = G + 0.3 * (P - TP) + 1e-6, k = 1.5 * w / BC;
      val += k * (1.0 - TP / den);
      a -= k * (den + 0.3 * TP) / (den * den);
      bb += k * 0.3 * TP / (den * den);
    }
    const double S = P + G + 1.0, dl = (G > 1.0 ? 1.0 : 0.0) - 2.0 * TP / S;
    if (terms & SDHIP_SEG_DICE) {                // mean_{b,c}([G > 1] - 2 TP / (P + G + 1))
      const double k = 1.0 / BC;
      val += k * dl;
      a -= 2.0 * k / S;
      bb += 2.0 * k * TP / (S * S);
    }
    if (terms & SDHIP_SEG_DICE_ENTROPY) {        // mean_pix sum_c -T*lp*D_bc, D = 10 * dice term, differentiated through D too
      const double D = 10.0 * dl;
      d += D / N;
      val -= D / N * Q;
      a += 20.0 * Q / (N * S);
      bb -= 20.0 * Q * TP / (N * S * S);
    }
    coef[3 * i] = (float)a; coef[3 * i + 1] = (float)bb; coef[3 * i + 2] = (float)d;
    acc += val;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += sh[i];
    loss[0] += tot;                              // stream order makes this the only writer
  }
}

// gy[p, k] = p_k*(q_k - sum_c q_c p_c + sum_c T_c d_c) - T_k d_k.  Dynamic LDS: [logit rows | target rows | gradient rows |
// 3*CP coefficients]; the gradient rows are staged only when gy is dense (ldg == C), so pad channels of a wider pixel stride
// are never written.
template <typename T, int CP, bool STAGE>
__global__ __launch_bounds__(256) void seg_bwd_kernel(const T* __restrict__ y, int ldy, const float* __restrict__ t, int ldt,
                                                      T* __restrict__ gy, int ldg, const float* __restrict__ coef, long hw, int C,
                                                      int off_t, int off_g, int off_c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
  T* const ly = reinterpret_cast<T*>(rsm);
  float* const lt = reinterpret_cast<float*>(rsm + off_t);
  T* const lg = reinterpret_cast<T*>(rsm + off_g);
  float* const lc = reinterpret_cast<float*>(rsm + off_c);
  const int tid = threadIdx.x, b = blockIdx.y;
  const long ntiles = (hw + 255) / 256;
  y += (long)b * hw * ldy;
  t += (long)b * hw * ldt;
  gy += (long)b * hw * ldg;
  if (tid < 3 * C) lc[tid] = coef[(long)b * C * 3 + tid];
  __syncthreads();
  float ca[CP], cb[CP], cd[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    ca[c] = c < C ? lc[3 * c] : 0.f;
    cb[c] = c < C ? lc[3 * c + 1] : 0.f;
    cd[c] = c < C ? lc[3 * c + 2] : 0.f;
  }
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * 256;
    const int n = (int)min(256L, hw - p0);
    if constexpr (STAGE) {
      // (the tensor's very last row is read up to its last channel only: a channel slice may end with the buffer)
      const bool last = b == (int)gridDim.y - 1 && p0 + n == hw;
      rows_to_lds(y + p0 * ldy, ly, (last ? (n - 1) * ldy + C : n * ldy) * (int)sizeof(T), tid);
      rows_to_lds(t + p0 * ldt, lt, (last ? (n - 1) * ldt + C : n * ldt) * 4, tid);
      __syncthreads();
    }
    if (tid < n) {
      const T* yp = STAGE ? ly + tid * ldy : y + (p0 + tid) * ldy;
      const float* tp = STAGE ? lt + tid * ldt : t + (p0 + tid) * ldt;
      T* gp = STAGE ? lg + tid * ldg : gy + (p0 + tid) * ldg;
      float zc[CP], e[CP];
      const float se = seg_softmax_row<T, CP>(yp, C, zc, e);
      const float inv = 1.f / se;
      float sq = 0.f, sd = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float tc = c < C ? tp[c] : 0.f;
        e[c] *= inv;                              // p_c
        zc[c] = tc;                               // (the logits are no longer needed: keep the target row instead)
        sq += (ca[c] * tc + cb[c]) * e[c];
        sd += tc * cd[c];
      }
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) Elem<T>::st(gp + c, e[c] * (ca[c] * zc[c] + cb[c] - sq + sd) - zc[c] * cd[c]);
    }
    if constexpr (STAGE) {
      __syncthreads();
      rows_from_lds(gy + p0 * ldg, lg, n * ldg * (int)sizeof(T), tid);
      __syncthreads();
    }
  }
}

// channel count of the register rows: 2, or C rounded up to a multiple of 4
inline int seg_cp(int C) { return C <= 2 ? 2 : (C + 3) & ~3; }

// rows of an image can be staged through LDS: every image starts 4-byte aligned
inline bool seg_rows_aligned(const void* p, int B, long hw, int ld, int es) {
  return (((uintptr_t)p) & 3) == 0 && (B == 1 || ((hw * ld * es) & 3) == 0);
}

template <typename T, int CP>
void seg_sums_launch(const void* y, int ldy, const float* t, int ldt, double* slots, int B, long hw, int C, hipStream_t s) {
  const int parts = seg_parts(B, hw);
  const size_t by = rows_lds_bytes(ldy, sizeof(T)), bt = rows_lds_bytes(ldt, 4), br = (size_t)4 * 4 * CP * sizeof(float);
  const dim3 grid((unsigned)parts, (unsigned)B);
  if (by + bt + br <= SEG_LDS_BUDGET && seg_rows_aligned(y, B, hw, ldy, sizeof(T)))
    hipLaunchKernelGGL((seg_sums_kernel<T, CP, true>), grid, dim3(256), by + bt + br, s, (const T*)y, ldy, t, ldt, slots, hw, C, parts,
                       (int)by, (int)(by + bt));
  else
    hipLaunchKernelGGL((seg_sums_kernel<T, CP, false>), grid, dim3(256), br, s, (const T*)y, ldy, t, ldt, slots, hw, C, parts, 0, 0);
}

template <typename T, int CP>
void seg_bwd_launch(const void* y, int ldy, const float* t, int ldt, void* gy, int ldg, const float* coef, int B, long hw, int C,
                    hipStream_t s) {
  const size_t by = rows_lds_bytes(ldy, sizeof(T)), bt = rows_lds_bytes(ldt, 4), bg = rows_lds_bytes(ldg, sizeof(T));
  const size_t bc = (size_t)3 * CP * sizeof(float);
  long gx = (hw + 255) / 256, cap = 2048 / B;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)B);
  if (ldg == C && by + bt + bg + bc <= SEG_LDS_BUDGET && seg_rows_aligned(y, B, hw, ldy, sizeof(T)) &&
      seg_rows_aligned(gy, B, hw, ldg, sizeof(T)))
    hipLaunchKernelGGL((seg_bwd_kernel<T, CP, true>), grid, dim3(256), by + bt + bg + bc, s, (const T*)y, ldy, t, ldt, (T*)gy, ldg, coef,
                       hw, C, (int)by, (int)(by + bt), (int)(by + bt + bg));
  else
    hipLaunchKernelGGL((seg_bwd_kernel<T, CP, false>), grid, dim3(256), bc, s, (const T*)y, ldy, t, ldt, (T*)gy, ldg, coef, hw, C, 0, 0, 0);
}

// width of the register rows, seg_cp(C) -> template argument: f(std::integral_constant<int, CP>)
template <typename F>
void seg_by_cp(int C, F&& f) {
  switch (seg_cp(C)) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 20: return f(std::integral_constant<int, 20>{});
    case 24: return f(std::integral_constant<int, 24>{});
    case 28: return f(std::integral_constant<int, 28>{});
    default: return f(std::integral_constant<int, 32>{});
  }
}

inline bool seg_shape_ok(int B, long hw, int C) { return B > 0 && B <= 65535 && hw > 0 && C > 0 && C <= SEG_MAX_C && (long)B * C <= (1L << 20); }

}  // namespace

extern "C" int sdhip_seg_terms_workspace_bytes(int B, long hw, int C) {
  if (!seg_shape_ok(B, hw, C)) return SDHIP_ERR_ARG;
  return (int)seg_ws_bytes(B, hw, C);
}

extern "C" int sdhip_seg_sums(const void* logits, int ldy, const float* target, int ldt, int B, long hw, int C, void* workspace,
                              long workspace_bytes, int dtype, void* stream) {
  SDHIP_CHECK_ARG(logits && target && workspace, "seg_sums: null pointer");
  SDHIP_CHECK_ARG(seg_shape_ok(B, hw, C), "seg_sums: B %d, %ld pixels per image, C %d (1 <= C <= %d)", B, hw, C, SEG_MAX_C);
  SDHIP_CHECK_ARG(ldy >= C && ldt >= C, "seg_sums: pixel strides %d / %d below C = %d", ldy, ldt, C);
  SDHIP_CHECK_DTYPE("seg_sums", dtype);
  SDHIP_CHECK_ARG(workspace_bytes >= (long)seg_ws_bytes(B, hw, C) && (((uintptr_t)workspace) & 15) == 0,
                  "seg_sums: workspace of %ld bytes (16-byte aligned), %ld needed", workspace_bytes, (long)seg_ws_bytes(B, hw, C));
  hipStream_t s = (hipStream_t)stream;
  double* slots = (double*)workspace;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    seg_by_cp(C, [&](auto CP) { seg_sums_launch<T, CP()>(logits, ldy, target, ldt, slots, B, hw, C, s); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_seg_finish(void* workspace, long workspace_bytes, const float* class_weights, double* loss, int B, long hw,
                                int C, float ce_weight, int terms, void* stream) {
  SDHIP_CHECK_ARG(workspace && loss, "seg_finish: null pointer");
  SDHIP_CHECK_ARG(seg_shape_ok(B, hw, C), "seg_finish: B %d, %ld pixels per image, C %d (1 <= C <= %d)", B, hw, C, SEG_MAX_C);
  SDHIP_CHECK_ARG((terms & ~(SDHIP_SEG_TVERSKY | SDHIP_SEG_DICE | SDHIP_SEG_DICE_ENTROPY)) == 0, "seg_finish: unknown term bits %d", terms);
  SDHIP_CHECK_ARG(workspace_bytes >= (long)seg_ws_bytes(B, hw, C) && (((uintptr_t)workspace) & 15) == 0,
                  "seg_finish: workspace of %ld bytes (16-byte aligned), %ld needed", workspace_bytes, (long)seg_ws_bytes(B, hw, C));
  float* coef = (float*)((unsigned char*)workspace + seg_slot_bytes(B, hw, C));
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, coef, class_weights, loss,
                     B, hw, C, seg_parts(B, hw), ce_weight, terms);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_seg_terms_bwd(const void* logits, int ldy, const float* target, int ldt, void* grad, int ldg,
                                   const void* workspace, long workspace_bytes, int B, long hw, int C, int dtype, void* stream) {
  SDHIP_CHECK_ARG(logits && target && grad && workspace, "seg_terms_bwd: null pointer");
  SDHIP_CHECK_ARG(seg_shape_ok(B, hw, C), "seg_terms_bwd: B %d, %ld pixels per image, C %d (1 <= C <= %d)", B, hw, C, SEG_MAX_C);
  SDHIP_CHECK_ARG(ldy >= C && ldt >= C && ldg >= C, "seg_terms_bwd: pixel strides %d / %d / %d below C = %d", ldy, ldt, ldg, C);
  SDHIP_CHECK_DTYPE("seg_terms_bwd", dtype);
  SDHIP_CHECK_ARG(workspace_bytes >= (long)seg_ws_bytes(B, hw, C) && (((uintptr_t)workspace) & 15) == 0,
                  "seg_terms_bwd: workspace of %ld bytes (16-byte aligned), %ld needed", workspace_bytes, (long)seg_ws_bytes(B, hw, C));
  hipStream_t s = (hipStream_t)stream;
  const float* coef = (const float*)((const unsigned char*)workspace + seg_slot_bytes(B, hw, C));
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    seg_by_cp(C, [&](auto CP) { seg_bwd_launch<T, CP()>(logits, ldy, target, ldt, grad, ldg, coef, B, hw, C, s); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
