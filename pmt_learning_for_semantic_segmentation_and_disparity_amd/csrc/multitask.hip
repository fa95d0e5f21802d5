// Uncertainty-weighted multitask loss (`-multaskloss`, util/utilTorchLoss.py:521-540, multiTask_loss): per-pixel maps
//   seg:  exp(-lv) * CE(logits, label, ignore_index, reduction='none') + lv         (B,H,W)
//   disp: exp(-lv) * |pred - target| + lv                                           (B,1,H,W)
// with the log-variance lv read from device memory at every launch (it is a parameter that the captured step's Adam
// updates), and their backward passes for an arbitrary upstream gradient map (read as g[p * g_stride]; g_stride = 0 for an
// expanded scalar) plus an optional uniform term gmean[0] * gmean_scale (the gradient of the map's mean, produced by the
// forward pass itself).  Nothing here synchronises with the host.
//
// Many classes (5 <= C <= 64) move through LDS a workgroup's 256 pixel rows at a time (rows_lds.h).  A logits row may sit
// inside a wider pixel stride (ld > C, a channel slice): the global span a workgroup reads ends at its last pixel's channel
// C-1, and gradient rows are written back channel by channel, C logical channels per pixel, so the neighbouring channels of
// a wider buffer are never written.
#include "sdhip_common.h"
#include "rows_lds.h"

namespace {

// a label counts when it names one of the C classes and is not ignore_index; anything else (ignore_index itself, or an
// out-of-range label, which the reference rejects with an error) contributes CE 0
__device__ __forceinline__ bool mt_counted(long l, int C, int ignore) { return l != (long)ignore && l >= 0 && l < (long)C; }

// per-pixel CE terms of one row (in global memory or LDS): returns lse, sets ce (0 for a pixel that does not count)
template <typename T>
__device__ __forceinline__ float mt_row_lse(const T* row, int C, long l, bool counted, float& ce) {
  float mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, Elem<T>::ld(row + c));
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += expf(Elem<T>::ld(row + c) - mx);
  const float lse = mx + logf(se);
  ce = counted ? lse - Elem<T>::ld(row + l) : 0.f;
  return lse;
}

// gradient row (in place allowed: every channel is read before it is written): g_c = s * (softmax_c - [c == l]), 0 if not counted
template <typename T>
__device__ __forceinline__ void mt_row_grad(const T* row, T* out, int C, long l, bool counted, float lse, float s) {
  for (int c = 0; c < C; ++c) {
    const float v = counted ? s * (expf(Elem<T>::ld(row + c) - lse) - (c == l ? 1.f : 0.f)) : 0.f;
    Elem<T>::st(out + c, v);
  }
}

// ---- segmentation forward ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mt_seg_fwd_kernel(const T* __restrict__ y, int ldy, const long* __restrict__ lab,
                                                         const float* __restrict__ lv, float* __restrict__ map,
                                                         float* __restrict__ lse_out, double* __restrict__ sum, long npix, int C,
                                                         int ignore, float wsum) {
  __shared__ float sh[4];
  const float l_v = lv[0], e = expf(-l_v);
  float part = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long l = lab[p];
    const bool counted = mt_counted(l, C, ignore);
    float ce;
    const float lse = mt_row_lse(y + p * ldy, C, l, counted, ce);
    const float m = e * ce + l_v;
    map[p] = m;
    lse_out[p] = lse;
    part += m;
  }
  const float tot = block_sum(part, sh);
  if (threadIdx.x == 0) atomicAdd(sum, (double)tot * (double)wsum);
}

template <typename T>
__global__ __launch_bounds__(256) void mt_seg_fwd_rows_kernel(const T* __restrict__ y, int ldy, const long* __restrict__ lab,
                                                              const float* __restrict__ lv, float* __restrict__ map,
                                                              float* __restrict__ lse_out, double* __restrict__ sum, long npix,
                                                              int C, int ignore, float wsum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
  __shared__ float sh[4];
  T* const ly = reinterpret_cast<T*>(rsm);
  const int tid = threadIdx.x;
  const float l_v = lv[0], e = expf(-l_v);
  const long ntiles = (npix + 255) / 256;
  float part = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * 256;
    const int n = (int)min(256L, npix - p0);
    rows_to_lds(y + p0 * ldy, ly, ((n - 1) * ldy + C) * (int)sizeof(T), tid);   // ends at the last pixel's channel C-1
    __syncthreads();
    if (tid < n) {
      const long p = p0 + tid;
      const long l = lab[p];
      const bool counted = mt_counted(l, C, ignore);
      float ce;
      const float lse = mt_row_lse(ly + tid * ldy, C, l, counted, ce);
      const float m = e * ce + l_v;
      map[p] = m;
      lse_out[p] = lse;
      part += m;
    }
    __syncthreads();
  }
  const float tot = block_sum(part, sh);
  if (tid == 0) atomicAdd(sum, (double)tot * (double)wsum);
}

// ---- segmentation backward --------------------------------------------------------------------------------------------
// dlogits = gp * exp(-lv) * (softmax - onehot) for counted pixels, 0 otherwise;  dlv += sum_p gp * (1 - exp(-lv) * ce_p)
template <typename T>
__global__ __launch_bounds__(256) void mt_seg_bwd_kernel(const T* __restrict__ y, int ldy, const long* __restrict__ lab,
                                                         const float* __restrict__ lse_in, const float* __restrict__ lv,
                                                         const float* __restrict__ g, long g_stride, const float* __restrict__ gmean,
                                                         float gmean_scale, T* __restrict__ gy, int ldg, float* __restrict__ dlv,
                                                         long npix, int C, int ignore) {
  __shared__ float sh[4];
  const float e = expf(-lv[0]);
  const float gm = gmean ? gmean[0] * gmean_scale : 0.f;
  float part = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const float gp = (g ? g[p * g_stride] : 0.f) + gm;
    const long l = lab[p];
    const bool counted = mt_counted(l, C, ignore);
    const T* row = y + p * ldy;
    const float lse = lse_in[p];
    const float ce = counted ? lse - Elem<T>::ld(row + l) : 0.f;
    part += gp * (1.f - e * ce);
    if (gy) mt_row_grad(row, gy + p * ldg, C, l, counted, lse, gp * e);
  }
  if (dlv) {
    const float tot = block_sum(part, sh);
    if (threadIdx.x == 0) atomicAdd(dlv, tot);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mt_seg_bwd_rows_kernel(const T* __restrict__ y, int ldy, const long* __restrict__ lab,
                                                              const float* __restrict__ lse_in, const float* __restrict__ lv,
                                                              const float* __restrict__ g, long g_stride,
                                                              const float* __restrict__ gmean, float gmean_scale,
                                                              T* __restrict__ gy, int ldg, float* __restrict__ dlv, long npix,
                                                              int C, int ignore, int dense_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
  __shared__ float sh[4];
  T* const ly = reinterpret_cast<T*>(rsm);
  const int tid = threadIdx.x;
  const float e = expf(-lv[0]);
  const float gm = gmean ? gmean[0] * gmean_scale : 0.f;
  const long ntiles = (npix + 255) / 256;
  float part = 0.f;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * 256;
    const int n = (int)min(256L, npix - p0);
    rows_to_lds(y + p0 * ldy, ly, ((n - 1) * ldy + C) * (int)sizeof(T), tid);
    __syncthreads();
    if (tid < n) {
      const long p = p0 + tid;
      const float gp = (g ? g[p * g_stride] : 0.f) + gm;
      const long l = lab[p];
      const bool counted = mt_counted(l, C, ignore);
      T* row = ly + tid * ldy;
      const float lse = lse_in[p];
      const float ce = counted ? lse - Elem<T>::ld(row + l) : 0.f;
      part += gp * (1.f - e * ce);
      if (gy) mt_row_grad(row, row, C, l, counted, lse, gp * e);     // in place: the row now holds its gradient
    }
    __syncthreads();
    if (gy) {
      if (dense_out) {      // ldy == ldg == C: the tile is one contiguous region on both sides
        rows_from_lds(gy + p0 * ldg, ly, n * C * (int)sizeof(T), tid);
      } else {              // C logical channels per pixel only: neighbouring channels of a wider buffer stay untouched
        for (int i = tid; i < n * C; i += 256) {
          const int r = i / C, c = i - r * C;
          gy[(p0 + r) * ldg + c] = ly[r * ldy + c];
        }
      }
    }
    __syncthreads();
  }
  if (dlv) {
    const float tot = block_sum(part, sh);
    if (tid == 0) atomicAdd(dlv, tot);
  }
}

// ---- disparity (L1) forward / backward --------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mt_l1_fwd_kernel(const T* __restrict__ a, int lda, const float* __restrict__ b,
                                                        const float* __restrict__ lv, float* __restrict__ map,
                                                        double* __restrict__ sum, long n, float wsum) {
  __shared__ float sh[4];
  const float l_v = lv[0], e = expf(-l_v);
  float part = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float m = e * fabsf(Elem<T>::ld(a + i * lda) - b[i]) + l_v;
    map[i] = m;
    part += m;
  }
  const float tot = block_sum(part, sh);
  if (threadIdx.x == 0) atomicAdd(sum, (double)tot * (double)wsum);
}

// da = gp * exp(-lv) * sign(a - b) (sign(0) = 0, as torch);  dlv += sum_i gp * (1 - exp(-lv) * |a - b|)
template <typename T>
__global__ __launch_bounds__(256) void mt_l1_bwd_kernel(const T* __restrict__ a, int lda, const float* __restrict__ b,
                                                        const float* __restrict__ lv, const float* __restrict__ g, long g_stride,
                                                        const float* __restrict__ gmean, float gmean_scale, T* __restrict__ ga,
                                                        int ldg, float* __restrict__ dlv, long n) {
  __shared__ float sh[4];
  const float e = expf(-lv[0]);
  const float gm = gmean ? gmean[0] * gmean_scale : 0.f;
  float part = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float gp = (g ? g[i * g_stride] : 0.f) + gm;
    const float d = Elem<T>::ld(a + i * lda) - b[i];
    part += gp * (1.f - e * fabsf(d));
    if (ga) Elem<T>::st(ga + i * ldg, d > 0.f ? gp * e : (d < 0.f ? -gp * e : 0.f));
  }
  if (dlv) {
    const float tot = block_sum(part, sh);
    if (threadIdx.x == 0) atomicAdd(dlv, tot);
  }
}

// mean[0] = sum[0] (the sum was accumulated with weight 1/n): the f32 scalar autograd carries, without a host round trip
__global__ void mt_mean_kernel(const double* __restrict__ sum, float* __restrict__ mean) {
  if (threadIdx.x == 0 && blockIdx.x == 0) mean[0] = (float)sum[0];
}

inline dim3 mt_grid(long items) {      // one f64 / f32 atomic per workgroup on the same scalar (as optim_loss.hip's loss kernels)
  long b = (items + 255) / 256;
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

inline dim3 mt_rows_grid(long npix) {
  long b = (npix + 255) / 256;
  if (b > 768) b = 768;
  return dim3((unsigned)b);
}

// the LDS-rows path: many classes, the row tile fits, the global side of the row copies is 4-byte aligned (rows_lds.h)
inline bool mt_rows_ok(int C, int ldy, int es, const void* logits) {
  return C > 4 && C <= 64 && rows_lds_bytes(ldy, es) <= 60 * 1024 && (((uintptr_t)logits) & 3) == 0;
}

}  // namespace

extern "C" int sdhip_mt_seg_fwd(const void* logits, int ldy, const int64_t* labels, const float* log_var, float* map, float* lse,
                                double* sum, float* mean, long npix, int C, int ignore_index, float sum_weight, int dtype, void* stream) {
  SDHIP_CHECK_ARG(logits && labels && log_var && map && lse && sum && npix > 0 && C > 0 && ldy >= C, "mt_seg_fwd: bad arguments");
  SDHIP_CHECK_DTYPE("mt_seg_fwd", dtype);
  hipStream_t s = (hipStream_t)stream;
  const long* lab = reinterpret_cast<const long*>(labels);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (mt_rows_ok(C, ldy, sizeof(T), logits))
      hipLaunchKernelGGL(mt_seg_fwd_rows_kernel<T>, mt_rows_grid(npix), dim3(256), rows_lds_bytes(ldy, sizeof(T)), s, (const T*)logits, ldy, lab, log_var, map, lse, sum, npix, C, ignore_index, sum_weight);
    else
      hipLaunchKernelGGL(mt_seg_fwd_kernel<T>, mt_grid(npix), dim3(256), 0, s, (const T*)logits, ldy, lab, log_var, map, lse, sum, npix, C, ignore_index, sum_weight);
  });
  if (mean) hipLaunchKernelGGL(mt_mean_kernel, dim3(1), dim3(64), 0, s, sum, mean);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_mt_seg_bwd(const void* logits, int ldy, const int64_t* labels, const float* lse, const float* log_var,
                                const float* gmap, long g_stride, const float* gmean, float gmean_scale, void* grad, int ldg,
                                float* grad_log_var, long npix, int C, int ignore_index, int dtype, void* stream) {
  SDHIP_CHECK_ARG(logits && labels && lse && log_var && npix > 0 && C > 0 && ldy >= C && (!grad || ldg >= C) && g_stride >= 0,
                  "mt_seg_bwd: bad arguments");
  SDHIP_CHECK_DTYPE("mt_seg_bwd", dtype);
  if (!grad && !grad_log_var) return SDHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  const long* lab = reinterpret_cast<const long*>(labels);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (mt_rows_ok(C, ldy, sizeof(T), logits)) {
      const int dense = grad && ldy == C && ldg == C && (((uintptr_t)grad) & 3) == 0;
      hipLaunchKernelGGL(mt_seg_bwd_rows_kernel<T>, mt_rows_grid(npix), dim3(256), rows_lds_bytes(ldy, sizeof(T)), s, (const T*)logits, ldy, lab, lse, log_var, gmap, g_stride, gmean, gmean_scale, (T*)grad, ldg, grad_log_var, npix, C, ignore_index, dense);
    } else {
      hipLaunchKernelGGL(mt_seg_bwd_kernel<T>, mt_grid(npix), dim3(256), 0, s, (const T*)logits, ldy, lab, lse, log_var, gmap, g_stride, gmean, gmean_scale, (T*)grad, ldg, grad_log_var, npix, C, ignore_index);
    }
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_mt_l1_fwd(const void* pred, int ldp, const float* target, const float* log_var, float* map, double* sum,
                               float* mean, long n, float sum_weight, int dtype, void* stream) {
  SDHIP_CHECK_ARG(pred && target && log_var && map && sum && n > 0 && ldp >= 1, "mt_l1_fwd: bad arguments");
  SDHIP_CHECK_DTYPE("mt_l1_fwd", dtype);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(mt_l1_fwd_kernel<T>, mt_grid(n), dim3(256), 0, s, (const T*)pred, ldp, target, log_var, map, sum, n, sum_weight);
  });
  if (mean) hipLaunchKernelGGL(mt_mean_kernel, dim3(1), dim3(64), 0, s, sum, mean);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_mt_l1_bwd(const void* pred, int ldp, const float* target, const float* log_var, const float* gmap, long g_stride,
                               const float* gmean, float gmean_scale, void* grad, int ldg, float* grad_log_var, long n, int dtype,
                               void* stream) {
  SDHIP_CHECK_ARG(pred && target && log_var && n > 0 && ldp >= 1 && (!grad || ldg >= 1) && g_stride >= 0, "mt_l1_bwd: bad arguments");
  SDHIP_CHECK_DTYPE("mt_l1_bwd", dtype);
  if (!grad && !grad_log_var) return SDHIP_OK;
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(mt_l1_bwd_kernel<T>, mt_grid(n), dim3(256), 0, s, (const T*)pred, ldp, target, log_var, gmap, g_stride, gmean, gmean_scale, (T*)grad, ldg, grad_log_var, n);
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
