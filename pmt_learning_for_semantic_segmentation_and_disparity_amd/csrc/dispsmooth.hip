// Edge-aware smoothness penalty on the predicted disparity, gated by the ground-truth segmentation: smoothing_gradients
// (util/utilTorchLoss.py:41-101), the `smooth_grad` term of lossDisp_fn (losses/multiLosses.py:143-146).  For a one-hot target
// (values 0 or 1, at most one 1 per pixel) the reference's per-class formula collapses to
//     Y  = 0.2126 R + 0.7152 G + 0.0722 B,   Ys = G7x7(sigma 2) * Y  (zero padding 3)
//     M(p)   = 1 iff p has a label and its eight neighbours lie inside the image and carry the same label
//     w_v(p) = M(p) exp(1 - |Ys(y,x) - Ys(y+1,x)|),   w_h(p) = M(p) exp(1 - |Ys(y,x) - Ys(y,x+1)|)
//     value  = s * sum_p [ w_v(p) |d(y,x) - d(y+1,x)| + w_h(p) |d(y,x) - d(y,x+1)| ],   s = weight * 0.7 / (128 B H W)
//     g(y,x) = s * [ w_v(y,x) sgn(d(y,x)-d(y+1,x)) - w_v(y-1,x) sgn(d(y-1,x)-d(y,x))
//                  + w_h(y,x) sgn(d(y,x)-d(y,x+1)) - w_h(y,x-1) sgn(d(y,x-1)-d(y,x)) ],   sgn(0) = 0
// The weights do not depend on d, so value and gradient come out of ONE stencil pass:
//   1. disp_smooth_kernel  one workgroup per 64 x 16 tile of one image.  It stages in LDS, once: the luma with a halo of 4 (3 for
//                          the Gaussian, 1 for the forward difference), one small label per pixel with a halo of 2 up / left and 1
//                          down / right (the C target channels are reduced while staging: C costs reads only), the disparity with a
//                          halo of 1.  The Gaussian runs separably in LDS (rows, then columns), the two weight planes follow, and
//                          every thread then writes the gradient of four pixels and adds their value terms in f64.  The
//                          workgroup STORES its f64 partial into a slot of its own (no float atomics);
//   2. slot_fold_kernel    (loss_common.h) one workgroup folds the slots in slot order and does loss += s * sum.
// Value and gradient are bitwise reproducible.  Everything outside the image reads as: luma 0, no label, disparity 0.
#include <math.h>

#include "loss_common.h"

namespace {

constexpr int DS_MAX_C = 32;
constexpr int DS_TW = 64, DS_TH = 16;                  // pixels a workgroup owns
constexpr int DS_YW = DS_TW + 8, DS_YH = DS_TH + 8;    // luma:              origin (y0 - 4, x0 - 4)
constexpr int DS_SW = DS_TW + 2, DS_SH = DS_TH + 2;    // Ys and disparity:  origin (y0 - 1, x0 - 1)
constexpr int DS_LW = DS_TW + 3, DS_LH = DS_TH + 3;    // labels:            origin (y0 - 2, x0 - 2)
constexpr int DS_MW = DS_TW + 1, DS_MH = DS_TH + 1;    // weights:           origin (y0 - 1, x0 - 1)

struct DsGauss { float g[4]; };     // g[|k|], k = -3..3: the 7 x 7 table is their outer product

inline long ds_tiles_x(int W) { return (W + DS_TW - 1) / DS_TW; }
inline long ds_tiles_y(int H) { return (H + DS_TH - 1) / DS_TH; }
inline long ds_slots(int B, int H, int W) { return (long)B * ds_tiles_x(W) * ds_tiles_y(H); }
inline bool ds_shape_ok(int B, int H, int W) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && ds_tiles_y(H) <= 65535 && (long)B * H * W <= (1L << 40);
}

// index of the first non-zero of a pixel's C target channels, -1 for an all-zero row; V floats per load
template <int V>
__device__ __forceinline__ int ds_label(const float* __restrict__ tp, int C) {
  int lab = -1;
  if constexpr (V == 1) {
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      const float v = tp[c];
      lab = (lab < 0 && v != 0.f) ? c : lab;
    }
  } else {
    typedef __attribute__((ext_vector_type(V))) float vec_t;
#pragma unroll 2
    for (int c = 0; c < C; c += V) {
      const vec_t v = *reinterpret_cast<const vec_t*>(tp + c);
#pragma unroll
      for (int k = 0; k < V; ++k) lab = (lab < 0 && v[k] != 0.f) ? c + k : lab;
    }
  }
  return lab;
}

__device__ __forceinline__ float ds_sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

template <typename T, int V>
__global__ __launch_bounds__(256) void disp_smooth_kernel(const float* __restrict__ left, long lbs, long lcs, int lps,
                                                          const float* __restrict__ target, int ldt, const T* __restrict__ disp,
                                                          T* __restrict__ grad, double* __restrict__ slots, int H, int W, int C,
                                                          float sf, DsGauss gs) {
  __shared__ float sY[DS_YH][DS_YW];      // luma
  __shared__ float sT[DS_YH][DS_SW];      // luma after the row pass
  __shared__ float sS[DS_SH][DS_SW];      // Ys
  __shared__ float sD[DS_SH][DS_SW];      // disparity
  __shared__ float sWv[DS_MH][DS_MW], sWh[DS_MH][DS_MW];
  __shared__ signed char sL[DS_LH][DS_LW];
  __shared__ double red[4];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * DS_TW, y0 = blockIdx.y * DS_TH;
  const long hw = (long)H * W;
  left += b * lbs;
  target += b * hw * ldt;
  disp += b * hw;
  grad += b * hw;

  for (int i = tid; i < DS_YH * DS_YW; i += 256) {
    const int r = i / DS_YW, c = i % DS_YW, y = y0 - 4 + r, x = x0 - 4 + c;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float* p = left + ((long)y * W + x) * lps;
      v = 0.2126f * p[0] + 0.7152f * p[lcs] + 0.0722f * p[2 * lcs];
    }
    sY[r][c] = v;
  }
  for (int i = tid; i < DS_LH * DS_LW; i += 256) {
    const int r = i / DS_LW, c = i % DS_LW, y = y0 - 2 + r, x = x0 - 2 + c;
    int lab = -1;
    if (y >= 0 && y < H && x >= 0 && x < W) lab = ds_label<V>(target + ((long)y * W + x) * ldt, C);
    sL[r][c] = (signed char)lab;
  }
  for (int i = tid; i < DS_SH * DS_SW; i += 256) {
    const int r = i / DS_SW, c = i % DS_SW, y = y0 - 1 + r, x = x0 - 1 + c;
    sD[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? Elem<T>::ld(disp + (long)y * W + x) : 0.f;
  }
  __syncthreads();
  // Gaussian, rows: sT[r][c] is column x0 - 1 + c = luma column c + 3
  for (int i = tid; i < DS_YH * DS_SW; i += 256) {
    const int r = i / DS_SW, c = i % DS_SW;
    const float* a = &sY[r][c + 3];
    sT[r][c] = gs.g[3] * (a[-3] + a[3]) + gs.g[2] * (a[-2] + a[2]) + gs.g[1] * (a[-1] + a[1]) + gs.g[0] * a[0];
  }
  __syncthreads();
  // columns: sS[r][c] is row y0 - 1 + r = sT row r + 3
  for (int i = tid; i < DS_SH * DS_SW; i += 256) {
    const int r = i / DS_SW, c = i % DS_SW;
    sS[r][c] = gs.g[3] * (sT[r][c] + sT[r + 6][c]) + gs.g[2] * (sT[r + 1][c] + sT[r + 5][c]) + gs.g[1] * (sT[r + 2][c] + sT[r + 4][c]) +
               gs.g[0] * sT[r + 3][c];
  }
  __syncthreads();
  // weights of pixel (y0 - 1 + r, x0 - 1 + c): its label is sL[r + 1][c + 1]
  for (int i = tid; i < DS_MH * DS_MW; i += 256) {
    const int r = i / DS_MW, c = i % DS_MW;
    const int lab = sL[r + 1][c + 1];
    bool m = lab >= 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = m && sL[r + dy][c + dx] == lab;
    const float s = sS[r][c];
    sWv[r][c] = m ? expf(1.f - fabsf(s - sS[r + 1][c])) : 0.f;
    sWh[r][c] = m ? expf(1.f - fabsf(s - sS[r][c + 1])) : 0.f;
  }
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < DS_TW * DS_TH / 256; ++k) {
    const int i = tid + k * 256, r = i / DS_TW, c = i % DS_TW, y = y0 + r, x = x0 + c;
    if (y < H && x < W) {
      const float d = sD[r + 1][c + 1];
      const float dv = d - sD[r + 2][c + 1], dh = d - sD[r + 1][c + 2];
      const float wv = sWv[r + 1][c + 1], wh = sWh[r + 1][c + 1];
      const float g = wv * ds_sgn(dv) - sWv[r][c + 1] * ds_sgn(sD[r][c + 1] - d) + wh * ds_sgn(dh) - sWh[r + 1][c] * ds_sgn(sD[r + 1][c] - d);
      Elem<T>::st(grad + (long)y * W + x, sf * g);
      acc += (double)(wv * fabsf(dv) + wh * fabsf(dh));
    }
  }
  // block_tail (sdhip_common.h) written out: as a call, the compiler schedules the stencil section above differently
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)                                   // wave order: fixed
    slots[((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// matlab_style_gauss2D((7, 7), 2) = outer(g, g) with g = e / sum(e), e_k = exp(-k^2 / 8): float64, then rounded to f32
inline DsGauss ds_gauss() {
  double e[4], sum = 0.0;
  for (int k = 0; k < 4; ++k) { e[k] = exp(-(double)(k * k) / 8.0); sum += k ? 2.0 * e[k] : e[k]; }
  DsGauss g;
  for (int k = 0; k < 4; ++k) g.g[k] = (float)(e[k] / sum);
  return g;
}

}  // namespace

extern "C" long sdhip_disp_smooth_workspace_bytes(int B, int H, int W) {
  if (!ds_shape_ok(B, H, W)) return SDHIP_ERR_ARG;
  return ds_slots(B, H, W) * (long)sizeof(double);
}

extern "C" int sdhip_disp_smooth(const float* left, long left_bs, long left_cs, int left_ps, const float* target, int ldt,
                                 const void* disp, int dtype, void* grad, double* loss, int B, int H, int W, int C, float weight,
                                 void* workspace, long workspace_bytes, void* stream) {
  SDHIP_CHECK_ARG(left && target && disp && grad && loss && workspace, "disp_smooth: null pointer");
  SDHIP_CHECK_ARG(ds_shape_ok(B, H, W), "disp_smooth: B %d, H %d, W %d (all positive, B <= 65535, H <= %d)", B, H, W, 65535 * DS_TH);
  SDHIP_CHECK_ARG(C >= 1 && C <= DS_MAX_C, "disp_smooth: C %d (1 <= C <= %d)", C, DS_MAX_C);
  SDHIP_CHECK_ARG(ldt >= C, "disp_smooth: target pixel stride %d below C = %d", ldt, C);
  SDHIP_CHECK_IMAGE_STRIDES("disp_smooth", left_bs, left_cs, left_ps);
  SDHIP_CHECK_DTYPE("disp_smooth", dtype);
  const long need = ds_slots(B, H, W) * (long)sizeof(double);
  SDHIP_CHECK_WORKSPACE("disp_smooth", workspace, workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const double scale = (double)weight * 0.7 / (128.0 * (double)B * (double)H * (double)W);
  const dim3 grid((unsigned)ds_tiles_x(W), (unsigned)ds_tiles_y(H), (unsigned)B);
  const DsGauss gs = ds_gauss();
  // channel rows of the target as 16- or 8-byte loads where every row starts on such a boundary
  const uintptr_t ta = (uintptr_t)target;
  const int V = (C % 4 == 0 && ldt % 4 == 0 && (ta & 15) == 0) ? 4 : (C % 2 == 0 && ldt % 2 == 0 && (ta & 7) == 0) ? 2 : 1;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto VV) {
      hipLaunchKernelGGL((disp_smooth_kernel<T, VV()>), grid, dim3(256), 0, s, left, left_bs, left_cs, left_ps, target, ldt, (const T*)disp,
                         (T*)grad, (double*)workspace, H, W, C, (float)scale, gs);
    };
    if (V == 4) launch(std::integral_constant<int, 4>{});
    else if (V == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
  });
  SDHIP_LAUNCH_CHECK();
  return sdhip_slot_fold(__func__, (const double*)workspace, ds_slots(B, H, W), scale, loss, s);
}
