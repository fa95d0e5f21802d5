// Horizontal disparity warp and the gated blend around it (models/torch_dsnet.py:10-86 apply_disparity with
// wrap_mode='edge'; the blend of models/dsnet_t2_warp.py minidsnetDivide / minidsnetDivideSoftmax):
//   x  = clamp(j + sign * disp[b,y,j], 0, W-1)     x0 = floor(x)     x1 = min(x0 + 1, W-1)
//   warped[b,c,y,j] = (x1 - x) * right[b,c,y,x0] + (x - x0) * right[b,c,y,x1]
//   both = (1 - a) * left + a * warped              a: one gate per pixel, one per channel, or softmax_c(raw scores)
// The coordinate arithmetic is f32 in the reference's order (add, clamp, floor, subtract) whatever the storage type, so the
// interpolation weights are bit-equal to the reference's; x == W-1 gives x1 == x0 and BOTH weights 0 (the right edge
// writes 0, not the edge pixel).  Channel sums are f32.
//
// A group of G = 2^k lanes (the smallest power of two >= C, at most 64) owns one pixel, lane l its channels l, l + G, ...:
// neighbouring lanes read neighbouring channels, so the NHWC rows are read and written coalesced whatever C is (a thread
// that walks its own 19-channel row keeps 64 cache lines busy for one element each: rows_lds.h), and the sums over the
// channels are xor-shuffles inside the group.  Every lane of a group computes the pixel's coordinates itself (one
// broadcast load of the disparity).  Pad lanes of a wider pixel stride are never touched.
//
// Backward: the per-pixel pass produces g_left, g_gate and g_disp; the adjoint of the row gather (g_right) is a second
// launch in which a workgroup owns one image row x one channel group, accumulates it in LDS with float LDS atomics
// (several output pixels land on one source pixel, in any order) and writes it out once with plain stores: no global
// atomics, no workspace, nothing to clear.  Where one workgroup holds all channels of a dense row that starts and ends on 16
// bytes (1024 px x 19 bf16 classes, 512 px x 2) the stores are 16 bytes per lane; a row split into channel groups, a padded
// pixel stride or an unaligned row is stored element by element.  The order of the LDS adds is not fixed, so g_right is
// reproducible to f32
// rounding, not bit for bit.
#include "sdhip_common.h"

namespace {

// sums / maxima over the G = 2^k lanes of a pixel group (every lane receives the result)
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct WarpCoord {
  int i0, i1;        // source columns, always inside [0, W-1]
  float w0, w1;      // their weights
  bool inside;       // 0 <= j + offset <= W-1: the clamp is inactive and the offset receives gradient
};

__device__ __forceinline__ WarpCoord warp_coord(int j, float off, int W) {
  const float wm = (float)(W - 1);
  const float xf = (float)j + off;
  WarpCoord k;
  k.inside = xf >= 0.f && xf <= wm;
  const float x = fminf(fmaxf(xf, 0.f), wm);      // NaN offsets end at column 0
  const float x0 = floorf(x);
  const float x1 = fminf(x0 + 1.f, wm);
  k.w0 = x1 - x;
  k.w1 = x - x0;
  k.i0 = min(max((int)x0, 0), W - 1);
  k.i1 = min(max((int)x1, 0), W - 1);
  return k;
}

// gate modes
enum { GATE_NONE = 0, GATE_PIXEL = 1, GATE_CHANNEL = 2, GATE_SOFTMAX = 3 };

template <typename T>
__global__ __launch_bounds__(256) void warp_fwd_kernel(const T* __restrict__ left, int ldl, const T* __restrict__ right, int ldr,
                                                       const T* __restrict__ disp, int ldd, float sign,
                                                       const T* __restrict__ gate, int ldgt, int mode, T* __restrict__ warped,
                                                       int ldw, T* __restrict__ both, int ldb, T* __restrict__ prob, int ldp,
                                                       int W, int C, int lg) {
  const int t = blockIdx.y * 256 + threadIdx.x;       // grid: (image rows, chunks of 256 >> lg pixels) - no division by W
  const int j = t >> lg;
  const int G = 1 << lg, lc = t & (G - 1);
  if (j >= W) return;                     // a whole group leaves together: 64 % G == 0
  const long row = (long)blockIdx.x * W;
  const long p = row + j;
  const WarpCoord k = warp_coord(j, sign * Elem<T>::ld(disp + p * ldd), W);
  const T* r0 = right + (row + k.i0) * ldr;
  const T* r1 = right + (row + k.i1) * ldr;
  float a = 0.f, mx = 0.f, inv = 0.f;
  if (mode == GATE_PIXEL) a = Elem<T>::ld(gate + p * ldgt);
  if (mode == GATE_SOFTMAX) {
    mx = -INFINITY;
    for (int c = lc; c < C; c += G) mx = fmaxf(mx, Elem<T>::ld(gate + p * ldgt + c));
    mx = group_max(mx, G);
    float se = 0.f;
    for (int c = lc; c < C; c += G) se += expf(Elem<T>::ld(gate + p * ldgt + c) - mx);
    inv = 1.f / group_sum(se, G);
  }
  for (int c = lc; c < C; c += G) {
    const float wv = k.w0 * Elem<T>::ld(r0 + c) + k.w1 * Elem<T>::ld(r1 + c);
    Elem<T>::st(warped + p * ldw + c, wv);
    if (mode == GATE_NONE) continue;
    if (mode == GATE_CHANNEL) a = Elem<T>::ld(gate + p * ldgt + c);
    if (mode == GATE_SOFTMAX) {
      a = expf(Elem<T>::ld(gate + p * ldgt + c) - mx) * inv;
      Elem<T>::st(prob + p * ldp + c, a);
      a = Elem<T>::rnd(a);            // the blend uses the probability as stored, which is what the backward pass reads
    }
    Elem<T>::st(both + p * ldb + c, (1.f - a) * Elem<T>::ld(left + p * ldl + c) + a * Elem<T>::rnd(wv));
  }
}

// gradient that reaches warped[p][c]: its own upstream gradient plus the blend's share
template <typename T>
__device__ __forceinline__ float warp_gw(const T* gb, const T* gwp, float a, int c) {
  return (gwp ? Elem<T>::ld(gwp + c) : 0.f) + (gb ? a * Elem<T>::ld(gb + c) : 0.f);
}

// `gate` holds probabilities here (GATE_SOFTMAX: the prob output of the forward pass; g_gate is then w.r.t. the raw scores)
template <typename T>
__global__ __launch_bounds__(256) void warp_bwd_pixel_kernel(const T* __restrict__ g_both, int ldgb, const T* __restrict__ g_warped,
                                                             int ldgw, const T* __restrict__ left, int ldl,
                                                             const T* __restrict__ right, int ldr, const T* __restrict__ disp,
                                                             int ldd, float sign, const T* __restrict__ gate, int ldgt, int mode,
                                                             T* __restrict__ g_left, int ldgl, T* __restrict__ g_disp, int ldgd,
                                                             T* __restrict__ g_gate, int ldgg, int W, int C, int lg) {
  const int t = blockIdx.y * 256 + threadIdx.x;
  const int j = t >> lg;
  const int G = 1 << lg, lc = t & (G - 1);
  if (j >= W) return;
  const long row = (long)blockIdx.x * W;
  const long p = row + j;
  const WarpCoord k = warp_coord(j, sign * Elem<T>::ld(disp + p * ldd), W);
  const T* r0 = right + (row + k.i0) * ldr;
  const T* r1 = right + (row + k.i1) * ldr;
  const T* gb = g_both ? g_both + p * ldgb : nullptr;
  const T* gwp = g_warped ? g_warped + p * ldgw : nullptr;
  const T* gt = mode != GATE_NONE ? gate + p * ldgt : nullptr;
  const T* lf = mode != GATE_NONE ? left + p * ldl : nullptr;
  float a = mode == GATE_PIXEL ? Elem<T>::ld(gt) : 0.f;
  float goff = 0.f, gsum = 0.f;     // gsum: sum_c dL/da_c (GATE_PIXEL), sum_c dL/da_c * a_c (GATE_SOFTMAX)
  for (int c = lc; c < C; c += G) {
    const float v0 = Elem<T>::ld(r0 + c), v1 = Elem<T>::ld(r1 + c);
    if (mode >= GATE_CHANNEL) a = Elem<T>::ld(gt + c);
    goff += warp_gw(gb, gwp, a, c) * (v1 - v0);
    if (mode == GATE_NONE) continue;
    const float g = gb ? Elem<T>::ld(gb + c) : 0.f;
    if (g_left) Elem<T>::st(g_left + p * ldgl + c, (1.f - a) * g);
    const float ga = g * (Elem<T>::rnd(k.w0 * v0 + k.w1 * v1) - Elem<T>::ld(lf + c));
    if (mode == GATE_PIXEL) gsum += ga;
    else if (mode == GATE_SOFTMAX) gsum += ga * a;
    else if (g_gate) Elem<T>::st(g_gate + p * ldgg + c, ga);
  }
  goff = group_sum(goff, G);
  gsum = group_sum(gsum, G);
  if (g_disp && lc == 0) Elem<T>::st(g_disp + p * ldgd, k.inside ? sign * goff : 0.f);
  if (!g_gate) return;
  if (mode == GATE_PIXEL && lc == 0) Elem<T>::st(g_gate + p * ldgg, gsum);
  if (mode == GATE_SOFTMAX) {
    for (int c = lc; c < C; c += G) {
      const float pc = Elem<T>::ld(gt + c);
      const float g = gb ? Elem<T>::ld(gb + c) : 0.f;
      const float ga = g * (Elem<T>::rnd(k.w0 * Elem<T>::ld(r0 + c) + k.w1 * Elem<T>::ld(r1 + c)) - Elem<T>::ld(lf + c));
      Elem<T>::st(g_gate + p * ldgg + c, pc * (ga - gsum));
    }
  }
}

// g_right: grid (B*H image rows, channel groups of CG); acc[W][CG] f32 in LDS
template <typename T>
__global__ __launch_bounds__(256) void warp_bwd_scatter_kernel(const T* __restrict__ g_both, int ldgb, const T* __restrict__ g_warped,
                                                               int ldgw, const T* __restrict__ disp, int ldd, float sign,
                                                               const T* __restrict__ gate, int ldgt, int mode,
                                                               T* __restrict__ g_right, int ldgr, int W, int C, int CG, int lg) {
  extern __shared__ __attribute__((aligned(16))) float acc[];
  const int tid = threadIdx.x;
  const long row = (long)blockIdx.x * W;
  const int c0 = blockIdx.y * CG;
  const int n = min(CG, C - c0);
  for (int i = tid; i < W * n; i += 256) acc[i] = 0.f;
  __syncthreads();
  const int G = 1 << lg, lc = tid & (G - 1);
  for (int j = tid >> lg; j < W; j += 256 >> lg) {
    const long p = row + j;
    const WarpCoord k = warp_coord(j, sign * Elem<T>::ld(disp + p * ldd), W);
    const T* gb = g_both ? g_both + p * ldgb + c0 : nullptr;
    const T* gwp = g_warped ? g_warped + p * ldgw + c0 : nullptr;
    float a = mode == GATE_PIXEL ? Elem<T>::ld(gate + p * ldgt) : 0.f;
    for (int c = lc; c < n; c += G) {
      if (mode >= GATE_CHANNEL) a = Elem<T>::ld(gate + p * ldgt + c0 + c);
      const float g = warp_gw(gb, gwp, a, c);
      atomicAdd(&acc[k.i0 * n + c], g * k.w0);
      atomicAdd(&acc[k.i1 * n + c], g * k.w1);
    }
  }
  __syncthreads();
  if (n == C && ldgr == C) {        // the whole row is one contiguous run: 16-byte stores when it starts and ends on 16 bytes
    constexpr int N = Chunk<T>::N;
    T* const dst = g_right + row * ldgr;
    if ((((uintptr_t)dst) & 15) == 0 && (W * n) % N == 0) {
      for (int i = tid; i < (W * n) / N; i += 256) *reinterpret_cast<u32x4*>(dst + i * N) = Chunk<T>::pack(acc + i * N);
    } else {
      for (int i = tid; i < W * n; i += 256) Elem<T>::st(dst + i, acc[i]);
    }
  } else {
    for (int i = tid; i < W * n; i += 256) {
      const int x = i / n, c = i - x * n;
      Elem<T>::st(g_right + (row + x) * ldgr + c0 + c, acc[i]);
    }
  }
}

constexpr int kWarpLdsFloats = 20480;      // 80 KB of accumulator per workgroup (two workgroups per CU): 1024 px x 19 classes in one pass

// more than 64 KB of dynamic LDS has to be allowed per kernel, once per device (the attribute belongs to the device that is
// current when it is set); a device index beyond the table sets it at every call
template <typename T>
inline bool warp_scatter_allow_lds() {
  static bool done[64];
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const bool tracked = dev >= 0 && dev < 64;
  if (tracked && done[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&warp_bwd_scatter_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          kWarpLdsFloats * (int)sizeof(float)) != hipSuccess)
    return false;
  if (tracked) done[dev] = true;
  return true;
}

// log2 of the lanes per pixel: the smallest power of two >= C, at most 64
inline int warp_group_log2(int C) {
  int lg = 0;
  while ((1 << lg) < C && lg < 6) ++lg;
  return lg;
}

inline int warp_gate_mode(const void* gate, int gate_ch, int gate_softmax) {
  if (!gate) return GATE_NONE;
  if (gate_softmax) return GATE_SOFTMAX;
  return gate_ch == 1 ? GATE_PIXEL : GATE_CHANNEL;
}

// shared argument checks; returns 0 when they pass
inline int warp_check(const char* fn, const void* right, int ldr, const void* disp, int ldd, const void* left, int ldl,
                      const void* gate, int ldgt, int gate_ch, int gate_softmax, int B, int H, int W, int C, int dtype) {
  SDHIP_CHECK_ARG(right && disp, "%s: null seg_right / disp pointer", fn);
  SDHIP_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "%s: bad shape B=%d H=%d W=%d C=%d", fn, B, H, W, C);
  SDHIP_CHECK_ARG(W <= (1 << 17) && (long)B * H < (1L << 31), "%s: shape too large (W <= 131072, B*H < 2^31)", fn);
  SDHIP_CHECK_DTYPE(fn, dtype);
  SDHIP_CHECK_ARG(ldr >= C, "%s: seg_right pixel stride %d < C=%d", fn, ldr, C);
  SDHIP_CHECK_ARG(ldd >= 1, "%s: disp must be ONE channel with pixel stride >= 1 (got %d)", fn, ldd);
  if (gate) {
    SDHIP_CHECK_ARG(gate_ch == 1 || gate_ch == C, "%s: gate has %d channels, must be 1 or C=%d", fn, gate_ch, C);
    SDHIP_CHECK_ARG(!gate_softmax || gate_ch == C, "%s: a softmax gate needs C=%d channels, got %d", fn, C, gate_ch);
    SDHIP_CHECK_ARG(ldgt >= gate_ch, "%s: gate pixel stride %d < its %d channels", fn, ldgt, gate_ch);
    SDHIP_CHECK_ARG(left && ldl >= C, "%s: a gate needs seg_left (pixel stride >= C)", fn);
  } else {
    SDHIP_CHECK_ARG(!gate_softmax && gate_ch == 0, "%s: gate channels / softmax given without a gate", fn);
  }
  return 0;
}

}  // namespace

extern "C" int sdhip_warp_blend_fwd(const void* seg_left, int ldl, const void* seg_right, int ldr, const void* disp, int ldd,
                                    float offset_sign, const void* gate, int ldgt, int gate_ch, int gate_softmax, void* warped,
                                    int ldw, void* both, int ldb, void* prob, int ldp, int B, int H, int W, int C, int dtype,
                                    void* stream) {
  if (int rc = warp_check("warp_blend_fwd", seg_right, ldr, disp, ldd, seg_left, ldl, gate, ldgt, gate_ch, gate_softmax, B, H, W, C, dtype)) return rc;
  SDHIP_CHECK_ARG(warped && ldw >= C, "warp_blend_fwd: null warped output or pixel stride %d < C=%d", ldw, C);
  SDHIP_CHECK_ARG(offset_sign == 1.f || offset_sign == -1.f, "warp_blend_fwd: offset_sign must be +1 or -1");
  SDHIP_CHECK_ARG(gate ? (both && ldb >= C) : !both, "warp_blend_fwd: `both` goes with a gate (pixel stride >= C)");
  SDHIP_CHECK_ARG(gate_softmax ? (prob && ldp >= C) : !prob, "warp_blend_fwd: `prob` goes with a softmax gate (pixel stride >= C)");
  const int mode = warp_gate_mode(gate, gate_ch, gate_softmax);
  hipStream_t s = (hipStream_t)stream;
  const int lg = warp_group_log2(C);
  const dim3 grid((unsigned)((long)B * H), (unsigned)((((long)W << lg) + 255) / 256));
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(warp_fwd_kernel<T>, grid, dim3(256), 0, s, (const T*)seg_left, ldl, (const T*)seg_right, ldr, (const T*)disp, ldd, offset_sign, (const T*)gate, ldgt, mode, (T*)warped, ldw, (T*)both, ldb, (T*)prob, ldp, W, C, lg);
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_warp_blend_bwd(const void* g_both, int ldgb, const void* g_warped, int ldgw, const void* seg_left, int ldl,
                                    const void* seg_right, int ldr, const void* disp, int ldd, float offset_sign, const void* gate,
                                    int ldgt, int gate_ch, int gate_softmax, void* g_left, int ldgl, void* g_right, int ldgr,
                                    void* g_disp, int ldgd, void* g_gate, int ldgg, int B, int H, int W, int C, int dtype,
                                    void* stream) {
  if (int rc = warp_check("warp_blend_bwd", seg_right, ldr, disp, ldd, seg_left, ldl, gate, ldgt, gate_ch, gate_softmax, B, H, W, C, dtype)) return rc;
  SDHIP_CHECK_ARG(offset_sign == 1.f || offset_sign == -1.f, "warp_blend_bwd: offset_sign must be +1 or -1");
  SDHIP_CHECK_ARG(g_both || g_warped, "warp_blend_bwd: neither g_both nor g_warped given");
  SDHIP_CHECK_ARG((!g_both || (gate && ldgb >= C)) && (!g_warped || ldgw >= C), "warp_blend_bwd: g_both needs a gate; gradient pixel strides must be >= C=%d", C);
  SDHIP_CHECK_ARG((!g_left || (gate && ldgl >= C)) && (!g_right || ldgr >= C) && (!g_disp || ldgd >= 1) && (!g_gate || (gate && ldgg >= gate_ch)),
                  "warp_blend_bwd: bad output pixel stride, or g_left / g_gate without a gate");
  SDHIP_CHECK_ARG(W <= kWarpLdsFloats || !g_right, "warp_blend_bwd: rows of W=%d pixels exceed the LDS accumulator (%d)", W, kWarpLdsFloats);
  if (!g_left && !g_right && !g_disp && !g_gate) return SDHIP_OK;
  const int mode = warp_gate_mode(gate, gate_ch, gate_softmax);
  hipStream_t s = (hipStream_t)stream;
  if (g_left || g_disp || g_gate) {
    const int lg = warp_group_log2(C);
    const dim3 grid((unsigned)((long)B * H), (unsigned)((((long)W << lg) + 255) / 256));
    sdhip_by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(warp_bwd_pixel_kernel<T>, grid, dim3(256), 0, s, (const T*)g_both, ldgb, (const T*)g_warped, ldgw, (const T*)seg_left, ldl, (const T*)seg_right, ldr, (const T*)disp, ldd, offset_sign, (const T*)gate, ldgt, mode, (T*)g_left, ldgl, (T*)g_disp, ldgd, (T*)g_gate, ldgg, W, C, lg);
    });
  }
  if (g_right) {
    int CG = kWarpLdsFloats / W;
    if (CG > C) CG = C;
    const dim3 grid((unsigned)((long)B * H), (unsigned)((C + CG - 1) / CG));
    const size_t lds = (size_t)W * CG * sizeof(float);
    const int lg = warp_group_log2(CG);
    const int rc = sdhip_by_dtype(dtype, [&](auto tag) -> int {
      using T = typename decltype(tag)::type;
      if (!warp_scatter_allow_lds<T>())
        SDHIP_FAIL(SDHIP_ERR_LAUNCH, "warp_blend_bwd: the runtime refused %d bytes of dynamic LDS", kWarpLdsFloats * (int)sizeof(float));
      hipLaunchKernelGGL(warp_bwd_scatter_kernel<T>, grid, dim3(256), lds, s, (const T*)g_both, ldgb, (const T*)g_warped, ldgw, (const T*)disp, ldd, offset_sign, (const T*)gate, ldgt, mode, (T*)g_right, ldgr, W, C, CG, lg);
      return SDHIP_OK;
    });
    if (rc) return rc;
  }
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
