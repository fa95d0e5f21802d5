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
#include "loss_common.h"

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

// ------------------------------------------------------------------------------------------------ *_disp networks
// (models/dsnet_t2_warp.py:704-972)  Three streaming kernels on images of C <= 4 channels and on the class scores.
constexpr int WI_MAX_C = 4;

// out = [gt > 0] * apply_disparity(img, -gt): one thread per pixel walks the C <= 4 channels.  The image is read through its
// strides (planar: consecutive lanes on consecutive pixels of a plane; interleaved: on consecutive pixels of the row).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void warp_image_masked_kernel(const TI* __restrict__ img, long bs, long cs, long ps,
                                                                const float* __restrict__ gt, TO* __restrict__ out, int ldy, int H,
                                                                int W, int C, long npix) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int j = (int)(p % W);
    const long r = p / W;
    const float d = gt[p];
    TO* o = out + p * ldy;
    if (!(d > 0.f)) {                     // the mask cuts (NaN included): exact zeros
#pragma unroll
      for (int c = 0; c < WI_MAX_C; ++c)
        if (c < C) Elem<TO>::st(o + c, 0.f);
      continue;
    }
    const WarpCoord k = warp_coord(j, -d, W);
    const TI* q = img + (r / H) * bs + (r % H) * (long)W * ps;
    const TI* q0 = q + (long)k.i0 * ps;
    const TI* q1 = q + (long)k.i1 * ps;
#pragma unroll
    for (int c = 0; c < WI_MAX_C; ++c)
      if (c < C) Elem<TO>::st(o + c, k.w0 * Elem<TI>::ld(q0 + c * cs) + k.w1 * Elem<TI>::ld(q1 + c * cs));
  }
}

// y = (1 - g) a + g b; `units` chunks of N channels per pixel, one chunk per lane
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_blend_fwd_kernel(const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb,
                                                             const T* __restrict__ g, int ldg, T* __restrict__ y, int ldy, long npix,
                                                             int C) {
  constexpr int N = Unit<T, VEC>::N;
  const int units = C / N;
  const long items = npix * units;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
    const long pix = i / units;
    const int c0 = (int)(i - pix * units) * N;
    const float gv = Elem<T>::ld(g + pix * ldg), hv = 1.f - gv;
    float av[N], bv[N];
    Unit<T, VEC>::load(a + pix * lda + c0, av);
    Unit<T, VEC>::load(b + pix * ldb + c0, bv);
#pragma unroll
    for (int e = 0; e < N; ++e) av[e] = hv * av[e] + gv * bv[e];
    Unit<T, VEC>::store(y + pix * ldy + c0, av);
  }
}

// a pixel's chunks are handled by G = 2^k lanes side by side (G >= min(units, 64)): lane s takes the chunks s, s + G, ...;
// the channel sum of gg is an xor-shuffle among them
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_blend_bwd_kernel(const T* __restrict__ gy, int ldgy, const T* __restrict__ a, int lda,
                                                             const T* __restrict__ b, int ldb, const T* __restrict__ g, int ldg,
                                                             T* __restrict__ ga, int ldga, T* __restrict__ gb, int ldgb,
                                                             T* __restrict__ gg, int ldgg, long npix, int C, int G) {
  constexpr int N = Unit<T, VEC>::N;
  const int units = C / N;
  const long slots = npix * G;
  // the trip count is the same for every lane of a workgroup: all 64 lanes of a wave reach the shuffles
  for (long base = (long)blockIdx.x * 256; base < slots; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    const long pix = i / G;
    const int sub = (int)(i - pix * G);
    float s = 0.f;
    if (pix < npix) {
      const float gv = Elem<T>::ld(g + pix * ldg), hv = 1.f - gv;
      for (int u = sub; u < units; u += G) {
        const int c0 = u * N;
        float yv[N], av[N], bv[N];
        Unit<T, VEC>::load(gy + pix * ldgy + c0, yv);
        Unit<T, VEC>::load(a + pix * lda + c0, av);
        Unit<T, VEC>::load(b + pix * ldb + c0, bv);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          s = fmaf(yv[e], bv[e] - av[e], s);
          av[e] = hv * yv[e];
          bv[e] = gv * yv[e];
        }
        Unit<T, VEC>::store(ga + pix * ldga + c0, av);
        Unit<T, VEC>::store(gb + pix * ldgb + c0, bv);
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (pix < npix && sub == 0) Elem<T>::st(gg + pix * ldgg, s);
  }
}

// Photometric MSE.  A workgroup handles PM_CHUNK pixels per trip, thread t the pixels base + t, base + 256 + t, ...: which
// pixels a workgroup and a thread own depends on npix alone, never on a stride or an alignment.
constexpr int PM_CHUNK = 1024;
constexpr int PM_MAX_TILES = 1024;
constexpr long PM_MAX_NPIX = 1L << 40;

inline long pm_tiles(long npix) {
  const long t = (npix + PM_CHUNK - 1) / PM_CHUNK;
  return t > PM_MAX_TILES ? PM_MAX_TILES : t;
}

template <typename T>
__global__ __launch_bounds__(256) void photo_mse_kernel(const T* __restrict__ w, int ldw, const float* __restrict__ l, long bs, long cs,
                                                        long ps, T* __restrict__ grad, double* __restrict__ parts, float scale, long hw,
                                                        int C, long npix) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (long base = (long)blockIdx.x * PM_CHUNK; base < npix; base += (long)gridDim.x * PM_CHUNK) {
#pragma unroll
    for (int k = 0; k < PM_CHUNK / 256; ++k) {
      const long p = base + k * 256 + tid;
      if (p >= npix) continue;
      const long bi = p / hw;
      const float* lp = l + bi * bs + (p - bi * hw) * ps;
      const T* wp = w + p * ldw;
      T* gp = grad + p * C;
#pragma unroll
      for (int c = 0; c < WI_MAX_C; ++c) {
        if (c < C) {
          const float d = Elem<T>::ld(wp + c) - lp[c * cs];
          acc += (double)d * (double)d;
          Elem<T>::st(gp + c, scale * d);
        }
      }
    }
  }
  const double tot = block_tail(acc, red);
  if (tid == 0) parts[blockIdx.x] = tot;
}

// shared checks of an image read through (batch, channel, pixel) strides
inline int image_check(const char* fn, const void* img, long bs, long cs, long ps, int B, int H, int W, int C) {
  SDHIP_CHECK_ARG(img, "%s: null image pointer", fn);
  SDHIP_CHECK_ARG(C >= 1 && C <= WI_MAX_C, "%s: C %d (1 <= C <= %d)", fn, C, WI_MAX_C);
  SDHIP_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= PM_MAX_NPIX, "%s: B %d, H %d, W %d", fn, B, H, W);
  SDHIP_CHECK_IMAGE_STRIDES(fn, bs, cs, ps);
  return 0;
}

}  // namespace

extern "C" int sdhip_warp_image_masked(const void* img, long img_bs, long img_cs, long img_ps, int in_dtype, const float* gt, void* out,
                                       int ldy, int out_dtype, int B, int H, int W, int C, void* stream) {
  if (int rc = image_check("warp_image_masked", img, img_bs, img_cs, img_ps, B, H, W, C)) return rc;
  SDHIP_CHECK_ARG(gt && out, "warp_image_masked: null disparity / output pointer");
  SDHIP_CHECK_ARG(W <= (1 << 24), "warp_image_masked: W %d (columns must be exact in f32: W <= 2^24)", W);
  SDHIP_CHECK_ARG(ldy >= C, "warp_image_masked: output pixel stride %d below C = %d", ldy, C);
  SDHIP_CHECK_DTYPE("warp_image_masked (input)", in_dtype);
  SDHIP_CHECK_DTYPE("warp_image_masked (output)", out_dtype);
  const long npix = (long)B * H * W;
  sdhip_by_dtype(in_dtype, [&](auto ti) {
    using TI = typename decltype(ti)::type;
    sdhip_by_dtype(out_dtype, [&](auto to) {
      using TO = typename decltype(to)::type;
      hipLaunchKernelGGL((warp_image_masked_kernel<TI, TO>), stream_grid(npix), dim3(256), 0, (hipStream_t)stream, (const TI*)img, img_bs,
                         img_cs, img_ps, gt, (TO*)out, ldy, H, W, C, npix);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_gate_blend_fwd(const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* y, int ldy, long npix,
                                    int C, int dtype, void* stream) {
  SDHIP_CHECK_ARG(a && b && g && y, "gate_blend_fwd: null pointer");
  SDHIP_CHECK_ARG(npix >= 1 && npix <= (1L << 40) && C >= 1 && C <= (1 << 20), "gate_blend_fwd: npix %ld, C %d", npix, C);
  SDHIP_CHECK_ARG(lda >= C && ldb >= C && ldg >= 1 && ldy >= C, "gate_blend_fwd: pixel strides %d / %d / %d / %d (a, b, g, y) for C = %d",
                  lda, ldb, ldg, ldy, C);
  SDHIP_CHECK_DTYPE("gate_blend_fwd", dtype);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {lda, ldb, ldy}, {a, b, y}), [&](auto V) {
      hipLaunchKernelGGL((gate_blend_fwd_kernel<T, V()>), stream_grid(npix * (C / Unit<T, V()>::N)), dim3(256), 0, (hipStream_t)stream,
                         (const T*)a, lda, (const T*)b, ldb, (const T*)g, ldg, (T*)y, ldy, npix, C);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_gate_blend_bwd(const void* gy, int ldgy, const void* a, int lda, const void* b, int ldb, const void* g, int ldg,
                                    void* ga, int ldga, void* gb, int ldgb, void* gg, int ldgg, long npix, int C, int dtype,
                                    void* stream) {
  SDHIP_CHECK_ARG(gy && a && b && g && ga && gb && gg, "gate_blend_bwd: null pointer");
  SDHIP_CHECK_ARG(npix >= 1 && npix <= (1L << 40) && C >= 1 && C <= (1 << 20), "gate_blend_bwd: npix %ld, C %d", npix, C);
  SDHIP_CHECK_ARG(ldgy >= C && lda >= C && ldb >= C && ldg >= 1 && ldga >= C && ldgb >= C && ldgg >= 1,
                  "gate_blend_bwd: pixel strides %d / %d / %d / %d / %d / %d / %d (gy, a, b, g, ga, gb, gg) for C = %d", ldgy, lda, ldb, ldg,
                  ldga, ldgb, ldgg, C);
  SDHIP_CHECK_DTYPE("gate_blend_bwd", dtype);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {ldgy, lda, ldb, ldga, ldgb}, {gy, a, b, ga, gb}), [&](auto V) {
      const int G = lane_group(C / Unit<T, V()>::N);
      hipLaunchKernelGGL((gate_blend_bwd_kernel<T, V()>), stream_grid(npix * G), dim3(256), 0, (hipStream_t)stream, (const T*)gy, ldgy,
                         (const T*)a, lda, (const T*)b, ldb, (const T*)g, ldg, (T*)ga, ldga, (T*)gb, ldgb, (T*)gg, ldgg, npix, C, G);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" long sdhip_photo_mse_workspace_bytes(long npix) {
  if (npix < 1 || npix > PM_MAX_NPIX) return SDHIP_ERR_ARG;
  return pm_tiles(npix) * (long)sizeof(double);
}

extern "C" int sdhip_photo_mse(const void* w, int ldw, int dtype, const float* l, long l_bs, long l_cs, long l_ps, void* grad,
                               double* loss, float weight, int B, int H, int W, int C, void* workspace, long workspace_bytes,
                               void* stream) {
  if (int rc = image_check("photo_mse", l, l_bs, l_cs, l_ps, B, H, W, C)) return rc;
  SDHIP_CHECK_ARG(w && grad && loss && workspace, "photo_mse: null pointer");
  SDHIP_CHECK_ARG(ldw >= C, "photo_mse: warped pixel stride %d below C = %d", ldw, C);
  SDHIP_CHECK_DTYPE("photo_mse", dtype);
  const long npix = (long)B * H * W;
  const long tiles = pm_tiles(npix);
  SDHIP_CHECK_WORKSPACE("photo_mse", workspace, workspace_bytes, tiles * (long)sizeof(double));
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)npix * C;
  double* parts = (double*)workspace;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((photo_mse_kernel<T>), dim3((unsigned)tiles), dim3(256), 0, s, (const T*)w, ldw, l, l_bs, l_cs, l_ps, (T*)grad, parts,
                       (float)(2.0 * (double)weight / n), (long)H * W, C, npix);
  });
  SDHIP_LAUNCH_CHECK();
  return sdhip_slot_fold(__func__, parts, tiles, (double)weight / n, loss, s);
}

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
