// Operators of the Ext_small edge networks (models/dsnet_t2_ext_small.py, output type `edgeOut`): three streaming kernels.
//
// 1. sdhip_grad_mag — the edge map netForward feeds the network (torch_implementation.py:136), compute_grad_mag(left, True, False)
//    of util/utilTorchGate.py:198-204.  Upstream's convTri returns its input (:123), the one-sided border differences are never
//    recomputed and normalize is False, so per channel, with E read as 0 outside the image:
//        Ox(y,x) = 0.5 (E(y,x+1) - E(y,x-1)),  Oy(y,x) = 0.5 (E(y+1,x) - E(y-1,x)),  mag = sqrt(Ox^2 + Oy^2 + 1e-6)
//    One thread per pixel walks the C <= 4 channels; the output is written NHWC at a pixel stride, where the conv nodes read it.
//    A 4-channel interleaved image is read as one 16-byte (f32) / 8-byte (bf16) load per neighbour; planar images are read
//    element by element, consecutive lanes on consecutive pixels.
//
// 2. sdhip_edge_bce — lossEdge_fn (losses/multiLosses.py:166-182): mean(w * BCEWithLogits(z, t)) with the class-balancing weight
//    w = N/(P+N) where t == 1, P/(P+N) where t == 0, 0 elsewhere; P and N count the ones and zeros of the whole batch.
//      edge_count_kernel   every workgroup counts P and N of its elements as integers and stores the pair in a slot of its own;
//      edge_bce_kernel     every workgroup folds the slots (integers: the order does not matter), forms both weights in f32 as the
//                          reference does, then computes max(z,0) - z t + log1p(exp(-|z|)) and the gradient w (sigmoid(z) - t) / n
//                          of its elements and stores its f64 partial of sum(w * bce) in a slot of its own;
//      slot_fold_kernel    (loss_common.h) one workgroup folds the partials in slot order: loss += sum / n.
//    No float atomics: value and gradient are bitwise reproducible.  Which elements a workgroup and a thread own depends on n
//    alone, never on alignment or strides, so the bits do not depend on how the logits are laid out either.
//
// 3. sdhip_gate_pair_fwd / _bwd — y = cat(a * g, b * (1 - g)) over the channels, g one channel, written into ONE 2C-channel NHWC
//    buffer (models/dsnet_t2_ext_small.py:361).  One 16-byte chunk per lane, the lanes of a pixel side by side; the backward
//    pass forms ga = gy_a g, gb = gy_b (1 - g) and gg = sum_c (gy_a a - gy_b b), the sum by shuffles among the pixel's lanes.
#include <math.h>

#include "loss_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ edge map
constexpr int GM_MAX_C = 4;

template <typename T> __device__ __forceinline__ void gm_load4(const T* p, float* f);
template <> __device__ __forceinline__ void gm_load4<float>(const float* p, float* f) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = v[i];
}
template <> __device__ __forceinline__ void gm_load4<bf16_t>(const bf16_t* p, float* f) {
  const u32x2 u = *reinterpret_cast<const u32x2*>(p);
  f[0] = bflo(u[0]); f[1] = bfhi(u[0]); f[2] = bflo(u[1]); f[3] = bfhi(u[1]);
}
template <typename T> __device__ __forceinline__ void gm_store4(T* p, const float* f);
template <> __device__ __forceinline__ void gm_store4<float>(float* p, const float* f) {
  *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
}
template <> __device__ __forceinline__ void gm_store4<bf16_t>(bf16_t* p, const float* f) {
  *reinterpret_cast<u32x2*>(p) = u32x2{pack2bf(f[0], f[1]), pack2bf(f[2], f[3])};
}

__device__ __forceinline__ float gm_mag(float l, float r, float u, float d) {
  const float ox = 0.5f * (r - l), oy = 0.5f * (d - u);
  return sqrtf(ox * ox + oy * oy + 1e-6f);
}

// VIN: C == 4 interleaved (channel stride 1), every pixel a 16- / 8-byte aligned chunk.  VOUT: C == 4, every output pixel likewise.
template <typename TI, typename TO, bool VIN, bool VOUT>
__global__ __launch_bounds__(256) void grad_mag_kernel(const TI* __restrict__ img, long bs, long cs, long ps, TO* __restrict__ out,
                                                       int ldy, int H, int W, int C, long npix) {
  const long row = (long)W * ps;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int x = (int)(p % W);
    const long r = p / W;
    const int y = (int)(r % H);
    const TI* q = img + (r / H) * bs + ((long)y * W + x) * ps;
    const bool hl = x > 0, hr = x < W - 1, hu = y > 0, hd = y < H - 1;
    float v[GM_MAX_C];
    if constexpr (VIN) {
      float l[4] = {0.f, 0.f, 0.f, 0.f}, rr[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
      if (hl) gm_load4<TI>(q - ps, l);
      if (hr) gm_load4<TI>(q + ps, rr);
      if (hu) gm_load4<TI>(q - row, u);
      if (hd) gm_load4<TI>(q + row, d);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = gm_mag(l[c], rr[c], u[c], d[c]);
    } else {
#pragma unroll
      for (int c = 0; c < GM_MAX_C; ++c) {
        if (c < C) {
          const TI* qc = q + c * cs;
          const float l = hl ? Elem<TI>::ld(qc - ps) : 0.f, rr = hr ? Elem<TI>::ld(qc + ps) : 0.f;
          const float u = hu ? Elem<TI>::ld(qc - row) : 0.f, d = hd ? Elem<TI>::ld(qc + row) : 0.f;
          v[c] = gm_mag(l, rr, u, d);
        }
      }
    }
    TO* o = out + p * ldy;
    if constexpr (VOUT) {
      gm_store4<TO>(o, v);
    } else {
#pragma unroll
      for (int c = 0; c < GM_MAX_C; ++c)
        if (c < C) Elem<TO>::st(o + c, v[c]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ balanced BCE
constexpr int EB_CHUNK = 4096;        // elements a workgroup handles per trip: 4 rounds of 256 threads x 4 elements
constexpr int EB_MAX_TILES = 1024;    // workgroups (slots) at most; beyond, a workgroup takes chunks b, b + tiles, ...
constexpr long EB_MAX_N = 1L << 40;

inline long eb_tiles(long n) {
  const long t = (n + EB_CHUNK - 1) / EB_CHUNK;
  return t > EB_MAX_TILES ? EB_MAX_TILES : t;
}
inline long eb_bytes(long n) { return eb_tiles(n) * (long)(2 * sizeof(unsigned long long) + sizeof(double)); }

// the four targets of elements i .. i + 3; an element past n reads as 2: neither class, weight 0
__device__ __forceinline__ void eb_targets(const float* __restrict__ t, long i, long n, bool vec, float* f) {
  if (vec && i + 4 <= n) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(t + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = i + k < n ? t[i + k] : 2.f;
  }
}

__global__ __launch_bounds__(256) void edge_count_kernel(const float* __restrict__ t, long n, bool vec,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long red[2][4];
  unsigned long long pos = 0, neg = 0;
  for (long base = (long)blockIdx.x * EB_CHUNK; base < n; base += (long)gridDim.x * EB_CHUNK) {
#pragma unroll
    for (int k = 0; k < EB_CHUNK / 1024; ++k) {
      float f[4];
      eb_targets(t, base + (long)(k * 256 + threadIdx.x) * 4, n, vec, f);
#pragma unroll
      for (int e = 0; e < 4; ++e) { pos += f[e] == 1.f; neg += f[e] == 0.f; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o, 64); neg += __shfl_xor(neg, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = pos; red[1][threadIdx.x >> 6] = neg; }
  __syncthreads();
  if (threadIdx.x < 2)
    counts[2 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

template <typename T>
__global__ __launch_bounds__(256) void edge_bce_kernel(const T* __restrict__ z, long ldz, bool zvec, const float* __restrict__ t, bool tvec,
                                                       T* __restrict__ grad, bool gvec, const unsigned long long* __restrict__ counts,
                                                       double* __restrict__ parts, long n, float inv_n) {
  __shared__ unsigned long long cnt[2][4];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  unsigned long long pos = 0, neg = 0;
  for (int i = tid; i < (int)gridDim.x; i += 256) { pos += counts[2 * i]; neg += counts[2 * i + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { pos += __shfl_xor(pos, o, 64); neg += __shfl_xor(neg, o, 64); }
  if ((tid & 63) == 0) { cnt[0][tid >> 6] = pos; cnt[1][tid >> 6] = neg; }
  __syncthreads();
  pos = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3];
  neg = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
  // f32 quotients of the f32-rounded counts, as `neg_num * 1.0 / sum_num` is (losses/multiLosses.py:175-176)
  const float sum = (float)(pos + neg);
  const float wpos = (pos + neg) ? (float)neg / sum : 0.f, wneg = (pos + neg) ? (float)pos / sum : 0.f;

  double acc = 0.0;
  for (long base = (long)blockIdx.x * EB_CHUNK; base < n; base += (long)gridDim.x * EB_CHUNK) {
#pragma unroll
    for (int k = 0; k < EB_CHUNK / 1024; ++k) {
      const long i = base + (long)(k * 256 + tid) * 4;
      if (i >= n) continue;
      const bool full = i + 4 <= n;
      float tv[4], zv[4], gv[4];
      eb_targets(t, i, n, tvec, tv);
      if (zvec && full) {
        gm_load4<T>(z + i, zv);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) zv[e] = i + e < n ? Elem<T>::ld(z + (i + e) * ldz) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float w = tv[e] == 1.f ? wpos : (tv[e] == 0.f ? wneg : 0.f);
        const float ex = expf(-fabsf(zv[e]));
        const float bce = fmaxf(zv[e], 0.f) - zv[e] * tv[e] + log1pf(ex);
        const float sg = (zv[e] >= 0.f ? 1.f : ex) / (1.f + ex);
        acc += (double)w * (double)bce;
        gv[e] = w * (sg - tv[e]) * inv_n;
      }
      if (gvec && full) {
        gm_store4<T>(grad + i, gv);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < n) Elem<T>::st(grad + i + e, gv[e]);
      }
    }
  }
  const double tot = block_tail(acc, red);
  if (tid == 0) parts[blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------------------------ gated pair
// `units` chunks of N channels per pixel
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_pair_fwd_kernel(const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb,
                                                            const T* __restrict__ g, int ldg, T* __restrict__ y, int ldy, long npix, int C) {
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
    for (int e = 0; e < N; ++e) { av[e] *= gv; bv[e] *= hv; }
    Unit<T, VEC>::store(y + pix * ldy + c0, av);
    Unit<T, VEC>::store(y + pix * ldy + C + c0, bv);
  }
}

// a pixel's chunks are handled by G = 2^k lanes side by side, G >= min(units, 64): lane s takes the chunks s, s + G, ...
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gate_pair_bwd_kernel(const T* __restrict__ gy, int ldgy, const T* __restrict__ a, int lda,
                                                            const T* __restrict__ b, int ldb, const T* __restrict__ g, int ldg,
                                                            T* __restrict__ ga, int ldga, T* __restrict__ gb, int ldgb, T* __restrict__ gg,
                                                            int ldgg, long npix, int C, int G) {
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
        float ya[N], yb[N], av[N], bv[N];
        Unit<T, VEC>::load(gy + pix * ldgy + c0, ya);
        Unit<T, VEC>::load(gy + pix * ldgy + C + c0, yb);
        Unit<T, VEC>::load(a + pix * lda + c0, av);
        Unit<T, VEC>::load(b + pix * ldb + c0, bv);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          s = fmaf(ya[e], av[e], s);
          s = fmaf(-yb[e], bv[e], s);
          ya[e] *= gv;
          yb[e] *= hv;
        }
        Unit<T, VEC>::store(ga + pix * ldga + c0, ya);
        Unit<T, VEC>::store(gb + pix * ldgb + c0, yb);
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (pix < npix && sub == 0) Elem<T>::st(gg + pix * ldgg, s);
  }
}

}  // namespace

extern "C" int sdhip_grad_mag(const void* img, long img_bs, long img_cs, long img_ps, int in_dtype, void* out, int ldy, int out_dtype,
                              int B, int H, int W, int C, void* stream) {
  SDHIP_CHECK_ARG(img && out, "grad_mag: null pointer");
  SDHIP_CHECK_ARG(C >= 1 && C <= GM_MAX_C, "grad_mag: C %d (1 <= C <= %d)", C, GM_MAX_C);
  SDHIP_CHECK_ARG(B >= 1 && H >= 2 && W >= 2 && (long)B * H * W <= (1L << 40), "grad_mag: B %d, H %d, W %d (B >= 1, H and W >= 2)", B, H, W);
  SDHIP_CHECK_IMAGE_STRIDES("grad_mag", img_bs, img_cs, img_ps);
  SDHIP_CHECK_ARG(ldy >= C, "grad_mag: output pixel stride %d below C = %d", ldy, C);
  SDHIP_CHECK_DTYPE("grad_mag (input)", in_dtype);
  SDHIP_CHECK_DTYPE("grad_mag (output)", out_dtype);
  const long npix = (long)B * H * W;
  const uintptr_t ia = (uintptr_t)img, oa = (uintptr_t)out;
  const size_t ib = in_dtype == SDHIP_F32 ? 4 : 2, ob = out_dtype == SDHIP_F32 ? 4 : 2;
  const bool vin = C == 4 && img_cs == 1 && img_ps % 4 == 0 && img_bs % 4 == 0 && (ia & (4 * ib - 1)) == 0;
  const bool vout = C == 4 && ldy % 4 == 0 && (oa & (4 * ob - 1)) == 0;
  sdhip_by_dtype(in_dtype, [&](auto ti) {
    using TI = typename decltype(ti)::type;
    sdhip_by_dtype(out_dtype, [&](auto to) {
      using TO = typename decltype(to)::type;
      sdhip_by_flag(vin, [&](auto VI) {
        sdhip_by_flag(vout, [&](auto VO) {
          hipLaunchKernelGGL((grad_mag_kernel<TI, TO, VI(), VO()>), stream_grid(npix), dim3(256), 0, (hipStream_t)stream, (const TI*)img, img_bs,
                             img_cs, img_ps, (TO*)out, ldy, H, W, C, npix);
        });
      });
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" long sdhip_edge_bce_workspace_bytes(long n) {
  if (n < 1 || n > EB_MAX_N) return SDHIP_ERR_ARG;
  return eb_bytes(n);
}

extern "C" int sdhip_edge_bce(const void* logits, long ldz, int dtype, const float* target, void* grad, double* loss, long n,
                              void* workspace, long workspace_bytes, void* stream) {
  SDHIP_CHECK_ARG(logits && target && grad && loss && workspace, "edge_bce: null pointer");
  SDHIP_CHECK_ARG(n >= 1 && n <= EB_MAX_N, "edge_bce: n %ld (1 <= n <= 2^40)", n);
  SDHIP_CHECK_ARG(ldz >= 1, "edge_bce: logit stride %ld must be positive", ldz);
  SDHIP_CHECK_DTYPE("edge_bce", dtype);
  const long need = eb_bytes(n);
  SDHIP_CHECK_WORKSPACE("edge_bce", workspace, workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const long tiles = eb_tiles(n);
  unsigned long long* counts = (unsigned long long*)workspace;
  double* parts = (double*)(counts + 2 * tiles);
  const size_t eb = dtype == SDHIP_F32 ? 4 : 2;
  const bool tvec = (((uintptr_t)target) & 15) == 0;
  const bool zvec = ldz == 1 && (((uintptr_t)logits) & (4 * eb - 1)) == 0;
  const bool gvec = (((uintptr_t)grad) & (4 * eb - 1)) == 0;
  hipLaunchKernelGGL(edge_count_kernel, dim3((unsigned)tiles), dim3(256), 0, s, target, n, tvec, counts);
  SDHIP_LAUNCH_CHECK();
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((edge_bce_kernel<T>), dim3((unsigned)tiles), dim3(256), 0, s, (const T*)logits, ldz, zvec, target, tvec, (T*)grad, gvec,
                       (const unsigned long long*)counts, parts, n, (float)(1.0 / (double)n));
  });
  SDHIP_LAUNCH_CHECK();
  return sdhip_slot_fold(__func__, parts, tiles, 1.0 / (double)n, loss, s);
}

extern "C" int sdhip_gate_pair_fwd(const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* y, int ldy, long npix,
                                   int C, int dtype, void* stream) {
  SDHIP_CHECK_ARG(a && b && g && y, "gate_pair_fwd: null pointer");
  SDHIP_CHECK_ARG(npix >= 1 && npix <= (1L << 40) && C >= 1 && C <= (1 << 20), "gate_pair_fwd: npix %ld, C %d", npix, C);
  SDHIP_CHECK_ARG(lda >= C && ldb >= C && ldg >= 1 && ldy >= 2 * C, "gate_pair_fwd: pixel strides %d / %d / %d / %d (a, b, g, y) for C = %d",
                  lda, ldb, ldg, ldy, C);
  SDHIP_CHECK_DTYPE("gate_pair_fwd", dtype);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {lda, ldb, ldy}, {a, b, y}), [&](auto V) {
      hipLaunchKernelGGL((gate_pair_fwd_kernel<T, V()>), stream_grid(npix * (C / Unit<T, V()>::N)), dim3(256), 0, (hipStream_t)stream, (const T*)a,
                         lda, (const T*)b, ldb, (const T*)g, ldg, (T*)y, ldy, npix, C);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_gate_pair_bwd(const void* gy, int ldgy, const void* a, int lda, const void* b, int ldb, const void* g, int ldg, void* ga,
                                   int ldga, void* gb, int ldgb, void* gg, int ldgg, long npix, int C, int dtype, void* stream) {
  SDHIP_CHECK_ARG(gy && a && b && g && ga && gb && gg, "gate_pair_bwd: null pointer");
  SDHIP_CHECK_ARG(npix >= 1 && npix <= (1L << 40) && C >= 1 && C <= (1 << 20), "gate_pair_bwd: npix %ld, C %d", npix, C);
  SDHIP_CHECK_ARG(ldgy >= 2 * C && lda >= C && ldb >= C && ldg >= 1 && ldga >= C && ldgb >= C && ldgg >= 1,
                  "gate_pair_bwd: pixel strides %d / %d / %d / %d / %d / %d / %d (gy, a, b, g, ga, gb, gg) for C = %d", ldgy, lda, ldb, ldg, ldga,
                  ldgb, ldgg, C);
  SDHIP_CHECK_DTYPE("gate_pair_bwd", dtype);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {ldgy, lda, ldb, ldga, ldgb}, {gy, a, b, ga, gb}), [&](auto V) {
      const int G = lane_group(C / Unit<T, V()>::N);
      hipLaunchKernelGGL((gate_pair_bwd_kernel<T, V()>), stream_grid(npix * G), dim3(256), 0, (hipStream_t)stream, (const T*)gy, ldgy, (const T*)a,
                         lda, (const T*)b, ldb, (const T*)g, ldg, (T*)ga, ldga, (T*)gb, ldgb, (T*)gg, ldgg, npix, C, G);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
