// MobileNetV3-Large operators for gfx950: depthwise convolution (forward, data gradient, weight gradient) and the
// squeeze-excite MLP (models/mobilenetv3.py:64-77,99,110).
//
// Depthwise layers are memory / latency bound (k*k FMAs per loaded element): plain VALU FMA in f32, no MFMA.
//   * a thread owns one 16-byte channel chunk (8 bf16 / 4 f32; element-wise when C, ld or a pointer is not 16-byte
//     aligned) and R = 4 neighbouring outputs of one row: a source column is loaded once per kernel row and feeds every
//     output of the strip it reaches (for k = 3 / stride 1: 6 loads per row for 4 outputs instead of 12);
//   * the block's weights are staged in LDS as [tap][channel] (the parameter is (C, 1, k, k)), so a thread reads the k
//     weights of a row as 16-byte LDS vectors;
//   * the data gradient is the same gather with the roles of input and output exchanged: a stride-2 layer reads, per
//     input pixel, only the ceil(k/2)^2 output pixels whose taps reach it (the column / tap pairing is resolved at
//     compile time from the strip's parity), without zero-stuffing and without atomics;
//   * the forward epilogue sums (x, x^2) per statistics group for the BatchNorm behind the layer (a block reduction in LDS,
//     one f64 atomic per block and channel) and, optionally, x per image for SELayer's average pool: each block stores its
//     partial sums in a slot of its own, and the SE kernel adds the slots in a fixed order (deterministic);
//   * the weight gradient stores per-block partials [block][tap][channel] (no atomics) and a second launch sums them in a
//     fixed order into the (C, 1, k, k) parameter gradient.
#include "sdhip_common.h"

namespace {

constexpr int DW_R = 4;   // outputs per thread along W

struct DwGeom {
  int tx, ty, units;      // threads across channel units / across strips; channel units (16-byte chunks or elements)
};

inline DwGeom dw_geom(int units) {
  DwGeom g;
  g.units = units;
  g.tx = units < 64 ? units : 64;
  g.ty = 256 / g.tx;
  return g;
}

__host__ __device__ constexpr int dw_kw(bool bwd, int K, int S, int d, int r) {
  // tap column pairing source column d (relative) with strip output r; see dw_gather
  return bwd ? r + (K - 1) / 2 - S * d : d + (K - 1) / 2 - S * r;
}

__host__ __device__ constexpr bool dw_col_used(bool bwd, int K, int S, int d) {
  for (int r = 0; r < DW_R; ++r) {
    const int kw = dw_kw(bwd, K, S, d, r);
    if (kw >= 0 && kw < K) return true;
  }
  return false;
}

// Stage w (C, k*k) f32 of channels [cb0, cb0 + nch) as wl[t][nch] (zero beyond C).
__device__ __forceinline__ void dw_stage_weights(const float* __restrict__ w, float* wl, int cb0, int nch, int C, int KK) {
  for (int i = threadIdx.x; i < nch * KK; i += blockDim.x) {
    const int cl = i / KK, t = i - cl * KK;
    const int c = cb0 + cl;
    wl[t * nch + cl] = c < C ? w[(long)c * KK + t] : 0.f;
  }
}

// One strip of DW_R outputs (row `orow`, columns o0 .. o0+R-1 of an image) gathered from the source image.
//   forward : out = y (Ho x Wo), src = x (H x W):   src row  = orow*S - P + kh,  src col = o0*S + d,  kw = d + P - S*r
//   backward: out = gx (H x W), src = gy (Ho x Wo): src row  = (orow + P - kh)/S when integral,  src col = o0/S + d,
//             kw = r + P - S*d   (o0 is a multiple of R, hence of S)
template <typename T, bool VEC, int K, int S, bool BWD>
__device__ __forceinline__ void dw_gather(const T* __restrict__ src, int lds, int SH, int SW, const float* wl, int nch, int cl,
                                          int orow, int o0, float (&acc)[DW_R][Unit<T, VEC>::N]) {
  constexpr int N = Unit<T, VEC>::N;
  constexpr int P = (K - 1) / 2;
  constexpr int DLO = BWD ? -K : -P;
  constexpr int DHI = BWD ? DW_R + P : (DW_R - 1) * S + K - 1 - P;
#pragma unroll
  for (int r = 0; r < DW_R; ++r)
#pragma unroll
    for (int e = 0; e < N; ++e) acc[r][e] = 0.f;
#pragma unroll
  for (int kh = 0; kh < K; ++kh) {
    int srow;
    if constexpr (BWD) {
      const int t = orow + P - kh;
      if (t < 0 || (S == 2 && (t & 1))) continue;
      srow = t / S;
    } else {
      srow = orow * S - P + kh;
    }
    if (srow < 0 || srow >= SH) continue;
    float wr[K][N];
#pragma unroll
    for (int kw = 0; kw < K; ++kw)
#pragma unroll
      for (int e = 0; e < N; ++e) wr[kw][e] = wl[(kh * K + kw) * nch + cl + e];
    const T* rowp = src + (long)srow * SW * lds;
    const int cbase = BWD ? o0 / S : o0 * S;
#pragma unroll
    for (int d = DLO; d <= DHI; ++d) {
      if (!dw_col_used(BWD, K, S, d)) continue;
      const int scol = cbase + d;
      if (scol < 0 || scol >= SW) continue;
      float v[N];
      Unit<T, VEC>::load(rowp + (long)scol * lds, v);
#pragma unroll
      for (int r = 0; r < DW_R; ++r) {
        const int kw = dw_kw(BWD, K, S, d, r);
        if (kw >= 0 && kw < K) {
#pragma unroll
          for (int e = 0; e < N; ++e) acc[r][e] = fmaf(v[e], wr[kw][e], acc[r][e]);
        }
      }
    }
  }
}

// Forward (BWD = false) and data gradient (BWD = true).  grid: (strip blocks, channel-unit groups, images).
template <typename T, bool VEC, int K, int S, bool BWD>
__global__ __launch_bounds__(256) void dw_conv_kernel(const T* __restrict__ src, int lds, const float* __restrict__ w,
                                                      T* __restrict__ out, int ldo, double* __restrict__ stats, int sld, int nrep,
                                                      float* __restrict__ pool, int pool_parts, int SH, int SW, int OH, int OW, int C,
                                                      int imgs_per_group, DwGeom dg) {
  constexpr int N = Unit<T, VEC>::N;
  constexpr int KK = K * K;
  constexpr int WL = KK * 64 * N;
  constexpr int RED = 2 * 256 * N;
  __shared__ float lds_buf[WL > RED ? WL : RED];
  const int nch = dg.tx * N;
  const int cb0 = blockIdx.y * nch;
  dw_stage_weights(w, lds_buf, cb0, nch, C, KK);
  __syncthreads();
  const int tx = threadIdx.x % dg.tx, ty = threadIdx.x / dg.tx;
  const int u = blockIdx.y * dg.tx + tx;
  const int b = blockIdx.z;
  const int nstrip_row = (OW + DW_R - 1) / DW_R;
  const int q = blockIdx.x * dg.ty + ty;
  const bool live = ty < dg.ty && u < dg.units && q < OH * nstrip_row;
  const int c0 = u * N;
  float s1[N], s2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  if (live) {
    const int orow = q / nstrip_row;
    const int o0 = (q - orow * nstrip_row) * DW_R;
    float acc[DW_R][N];
    dw_gather<T, VEC, K, S, BWD>(src + (long)b * SH * SW * lds + c0, lds, SH, SW, lds_buf, nch, tx * N, orow, o0, acc);
    T* op = out + ((long)b * OH + orow) * OW * ldo + c0;
#pragma unroll
    for (int r = 0; r < DW_R; ++r) {
      if (o0 + r < OW) {
        float f[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
          f[e] = Elem<T>::rnd(acc[r][e]);
          s1[e] += f[e];
          s2[e] = fmaf(f[e], f[e], s2[e]);
        }
        Unit<T, VEC>::store(op + (long)(o0 + r) * ldo, f);
      }
    }
  }
  if (BWD || (!stats && !pool)) return;   // uniform
  __syncthreads();                         // the weight tile is dead: its LDS takes the block reduction
  float* r1 = lds_buf;
  float* r2 = lds_buf + 256 * N;
#pragma unroll
  for (int e = 0; e < N; ++e) { r1[threadIdx.x * N + e] = s1[e]; r2[threadIdx.x * N + e] = s2[e]; }
  __syncthreads();
  // thread i < nch sums channel cb0 + i over the ty rows
  for (int i = threadIdx.x; i < nch; i += blockDim.x) {
    const int c = cb0 + i;
    if (c >= C) continue;
    const int txi = i / N, e = i - txi * N;
    float a = 0.f, q2 = 0.f;
    for (int y = 0; y < dg.ty; ++y) {
      a += r1[(y * dg.tx + txi) * N + e];
      q2 += r2[(y * dg.tx + txi) * N + e];
    }
    if (stats) {
      const int g = b / imgs_per_group;
      double* sp = stats + ((long)(blockIdx.x % nrep) * (gridDim.z / imgs_per_group) + g) * 2 * sld;
      atomicAdd(sp + c, (double)a);
      atomicAdd(sp + sld + c, (double)q2);
    }
    if (pool) pool[((long)b * pool_parts + blockIdx.x) * C + c] = a;   // slot blockIdx.x of image b
  }
}

// Weight gradient: block (strip blocks, channel-unit groups, kernel row kh); each thread walks strips of the whole batch,
// accumulating the K taps of row kh for its N channels in registers; LDS reduction over the strip rows, then the block
// stores its partial sums to part[blockIdx.x][kh*K + kw][c] (channel-contiguous, every element written by one block).
template <typename T, bool VEC, int K, int S>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ gy, int ldg,
                                                       float* __restrict__ part, int B, int H, int W, int Ho, int Wo, int C, DwGeom dg) {
  constexpr int N = Unit<T, VEC>::N;
  constexpr int P = (K - 1) / 2;
  __shared__ float red[256 * K * N];
  const int tx = threadIdx.x % dg.tx, ty = threadIdx.x / dg.tx;
  const int u = blockIdx.y * dg.tx + tx;
  const int kh = blockIdx.z;
  const int nstrip_row = (Wo + DW_R - 1) / DW_R;
  const long nstrip = (long)B * Ho * nstrip_row;
  const int c0 = u * N;
  float acc[K][N];
#pragma unroll
  for (int kw = 0; kw < K; ++kw)
#pragma unroll
    for (int e = 0; e < N; ++e) acc[kw][e] = 0.f;
  if (ty < dg.ty && u < dg.units) {
    for (long q = (long)blockIdx.x * dg.ty + ty; q < nstrip; q += (long)gridDim.x * dg.ty) {
      const int b = (int)(q / ((long)Ho * nstrip_row));
      const int rem = (int)(q - (long)b * Ho * nstrip_row);
      const int oh = rem / nstrip_row;
      const int o0 = (rem - oh * nstrip_row) * DW_R;
      const int ih = oh * S - P + kh;
      if (ih < 0 || ih >= H) continue;
      float g[DW_R][N];
      const T* gp = gy + ((long)b * Ho + oh) * Wo * ldg + c0;
#pragma unroll
      for (int r = 0; r < DW_R; ++r) {
        if (o0 + r < Wo) Unit<T, VEC>::load(gp + (long)(o0 + r) * ldg, g[r]);
        else {
#pragma unroll
          for (int e = 0; e < N; ++e) g[r][e] = 0.f;
        }
      }
      const T* xr = x + ((long)b * H + ih) * W * ldx + c0;
#pragma unroll
      for (int d = -P; d <= (DW_R - 1) * S + K - 1 - P; ++d) {
        const int col = o0 * S + d;
        if (col < 0 || col >= W) continue;
        float v[N];
        Unit<T, VEC>::load(xr + (long)col * ldx, v);
#pragma unroll
        for (int r = 0; r < DW_R; ++r) {
          const int kw = d + P - S * r;
          if (kw >= 0 && kw < K) {
#pragma unroll
            for (int e = 0; e < N; ++e) acc[kw][e] = fmaf(v[e], g[r][e], acc[kw][e]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int kw = 0; kw < K; ++kw)
#pragma unroll
    for (int e = 0; e < N; ++e) red[(kw * 256 + threadIdx.x) * N + e] = acc[kw][e];
  __syncthreads();
  const int nch = dg.tx * N;
  const int cb0 = blockIdx.y * nch;
  for (int i = threadIdx.x; i < nch * K; i += blockDim.x) {
    const int kw = i / nch, cl = i - kw * nch;
    const int c = cb0 + cl;
    if (c >= C) continue;
    const int txi = cl / N, e = cl - txi * N;
    float a = 0.f;
    for (int y = 0; y < dg.ty; ++y) a += red[(kw * 256 + y * dg.tx + txi) * N + e];
    part[((long)blockIdx.x * K * K + kh * K + kw) * C + c] = a;
  }
}

// dw[c][t] += sum over the partial slots in a fixed order (deterministic): a block serves 32 consecutive (t, c) outputs with
// 8 lanes each; lane j sums the slots p = j, j + 8, ... in order, and the 8 lane sums are added in lane order.
__global__ __launch_bounds__(256) void dw_wgrad_sum_kernel(const float* __restrict__ part, int nparts, float* __restrict__ dw, int KK,
                                                           int C) {
  __shared__ float red[8][32];
  const int o = threadIdx.x & 31, j = threadIdx.x >> 5;
  const long i = (long)blockIdx.x * 32 + o;
  const long n = (long)KK * C;
  float a = 0.f;
  if (i < n)
    for (int p = j; p < nparts; p += 8) a += part[(long)p * n + i];
  red[j][o] = a;
  __syncthreads();
  if (j == 0 && i < n) {
#pragma unroll
    for (int q = 1; q < 8; ++q) a += red[q][o];
    const int t = (int)(i / C), c = (int)(i - (long)t * C);
    dw[(long)c * KK + t] += a;
  }
}

// (k, stride) of the plain depthwise kernels -> template arguments (the entry points admit k = 3 / 5 and stride = 1 / 2 only)
template <typename F>
void dw_by_ks(int k, int stride, F&& f) {
  sdhip_by_flag(k == 5, [&](auto K5) { sdhip_by_flag(stride == 2, [&](auto S2) {
    f(std::integral_constant<int, K5() ? 5 : 3>{}, std::integral_constant<int, S2() ? 2 : 1>{});
  }); });
}

// forward (bwd = false: src = x, out = y) and data gradient (bwd = true: src = gy, out = gx) are one kernel
void dw_conv(bool bwd, int dtype, int k, int stride, const void* src, int lds, const float* w, void* out, int ldo, double* stats, int sld,
             int nrep, float* pool, int pool_parts, int B, int SH, int SW, int OH, int OW, int C, int ipg, hipStream_t s) {
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {lds, ldo}, {src, out}), [&](auto V) { sdhip_by_flag(bwd, [&](auto BWD) {
      dw_by_ks(k, stride, [&](auto K, auto S) {
        const DwGeom dg = dw_geom(C / Unit<T, V()>::N);
        const int nstrip = OH * ((OW + DW_R - 1) / DW_R);
        dim3 grid((unsigned)sdhip_cdiv(nstrip, dg.ty), (unsigned)sdhip_cdiv(dg.units, dg.tx), (unsigned)B);
        hipLaunchKernelGGL((dw_conv_kernel<T, V(), K(), S(), BWD()>), grid, dim3(256), 0, s, (const T*)src, lds, w, (T*)out, ldo, stats, sld,
                           nrep, pool, pool_parts, SH, SW, OH, OW, C, ipg, dg);
      });
    }); });
  });
}

inline int dw_out(int n, int k, int s) { return (n + 2 * ((k - 1) / 2) - k) / s + 1; }

// strip blocks of the weight gradient: ~16 K (strip x channel) items each, at most 256 (independent of the vector path, so
// that the caller can size the partial slab from the shape alone)
inline int dw_wgrad_parts(int B, int H, int W, int C, int k, int stride) {
  const long nstrip = (long)B * dw_out(H, k, stride) * ((dw_out(W, k, stride) + DW_R - 1) / DW_R);
  long bx = (nstrip * C + 16383) / 16384;
  return (int)(bx < 1 ? 1 : (bx > 256 ? 256 : bx));
}

// pool slots of the forward: its strip-block count on the vector or the element-wise path, whichever is larger
inline int dw_pool_parts(int H, int W, int C, int k, int stride, int dtype) {
  const int Ho = dw_out(H, k, stride), Wo = dw_out(W, k, stride);
  const int nstrip = Ho * ((Wo + DW_R - 1) / DW_R);
  const int N = sdhip_by_dtype(dtype, [](auto tag) { return Chunk<typename decltype(tag)::type>::N; });
  int parts = sdhip_cdiv(nstrip, dw_geom(C).ty);
  if (C % N == 0) {
    const int pv = sdhip_cdiv(nstrip, dw_geom(C / N).ty);
    if (pv > parts) parts = pv;
  }
  return parts;
}

// ---------------------------------------------------------------------------------------------------------------- SE MLP
// One launch per direction; a block serves SE_IMGS images, so each weight row read from L2 feeds SE_IMGS dot products and
// each parameter-gradient atomic carries the sum of SE_IMGS images.  Rows of w1 (r, C) are read across lanes (coalesced);
// w2 (C, r) is read with lanes across r.
constexpr int SE_IMGS = 4;
constexpr int SE_MAXC = 1024;   // LDS capacity per image (largest SELayer: 960 channels, 240 hidden)
constexpr int SE_THREADS = 1024;   // 16 waves: the MLP is latency bound (a few rows per wave, unrolled independent loads)
constexpr int SE_WAVES = SE_THREADS / 64;

__global__ __launch_bounds__(SE_THREADS) void se_fwd_kernel(const float* __restrict__ pool, int parts, float inv_hw,
                                                     const float* __restrict__ scale,
                                                     const float* __restrict__ shift, int imgs_per_group,
                                                     const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ s_out, float* __restrict__ ws, int B, int C, int r) {
  __shared__ float v[SE_IMGS][SE_MAXC];
  __shared__ float h[SE_IMGS][SE_MAXC / 4];
  const int b0 = blockIdx.x * SE_IMGS;
  const int nimg = min(SE_IMGS, B - b0);
  float* ws_v = ws;
  float* ws_h = ws + (long)B * C;
  float* ws_a = ws_h + (long)B * r;
  for (int i = threadIdx.x; i < SE_IMGS * C; i += blockDim.x) {
    const int m = i / C, c = i - m * C;
    float val = 0.f;
    if (m < nimg) {
      const int b = b0 + m;
      for (int p = 0; p < parts; ++p) val += pool[((long)b * parts + p) * C + c];   // slot order: deterministic
      val *= inv_hw;
      if (scale) {
        const int g = b / imgs_per_group;
        val = fmaf(val, scale[(long)g * C + c], shift[(long)g * C + c]);
      }
      ws_v[(long)b * C + c] = val;
    }
    v[m][c] = val;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < r; j += SE_WAVES) {   // fc1: a wave per hidden unit, lanes across C
    float a[SE_IMGS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
      const float wv = w1[(long)j * C + c];
#pragma unroll
      for (int m = 0; m < SE_IMGS; ++m) a[m] = fmaf(wv, v[m][c], a[m]);
    }
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) {
      const float t = fmaxf(wave_sum(a[m]) + b1[j], 0.f);
      if (lane == 0) {
        h[m][j] = t;
        if (m < nimg) ws_h[(long)(b0 + m) * r + j] = t;
      }
    }
  }
  __syncthreads();
  for (int c = wave; c < C; c += SE_WAVES) {   // fc2: a wave per channel, lanes across r
    float a[SE_IMGS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = lane; j < r; j += 64) {
      const float wv = w2[(long)c * r + j];
#pragma unroll
      for (int m = 0; m < SE_IMGS; ++m) a[m] = fmaf(wv, h[m][j], a[m]);
    }
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) {
      const float t = wave_sum(a[m]) + b2[c];
      if (lane == 0 && m < nimg) {
        ws_a[(long)(b0 + m) * C + c] = t;
        s_out[(long)(b0 + m) * C + c] = hsig_f(t);
      }
    }
  }
}

__global__ __launch_bounds__(SE_THREADS) void se_bwd_kernel(const float* __restrict__ ds, int nrep, const float* __restrict__ ws,
                                                     const float* __restrict__ w1, const float* __restrict__ w2,
                                                     float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                                                     float* __restrict__ gb2, float* __restrict__ gpool, float inv_hw,
                                                     int B, int C, int r) {
  __shared__ float da2[SE_IMGS][SE_MAXC];
  __shared__ float hh[SE_IMGS][SE_MAXC / 4];
  __shared__ float da1[SE_IMGS][SE_MAXC / 4];
  __shared__ float dhp[SE_THREADS / 256][SE_IMGS][SE_MAXC / 4];   // partial dh of each quarter of the channels
  const int b0 = blockIdx.x * SE_IMGS;
  const int nimg = min(SE_IMGS, B - b0);
  const float* ws_v = ws;
  const float* ws_h = ws + (long)B * C;
  const float* ws_a = ws_h + (long)B * r;
  for (int i = threadIdx.x; i < SE_IMGS * C; i += blockDim.x) {
    const int m = i / C, c = i - m * C;
    float g = 0.f;
    if (m < nimg) {
      const long bc = (long)(b0 + m) * C + c;
      float sum = 0.f;
      for (int k = 0; k < nrep; ++k) sum += ds[(long)k * B * C + bc];
      g = sum * act_hs_d(ws_a[bc], SDHIP_ACT_HSIGMOID);
    }
    da2[m][c] = g;
  }
  for (int i = threadIdx.x; i < SE_IMGS * r; i += blockDim.x) {
    const int m = i / r, j = i - m * r;
    hh[m][j] = m < nimg ? ws_h[(long)(b0 + m) * r + j] : 0.f;
  }
  __syncthreads();
  // fc2: gb2[c] += sum_m da2, gw2[c][j] += sum_m da2[m][c] h[m][j]; dh[m][j] = sum_c w2[c][j] da2[m][c]  (thread per j)
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = 0.f;
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) a += da2[m][c];
    atomicAdd(gb2 + c, a);
  }
  {
    const int j = threadIdx.x % 256, qr = threadIdx.x / 256;     // hidden unit, quarter of the channel range
    const int cq0 = (int)((long)C * qr / (SE_THREADS / 256)), cq1 = (int)((long)C * (qr + 1) / (SE_THREADS / 256));
    float dh[SE_IMGS] = {0.f, 0.f, 0.f, 0.f};
    if (j < r) {
      float hj[SE_IMGS];
#pragma unroll
      for (int m = 0; m < SE_IMGS; ++m) hj[m] = hh[m][j];
#pragma unroll 4
      for (int c = cq0; c < cq1; ++c) {
        const float wv = w2[(long)c * r + j];
        float gsum = 0.f;
#pragma unroll
        for (int m = 0; m < SE_IMGS; ++m) {
          dh[m] = fmaf(wv, da2[m][c], dh[m]);
          gsum = fmaf(da2[m][c], hj[m], gsum);
        }
        atomicAdd(gw2 + (long)c * r + j, gsum);
      }
    }
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) dhp[qr][m][j] = dh[m];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SE_IMGS * r; i += blockDim.x) {
    const int m = i / r, j = i - m * r;
    float dh = 0.f;
#pragma unroll
    for (int q = 0; q < SE_THREADS / 256; ++q) dh += dhp[q][m][j];
    da1[m][j] = hh[m][j] > 0.f ? dh : 0.f;
  }
  __syncthreads();
  // fc1: gb1[j] += sum_m da1, gw1[j][c] += sum_m da1[m][j] v[m][c]; dv[m][c] = sum_j w1[j][c] da1[m][j]  (thread per c)
  for (int j = threadIdx.x; j < r; j += blockDim.x) {
    float a = 0.f;
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) a += da1[m][j];
    atomicAdd(gb1 + j, a);
  }
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float vc[SE_IMGS], dv[SE_IMGS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m) vc[m] = m < nimg ? ws_v[(long)(b0 + m) * C + c] : 0.f;
#pragma unroll 4
    for (int j = 0; j < r; ++j) {
      const float wv = w1[(long)j * C + c];
      float gsum = 0.f;
#pragma unroll
      for (int m = 0; m < SE_IMGS; ++m) {
        dv[m] = fmaf(wv, da1[m][j], dv[m]);
        gsum = fmaf(da1[m][j], vc[m], gsum);
      }
      atomicAdd(gw1 + (long)j * C + c, gsum);
    }
#pragma unroll
    for (int m = 0; m < SE_IMGS; ++m)
      if (m < nimg) gpool[(long)(b0 + m) * C + c] = dv[m] * inv_hw;
  }
}

// gx = gy * act'(x*s) * s + gadd   (per image b = blockIdx.z)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void se_scale_bwd_kernel(const T* __restrict__ gy, int ldg, const T* __restrict__ x, int ldx,
                                                           T* __restrict__ gx, int ldgx, const float* __restrict__ s,
                                                           const float* __restrict__ gadd, long npix, int C, int act, DwGeom dg) {
  constexpr int N = Unit<T, VEC>::N;
  const int tx = threadIdx.x % dg.tx, ty = threadIdx.x / dg.tx;
  const int u = blockIdx.y * dg.tx + tx;
  if (ty >= dg.ty || u >= dg.units) return;
  const int b = blockIdx.z, c0 = u * N;
  float sc[N], ad[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { sc[e] = s[(long)b * C + c0 + e]; ad[e] = gadd ? gadd[(long)b * C + c0 + e] : 0.f; }
  const long base = (long)b * npix;
  for (long p = (long)blockIdx.x * dg.ty + ty; p < npix; p += (long)gridDim.x * dg.ty) {
    float g[N], xv[N];
    Unit<T, VEC>::load(gy + (base + p) * ldg + c0, g);
    Unit<T, VEC>::load(x + (base + p) * ldx + c0, xv);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float z = xv[e] * sc[e];
      float gm = g[e];
      if (act == 1) gm = z > 0.f ? gm : 0.f;
      else if (act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID) gm *= act_hs_d(z, act);
      g[e] = fmaf(gm, sc[e], ad[e]);
    }
    Unit<T, VEC>::store(gx + (base + p) * ldgx + c0, g);
  }
}

// ------------------------------------------------------------------------------------------ dilated depthwise 3x3
// SeparableConv2d of DeepLabV3+ / Xception-65 (models_deeplab_mod/common.py:24-50): nn.Conv2d(C, C, 3, stride, padding=d,
// dilation=d, groups=C).  With a dilation the neighbouring outputs of a row share no source column, so a thread gathers the
// nine taps of one output pixel for one 16-byte channel chunk, and walks up to DWD_MAX_PIX pixels so that the weight tile in
// LDS is staged once for all of them; a tap outside the map costs a compare, no load (for the ASPP dilations 12 / 24 / 36
// on a 33 x 65 map most taps are outside).  The nine-fold reuse of the source is left to
// L2 / the Infinity Cache; that HBM then sees the source once is the design's assumption — no counter run has measured it.
//   * the channel tail is masked: the last chunk of a channel count that is no multiple of the chunk (304, 412 in bf16) is
//     loaded and stored element by element, so the vector path needs aligned pointers and strides only;
//   * IN_RELU (relu_first of SeparableConv2d): the forward rectifies in the load; the data gradient multiplies by [x > 0]
//     read at the pixel it writes; the weight gradient rectifies x in the load — the un-rectified x stays the saved tensor;
//   * the data gradient is the same gather over gy: tap (kh, kw) of input pixel (ih, iw) reads output pixel
//     ((ih - (kh-1) d) / s, (iw - (kw-1) d) / s) where that is integral and inside — no zero-stuffing, no atomics.
constexpr int DWD_MAX_PIX = 16;   // pixels per thread of the forward / data gradient (the statistics add them in f32)

template <typename T, bool VEC>
__device__ __forceinline__ void dwd_load(const T* p, float* f, int n) {
  constexpr int N = Unit<T, VEC>::N;
  if (n >= N) { Unit<T, VEC>::load(p, f); return; }
#pragma unroll
  for (int e = 0; e < N; ++e) f[e] = e < n ? Elem<T>::ld(p + e) : 0.f;
}

template <typename T, bool VEC>
__device__ __forceinline__ void dwd_store(T* p, const float* f, int n) {
  constexpr int N = Unit<T, VEC>::N;
  if (n >= N) { Unit<T, VEC>::store(p, f); return; }
#pragma unroll
  for (int e = 0; e < N; ++e)
    if (e < n) Elem<T>::st(p + e, f[e]);
}

// source index of tap k (0..2) for output index o: forward o*S + (k-1)*D, backward (o - (k-1)*D) / S when integral; -1: none
template <bool BWD>
__device__ __forceinline__ int dwd_src(int o, int k, int S, int D, int n) {
  int s;
  if constexpr (BWD) {
    const int t = o - (k - 1) * D;
    if (t < 0 || (S == 2 && (t & 1))) return -1;
    s = S == 2 ? t >> 1 : t;
  } else {
    s = o * S + (k - 1) * D;
  }
  return (s < 0 || s >= n) ? -1 : s;
}

// Forward (BWD = false: src = x, out = y) and data gradient (BWD = true: src = gy, out = gx, xm = x or NULL).
// grid: (pixel blocks, channel-unit groups, images).
template <typename T, bool VEC, bool BWD>
__global__ __launch_bounds__(256) void dwd_conv_kernel(const T* __restrict__ src, int lds, const float* __restrict__ w,
                                                       const T* __restrict__ xm, int ldm, T* __restrict__ out, int ldo,
                                                       double* __restrict__ stats, int sld, int nrep, int SH, int SW, int OH, int OW,
                                                       int C, int S, int D, int in_relu, int imgs_per_group, int pix, DwGeom dg) {
  constexpr int N = Unit<T, VEC>::N;
  constexpr int WL = 9 * 64 * N;
  constexpr int RED = 2 * 256 * N;
  __shared__ float lds_buf[WL > RED ? WL : RED];
  const int nch = dg.tx * N;
  const int cb0 = blockIdx.y * nch;
  dw_stage_weights(w, lds_buf, cb0, nch, C, 9);
  __syncthreads();
  const int tx = threadIdx.x % dg.tx, ty = threadIdx.x / dg.tx;
  const int u = blockIdx.y * dg.tx + tx;
  const int b = blockIdx.z;
  const int c0 = u * N;
  const int nv = C - c0 < N ? C - c0 : N;
  const T* sp = src + (long)b * SH * SW * lds + c0;
  float s1[N], s2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  // `pix` pixels per thread (rows of dg.ty pixels, consecutive in the image): the weight tile is staged once for all of them
  for (int p = 0; p < pix; ++p) {
    const int q = (blockIdx.x * pix + p) * dg.ty + ty;
    if (!(ty < dg.ty && u < dg.units && q < OH * OW)) continue;
    const int orow = q / OW, ocol = q - orow * OW;
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int srow = dwd_src<BWD>(orow, kh, S, D, SH);
      if (srow < 0) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int scol = dwd_src<BWD>(ocol, kw, S, D, SW);
        if (scol < 0) continue;
        float v[N];
        dwd_load<T, VEC>(sp + ((long)srow * SW + scol) * lds, v, nv);
        const float* wt = lds_buf + (kh * 3 + kw) * nch + tx * N;
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const float a = (!BWD && in_relu) ? fmaxf(v[e], 0.f) : v[e];
          acc[e] = fmaf(a, wt[e], acc[e]);
        }
      }
    }
    if (BWD && xm) {
      float xv[N];
      dwd_load<T, VEC>(xm + ((long)b * OH * OW + q) * ldm + c0, xv, nv);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = xv[e] > 0.f ? acc[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
      acc[e] = Elem<T>::rnd(acc[e]);
      s1[e] += acc[e];
      s2[e] = fmaf(acc[e], acc[e], s2[e]);
    }
    dwd_store<T, VEC>(out + ((long)b * OH * OW + q) * ldo + c0, acc, nv);
  }
  if (BWD || !stats) return;   // uniform
  __syncthreads();             // the weight tile is dead: its LDS takes the block reduction
  float* r1 = lds_buf;
  float* r2 = lds_buf + 256 * N;
#pragma unroll
  for (int e = 0; e < N; ++e) { r1[threadIdx.x * N + e] = s1[e]; r2[threadIdx.x * N + e] = s2[e]; }
  __syncthreads();
  for (int i = threadIdx.x; i < nch; i += blockDim.x) {
    const int c = cb0 + i;
    if (c >= C) continue;
    const int txi = i / N, e = i - txi * N;
    float a = 0.f, q2 = 0.f;
    for (int y = 0; y < dg.ty; ++y) {
      a += r1[(y * dg.tx + txi) * N + e];
      q2 += r2[(y * dg.tx + txi) * N + e];
    }
    const int g = b / imgs_per_group;
    double* sp = stats + ((long)(blockIdx.x % nrep) * (gridDim.z / imgs_per_group) + g) * 2 * sld;
    atomicAdd(sp + c, (double)a);
    atomicAdd(sp + sld + c, (double)q2);
  }
}

// Weight gradient: block (pixel blocks, channel-unit groups, kernel row kh); a thread walks output pixels of the whole batch
// and accumulates the three taps of row kh for its N channels; LDS reduction over the pixel rows of the block, then
// part[blockIdx.x][kh*3 + kw][c] (every element written by exactly one block; dw_wgrad_sum_kernel folds the slots).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dwd_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ gy, int ldg,
                                                        float* __restrict__ part, int B, int H, int W, int Ho, int Wo, int C, int S,
                                                        int D, int in_relu, DwGeom dg) {
  constexpr int N = Unit<T, VEC>::N;
  __shared__ float red[256 * 3 * N];
  const int tx = threadIdx.x % dg.tx, ty = threadIdx.x / dg.tx;
  const int u = blockIdx.y * dg.tx + tx;
  const int kh = blockIdx.z;
  const int rows = (Ho * Wo + dg.ty - 1) / dg.ty;      // rows of dg.ty pixels per image
  const int c0 = u * N;
  float acc[3][N];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int e = 0; e < N; ++e) acc[kw][e] = 0.f;
  if (ty < dg.ty && u < dg.units) {
    const int nv = C - c0 < N ? C - c0 : N;
    for (int it = blockIdx.x; it < B * rows; it += gridDim.x) {
      const int b = it / rows;
      const int rem = (it - b * rows) * dg.ty + ty;
      if (rem >= Ho * Wo) continue;
      const int oh = rem / Wo, ow = rem - oh * Wo;
      const int ih = dwd_src<false>(oh, kh, S, D, H);
      if (ih < 0) continue;
      float g[N];
      dwd_load<T, VEC>(gy + ((long)b * Ho * Wo + rem) * ldg + c0, g, nv);
      const T* xr = x + ((long)b * H + ih) * W * ldx + c0;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = dwd_src<false>(ow, kw, S, D, W);
        if (iw < 0) continue;
        float v[N];
        dwd_load<T, VEC>(xr + (long)iw * ldx, v, nv);
#pragma unroll
        for (int e = 0; e < N; ++e) acc[kw][e] = fmaf(in_relu ? fmaxf(v[e], 0.f) : v[e], g[e], acc[kw][e]);
      }
    }
  }
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int e = 0; e < N; ++e) red[(kw * 256 + threadIdx.x) * N + e] = acc[kw][e];
  __syncthreads();
  const int nch = dg.tx * N;
  const int cb0 = blockIdx.y * nch;
  for (int i = threadIdx.x; i < nch * 3; i += blockDim.x) {
    const int kw = i / nch, cl = i - kw * nch;
    const int c = cb0 + cl;
    if (c >= C) continue;
    const int txi = cl / N, e = cl - txi * N;
    float a = 0.f;
    for (int y = 0; y < dg.ty; ++y) a += red[(kw * 256 + y * dg.tx + txi) * N + e];
    part[((long)blockIdx.x * 9 + kh * 3 + kw) * C + c] = a;
  }
}

// forward / data gradient of the dilated kernel.  Its 16-byte path needs aligned strides and pointers only (the channel tail
// is masked): the C handed to sdhip_vec_ok is one that always divides.
void dwd_conv(bool bwd, int dtype, const void* src, int lds, const float* w, const void* xm, int ldm, void* out, int ldo, double* stats,
              int sld, int nrep, int B, int SH, int SW, int OH, int OW, int C, int S, int D, int in_relu, int ipg, hipStream_t s) {
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(0, {lds, ldo, xm ? ldm : 0}, {src, out, xm}), [&](auto V) { sdhip_by_flag(bwd, [&](auto BWD) {
      constexpr int N = Unit<T, V()>::N;
      const DwGeom dg = dw_geom((C + N - 1) / N);
      // pixels per thread: as many as leave ~2048 workgroups (8 per CU) to the launch, at most DWD_MAX_PIX
      const long rows = sdhip_cdiv((long)OH * OW, dg.ty);
      const long others = (long)sdhip_cdiv(dg.units, dg.tx) * B;
      long pix = rows * others / 2048;
      pix = pix < 1 ? 1 : (pix > DWD_MAX_PIX ? DWD_MAX_PIX : pix);
      dim3 grid((unsigned)sdhip_cdiv(rows, pix), (unsigned)sdhip_cdiv(dg.units, dg.tx), (unsigned)B);
      hipLaunchKernelGGL((dwd_conv_kernel<T, V(), BWD()>), grid, dim3(256), 0, s, (const T*)src, lds, w, (const T*)xm, ldm, (T*)out, ldo,
                         stats, sld, nrep, SH, SW, OH, OW, C, S, D, in_relu, ipg, (int)pix, dg);
    }); });
  });
}

inline int dwd_out(int n, int stride) { return (n - 1) / stride + 1; }

// pixel blocks of the dilated weight gradient: ~64 K (pixel x channel) items each, at most 256
inline int dwd_wgrad_parts(int B, int H, int W, int C, int stride) {
  const long npix = (long)B * dwd_out(H, stride) * dwd_out(W, stride);
  long bx = (npix * C + 65535) / 65536;
  return (int)(bx < 1 ? 1 : (bx > 256 ? 256 : bx));
}

inline bool dwd_shape_ok(int B, int H, int W, int C, int stride, int dil) {
  // 32-bit pixel indices over the batch, and (dil, stride) small enough that tap offsets cannot overflow
  return B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && (long)B * H * W < (1L << 30) && (stride == 1 || stride == 2) && dil >= 1 &&
         dil <= (1 << 20);
}

}  // namespace

extern "C" int sdhip_dw_dil_wgrad_parts(int B, int H, int W, int C, int stride) {
  if (!dwd_shape_ok(B, H, W, C, stride, 1)) return SDHIP_ERR_ARG;
  return dwd_wgrad_parts(B, H, W, C, stride);
}

extern "C" int sdhip_dw_dil_conv_fwd(const void* x, int ldx, const float* w, void* y, int ldy, double* stats, int sld, int nrep,
                                     int B, int H, int W, int C, int stride, int dil, int in_relu, int groups, int dtype,
                                     void* stream) {
  SDHIP_CHECK_ARG(x && w && y, "dw_dil_conv_fwd: null pointer");
  SDHIP_CHECK_ARG(dwd_shape_ok(B, H, W, C, stride, dil) && ldx >= C && ldy >= C, "dw_dil_conv_fwd: bad shape/strides (stride %d, dil %d)",
                  stride, dil);
  SDHIP_CHECK_DTYPE("dw_dil_conv_fwd", dtype);
  SDHIP_CHECK_ARG(groups > 0 && B % groups == 0, "dw_dil_conv_fwd: groups %d does not divide B %d", groups, B);
  if (nrep < 1) nrep = 1;
  if (sld <= 0) sld = C;
  SDHIP_CHECK_ARG(!stats || sld >= C, "dw_dil_conv_fwd: statistics stride");
  const int Ho = dwd_out(H, stride), Wo = dwd_out(W, stride);
  hipStream_t s = (hipStream_t)stream;
  dwd_conv(false, dtype, x, ldx, w, nullptr, 0, y, ldy, stats, sld, nrep, B, H, W, Ho, Wo, C, stride, dil, in_relu != 0, B / groups, s);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_dw_dil_conv_dgrad(const void* gy, int ldg, const float* w, const void* x, int ldx, void* gx, int ldgx,
                                       int B, int H, int W, int C, int stride, int dil, int dtype, void* stream) {
  SDHIP_CHECK_ARG(gy && w && gx, "dw_dil_conv_dgrad: null pointer");
  SDHIP_CHECK_ARG(dwd_shape_ok(B, H, W, C, stride, dil) && ldg >= C && ldgx >= C && (!x || ldx >= C),
                  "dw_dil_conv_dgrad: bad shape/strides (stride %d, dil %d)", stride, dil);
  SDHIP_CHECK_DTYPE("dw_dil_conv_dgrad", dtype);
  const int Ho = dwd_out(H, stride), Wo = dwd_out(W, stride);
  hipStream_t s = (hipStream_t)stream;
  dwd_conv(true, dtype, gy, ldg, w, x, ldx, gx, ldgx, nullptr, 0, 1, B, Ho, Wo, H, W, C, stride, dil, 0, 1, s);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_dw_dil_conv_wgrad(const void* x, int ldx, const void* gy, int ldg, float* dw, float* part, int nparts,
                                       int B, int H, int W, int C, int stride, int dil, int in_relu, int dtype, void* stream) {
  SDHIP_CHECK_ARG(x && gy && dw && part, "dw_dil_conv_wgrad: null pointer");
  SDHIP_CHECK_ARG(dwd_shape_ok(B, H, W, C, stride, dil) && ldx >= C && ldg >= C, "dw_dil_conv_wgrad: bad shape/strides (stride %d, dil %d)",
                  stride, dil);
  SDHIP_CHECK_DTYPE("dw_dil_conv_wgrad", dtype);
  SDHIP_CHECK_ARG(nparts == dwd_wgrad_parts(B, H, W, C, stride), "dw_dil_conv_wgrad: %d partial slots, sdhip_dw_dil_wgrad_parts says %d",
                  nparts, dwd_wgrad_parts(B, H, W, C, stride));
  const int Ho = dwd_out(H, stride), Wo = dwd_out(W, stride);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(0, {ldx, ldg}, {x, gy}), [&](auto V) {   // (channel tail masked, as in dwd_conv)
      constexpr int N = Unit<T, V()>::N;
      const DwGeom dg = dw_geom((C + N - 1) / N);
      dim3 grid((unsigned)nparts, (unsigned)sdhip_cdiv(dg.units, dg.tx), 3u);
      hipLaunchKernelGGL((dwd_wgrad_kernel<T, V()>), grid, dim3(256), 0, s, (const T*)x, ldx, (const T*)gy, ldg, part, B, H, W, Ho, Wo,
                         C, stride, dil, in_relu != 0, dg);
    });
  });
  SDHIP_LAUNCH_CHECK();
  hipLaunchKernelGGL(dw_wgrad_sum_kernel, dim3((unsigned)sdhip_cdiv(9L * C, 32)), dim3(256), 0, s, part, nparts, dw, 9, C);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_dw_pool_parts(int H, int W, int C, int k, int stride, int dtype) {
  if (H <= 0 || W <= 0 || C <= 0 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return SDHIP_ERR_ARG;
  return dw_pool_parts(H, W, C, k, stride, dtype);
}

extern "C" int sdhip_dw_wgrad_parts(int B, int H, int W, int C, int k, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return SDHIP_ERR_ARG;
  return dw_wgrad_parts(B, H, W, C, k, stride);
}

extern "C" int sdhip_dw_conv_fwd(const void* x, int ldx, const float* w, void* y, int ldy, double* stats, int sld, int nrep, float* pool,
                                 int pool_parts, int B, int H, int W, int C, int k, int stride, int groups, int dtype, void* stream) {
  SDHIP_CHECK_ARG(x && w && y, "dw_conv_fwd: null pointer");
  SDHIP_CHECK_ARG((k == 3 || k == 5) && (stride == 1 || stride == 2), "dw_conv_fwd: k=%d stride=%d (3/5, 1/2 only)", k, stride);
  SDHIP_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && ldy >= C, "dw_conv_fwd: bad shape/strides");
  SDHIP_CHECK_DTYPE("dw_conv_fwd", dtype);
  SDHIP_CHECK_ARG(groups > 0 && B % groups == 0, "dw_conv_fwd: groups %d does not divide B %d", groups, B);
  if (nrep < 1) nrep = 1;
  if (sld <= 0) sld = C;
  SDHIP_CHECK_ARG(!stats || sld >= C, "dw_conv_fwd: statistics stride");
  SDHIP_CHECK_ARG(!pool || pool_parts >= dw_pool_parts(H, W, C, k, stride, dtype), "dw_conv_fwd: %d pool slots, %d needed", pool_parts,
                  dw_pool_parts(H, W, C, k, stride, dtype));
  const int Ho = dw_out(H, k, stride), Wo = dw_out(W, k, stride);
  hipStream_t s = (hipStream_t)stream;
  dw_conv(false, dtype, k, stride, x, ldx, w, y, ldy, stats, sld, nrep, pool, pool_parts, B, H, W, Ho, Wo, C, B / groups, s);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_dw_conv_dgrad(const void* gy, int ldg, const float* w, void* gx, int ldgx,
                                   int B, int H, int W, int C, int k, int stride, int dtype, void* stream) {
  SDHIP_CHECK_ARG(gy && w && gx, "dw_conv_dgrad: null pointer");
  SDHIP_CHECK_ARG((k == 3 || k == 5) && (stride == 1 || stride == 2), "dw_conv_dgrad: k=%d stride=%d (3/5, 1/2 only)", k, stride);
  SDHIP_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && ldg >= C && ldgx >= C, "dw_conv_dgrad: bad shape/strides");
  SDHIP_CHECK_DTYPE("dw_conv_dgrad", dtype);
  const int Ho = dw_out(H, k, stride), Wo = dw_out(W, k, stride);
  hipStream_t s = (hipStream_t)stream;
  dw_conv(true, dtype, k, stride, gy, ldg, w, gx, ldgx, nullptr, 0, 1, nullptr, 0, B, Ho, Wo, H, W, C, 1, s);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_dw_conv_wgrad(const void* x, int ldx, const void* gy, int ldg, float* dw, float* part, int nparts,
                                   int B, int H, int W, int C, int k, int stride, int dtype, void* stream) {
  SDHIP_CHECK_ARG(x && gy && dw && part, "dw_conv_wgrad: null pointer");
  SDHIP_CHECK_ARG((k == 3 || k == 5) && (stride == 1 || stride == 2), "dw_conv_wgrad: k=%d stride=%d (3/5, 1/2 only)", k, stride);
  SDHIP_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && ldg >= C, "dw_conv_wgrad: bad shape/strides");
  SDHIP_CHECK_DTYPE("dw_conv_wgrad", dtype);
  SDHIP_CHECK_ARG(nparts == dw_wgrad_parts(B, H, W, C, k, stride), "dw_conv_wgrad: %d partial slots, sdhip_dw_wgrad_parts says %d",
                  nparts, dw_wgrad_parts(B, H, W, C, k, stride));
  const int Ho = dw_out(H, k, stride), Wo = dw_out(W, k, stride);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {ldx, ldg}, {x, gy}), [&](auto V) { dw_by_ks(k, stride, [&](auto K, auto S) {
      const DwGeom dg = dw_geom(C / Unit<T, V()>::N);
      dim3 grid((unsigned)nparts, (unsigned)sdhip_cdiv(dg.units, dg.tx), (unsigned)K());
      hipLaunchKernelGGL((dw_wgrad_kernel<T, V(), K(), S()>), grid, dim3(256), 0, s, (const T*)x, ldx, (const T*)gy, ldg, part, B, H, W, Ho,
                         Wo, C, dg);
    }); });
  });
  SDHIP_LAUNCH_CHECK();
  hipLaunchKernelGGL(dw_wgrad_sum_kernel, dim3((unsigned)sdhip_cdiv((long)k * k * C, 32)), dim3(256), 0, s, part, nparts, dw, k * k, C);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_se_fwd(const float* pool, int pool_parts, float inv_hw, const float* scale, const float* shift, int groups,
                            const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* ws,
                            int B, int C, int r, void* stream) {
  SDHIP_CHECK_ARG(pool && w1 && b1 && w2 && b2 && s && ws, "se_fwd: null pointer");
  SDHIP_CHECK_ARG((scale == nullptr) == (shift == nullptr), "se_fwd: scale/shift must come together");
  SDHIP_CHECK_ARG(B > 0 && C > 0 && C <= SE_MAXC && r > 0 && r <= SE_MAXC / 4, "se_fwd: C=%d r=%d (C <= %d, r <= %d)", C, r, SE_MAXC,
                  SE_MAXC / 4);
  SDHIP_CHECK_ARG(groups > 0 && B % groups == 0 && pool_parts > 0, "se_fwd: groups %d, B %d, pool slots %d", groups, B, pool_parts);
  hipLaunchKernelGGL(se_fwd_kernel, dim3((unsigned)sdhip_cdiv(B, SE_IMGS)), dim3(SE_THREADS), 0, (hipStream_t)stream, pool, pool_parts,
                     inv_hw, scale, shift,
                     B / groups, w1, b1, w2, b2, s, ws, B, C, r);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_se_bwd(const float* ds, int nrep, const float* ws, const float* w1, const float* w2,
                            float* gw1, float* gb1, float* gw2, float* gb2, float* gpool, float inv_hw, int B, int C, int r, void* stream) {
  SDHIP_CHECK_ARG(ds && ws && w1 && w2 && gw1 && gb1 && gw2 && gb2 && gpool, "se_bwd: null pointer");
  SDHIP_CHECK_ARG(B > 0 && C > 0 && C <= SE_MAXC && r > 0 && r <= SE_MAXC / 4 && nrep > 0, "se_bwd: C=%d r=%d nrep=%d", C, r, nrep);
  hipLaunchKernelGGL(se_bwd_kernel, dim3((unsigned)sdhip_cdiv(B, SE_IMGS)), dim3(SE_THREADS), 0, (hipStream_t)stream, ds, nrep, ws, w1, w2,
                     gw1, gb1, gw2, gb2, gpool, inv_hw, B, C, r);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_se_scale_bwd(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx, const float* s, const float* gadd,
                                  long npix_img, int B, int C, int act, int dtype, void* stream) {
  SDHIP_CHECK_ARG(gy && x && gx && s, "se_scale_bwd: null pointer");
  SDHIP_CHECK_ARG(B > 0 && C > 0 && npix_img > 0 && ldg >= C && ldx >= C && ldgx >= C, "se_scale_bwd: bad shape/strides");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID, "se_scale_bwd: activation %d", act);
  SDHIP_CHECK_DTYPE("se_scale_bwd", dtype);
  hipStream_t st = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    sdhip_by_flag(sdhip_vec_ok<T>(C, {ldg, ldx, ldgx}, {gy, x, gx}), [&](auto V) {
      const DwGeom dg = dw_geom(C / Unit<T, V()>::N);
      long bx = sdhip_cdiv(npix_img, (long)dg.ty * 4); if (bx > 256) bx = 256;
      dim3 grid((unsigned)bx, (unsigned)sdhip_cdiv(dg.units, dg.tx), (unsigned)B);
      hipLaunchKernelGGL((se_scale_bwd_kernel<T, V()>), grid, dim3(256), 0, st, (const T*)gy, ldg, (const T*)x, ldx, (T*)gx, ldgx, s, gadd,
                         npix_img, C, act, dg);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
