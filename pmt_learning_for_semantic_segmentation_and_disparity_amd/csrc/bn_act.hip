// BatchNorm (train-mode batch statistics) + activation, decomposed for fusion, for gfx950.
//
// Replaces nn.BatchNorm2d (+ nn.ReLU / skip add) as used by convbn / deconvbn /
// Conv2DownUp (models/dsnet_t2.py:16-117), the DenseNet layers
// (models/densenet.py:25-93,119-128) and ASPP (models/aspp.py:7-32); semantics of
// the statistics as restated in sync_batchnorm/batchnorm.py:114-126 (sum, sum of
// squares, count -> mean, biased variance for normalisation, unbiased for
// running_var, momentum 0.1).
//
//   statistics  S[g] = (sum x, sum x^2) per channel and statistics group g (f64; produced by the
//               conv epilogue or by sdhip_channel_stats; a "group" is a sub-batch that the
//               reference normalises separately, e.g. the left and the right tower pass)
//   finalize    scale = gamma * invstd, shift = beta - mean * scale           (tiny, per channel)
//   apply       y = act(x * scale + shift) (+ residual)                        (HBM bound, 16 B/lane)
//   backward    gx = gy * act' * scale,  dscale = sum gy*act'*x,  dshift = sum gy*act'   (one pass)
//               finalize_bwd: (dscale, dshift) -> dgamma, dbeta, dS
//               stats_fix   : g += dS1 + 2 * x * dS2      (gradient through the statistics)
//
// All elementwise kernels view a tensor as [pixels][C] rows with pixel stride ld.
#include "sdhip_common.h"

namespace {

// h-swish / h-sigmoid run in their own instantiations (template flag HS): the kernels every other layer uses keep the
// code, registers and schedule they had before these codes existed
inline bool hard_act(int act) { return act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID; }

struct RowGeom {  // how a 256-thread block walks a [npix][C] matrix
  int tx, ty;     // threads across channel units / across pixels
  int units;      // channel units per row (16-byte chunks, or single elements in scalar mode)
  unsigned magic; // div_magic(tx): thread -> (tx, ty) without an integer division per lane (these kernels are often ~5 us)
};

inline RowGeom row_geom(int units) {
  RowGeom r;
  r.units = units;
  r.tx = units < 64 ? units : 64;
  r.ty = 256 / r.tx;
  r.magic = r.tx > 1 ? (unsigned)(0x100000000ULL / (unsigned)r.tx) + 1u : 0u;
  return r;
}

// threadIdx.x -> ty = tid / tx (tid < 256: exact with the 2^32/tx + 1 magic), tx = tid - ty * tx
#define ROW_TXTY(rg, tx, ty) const int ty = (rg).tx > 1 ? (int)__umulhi((unsigned)threadIdx.x, (rg).magic) : (int)threadIdx.x; \
                             const int tx = (int)threadIdx.x - ty * (rg).tx

// ---- streaming bodies ----------------------------------------------------------------------------------------------
// A thread owns the pixels first, first + stride, ... of its channel unit and visits them in ascending order, K per trip.
// A trip ISSUES every load it needs (K pixels x every input tensor) into raw registers, and only then unpacks, computes
// and stores: one HBM round trip per trip.  (Unit::load converts where it loads; inside `if (pix < npix_g)` each guarded
// load then waits for its own data, and the compiler does not hoist loads over divergent branches: the 4-pixel trips
// made seven dependent round trips.)  Full trips run in a loop without any guard; one last, ragged trip (FULL = false)
// follows.  No branch surrounds a load there either: a pixel past the end is loaded from the trip's own first row instead
// - inside the tensor - and its result dropped: the store is predicated, a sum keeps its old value by a select (not a
// multiply by zero: the row that stands in may hold anything).  Rows are reached by pointer steps (the
// uniform stride * ld), not by a 64-bit product per load: address arithmetic between the loads invites the scheduler to
// start on the first pixel while the last loads are not yet out; issued() forbids it that outright.  The tensor pointers of
// these kernels are not __restrict__: a load known not to alias the stores is sunk into the predicated block of its pixel,
// behind the stores of the pixels before it - and waits there.
template <int K, bool FULL> struct Trip {
  bool ok[K];
  __device__ __forceinline__ Trip(long pix0, long stride, long npix_g) {
#pragma unroll
    for (int k = 0; k < K; ++k) ok[k] = FULL || pix0 + k * stride < npix_g;
  }
  // row k of the trip whose first row p points at; step = stride * ld elements
  template <typename P> __device__ __forceinline__ P at(P p, int k, long step) const { return p + (ok[k] ? k * step : 0L); }
};

// every load above is issued before anything below is scheduled
__device__ __forceinline__ void issued() { __builtin_amdgcn_sched_barrier(0); }

// Pixels per trip.  The kernels that had 4 keep 4.  The others (affine_act, affine_act_bn, stats_fix, stats_fix_fin) were
// measured with 4 on top of the issue-then-use trips and lost 2 - 12 % at every shape of the step (their grids are not
// capped below the machine, so the workgroups already keep the memory system busy): they stay at 1, act_out_bwd at its 2.
// A map so small that no thread has a second pixel takes the one-pixel trip in the 4-pixel kernels as well: nothing to
// overlap, and the short body starts sooner.
constexpr int kPixTrip = 1;

// y = act(x*scale + shift) (+ res) over the thread's pixels
template <typename T, bool VEC, bool HS, bool RES, int K = kPixTrip>
__device__ __forceinline__ void affine_act_rows(const T* x, int ldx, T* y, int ldy,
                                                const T* res, int ldr, const float* sc, const float* sf,
                                                int c0, long base, long npix_g, long first, long stride, int act) {
  using U = Unit<T, VEC>;
  constexpr int N = U::N;
  const long sx = stride * ldx, sy = stride * ldy, sr = stride * ldr;
  const T* xp = x + (base + first) * ldx + c0;
  const T* rp = RES ? res + (base + first) * ldr + c0 : nullptr;
  T* yp = y + (base + first) * ldy + c0;
  long pix0 = first;
  auto trip = [&](auto full) {
    const Trip<K, decltype(full)::value> t(pix0, stride, npix_g);
    typename U::Raw xr[K], rr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) xr[k] = U::raw(t.at(xp, k, sx));
    if constexpr (RES) {
#pragma unroll
      for (int k = 0; k < K; ++k) rr[k] = U::raw(t.at(rp, k, sr));
    }
    issued();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float f[N], r[N];
      U::unpack(xr[k], f);
      if constexpr (RES) U::unpack(rr[k], r);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        float v = fmaf(f[e], sc[e], sf[e]);
        if (act == 1) v = fmaxf(v, 0.f);
        else if (act == 2) v = 1.f / (1.f + __expf(-v));
        else if (HS && (act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID)) v = act_hs(v, act);
        if constexpr (RES) v += r[e];
        f[e] = v;
      }
      if (t.ok[k]) U::store(yp + k * sy, f);
    }
  };
  for (; pix0 + (K - 1) * stride < npix_g; pix0 += K * stride, xp += K * sx, rp += RES ? K * sr : 0, yp += K * sy) trip(std::true_type{});
  if (pix0 < npix_g) trip(std::false_type{});
}

// y = act(x*scale + shift) (+ res);  grid: (pixel slabs, unit groups, stat groups)
template <typename T, bool VEC, bool HS = false>
__global__ __launch_bounds__(256) void affine_act_kernel(const T* x, int ldx, T* y, int ldy,
                                                         const T* res, int ldr,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         int C, long npix_g, int act, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int g = blockIdx.z, c0 = u * N;
  float sc[N], sf[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { sc[e] = scale ? scale[g * C + c0 + e] : 1.f; sf[e] = shift ? shift[g * C + c0 + e] : 0.f; }
  const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty, stride = (long)gridDim.x * rg.ty;
  if (res) affine_act_rows<T, VEC, HS, true>(x, ldx, y, ldy, res, ldr, sc, sf, c0, base, npix_g, first, stride, act);
  else affine_act_rows<T, VEC, HS, false>(x, ldx, y, ldy, res, ldr, sc, sf, c0, base, npix_g, first, stride, act);
}

// the thread's pixels of affine_act_bwd.  GX 0: reductions only; 1: gx written; 2: gx += (its old value is one more input)
template <typename T, bool VEC, bool HS, int GX>
__device__ __forceinline__ void affine_act_bwd_rows(const T* gy, int ldg, const T* x, int ldx, T* gx, int ldgx,
                                                    const float* sc, const float* sf, float* a1, float* a2,
                                                    int c0, long base, long npix_g, long first, long stride, int act) {
  using U = Unit<T, VEC>;
  constexpr int N = U::N, K = 4;
  const long sg = stride * ldg, sx = stride * ldx, so = stride * ldgx;
  const T* gp = gy + (base + first) * ldg + c0;
  const T* xp = x + (base + first) * ldx + c0;
  T* op = GX ? gx + (base + first) * ldgx + c0 : nullptr;
  long pix0 = first;
  auto trip = [&](auto full) {
    const Trip<K, decltype(full)::value> t(pix0, stride, npix_g);
    typename U::Raw gr[K], xr[K], orw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { gr[k] = U::raw(t.at(gp, k, sg)); xr[k] = U::raw(t.at(xp, k, sx)); }
    if constexpr (GX == 2) {
#pragma unroll
      for (int k = 0; k < K; ++k) orw[k] = U::raw(t.at((const T*)op, k, so));
    }
    issued();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float gv[N], xv[N], old[N];
      U::unpack(gr[k], gv);
      U::unpack(xr[k], xv);
      if constexpr (GX == 2) U::unpack(orw[k], old);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float z = fmaf(xv[e], sc[e], sf[e]);
        float gm = gv[e];
        if (act == 1) gm = z > 0.f ? gm : 0.f;
        else if (act == 2) { const float sg = 1.f / (1.f + __expf(-z)); gm *= sg * (1.f - sg); }
        else if (HS && (act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID)) gm *= act_hs_d(z, act);
        else if (act == 4) gm *= z * (1.f - z);  // x holds the sigmoid OUTPUT
        const float n1 = fmaf(gm, xv[e], a1[e]), n2 = a2[e] + gm;
        a1[e] = t.ok[k] ? n1 : a1[e];
        a2[e] = t.ok[k] ? n2 : a2[e];
        {   // rounded on its own: gx += adds the old value to the PRODUCT, as it always did (no fused multiply-add)
#pragma clang fp contract(off)
          gv[e] = gm * sc[e];
        }
        if constexpr (GX == 2) gv[e] += old[e];
      }
      if constexpr (GX != 0) { if (t.ok[k]) U::store(op + k * so, gv); }
    }
  };
  for (; pix0 + (K - 1) * stride < npix_g; pix0 += K * stride, gp += K * sg, xp += K * sx, op += GX ? K * so : 0) trip(std::true_type{});
  if (pix0 < npix_g) trip(std::false_type{});
}

// gx = gy * act'(x*scale+shift) * scale;  dscale += sum gy*act'*x;  dshift += sum gy*act'
// mode 0: both; mode 1: only the reductions (gx not written)
template <typename T, bool VEC, bool HS = false>
__global__ __launch_bounds__(256) void affine_act_bwd_kernel(const T* gy, int ldg, const T* x, int ldx,
                                                             T* gx, int ldgx,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ dscale, float* __restrict__ dshift, int nrep,
                                                             int C, long npix_g, int act, int accumulate, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  __shared__ float red[2][256 * (VEC ? Chunk<T>::N : 1)];
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  const bool live = ty < rg.ty && u < rg.units;
  const int g = blockIdx.z, c0 = u * N;
  float sc[N], sf[N], a1[N], a2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { sc[e] = 1.f; sf[e] = 0.f; a1[e] = 0.f; a2[e] = 0.f; }
  if (live) {
    if (scale) {
#pragma unroll
      for (int e = 0; e < N; ++e) sc[e] = scale[g * C + c0 + e];
    }
    if (shift) {
#pragma unroll
      for (int e = 0; e < N; ++e) sf[e] = shift[g * C + c0 + e];
    }
    // 4 pixels per trip, all 8 (12 when accumulating) loads issued before the first use: with the grid kept small for the
    // sake of the atomics below (see there) each thread has to keep more bytes in flight itself
    const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty, stride = (long)gridDim.x * rg.ty;
    if (!gx) affine_act_bwd_rows<T, VEC, HS, 0>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a1, a2, c0, base, npix_g, first, stride, act);
    else if (!accumulate) affine_act_bwd_rows<T, VEC, HS, 1>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a1, a2, c0, base, npix_g, first, stride, act);
    else affine_act_bwd_rows<T, VEC, HS, 2>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a1, a2, c0, base, npix_g, first, stride, act);
  }
  if (!dscale) return;  // uniform
  // Reduce over the ty rows of the block in LDS, then ONE atomic wave-instruction per sum with consecutive lanes on
  // consecutive channels.  Float atomics execute at the memory side, one 256-byte request at a time per line: thousands
  // of workgroups x 16 scattered 8-lane instructions into the same replica line serialised into most of this kernel's
  // run time (69 us on a 400 MB pass that streams in 25).
#pragma unroll
  for (int e = 0; e < N; ++e) { red[0][threadIdx.x * N + e] = a1[e]; red[1][threadIdx.x * N + e] = a2[e]; }
  __syncthreads();
  const int nch = min(rg.tx, rg.units - blockIdx.y * rg.tx) * N;   // channels of this block's unit group
  for (int cc = threadIdx.x; cc < 2 * nch; cc += 256) {
    const int which = cc >= nch, ch = cc - which * nch;
    const int txx = ch / N, e = ch - txx * N;
    float sum = 0.f;
    for (int r = 0; r < rg.ty; ++r) sum += red[which][(r * rg.tx + txx) * N + e];
    const long rep = (long)(blockIdx.x % nrep) * gridDim.z * C;   // replica r of [nrep][G][C]
    atomicAdd((which ? dshift : dscale) + rep + g * C + blockIdx.y * rg.tx * N + ch, sum);
  }
}

// graw = gy * act'(y) * scale with the derivative taken from the activation's OUTPUT y (frozen BatchNorm folded into the
// weight pack: the raw convolution output is never stored).  A pure stream of 2 reads and 1 write per element: 16 bytes per
// lane in the vector form, all loads of a trip issued before the first use - the block count, not the registers, bounds the
// bytes in flight.  grid: (pixel slabs, unit groups, scale groups)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void act_out_bwd_kernel(const T* gy, int ldg, const T* y, int ldy,
                                                          T* graw, int ldgr, const float* __restrict__ scale,
                                                          int C, long npix_g, int act, RowGeom rg) {
  using U = Unit<T, VEC>;
  constexpr int N = U::N, K = 2;
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int g = blockIdx.z, c0 = u * N;
  float sc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) sc[e] = scale[g * C + c0 + e];
  const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty;
  const long stride = (long)gridDim.x * rg.ty;
  const long sg = stride * ldg, sy = stride * ldy, so = stride * ldgr;
  const T* gp = gy + (base + first) * ldg + c0;
  const T* yp = y + (base + first) * ldy + c0;
  T* op = graw + (base + first) * ldgr + c0;
  long pix0 = first;
  auto trip = [&](auto full) {
    const Trip<K, decltype(full)::value> t(pix0, stride, npix_g);
    typename U::Raw gr[K], yr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { gr[k] = U::raw(t.at(gp, k, sg)); yr[k] = U::raw(t.at(yp, k, sy)); }
    issued();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float gv[N], yv[N];
      U::unpack(gr[k], gv);
      U::unpack(yr[k], yv);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        float gm = gv[e];
        if (act == 1) gm = yv[e] > 0.f ? gm : 0.f;          // -0.0 > 0 is false: an exact +0
        else if (act == 2) gm *= fmaf(-yv[e], yv[e], yv[e]);   // y (1 - y), rounded once
        gv[e] = gm * sc[e];
      }
      if (t.ok[k]) U::store(op + k * so, gv);
    }
  };
  for (; pix0 + (K - 1) * stride < npix_g; pix0 += K * stride, gp += K * sg, yp += K * sy, op += K * so) trip(std::true_type{});
  if (pix0 < npix_g) trip(std::false_type{});
}

// g_out = g_in + a + x * b2 over the thread's pixels (g_out may be g_in)
template <typename T, bool VEC, int K = kPixTrip>
__device__ __forceinline__ void stats_fix_rows(const T* gin, int ldgi, const T* x, int ldx, T* gout, int ldgo,
                                               const float* a, const float* b2, int c0, long base, long npix_g, long first,
                                               long stride) {
  using U = Unit<T, VEC>;
  constexpr int N = U::N;
  const long sg = stride * ldgi, sx = stride * ldx, so = stride * ldgo;
  const T* gp = gin + (base + first) * ldgi + c0;
  const T* xp = x + (base + first) * ldx + c0;
  T* op = gout + (base + first) * ldgo + c0;
  long pix0 = first;
  auto trip = [&](auto full) {
    const Trip<K, decltype(full)::value> t(pix0, stride, npix_g);
    typename U::Raw gr[K], xr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { gr[k] = U::raw(t.at(gp, k, sg)); xr[k] = U::raw(t.at(xp, k, sx)); }
    issued();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float gv[N], xv[N];
      U::unpack(gr[k], gv);
      U::unpack(xr[k], xv);
#pragma unroll
      for (int e = 0; e < N; ++e) gv[e] = gv[e] + fmaf(xv[e], b2[e], a[e]);
      if (t.ok[k]) U::store(op + k * so, gv);
    }
  };
  for (; pix0 + (K - 1) * stride < npix_g; pix0 += K * stride, gp += K * sg, xp += K * sx, op += K * so) trip(std::true_type{});
  if (pix0 < npix_g) trip(std::false_type{});
}

// g_out = g_in + dS1 + 2 * x * dS2   (dS is [G][2][C], f64 like the statistics it is the gradient of)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void stats_fix_kernel(const T* gin, int ldgi, const T* x, int ldx,
                                                        T* gout, int ldgo, const double* __restrict__ dS, int ldc,
                                                        int C, long npix_g, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int g = blockIdx.z, c0 = u * N;
  float a[N], b2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { a[e] = (float)dS[((long)g * 2 + 0) * ldc + c0 + e]; b2[e] = (float)(2.0 * dS[((long)g * 2 + 1) * ldc + c0 + e]); }
  stats_fix_rows<T, VEC>(gin, ldgi, x, ldx, gout, ldgo, a, b2, c0, (long)g * npix_g, npix_g, (long)blockIdx.x * rg.ty + ty,
                         (long)gridDim.x * rg.ty);
}

// gx = rnd(gy * act'(x*scale+shift) * scale) + a + x * b2 over the thread's pixels, 4 per trip (gx may be gy)
template <typename T, bool VEC, bool HS, int K>
__device__ __forceinline__ void bn_bwd_rows(const T* gy, int ldg, const T* x, int ldx, T* gx, int ldgx,
                                            const float* sc, const float* sf, const float* a, const float* b2,
                                            int c0, long base, long npix_g, long first, long stride, int act) {
  using U = Unit<T, VEC>;
  constexpr int N = U::N;
  const long sg = stride * ldg, sx = stride * ldx, so = stride * ldgx;
  const T* gp = gy + (base + first) * ldg + c0;
  const T* xp = x + (base + first) * ldx + c0;
  T* op = gx + (base + first) * ldgx + c0;
  long pix0 = first;
  auto trip = [&](auto full) {
    const Trip<K, decltype(full)::value> t(pix0, stride, npix_g);
    typename U::Raw gr[K], xr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { gr[k] = U::raw(t.at(gp, k, sg)); xr[k] = U::raw(t.at(xp, k, sx)); }
    issued();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float gv[N], xv[N];
      U::unpack(gr[k], gv);
      U::unpack(xr[k], xv);
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float z = fmaf(xv[e], sc[e], sf[e]);
        float gm = gv[e];
        if (act == 1) gm = z > 0.f ? gm : 0.f;
        else if (act == 2) { const float sg = 1.f / (1.f + __expf(-z)); gm *= sg * (1.f - sg); }
        else if (HS && (act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID)) gm *= act_hs_d(z, act);
        // the first-phase result the one-pass form would have stored is rounded to T before the statistics path is added
        gv[e] = Elem<T>::rnd(gm * sc[e]) + fmaf(xv[e], b2[e], a[e]);
      }
      if (t.ok[k]) U::store(op + k * so, gv);
    }
  };
  for (; pix0 + (K - 1) * stride < npix_g; pix0 += K * stride, gp += K * sg, xp += K * sx, op += K * so) trip(std::true_type{});
  if (pix0 < npix_g) trip(std::false_type{});
}

// Second phase of the two-phase BatchNorm backward: gx = gy * act'(x*scale+shift) * scale + dS1 + 2 * x * dS2 in ONE pass
// (the first phase is affine_act_bwd with gx == NULL: reductions only).  10 bytes per element instead of the 12 of
// "write gx, then read it back for the statistics path".
template <typename T, bool VEC, bool HS = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* gy, int ldg, const T* x, int ldx,
                                                           T* gx, int ldgx, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const double* __restrict__ dS, int ldc,
                                                           int C, long npix_g, int act, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int g = blockIdx.z, c0 = u * N;
  float sc[N], sf[N], a[N], b2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    sc[e] = scale[g * C + c0 + e]; sf[e] = shift[g * C + c0 + e];
    a[e] = (float)dS[((long)g * 2 + 0) * ldc + c0 + e]; b2[e] = (float)(2.0 * dS[((long)g * 2 + 1) * ldc + c0 + e]);
  }
  const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty, stride = (long)gridDim.x * rg.ty;
  if (npix_g <= stride) bn_bwd_rows<T, VEC, HS, 1>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a, b2, c0, base, npix_g, first, stride, act);
  else bn_bwd_rows<T, VEC, HS, 4>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a, b2, c0, base, npix_g, first, stride, act);
}

// ---- consumer-side finalize: the per-channel kernels between a reduction and the pass that uses its result are pure
// launch latency (~5 us + a graph node each, ~400 per training step).  These variants let every workgroup of the
// elementwise pass derive the coefficients of ITS channel slice from the replica sums (a few KB from L2), and let the
// first workgroup of each slice publish them / update the parameters' side outputs.

// Replica fold of one channel, the thread's share r = rl, rl + P, ... < nrep of the values p[r * rs], added in ascending r.
// fold_issue only loads: the first kFoldWin of the share, unrolled (a uniform test ends the window, the lane's own r is
// predicated), so that a workgroup has every replica load and every per-channel parameter load of its prologue in flight
// before it waits once.  fold_sum adds them and walks what lies beyond the window (nrep > 16 P) the plain way.  (The loop
// `for (r = rl; r < nrep; r += P) a += p[..]` compiled to one load + wait per iteration: 8 serial L2 round trips at
// C = 64, 16 at C = 128 with 32 replicas.)
constexpr int kFoldWin = 16;   // covers 32 replicas at C = 128 (2 replica lanes)
constexpr int kSffWin = 4;     // stats_fix_fin always has 8 replica lanes: 32 replicas

// `base` is the workgroup's (uniform) pointer to replica 0, `lane` the thread's own element offset c + rl * rs: the loads
// then share one 32-bit offset register over a scalar base instead of a 64-bit address pair each.  The offset is formed
// in 32 bits: (c + rl * rs) * sizeof(V) must stay below 4 GiB, which fold_span_ok() checks on the host before a launch.
template <typename V>
__device__ __forceinline__ V fold_at(const V* base, long j_rs, unsigned lane) {
  return *reinterpret_cast<const V*>(reinterpret_cast<const char*>(base + j_rs) + lane * (unsigned)sizeof(V));
}

template <typename V, int W>
__device__ __forceinline__ void fold_issue(const V* base, unsigned lane, long rs, int rl, int P, int nrep, V (&v)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    v[j] = 0;
    if (j * P < nrep) {           // uniform
      if (rl + j * P < nrep) v[j] = fold_at(base, (long)j * P * rs, lane);
    }
  }
}

template <typename V, int W>
__device__ __forceinline__ V fold_sum(const V* base, unsigned lane, long rs, int rl, int P, int nrep, const V (&v)[W]) {
  V a = 0;
#pragma unroll
  for (int j = 0; j < W; ++j)
    if (rl + j * P < nrep) a += v[j];
  for (int j = W; rl + j * P < nrep; ++j) a += fold_at(base, (long)j * P * rs, lane);
  return a;
}

// the plain loop over the whole share (kernels instantiated without the window, see WIN below)
// (both sums in ONE loop: a round trip per replica, not two)
template <typename V, typename A>
__device__ __forceinline__ void fold_plain(const V* base0, const V* base1, unsigned lane, long rs, int rl, int P, int nrep, A& a0, A& a1) {
  V s0 = 0, s1 = 0;
  for (int j = 0; rl + j * P < nrep; ++j) { s0 += fold_at(base0, (long)j * P * rs, lane); s1 += fold_at(base1, (long)j * P * rs, lane); }
  a0 = (A)s0; a1 = (A)s1;
}

// The writer workgroup of a channel slice (blockIdx.x == 0, group 0) needs the sums of ALL groups, in order.  With up to
// kFoldSlots groups it folds them into the one barrier pair every workgroup has (one window after the other: two f64
// windows side by side are 128 VGPRs, which would cost the streaming body below a wave per SIMD); with more it walks them
// one barrier pair each (`round`s).  The launch lasts as long as its slowest workgroup: with the two tower groups the
// serial walk made the writer's chain twice everybody else's.
// WIN: the window and the shared barrier pair.  Launches with two or more statistics groups (the DenseNet towers, where the
// writer's chain is what the launch waits for) take it; with ONE group it measured slower at every shape of the step whose
// grid is at the workgroup cap (+1.4 us on 7.4 for affine_act_bn, +2.5 on 7.6 for bn_bwd_apply_fin at 65536 x 64), so those
// launches keep the plain loop and the walk.
constexpr int kFoldSlots = 2;

// y = act(BatchNorm_train(x)) (+ res) straight from the statistics S (f64 [nrep][G][2][ldc]) of x.
// Also writes scale/shift/mean/invstd ([G][C], for the backward pass) and updates the running statistics (groups in order).
template <typename T, bool VEC, bool HS = false, bool WIN = true>
__global__ __launch_bounds__(256) void affine_act_bn_kernel(const T* x, int ldx, T* y, int ldy,
                                                            const T* res, int ldr,
                                                            const double* __restrict__ S, int ldc, int nrep,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ rmean, float* __restrict__ rvar,
                                                            float* __restrict__ scale_out, float* __restrict__ shift_out,
                                                            float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                                            int C, long npix_g, double count, float eps, float momentum, int act, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  __shared__ float s_sc[64 * 8], s_sf[64 * 8];
  __shared__ double s_red[kFoldSlots][2][256];
  const int G = gridDim.z, g = blockIdx.z;
  const int ch0 = blockIdx.y * rg.tx * N;
  const int nch = min(rg.tx, rg.units - (int)blockIdx.y * rg.tx) * N;
  // Replica fold of the workgroup's channels in ONE round trip: the 256 threads are (channel slot cl, replica lane rl) with as
  // many replica lanes as fit (64 channels: 4 lanes of 8 replicas each), one barrier pair per workgroup.  (The first
  // form walked the channels 32 at a time — four dependent load / barrier rounds for the 128-channel DenseNet bottlenecks,
  // most of this kernel's time on the small maps.)
  const int ncp = nch <= 32 ? 32 : nch <= 64 ? 64 : nch <= 128 ? 128 : 256;
  const int P = 256 / ncp;
  const int cl = threadIdx.x & (ncp - 1), rl = threadIdx.x / ncp;
  const bool writer = blockIdx.x == 0 && g == 0 && rmean;   // wave-uniform per workgroup: running statistics of the slice
  const int per = WIN && writer && G <= kFoldSlots ? G : 1;  // groups per round
  const int nround = writer && per == 1 ? G : 1;
  const long rs = (long)G * 2 * ldc;
  for (int cb = 0; cb < nch; cb += ncp) {
    const int c = ch0 + cb + cl;
    const bool okc = cb + cl < nch && c < C;
    const bool lead = rl == 0 && okc;
    const unsigned lane = (unsigned)(c + rl * rs);
    float rm = 0.f, rv = 0.f, gm = 1.f, bt = 0.f;
    for (int rd = 0; rd < nround; ++rd) {
      const int g0 = writer ? rd : g;                        // the writer sits in group 0: everybody's own group comes first
      double a1[kFoldSlots], a2[kFoldSlots];
#pragma unroll
      for (int s = 0; s < kFoldSlots; ++s) { a1[s] = 0.; a2[s] = 0.; }
      if (okc) {
#pragma unroll
        for (int s = 0; s < kFoldSlots; ++s) {
          if (s < per) {
            const double* S1 = S + ((long)(g0 + s) * 2 + 0) * ldc;
            const double* S2 = S + ((long)(g0 + s) * 2 + 1) * ldc;
            double v1[kFoldWin], v2[kFoldWin];
            if constexpr (WIN) {
              fold_issue(S1, lane, rs, rl, P, nrep, v1);
              fold_issue(S2, lane, rs, rl, P, nrep, v2);
            }
            if (s == 0 && rd == 0 && rl == 0) {              // the per-channel parameters travel with the replicas
              if (gamma) gm = gamma[c];
              if (beta) bt = beta[c];
              if (writer) { rm = rmean[c]; rv = rvar[c]; }
            }
            if constexpr (WIN) {
              issued();
              a1[s] = fold_sum(S1, lane, rs, rl, P, nrep, v1);
              a2[s] = fold_sum(S2, lane, rs, rl, P, nrep, v2);
            } else {
              fold_plain(S1, S2, lane, rs, rl, P, nrep, a1[s], a2[s]);
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kFoldSlots; ++s)
        if (s < per) { s_red[s][0][threadIdx.x] = a1[s]; s_red[s][1][threadIdx.x] = a2[s]; }
      __syncthreads();
      if (lead) {
#pragma unroll
        for (int s = 0; s < kFoldSlots; ++s) {
          if (s >= per) continue;
          const int gg = g0 + s;
          double s1 = 0., s2 = 0.;
          for (int r = 0; r < P; ++r) { s1 += s_red[s][0][r * ncp + cl]; s2 += s_red[s][1][r * ncp + cl]; }
          const double mu = s1 / count;
          double var = s2 / count - mu * mu;
          if (var < 0.) var = 0.;
          if (gg == g) {
            const float inv = (float)(1.0 / sqrt(var + (double)eps));
            const float sc = gm * inv;
            const float sf = (float)((double)bt - mu * (double)sc);
            s_sc[cb + cl] = sc; s_sf[cb + cl] = sf;
            if (blockIdx.x == 0) {
              scale_out[g * C + c] = sc; shift_out[g * C + c] = sf; mean_out[g * C + c] = (float)mu; invstd_out[g * C + c] = inv;
            }
          }
          if (writer) {
            const double unb = count > 1. ? var * count / (count - 1.) : var;
            rm = (1.f - momentum) * rm + momentum * (float)mu;
            rv = (1.f - momentum) * rv + momentum * (float)unb;
          }
        }
      }
    }
    if (writer && lead) { rmean[c] = rm; rvar[c] = rv; }
  }
  __syncthreads();
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int c0 = u * N;
  float sc[N], sf[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { sc[e] = s_sc[tx * N + e]; sf[e] = s_sf[tx * N + e]; }
  const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty, stride = (long)gridDim.x * rg.ty;
  if (res) affine_act_rows<T, VEC, HS, true>(x, ldx, y, ldy, res, ldr, sc, sf, c0, base, npix_g, first, stride, act);
  else affine_act_rows<T, VEC, HS, false>(x, ldx, y, ldy, res, ldr, sc, sf, c0, base, npix_g, first, stride, act);
}

// gx = gy * act'(x*scale+shift) * scale + dS1 + 2*x*dS2 with dS derived in the kernel from the (dscale, dshift) replica
// sums of the first phase; the first workgroup of a channel slice also writes dgamma / dbeta (summed over groups).
template <typename T, bool VEC, bool HS = false, bool WIN = true>
__global__ __launch_bounds__(256) void bn_bwd_apply_fin_kernel(const T* gy, int ldg, const T* x, int ldx,
                                                               T* gx, int ldgx, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, const float* __restrict__ dscale,
                                                               const float* __restrict__ dshift, int nrep,
                                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int acc_par, float pscale, int C, long npix_g,
                                                               double inv_count, int act, const double* __restrict__ dsum, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  __shared__ float s_a[64 * 8], s_b2[64 * 8];
  __shared__ float s_red[kFoldSlots][2][256];
  const int G = gridDim.z, g = blockIdx.z;
  const int ch0 = blockIdx.y * rg.tx * N;
  const int nch = min(rg.tx, rg.units - (int)blockIdx.y * rg.tx) * N;
  // the streaming pass's own coefficients are asked for first: they arrive while the fold runs
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  const bool live = ty < rg.ty && u < rg.units;
  const int c0 = u * N;
  float sc[N], sf[N];
  if (live) {
#pragma unroll
    for (int e = 0; e < N; ++e) { sc[e] = scale[g * C + c0 + e]; sf[e] = shift[g * C + c0 + e]; }
  }
  // replica fold in one round trip (see affine_act_bn_kernel): threads = (channel slot cl, replica lane rl)
  const int ncp = nch <= 32 ? 32 : nch <= 64 ? 64 : nch <= 128 ? 128 : 256;
  const int P = 256 / ncp;
  const int cl = threadIdx.x & (ncp - 1), rl = threadIdx.x / ncp;
  const bool writer = blockIdx.x == 0 && g == 0 && dgamma;     // wave-uniform per workgroup
  const int per = WIN && writer && G <= kFoldSlots ? G : 1;    // groups per round
  const int nround = writer && per == 1 ? G : 1;
  for (int cb = 0; cb < nch; cb += ncp) {
    const int c = ch0 + cb + cl;
    const bool okc = cb + cl < nch && c < C;
    const bool lead = rl == 0 && okc;
    float dg = 0.f, db = 0.f, gm = 1.f, dg0 = 0.f, db0 = 0.f;
    for (int rd = 0; rd < nround; ++rd) {
      const int g0 = writer ? rd : g;
      float ds[kFoldSlots], dh[kFoldSlots], mu[kFoldSlots], inv[kFoldSlots];
#pragma unroll
      for (int s = 0; s < kFoldSlots; ++s) { ds[s] = 0.f; dh[s] = 0.f; mu[s] = 0.f; inv[s] = 0.f; }
      if (okc) {
#pragma unroll
        for (int s = 0; s < kFoldSlots; ++s) {
          if (s >= per) continue;
          const int gg = g0 + s;
          auto params = [&]() {                                 // the per-channel parameters travel with the replicas
            if (rl != 0) return;
            mu[s] = mean[gg * C + c]; inv[s] = invstd[gg * C + c];
            if (s == 0 && rd == 0) {
              if (gamma) gm = gamma[c];
              if (writer && acc_par) { dg0 = dgamma[c]; db0 = dbeta[c]; }
            }
          };
          if (dsum) {   // f64 [nrep][G][2][C] as written by the epilogue of sdhip_conv2d_fwd_bnbwd
            const long rs = (long)G * 2 * C;
            const unsigned lane = (unsigned)(c + rl * rs);
            const double* p0 = dsum + ((long)gg * 2 + 0) * C;
            const double* p1 = dsum + ((long)gg * 2 + 1) * C;
            if constexpr (WIN) {
              double v0[kFoldWin], v1[kFoldWin];
              fold_issue(p0, lane, rs, rl, P, nrep, v0);
              fold_issue(p1, lane, rs, rl, P, nrep, v1);
              params();
              issued();
              ds[s] = (float)fold_sum(p0, lane, rs, rl, P, nrep, v0);
              dh[s] = (float)fold_sum(p1, lane, rs, rl, P, nrep, v1);
            } else {
              params();
              fold_plain(p0, p1, lane, rs, rl, P, nrep, ds[s], dh[s]);
            }
          } else {
            const long rs = (long)G * C;
            const unsigned lane = (unsigned)(c + rl * rs);
            const float* p0 = dscale + (long)gg * C;
            const float* p1 = dshift + (long)gg * C;
            if constexpr (WIN) {
              float v0[kFoldWin], v1[kFoldWin];
              fold_issue(p0, lane, rs, rl, P, nrep, v0);
              fold_issue(p1, lane, rs, rl, P, nrep, v1);
              params();
              issued();
              ds[s] = fold_sum(p0, lane, rs, rl, P, nrep, v0);
              dh[s] = fold_sum(p1, lane, rs, rl, P, nrep, v1);
            } else {
              params();
              fold_plain(p0, p1, lane, rs, rl, P, nrep, ds[s], dh[s]);
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kFoldSlots; ++s)
        if (s < per) { s_red[s][0][threadIdx.x] = ds[s]; s_red[s][1][threadIdx.x] = dh[s]; }
      __syncthreads();
      if (lead) {
#pragma unroll
        for (int s = 0; s < kFoldSlots; ++s) {
          if (s >= per) continue;
          const int gg = g0 + s;
          float fs = 0.f, fh = 0.f;
          for (int r = 0; r < P; ++r) { fs += s_red[s][0][r * ncp + cl]; fh += s_red[s][1][r * ncp + cl]; }
          const float t = fs - mu[s] * fh;
          dg += inv[s] * t; db += fh;
          if (gg == g) {
            const double dinv = (double)gm * t;
            const double dvar = -0.5 * dinv * (double)inv[s] * inv[s] * inv[s];
            const double dmu = -(double)gm * inv[s] * fh - 2.0 * mu[s] * dvar;
            s_a[cb + cl] = (float)(dmu * inv_count);
            s_b2[cb + cl] = (float)(2.0 * dvar * inv_count);
          }
        }
      }
    }
    if (writer && lead) {      // pscale = 1 / world size when the sums are global (the gradient all-reduce adds the ranks' shares)
      dg *= pscale; db *= pscale;
      dgamma[c] = acc_par ? dg0 + dg : dg;
      dbeta[c] = acc_par ? db0 + db : db;
    }
  }
  __syncthreads();
  if (!live) return;
  float a[N], b2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { a[e] = s_a[tx * N + e]; b2[e] = s_b2[tx * N + e]; }
  const long base = (long)g * npix_g, first = (long)blockIdx.x * rg.ty + ty, stride = (long)gridDim.x * rg.ty;
  if (npix_g <= stride) bn_bwd_rows<T, VEC, HS, 1>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a, b2, c0, base, npix_g, first, stride, act);
  else bn_bwd_rows<T, VEC, HS, 4>(gy, ldg, x, ldx, gx, ldgx, sc, sf, a, b2, c0, base, npix_g, first, stride, act);
}


// S[g][0][c] += sum x, S[g][1][c] += sum x^2  (f64 atomics)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void channel_stats_kernel(const T* __restrict__ x, int ldx, double* __restrict__ S, int ldc, int nrep,
                                                            int C, long npix_g, RowGeom rg) {
  constexpr int N = Unit<T, VEC>::N;
  __shared__ float red[2][256 * (VEC ? Chunk<T>::N : 1)];
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  const bool live = ty < rg.ty && u < rg.units;
  const int g = blockIdx.z, c0 = u * N;
  float a1[N], a2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { a1[e] = 0.f; a2[e] = 0.f; }
  const long base = (long)g * npix_g;
  if (live) {
    for (long pix = (long)blockIdx.x * rg.ty + ty; pix < npix_g; pix += (long)gridDim.x * rg.ty) {
      float xv[N];
      Unit<T, VEC>::load(x + (base + pix) * ldx + c0, xv);
#pragma unroll
      for (int e = 0; e < N; ++e) { a1[e] += xv[e]; a2[e] = fmaf(xv[e], xv[e], a2[e]); }
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) { red[0][threadIdx.x * N + e] = a1[e]; red[1][threadIdx.x * N + e] = a2[e]; }
  __syncthreads();
  const int nch = min(rg.tx, rg.units - blockIdx.y * rg.tx) * N;   // channels of this block's unit group
  for (int cc = threadIdx.x; cc < 2 * nch; cc += 256) {             // consecutive lanes -> consecutive channels (see affine_act_bwd)
    const int which = cc >= nch, ch = cc - which * nch;
    const int txx = ch / N, e = ch - txx * N;
    double sum = 0.;
    for (int r = 0; r < rg.ty; ++r) sum += red[which][(r * rg.tx + txx) * N + e];
    double* Sr = S + (long)(blockIdx.x % nrep) * gridDim.z * 2 * ldc;   // replica r of [nrep][G][2][ldc]
    atomicAdd(Sr + ((long)g * 2 + which) * ldc + blockIdx.y * rg.tx * N + ch, sum);
  }
}

// ---- per-channel finalize (tiny) ------------------------------------------------
// train: S -> mean, invstd, scale, shift, running stats (groups applied in order)
__global__ void bn_finalize_kernel(const double* __restrict__ S, int ldc, int nrep, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ rmean, float* __restrict__ rvar,
                                   float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_out,
                                   float* __restrict__ invstd_out, int C, int G, double count, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float gm = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
  if (S == nullptr) {  // eval mode: running statistics
    const float inv = 1.f / sqrtf(rvar[c] + eps);
    for (int g = 0; g < G; ++g) {
      scale[g * C + c] = gm * inv;
      shift[g * C + c] = bt - rmean[c] * gm * inv;
      if (mean_out) { mean_out[g * C + c] = rmean[c]; invstd_out[g * C + c] = inv; }
    }
    return;
  }
  float rm = rmean ? rmean[c] : 0.f, rv = rvar ? rvar[c] : 0.f;
  for (int g = 0; g < G; ++g) {
    double s1 = 0., s2 = 0.;
#pragma unroll 8
    for (int r = 0; r < nrep; ++r) {
      const double* Sr = S + (long)r * G * 2 * ldc;
      s1 += Sr[((long)g * 2 + 0) * ldc + c];
      s2 += Sr[((long)g * 2 + 1) * ldc + c];
    }
    const double mu = s1 / count;
    double var = s2 / count - mu * mu;
    if (var < 0.) var = 0.;
    const float inv = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gm * inv;
    scale[g * C + c] = sc;
    shift[g * C + c] = (float)((double)bt - mu * (double)sc);
    mean_out[g * C + c] = (float)mu;
    invstd_out[g * C + c] = inv;
    const double unb = count > 1. ? var * count / (count - 1.) : var;
    rm = (1.f - momentum) * rm + momentum * (float)mu;
    rv = (1.f - momentum) * rv + momentum * (float)unb;
  }
  if (rmean) { rmean[c] = rm; rvar[c] = rv; }
}

// (dscale, dshift)[rep][G][C] -> dgamma[C], dbeta[C] (summed over groups), dS[G][2][C]
// One workgroup = 32 channels x 8 replica lanes: every thread sums nrep/8 replicas (independent loads, one round trip),
// the 8 partials meet in LDS.  (A single thread per channel walking 32 replicas made this per-layer kernel a 17 us
// latency chain on the backward critical path.)
__global__ __launch_bounds__(256) void bn_finalize_bwd_kernel(const float* __restrict__ dscale, const float* __restrict__ dshift, int nrep,
                                       const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ invstd,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta, double* __restrict__ dS, int ldc, int acc_flags,
                                       int C, int G, double inv_count, int train) {
  __shared__ float red[2][8][32];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const bool okc = c < C;
  const int acc_ds = acc_flags & 1, acc_par = acc_flags & 2;   // bit 0: dstats += ; bit 1: dgamma/dbeta +=
  float dg = 0.f, db = 0.f;
  for (int g = 0; g < G; ++g) {
    float ds = 0.f, dh = 0.f;
    if (okc) {
#pragma unroll 4
      for (int r = rl; r < nrep; r += 8) { ds += dscale[((long)r * G + g) * C + c]; dh += dshift[((long)r * G + g) * C + c]; }
    }
    __syncthreads();   // previous group's partials are consumed
    red[0][rl][cl] = ds; red[1][rl][cl] = dh;
    __syncthreads();
    if (rl == 0 && okc) {
      ds = 0.f; dh = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) { ds += red[0][r][cl]; dh += red[1][r][cl]; }
      const float gm = gamma ? gamma[c] : 1.f;
      const float mu = mean[g * C + c], inv = invstd[g * C + c];
      const float t = ds - mu * dh;       // d/d(gamma*invstd) collected
      dg += inv * t;
      db += dh;
      if (dS) {
        if (train) {
          const double dinv = (double)gm * t;
          const double dvar = -0.5 * dinv * (double)inv * inv * inv;
          const double dmu = -(double)gm * inv * dh - 2.0 * mu * dvar;
          double* d0 = dS + ((long)g * 2 + 0) * ldc + c;
          double* d1 = dS + ((long)g * 2 + 1) * ldc + c;
          *d0 = (acc_ds ? *d0 : 0.) + dmu * inv_count;
          *d1 = (acc_ds ? *d1 : 0.) + dvar * inv_count;
        } else if (!acc_ds) {
          dS[((long)g * 2 + 0) * ldc + c] = 0.;
          dS[((long)g * 2 + 1) * ldc + c] = 0.;
        }
      }
    }
  }
  if (rl == 0 && okc) {
    if (dgamma) dgamma[c] = acc_par ? dgamma[c] + dg : dg;
    if (dbeta) dbeta[c] = acc_par ? dbeta[c] + db : db;
  }
}

struct Plan { RowGeom rg; dim3 grid; };
Plan plan(int units, long npix_g, int G, int max_blocks = 2048) {
  Plan p;
  p.rg = row_geom(units);
  const int gy = sdhip_cdiv(units, p.rg.tx);
  long gx = (npix_g + p.rg.ty - 1) / p.rg.ty;
  const long cap = max_blocks / ((long)gy * G) > 0 ? max_blocks / ((long)gy * G) : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  p.grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)G);
  return p;
}

// workgroups of the consumer-side-finalize kernels: each one re-derives its coefficients from the replica sums (KBs from L2)
int tune_fused_blocks() { return sdhip_diag().tune_fused_blocks; }

// the 32-bit lane offset of fold_at: the last replica lane (at most 8 of them) of the last channel, in bytes
inline bool fold_span_ok(long rs, int C, size_t elem) { return (unsigned long)(7 * rs + C) * elem < (1UL << 32); }

int check_rows(const char* who, long npix, int C, int G, int dtype) {
  SDHIP_CHECK_ARG(npix > 0 && C > 0 && G >= 1 && npix % G == 0, "%s: bad shape npix=%ld C=%d groups=%d", who, npix, C, G);
  SDHIP_CHECK_DTYPE(who, dtype);
  return 0;
}

}  // namespace

// out[row*ldo + c] += sum_r ws[r*rep_stride + row*ldw + c]   (rows = 2*groups statistics rows)
__global__ void replica_sum_kernel(const double* __restrict__ ws, double* __restrict__ out, int nrep, long rep_stride,
                                   int rows, int C, int ldw, int ldo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C) return;
  const int row = i / C, c = i - row * C;
  double s = 0.;
#pragma unroll 8
  for (int r = 0; r < nrep; ++r) s += ws[(long)r * rep_stride + (long)row * ldw + c];
  out[(long)row * ldo + c] += s;
}

// fold + finalize in one launch (DenseNet: the statistics of a layer's 32 new slab channels are folded into the slab
// statistics and the NEXT layer's norm1 — which reads all channels up to and including the new ones — is finalized):
// channel c of [c_new0, c_new0 + Cn) first adds its replica sums into S, then every channel < C is finalized from S.
__global__ void bn_fold_finalize_kernel(const double* __restrict__ ws, int nrep, int ldw, int c_new0, int Cn, double* __restrict__ S, int ldc,
                                        const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ rmean,
                                        float* __restrict__ rvar, float* __restrict__ scale, float* __restrict__ shift,
                                        float* __restrict__ mean_out, float* __restrict__ invstd_out, int C, int G, double count, float eps,
                                        float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float gm = gamma[c], bt = beta[c];
  float rm = rmean ? rmean[c] : 0.f, rv = rvar ? rvar[c] : 0.f;
  const bool fresh = c >= c_new0 && c < c_new0 + Cn;
  for (int g = 0; g < G; ++g) {
    double s1 = S[((long)g * 2 + 0) * ldc + c], s2 = S[((long)g * 2 + 1) * ldc + c];
    if (fresh) {
      const int cn = c - c_new0;
#pragma unroll 8
      for (int r = 0; r < nrep; ++r) {
        const double* Sr = ws + (long)r * G * 2 * ldw;
        s1 += Sr[((long)g * 2 + 0) * ldw + cn];
        s2 += Sr[((long)g * 2 + 1) * ldw + cn];
      }
      S[((long)g * 2 + 0) * ldc + c] = s1;
      S[((long)g * 2 + 1) * ldc + c] = s2;
    }
    const double mu = s1 / count;
    double var = s2 / count - mu * mu;
    if (var < 0.) var = 0.;
    const float inv = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gm * inv;
    scale[g * C + c] = sc;
    shift[g * C + c] = (float)((double)bt - mu * (double)sc);
    mean_out[g * C + c] = (float)mu;
    invstd_out[g * C + c] = inv;
    const double unb = count > 1. ? var * count / (count - 1.) : var;
    rm = (1.f - momentum) * rm + momentum * (float)mu;
    rv = (1.f - momentum) * rv + momentum * (float)unb;
  }
  if (rmean) { rmean[c] = rm; rvar[c] = rv; }
}

extern "C" int sdhip_bn_fold_finalize(const double* ws, int nrep, int ldw, int c_new0, int Cn, double* S, int ldc,
                                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                                      float* scale, float* shift, float* mean_out, float* invstd_out, int C, int groups,
                                      double count, float eps, float momentum, void* stream) {
  SDHIP_CHECK_ARG(ws && S && gamma && beta && scale && shift && mean_out && invstd_out && nrep >= 1 && Cn > 0 && c_new0 >= 0 &&
                  c_new0 + Cn <= C && ldw >= Cn && ldc >= C && groups >= 1 && count > 0., "bn_fold_finalize: bad arguments");
  SDHIP_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn_fold_finalize: running statistics must come together");
  hipLaunchKernelGGL(bn_fold_finalize_kernel, dim3(sdhip_cdiv(C, 128)), dim3(128), 0, (hipStream_t)stream, ws, nrep, ldw, c_new0, Cn, S, ldc,
                     gamma, beta, running_mean, running_var, scale, shift, mean_out, invstd_out, C, groups, count, eps, momentum);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_stats_replica_sum(const double* ws, double* out, int nrep, int groups, int C, int ldw, int ldo, void* stream) {
  SDHIP_CHECK_ARG(ws && out && nrep >= 1 && groups >= 1 && C > 0 && ldw >= C && ldo >= C, "stats_replica_sum: bad arguments");
  const int rows = 2 * groups;
  hipLaunchKernelGGL(replica_sum_kernel, dim3(sdhip_cdiv((long)rows * C, 256)), dim3(256), 0, (hipStream_t)stream, ws, out, nrep,
                     (long)rows * ldw, rows, C, ldw, ldo);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_affine_act(const void* x, int ldx, void* y, int ldy, const void* res, int ldr,
                                const float* scale, const float* shift, long npix, int C, int groups, int act,
                                int dtype, void* stream) {
  const int G = groups;
  if (int rc = check_rows("affine_act", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(x && y && ldx >= C && ldy >= C && (!res || ldr >= C), "affine_act: bad pointers/strides");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == 2 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID, "affine_act: activation %d", act);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldx, ldy, res ? ldr : 0}, {x, y, res});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G);
    sdhip_by_flag(v, [&](auto V) { sdhip_by_flag(hard_act(act), [&](auto HS) {
      hipLaunchKernelGGL((affine_act_kernel<T, V(), HS()>), pl.grid, dim3(256), 0, s, (const T*)x, ldx, (T*)y, ldy, (const T*)res, ldr, scale, shift, C, npix / G, act, pl.rg);
    }); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_affine_act_bwd(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                                    const float* scale, const float* shift, float* dscale, float* dshift, int nrep,
                                    long npix, int C, int groups, int act, int accumulate, int prezeroed, int dtype, void* stream) {
  if (nrep < 1) nrep = 1;
  const int G = groups;
  if (int rc = check_rows("affine_act_bwd", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gy && x && ldg >= C && ldx >= C && (!gx || ldgx >= C), "affine_act_bwd: bad pointers/strides");
  SDHIP_CHECK_ARG((dscale == nullptr) == (dshift == nullptr), "affine_act_bwd: dscale/dshift must come together");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == 2 || act == 4 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID,
                  "affine_act_bwd: activation %d", act);
  hipStream_t s = (hipStream_t)stream;
  if (dscale && !prezeroed) {
    if (sdhip_zero_async(dscale, sizeof(float) * (size_t)nrep * G * C, s) != hipSuccess ||
        sdhip_zero_async(dshift, sizeof(float) * (size_t)nrep * G * C, s) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "affine_act_bwd: memset failed");
  }
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldg, ldx, gx ? ldgx : 0}, {gy, x, gx});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G, 1024);
    sdhip_by_flag(v, [&](auto V) { sdhip_by_flag(hard_act(act), [&](auto HS) {
      hipLaunchKernelGGL((affine_act_bwd_kernel<T, V(), HS()>), pl.grid, dim3(256), 0, s, (const T*)gy, ldg, (const T*)x, ldx, (T*)gx, ldgx, scale, shift, dscale, dshift, nrep, C, npix / G, act, accumulate, pl.rg);
    }); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_act_out_bwd(const void* gy, int ldg, const void* y, int ldy, void* graw, int ldgr, const float* scale,
                                 long npix, int C, int groups, int act, int dtype, void* stream) {
  const int G = groups;
  if (int rc = check_rows("act_out_bwd", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gy && y && graw && scale && ldg >= C && ldy >= C && ldgr >= C, "act_out_bwd: bad pointers/strides");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == 2, "act_out_bwd: activation %d", act);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldg, ldy, ldgr}, {gy, y, graw});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G);
    sdhip_by_flag(v, [&](auto V) {
      hipLaunchKernelGGL((act_out_bwd_kernel<T, V()>), pl.grid, dim3(256), 0, s, (const T*)gy, ldg, (const T*)y, ldy, (T*)graw, ldgr, scale, C, npix / G, act, pl.rg);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_stats_fix(const void* gin, int ldgi, const void* x, int ldx, void* gout, int ldgo,
                               const double* dS, int ldc, long npix, int C, int groups, int dtype, void* stream) {
  if (ldc <= 0) ldc = C;
  const int G = groups;
  if (int rc = check_rows("stats_fix", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gin && x && gout && dS && ldgi >= C && ldx >= C && ldgo >= C, "stats_fix: bad pointers/strides");
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldgi, ldx, ldgo}, {gin, x, gout});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G);
    sdhip_by_flag(v, [&](auto V) {
      hipLaunchKernelGGL((stats_fix_kernel<T, V()>), pl.grid, dim3(256), 0, s, (const T*)gin, ldgi, (const T*)x, ldx, (T*)gout, ldgo, dS, ldc, C, npix / G, pl.rg);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_bn_bwd_apply(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                                  const float* scale, const float* shift, const double* dS, int ldc,
                                  long npix, int C, int groups, int act, int dtype, void* stream) {
  if (ldc <= 0) ldc = C;
  const int G = groups;
  if (int rc = check_rows("bn_bwd_apply", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gy && x && gx && scale && shift && dS && ldg >= C && ldx >= C && ldgx >= C, "bn_bwd_apply: bad pointers/strides");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == 2 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID, "bn_bwd_apply: activation %d", act);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldg, ldx, ldgx}, {gy, x, gx});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G, 1024);
    sdhip_by_flag(v, [&](auto V) { sdhip_by_flag(hard_act(act), [&](auto HS) {
      hipLaunchKernelGGL((bn_bwd_apply_kernel<T, V(), HS()>), pl.grid, dim3(256), 0, s, (const T*)gy, ldg, (const T*)x, ldx, (T*)gx, ldgx, scale, shift, dS, ldc, C, npix / G, act, pl.rg);
    }); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_affine_act_bn(const void* x, int ldx, void* y, int ldy, const void* res, int ldr,
                                   const double* stats, int ldc, int nrep, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float* scale, float* shift, float* mean_out,
                                   float* invstd_out, long npix, int C, int groups, double count, float eps, float momentum,
                                   int act, int dtype, void* stream) {
  if (ldc <= 0) ldc = C;
  if (nrep < 1) nrep = 1;
  const int G = groups;
  if (int rc = check_rows("affine_act_bn", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(x && y && stats && scale && shift && mean_out && invstd_out && ldx >= C && ldy >= C && (!res || ldr >= C),
                  "affine_act_bn: bad pointers/strides");
  SDHIP_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr) && count > 0., "affine_act_bn: bad statistics arguments");
  SDHIP_CHECK_ARG(fold_span_ok((long)G * 2 * ldc, C, sizeof(double)), "affine_act_bn: statistics replicas too far apart");
  SDHIP_CHECK_ARG(act == 0 || act == 1 || act == 2 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID, "affine_act_bn: activation %d", act);
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldx, ldy, res ? ldr : 0}, {x, y, res});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G, tune_fused_blocks());
    sdhip_by_flag(v, [&](auto V) { sdhip_by_flag(hard_act(act), [&](auto HS) { sdhip_by_flag(G >= 2, [&](auto WIN) {
      hipLaunchKernelGGL((affine_act_bn_kernel<T, V(), HS(), WIN()>), pl.grid, dim3(256), 0, s, (const T*)x, ldx, (T*)y, ldy, (const T*)res, ldr, stats, ldc, nrep, gamma, beta, running_mean, running_var,
                         scale, shift, mean_out, invstd_out, C, npix / G, count, eps, momentum, act, pl.rg);
    }); }); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

static int bn_bwd_apply_fin_impl(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                                 const float* scale, const float* shift, const float* dscale, const float* dshift, const double* dsum, int nrep,
                                      const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                      int accumulate_params, float param_scale, long npix, int C, int groups, double count, int act, int dtype,
                                      void* stream) {
  if (nrep < 1) nrep = 1;
  const int G = groups;
  if (int rc = check_rows("bn_bwd_apply_fin", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gy && x && gx && scale && shift && ((dscale && dshift) || dsum) && mean && invstd && ldg >= C && ldx >= C && ldgx >= C,
                  "bn_bwd_apply_fin: bad pointers/strides");
  SDHIP_CHECK_ARG((act == 0 || act == 1 || act == 2 || act == SDHIP_ACT_HSWISH || act == SDHIP_ACT_HSIGMOID) && count > 0. && (dgamma == nullptr) == (dbeta == nullptr),
                  "bn_bwd_apply_fin: bad arguments");
  SDHIP_CHECK_ARG(fold_span_ok((long)G * 2 * C, C, sizeof(double)), "bn_bwd_apply_fin: replicas too far apart");
  hipStream_t s = (hipStream_t)stream;
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldg, ldx, ldgx}, {gy, x, gx});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G, tune_fused_blocks());
    sdhip_by_flag(v, [&](auto V) { sdhip_by_flag(hard_act(act), [&](auto HS) { sdhip_by_flag(G >= 2, [&](auto WIN) {
      hipLaunchKernelGGL((bn_bwd_apply_fin_kernel<T, V(), HS(), WIN()>), pl.grid, dim3(256), 0, s, (const T*)gy, ldg, (const T*)x, ldx, (T*)gx, ldgx, scale, shift, dscale, dshift, nrep, gamma, mean, invstd,
                         dgamma, dbeta, accumulate_params, param_scale, C, npix / G, 1.0 / count, act, dsum, pl.rg);
    }); }); });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_bn_bwd_apply_fin(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                                      const float* scale, const float* shift, const float* dscale, const float* dshift, int nrep,
                                      const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                      int accumulate_params, float param_scale, long npix, int C, int groups, double count, int act, int dtype,
                                      void* stream) {
  return bn_bwd_apply_fin_impl(gy, ldg, x, ldx, gx, ldgx, scale, shift, dscale, dshift, nullptr, nrep, gamma, mean, invstd, dgamma, dbeta,
                               accumulate_params, param_scale, npix, C, groups, count, act, dtype, stream);
}

// ... with the two reductions given as f64 [nrep][groups][2][C] (sum(gm*x), sum(gm)): the layout the epilogue of
// sdhip_conv2d_fwd_bnbwd adds them in.
extern "C" int sdhip_bn_bwd_apply_fin_d(const void* gy, int ldg, const void* x, int ldx, void* gx, int ldgx,
                                        const float* scale, const float* shift, const double* sums, int nrep,
                                        const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                        int accumulate_params, float param_scale, long npix, int C, int groups, double count, int act, int dtype,
                                        void* stream) {
  return bn_bwd_apply_fin_impl(gy, ldg, x, ldx, gx, ldgx, scale, shift, nullptr, nullptr, sums, nrep, gamma, mean, invstd, dgamma, dbeta,
                               accumulate_params, param_scale, npix, C, groups, count, act, dtype, stream);
}

extern "C" int sdhip_channel_stats(const void* x, int ldx, double* stats, int ldc, int nrep, long npix, int C, int groups,
                                   int zero_first, int dtype, void* stream) {
  if (ldc <= 0) ldc = C;
  if (nrep < 1) nrep = 1;
  const int G = groups;
  if (int rc = check_rows("channel_stats", npix, C, G, dtype)) return rc;
  SDHIP_CHECK_ARG(x && stats && ldx >= C, "channel_stats: bad pointers/strides");
  hipStream_t s = (hipStream_t)stream;
  if (zero_first) {
    // kernels, not memset nodes (sdhip_common.h): dense replicas in one launch, a strided slice row by row
    const size_t rows = 2 * (size_t)G * nrep;
    if (ldc == C) {
      if (sdhip_zero_async(stats, sizeof(double) * (size_t)C * rows, s) != hipSuccess) SDHIP_FAIL(SDHIP_ERR_LAUNCH, "channel_stats: clear failed");
    } else {
      for (size_t r = 0; r < rows; ++r)
        if (sdhip_zero_async(stats + r * (size_t)ldc, sizeof(double) * (size_t)C, s) != hipSuccess) SDHIP_FAIL(SDHIP_ERR_LAUNCH, "channel_stats: clear failed");
    }
  }
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const bool v = sdhip_vec_ok<T>(C, {ldx}, {x});
    const Plan pl = plan(v ? C / Chunk<T>::N : C, npix / G, G, 1024);
    sdhip_by_flag(v, [&](auto V) {
      hipLaunchKernelGGL((channel_stats_kernel<T, V()>), pl.grid, dim3(256), 0, s, (const T*)x, ldx, stats, ldc, nrep, C, npix / G, pl.rg);
    });
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_bn_finalize(const double* stats, int ldc, int nrep, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var,
                                 float* scale, float* shift, float* mean_out, float* invstd_out,
                                 int C, int groups, double count, float eps, float momentum, void* stream) {
  SDHIP_CHECK_ARG(C > 0 && groups >= 1 && scale && shift, "bn_finalize: bad arguments");
  SDHIP_CHECK_ARG(stats || (running_mean && running_var), "bn_finalize: eval mode needs running statistics");
  SDHIP_CHECK_ARG(!stats || (mean_out && invstd_out && count >= 1.), "bn_finalize: train mode needs mean/invstd outputs and a count");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(sdhip_cdiv(C, 128)), dim3(128), 0, (hipStream_t)stream, stats, ldc > 0 ? ldc : C, nrep > 0 ? nrep : 1, gamma, beta,
                     running_mean, running_var, scale, shift, mean_out, invstd_out, C, groups, count, eps, momentum);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

// bn_finalize_bwd of one DenseNet layer's norm1 + stats_fix of the NEXT layer to be processed, in one launch.
// The backward walk of a dense block (models/densenet.py:41-45) alternates a per-channel kernel (the statistics gradient
// dS of the slab channels a layer read) with an elementwise one (dy = g + dS0 + 2 x dS1 on the 32 channels the previous
// layer wrote, which needs exactly the top 32 of the dS just updated).  Here every workgroup re-derives the 32 coefficients
// it needs from the replica sums (a few KB from L2) while the first ceil(Cf/32) workgroups also do the per-channel work for
// all Cf channels (dgamma, dbeta, dS of the channels below the slice — the slice's own dS is consumed here and never again).
// one statistics group of the per-channel part of stats_fix_fin, as its replica lane sees it
struct SffGroup {
  float v0[kSffWin], v1[kSffWin];     // replica windows of dscale / dshift
  float ds, dh, mu, inv;
  double d0, d1;                      // dS of the channel before this call (outside the slice)
  const float *p0, *p1;
  unsigned lane;
  __device__ __forceinline__ void issue(const float* dscale, const float* dshift, const float* mean, const float* invstd,
                                        const double* dS, int ldc, int gg, int c, int Cf, long rs, int rl, int nrep,
                                        bool outside) {
    p0 = dscale + (long)gg * Cf; p1 = dshift + (long)gg * Cf;
    lane = (unsigned)(c + rl * rs);
    fold_issue(p0, lane, rs, rl, 8, nrep, v0);
    fold_issue(p1, lane, rs, rl, 8, nrep, v1);
    mu = 0.f; inv = 0.f; d0 = 0.; d1 = 0.;
    if (rl == 0) {
      mu = mean[gg * Cf + c]; inv = invstd[gg * Cf + c];
      if (outside) { d0 = dS[((long)gg * 2 + 0) * ldc + c]; d1 = dS[((long)gg * 2 + 1) * ldc + c]; }
    }
  }
  __device__ __forceinline__ void sum(long rs, int rl, int nrep) {
    ds = fold_sum(p0, lane, rs, rl, 8, nrep, v0);
    dh = fold_sum(p1, lane, rs, rl, 8, nrep, v1);
  }
};

// Both folds (the per-channel one of the first workgroups and the slice's) and every parameter they need are in flight before
// the one wait, and they share one barrier pair; a second group of the per-channel fold joins that pair after a round trip
// of its own, only groups beyond kFoldSlots cost the per-channel workgroups a further pair each.
template <typename T>
__global__ __launch_bounds__(256) void stats_fix_fin_kernel(const T* gin, int ldgi, const T* x, int ldx, T* gout, int ldgo,
                                                            long npix_g, RowGeom rg, double* __restrict__ dS, int ldc, int cs,
                                                            const float* __restrict__ dscale, const float* __restrict__ dshift, int nrep,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int acc_par, float pscale, int Cf, int G, double inv_count) {
  constexpr int N = Unit<T, true>::N;
  __shared__ float red[kFoldSlots + 1][2][8][32];       // the per-channel fold's group slots, then the slice's
  __shared__ float fa[32], fb[32];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int nfb = (Cf + 31) >> 5;
  const int g = blockIdx.z;
  const long rs = (long)G * Cf;
  const bool chan = blockIdx.z == 0 && blockIdx.y == 0 && (int)blockIdx.x < nfb;   // workgroup-uniform: per-channel work of block blockIdx.x
  const int per = G <= kFoldSlots ? G : 1, nround = G > kFoldSlots ? G : 1;
  const int c = blockIdx.x * 32 + cl;                     // per-channel part
  const bool okc = chan && c < Cf, lead = okc && rl == 0;
  const bool outside = c < cs || c >= cs + 32;            // the slice's dS is formed (and consumed) by the elementwise part below
  float dg = 0.f, db = 0.f, gmc = 0.f, dg0 = 0.f, db0 = 0.f;
  // the group in slot `slot` of red: t, dgamma / dbeta shares, dS outside the slice
  auto use = [&](const SffGroup& q, int slot, int gg) {
    float fs = 0.f, fh = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) { fs += red[slot][0][r][cl]; fh += red[slot][1][r][cl]; }
    const float t = fs - q.mu * fh;
    dg += q.inv * t;
    db += fh;
    if (outside) {
      const double dinv = (double)gmc * t;
      const double dvar = -0.5 * dinv * (double)q.inv * q.inv * q.inv;
      const double dmu = -(double)gmc * q.inv * fh - 2.0 * q.mu * dvar;
      dS[((long)gg * 2 + 0) * ldc + c] = q.d0 + dmu * inv_count;
      dS[((long)gg * 2 + 1) * ldc + c] = q.d1 + dvar * inv_count;
    }
  };
  // issue: the slice's fold for this workgroup's statistics group, group 0 of the per-channel fold, all parameters
  const int c2 = cs + cl;                                 // coefficients of the slice channels cs .. cs+31
  const float* q0 = dscale + (long)g * Cf;
  const float* q1 = dshift + (long)g * Cf;
  const unsigned lane2 = (unsigned)(c2 + rl * rs);
  float w0[kSffWin], w1[kSffWin];
  fold_issue(q0, lane2, rs, rl, 8, nrep, w0);
  fold_issue(q1, lane2, rs, rl, 8, nrep, w1);
  float gm2 = 0.f, mu2 = 0.f, inv2 = 0.f;
  double e0 = 0., e1 = 0.;
  SffGroup A, B;
  if (okc) {
    A.issue(dscale, dshift, mean, invstd, dS, ldc, 0, c, Cf, rs, rl, nrep, outside);
    if (rl == 0) {
      gmc = gamma[c];
      if (acc_par) { dg0 = dgamma[c]; db0 = dbeta[c]; }
    }
  }
  if (rl == 0) {   // last: the compiler converts some of these to f64 where they are loaded, which waits for them
    gm2 = gamma[c2]; mu2 = mean[g * Cf + c2]; inv2 = invstd[g * Cf + c2];
    e0 = dS[((long)g * 2 + 0) * ldc + c2]; e1 = dS[((long)g * 2 + 1) * ldc + c2];
  }
  issued();
  red[kFoldSlots][0][rl][cl] = fold_sum(q0, lane2, rs, rl, 8, nrep, w0);
  red[kFoldSlots][1][rl][cl] = fold_sum(q1, lane2, rs, rl, 8, nrep, w1);
  if (chan) {
    A.ds = 0.f; A.dh = 0.f; B.ds = 0.f; B.dh = 0.f;
    if (okc) {
      A.sum(rs, rl, nrep);
      if (per == 2) {
        B.issue(dscale, dshift, mean, invstd, dS, ldc, 1, c, Cf, rs, rl, nrep, outside);
        issued();
        B.sum(rs, rl, nrep);
      }
    }
    red[0][0][rl][cl] = A.ds; red[0][1][rl][cl] = A.dh;
    if (per == 2) { red[1][0][rl][cl] = B.ds; red[1][1][rl][cl] = B.dh; }
  }
  __syncthreads();
  if (lead) {
    use(A, 0, 0);
    if (per == 2) use(B, 1, 1);
  }
  if (rl == 0) {
    float fs = 0.f, fh = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) { fs += red[kFoldSlots][0][r][cl]; fh += red[kFoldSlots][1][r][cl]; }
    const float t = fs - mu2 * fh;
    const double dinv = (double)gm2 * t;
    const double dvar = -0.5 * dinv * (double)inv2 * inv2 * inv2;
    const double dmu = -(double)gm2 * inv2 * fh - 2.0 * mu2 * dvar;
    fa[cl] = (float)(e0 + dmu * inv_count);
    fb[cl] = (float)(2.0 * (e1 + dvar * inv_count));
  }
  if (chan) {
    for (int rd = 1; rd < nround; ++rd) {                  // groups beyond the slots, one barrier pair each
      A.ds = 0.f; A.dh = 0.f;
      if (okc) {
        A.issue(dscale, dshift, mean, invstd, dS, ldc, rd, c, Cf, rs, rl, nrep, outside);
        issued();
        A.sum(rs, rl, nrep);
      }
      __syncthreads();   // previous group's partials are consumed
      red[0][0][rl][cl] = A.ds; red[0][1][rl][cl] = A.dh;
      __syncthreads();
      if (lead) use(A, 0, rd);
    }
    if (lead) {
      dg *= pscale; db *= pscale;                    // (see bn_bwd_apply_fin_kernel)
      dgamma[c] = acc_par ? dg0 + dg : dg;
      dbeta[c] = acc_par ? db0 + db : db;
    }
  }
  __syncthreads();
  ROW_TXTY(rg, tx, ty);
  const int u = blockIdx.y * rg.tx + tx;
  if (ty >= rg.ty || u >= rg.units) return;
  const int c0 = u * N;
  float a[N], b2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) { a[e] = fa[c0 + e]; b2[e] = fb[c0 + e]; }
  stats_fix_rows<T, true>(gin, ldgi, x, ldx, gout, ldgo, a, b2, c0, (long)g * npix_g, npix_g, (long)blockIdx.x * rg.ty + ty,
                          (long)gridDim.x * rg.ty);
}

extern "C" int sdhip_stats_fix_fin(const void* gin, int ldgi, const void* x, int ldx, void* gout, int ldgo, long npix,
                                   double* dS, int ldc, int cs, const float* dscale, const float* dshift, int nrep,
                                   const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                                   int accumulate_params, float param_scale, int Cf, int groups, double count, int dtype, void* stream) {
  const int G = groups;
  if (int rc = check_rows("stats_fix_fin", npix, 32, G, dtype)) return rc;
  SDHIP_CHECK_ARG(gin && x && gout && dS && dscale && dshift && gamma && mean && invstd && dgamma && dbeta && ldgi >= 32 && ldx >= 32 &&
                  ldgo >= 32 && cs >= 0 && cs + 32 <= Cf && ldc >= Cf && nrep >= 1 && count > 0., "stats_fix_fin: bad arguments");
  SDHIP_CHECK_ARG(fold_span_ok((long)G * Cf, Cf, sizeof(float)), "stats_fix_fin: replicas too far apart");
  hipStream_t s = (hipStream_t)stream;
  const int nfb = sdhip_cdiv(Cf, 32);
  const int rc = sdhip_by_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    SDHIP_CHECK_ARG((sdhip_vec_ok<T>(32, {ldgi, ldx, ldgo}, {gin, x, gout})), "stats_fix_fin: rows must be 16-byte aligned");
    Plan pl = plan(32 / Chunk<T>::N, npix / G, G);
    if ((int)pl.grid.x < nfb) pl.grid.x = nfb;            // enough workgroups for the per-channel part
    hipLaunchKernelGGL((stats_fix_fin_kernel<T>), pl.grid, dim3(256), 0, s, (const T*)gin, ldgi, (const T*)x, ldx, (T*)gout, ldgo, npix / G, pl.rg,
                       dS, ldc, cs, dscale, dshift, nrep, gamma, mean, invstd, dgamma, dbeta, accumulate_params, param_scale, Cf, G, 1.0 / count);
    return SDHIP_OK;
  });
  if (rc) return rc;
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

extern "C" int sdhip_bn_finalize_bwd(const float* dscale, const float* dshift, int nrep, const float* gamma,
                                     const float* mean, const float* invstd,
                                     float* dgamma, float* dbeta, double* dstats, int ldc, int accumulate_dstats,
                                     int C, int groups, double count, int train, void* stream) {
  SDHIP_CHECK_ARG(C > 0 && groups >= 1 && dscale && dshift && mean && invstd, "bn_finalize_bwd: bad arguments");
  hipLaunchKernelGGL(bn_finalize_bwd_kernel, dim3(sdhip_cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream, dscale, dshift,
                     nrep > 0 ? nrep : 1, gamma, mean, invstd, dgamma, dbeta, dstats, ldc > 0 ? ldc : C, accumulate_dstats, C, groups,
                     1.0 / count, train);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
