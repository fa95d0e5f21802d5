// Pointwise (1x1, stride 1) convolution with an input prologue on small maps, bf16, for gfx950: the conv1 of the DenseNet
// bottlenecks (128 .. 1024 input channels -> 128) on the maps where the tower is a chain of short launches.
//
// conv_fast.h runs these layers as one tap over Cin / 64 channel chunks, each chunk a barrier plus a global round trip
// with nothing to hide it behind.  Here the reduction is split over the waves of the workgroup instead (split-K), so that
// the number of barriers and of dependent global round trips per workgroup does not depend on Cin:
//   - a workgroup owns 64 consecutive pixels of one image x BN = 32 output channels; 8 waves (512 threads);
//   - wave w takes the 32-channel k-steps w, w + 8, ... (at most KB = 4 of them: Cin <= 1024) and forms the full 64 x 32
//     partial tile over them.  A 1x1 has no halo, so both MFMA fragments come straight from global memory, 16 bytes per
//     lane: lane (l15, lg) reads channels [k0 + 8 lg, + 8) of pixel l15 of each 16-pixel tile and of weight row l15 of
//     each 16-channel tile of the packed weights (the 'fwd' packing, [Cin / 64][Mpad][64]);
//   - ALL of a wave's loads are issued first; they do not depend on the prologue's coefficients, so they cover the round
//     trip of the coefficient table: the consumer-side BatchNorm finalize of conv_fast.h (pin_finalize below) or a copy
//     of the given in_scale / in_shift rows of the workgroup's statistics group;
//   - one barrier publishes the table; prologue (fma, optional max, repack to bf16) in registers, then the MFMAs.  The
//     channels [Cin, ldx) of a pixel and the pixel rows past the end of the image are not data (other layers' channels,
//     NaN): such lanes are not loaded and come out of the prologue as zero (relu(shift) is not zero: the table holds
//     scale = shift = 0 past Cin, and a ragged last tile zeroes its dead rows AFTER the prologue);
//   - the partial tiles go to LDS, one barrier, and wave t sums the 16 x 16 tile t of all waves in wave order (no LDS
//     atomics: the same inputs give the same y bits), rounds to bf16 and stores 8 bytes per lane;
//   - statistics of the STORED values as in conv_fast.h: the 16 pixels of a tile by row16_sum, the four pixel tiles of a
//     channel through LDS (64 values in f32), then one f64 atomic into replica (blockIdx.x + blockIdx.z) % nrep.
// 8 waves rather than 4: with 4 the loads of a wave at Cin = 1024 (8 k-steps x 24 registers) do not fit the register file
// next to the 32 accumulators without a second batch.  LDS: 8 KiB per working wave + the table + 1 KiB <= 73 KiB.
#pragma once
#include "conv_fast.h"

namespace {

struct PointArgs {
  const void* x; const void* wp; void* y;
  const float* in_scale; const float* in_shift; double* stats;
  int HW, Cin, ldx, Cout, Mpad, ldy;
  int in_relu, bpg;                    // bpg: images per statistics group
  int stats_ld, nrep; long rep_stride;
  int tab_off, tab_cs;                 // LDS byte offset of the (scale, shift) table behind the partial tiles; floats per row
  // consumer-side BatchNorm finalize: the fields of FastArgs under the same names (pin_finalize reads them)
  const double* pin_stats; int pin_ld, pin_nrep, pin_groups;
  const float* pin_gamma; const float* pin_beta;
  float* pin_scale; float* pin_shift; float* pin_mean; float* pin_invstd; float* pin_rmean; float* pin_rvar;
  float pin_eps, pin_momentum; double pin_count;
  const double* pend_stats; double* pin_fold; int pend_ld, pend_nrep, pend_c0, pend_n;
};

constexpr int kPointWaves = 8, kPointBN = 32, kPointPix = 64;
constexpr int kPointMaxWG = 512;   // the dispatch's upper limit on the grid: two workgroups on each of 256 CUs
constexpr int kPointMaxMap = 512;  // ... and on the pixels of one image: the largest map measured faster (16x32)

// Consumer-side BatchNorm finalize, the block `if (p.pin_stats)` of conv_fast_kernel as a function of the argument struct
// (any struct with FastArgs's pin_* / pend_* fields) and the workgroup size: the NT threads build the (scale, shift) table
// of the workgroup's statistics group `grp` in LDS, arithmetic of bn_finalize_kernel; the one `writer` workgroup of the
// launch also writes the backward-pass vectors of every group, updates the running statistics and folds the pending
// replicas into the slab statistics.  The caller's barrier publishes the table.
// conv_fast_kernel keeps its own inline copy: calling this function from it changed the code of every register-staging
// instantiation (tools/kernel_identity.py), and the 8x32x64 form sits at the two-workgroups-per-CU register edge.
template <int NT, typename Args>
__device__ __forceinline__ void pin_finalize(const Args& p, int grp, int tid, bool writer, float* ptab_sc, float* ptab_sh) {
  const int G = p.pin_groups;
  auto sums_of = [&](int g, int c, double& a1, double& a2) {   // sum and sum of squares of channel c in group g
    a1 = 0.; a2 = 0.;
    const int cp = c - p.pend_c0;
    if (cp >= 0 && cp < p.pend_n) {
      for (int r = 0; r < p.pend_nrep; ++r) {
        const double* Sr = p.pend_stats + (long)r * G * 2 * p.pend_ld;
        a1 += Sr[((long)g * 2 + 0) * p.pend_ld + cp];
        a2 += Sr[((long)g * 2 + 1) * p.pend_ld + cp];
      }
    } else {
      for (int r = 0; r < p.pin_nrep; ++r) {
        const double* Sr = p.pin_stats + (long)r * G * 2 * p.pin_ld;
        a1 += Sr[((long)g * 2 + 0) * p.pin_ld + c];
        a2 += Sr[((long)g * 2 + 1) * p.pin_ld + c];
      }
    }
  };
  for (int c = tid; c < p.Cin; c += NT) {
    double a1, a2;
    sums_of(grp, c, a1, a2);
    const double mu = a1 / p.pin_count;
    double var = a2 / p.pin_count - mu * mu;
    if (var < 0.) var = 0.;
    const float inv = (float)(1.0 / sqrt(var + (double)p.pin_eps));
    const float scv = (p.pin_gamma ? p.pin_gamma[c] : 1.f) * inv;
    ptab_sc[c] = scv;
    ptab_sh[c] = (float)((double)(p.pin_beta ? p.pin_beta[c] : 0.f) - mu * (double)scv);
  }
  if (writer) {   // backward-pass vectors, running statistics, fold
    for (int c = tid; c < p.Cin; c += NT) {
      const float gm = p.pin_gamma ? p.pin_gamma[c] : 1.f, bt = p.pin_beta ? p.pin_beta[c] : 0.f;
      float rm = p.pin_rmean ? p.pin_rmean[c] : 0.f, rv = p.pin_rvar ? p.pin_rvar[c] : 0.f;
      const bool pend = c >= p.pend_c0 && c < p.pend_c0 + p.pend_n;
      for (int g = 0; g < G; ++g) {
        double a1, a2;
        sums_of(g, c, a1, a2);
        if (pend) {   // nobody reads these slab entries during this launch (every workgroup takes them from the replicas)
          p.pin_fold[((long)g * 2 + 0) * p.pin_ld + c] = a1;
          p.pin_fold[((long)g * 2 + 1) * p.pin_ld + c] = a2;
        }
        const double mu = a1 / p.pin_count;
        double var = a2 / p.pin_count - mu * mu;
        if (var < 0.) var = 0.;
        const float inv = (float)(1.0 / sqrt(var + (double)p.pin_eps));
        const float scv = gm * inv;
        p.pin_scale[g * p.Cin + c] = scv;
        p.pin_shift[g * p.Cin + c] = (float)((double)bt - mu * (double)scv);
        p.pin_mean[g * p.Cin + c] = (float)mu;
        p.pin_invstd[g * p.Cin + c] = inv;
        const double unb = p.pin_count > 1. ? var * p.pin_count / (p.pin_count - 1.) : var;
        rm = (1.f - p.pin_momentum) * rm + p.pin_momentum * (float)mu;
        rv = (1.f - p.pin_momentum) * rv + p.pin_momentum * (float)unb;
      }
      if (p.pin_rmean) { p.pin_rmean[c] = rm; p.pin_rvar[c] = rv; }
    }
  }
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// KB: k-steps per wave, ceil(Cin / 32 / 8).  Up to three of them fit 128 registers (two workgroups per CU) when the
// scheduler is held to that; four take ~150 (one workgroup per CU).
template <int KB, bool RELU>
__global__ __launch_bounds__(512, KB <= 3 ? 4 : 2) void conv_point_kernel(const PointArgs p) {
  constexpr int NW = kPointWaves, BN = kPointBN, NT_CO = BN / 16, NT_PIX = kPointPix / 16;
  static_assert(NT_CO * NT_PIX == NW, "one 16 x 16 output tile per wave in the reduction");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f32x4* const part = reinterpret_cast<f32x4*>(smem);                      // [working wave][tile][lane]
  float* const ptab_sc = reinterpret_cast<float*>(smem + p.tab_off);
  float* const ptab_sh = ptab_sc + p.tab_cs;
  float* const red = ptab_sh + p.tab_cs;                                   // [NT_PIX][2][BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z;
  const int grp = b < p.bpg ? 0 : b / p.bpg;
  const int pix0 = blockIdx.x * kPointPix, n0 = blockIdx.y * BN;
  const int nk = (p.Cin + 31) >> 5;            // 32-channel k-steps
  const int nwv = min(nk, NW);                 // waves with work
  const bf16_t* const xb = (const bf16_t*)p.x + (long)b * p.HW * p.ldx;
  const bf16_t* const wpk = (const bf16_t*)p.wp;

  // ---- every load of the wave, before anything waits ----
  u32x4 xf[KB][NT_PIX], wf[KB][NT_CO];
  bool pok[NT_PIX];
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni) pok[ni] = pix0 + ni * 16 + l15 < p.HW;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const int ks = wave + j * NW;
    // uniform.  A k-step past the end loads nothing: the launch is bound by the load requests a CU can keep in flight
    // (measured: a repeated load of a valid k-step in its place costs what a real one costs)
    if (ks < nk) {
      const int ch = ks * 32 + 8 * lg;
      const bool cok = ch < p.Cin;
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) {
        const bf16_t* src = (cok && pok[ni]) ? xb + (pix0 + ni * 16 + l15) * p.ldx + ch : (const bf16_t*)sdhip_zero16;
        xf[j][ni] = *reinterpret_cast<const u32x4*>(src);
      }
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi)   // packed weights [Cin / 64][Mpad][64], zero past Cin
        wf[j][mi] = *reinterpret_cast<const u32x4*>(wpk + ((long)(ks >> 1) * p.Mpad + n0 + mi * 16 + l15) * 64 + (ks & 1) * 32 + 8 * lg);
    }
  }

  // ---- the coefficient table of this workgroup's statistics group; its entries [Cin, tab_cs) are zero, so that a lane
  //      past Cin (x not loaded: zero) comes out of the prologue as zero ----
  if (p.pin_stats) {   // uniform
    pin_finalize<NW * 64>(p, grp, tid, blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0, ptab_sc, ptab_sh);
  } else {
    for (int c = tid * 4; c < p.Cin; c += NW * 64 * 4) {   // Cin % 8 == 0: whole vectors, nothing past the Cin entries of the row
      *reinterpret_cast<f32x4*>(ptab_sc + c) = *reinterpret_cast<const f32x4*>(p.in_scale + (long)grp * p.Cin + c);
      *reinterpret_cast<f32x4*>(ptab_sh + c) = *reinterpret_cast<const f32x4*>(p.in_shift + (long)grp * p.Cin + c);
    }
  }
  if (p.Cin + tid < p.tab_cs) { ptab_sc[p.Cin + tid] = 0.f; ptab_sh[p.Cin + tid] = 0.f; }   // tab_cs - Cin < 64
  __syncthreads();

  // ---- prologue in registers, MFMAs, partial tile to LDS ----
  // One dword of a fragment = two channels: (lo, hi) -> one packed fma with the table's (even, odd) entries, two max, one
  // packed conversion.  RELU is a template argument and "this tile ends inside the image" is decided once per workgroup.
  const bool ragged = pix0 + kPointPix > p.HW;
  if (wave < nwv) {
    f32x4 acc[NT_CO][NT_PIX];
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const int ks = wave + j * NW;
      if (ks < nk) {   // uniform
        const int ch = ks * 32 + 8 * lg;   // < tab_cs
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(ptab_sc + ch), sc1 = *reinterpret_cast<const f32x4*>(ptab_sc + ch + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4*>(ptab_sh + ch), sh1 = *reinterpret_cast<const f32x4*>(ptab_sh + ch + 4);
        const f32x2 sc2[4] = {f32x2{sc0[0], sc0[1]}, f32x2{sc0[2], sc0[3]}, f32x2{sc1[0], sc1[1]}, f32x2{sc1[2], sc1[3]}};
        const f32x2 sh2[4] = {f32x2{sh0[0], sh0[1]}, f32x2{sh0[2], sh0[3]}, f32x2{sh1[0], sh1[1]}, f32x2{sh1[2], sh1[3]}};
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni) {
          const u32x4 raw = xf[j][ni];
          u32x4 bfrag;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            f32x2 z = __builtin_elementwise_fma(f32x2{bflo(raw[i]), bfhi(raw[i])}, sc2[i], sh2[i]);
            if constexpr (RELU) z = f32x2{fmaxf(z[0], 0.f), fmaxf(z[1], 0.f)};
            bfrag[i] = __builtin_bit_cast(unsigned int, __builtin_convertvector(z, bf16x2_t));   // RNE, one v_cvt_pk_bf16_f32
          }
          if (ragged && !pok[ni]) bfrag = u32x4{0u, 0u, 0u, 0u};   // a pixel row past the image: zero AFTER the prologue
#pragma unroll
          for (int mi = 0; mi < NT_CO; ++mi) Mma<bf16_t>::run(acc[mi][ni], wf[j][mi], bfrag);
          __builtin_amdgcn_sched_barrier(0);   // fragment by fragment: hoisting all prologues above the MFMAs costs 40 registers
        }
      }
    }
#pragma unroll
    for (int ni = 0; ni < NT_PIX; ++ni)
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi) part[(wave * NW + ni * NT_CO + mi) * 64 + lane] = acc[mi][ni];
  }
  __syncthreads();

  // ---- reduction in wave order: this wave owns tile (ni, mi) = (wave / NT_CO, wave % NT_CO), MFMA result layout ----
  const int ni = wave / NT_CO, mi = wave % NT_CO;
  f32x4 v = part[wave * 64 + lane];
  for (int w = 1; w < nwv; ++w) v += part[(w * NW + wave) * 64 + lane];

  // ---- epilogue: round, store, statistics of the stored values ----
  const int pix = pix0 + ni * 16 + l15;
  const bool valid = pix < p.HW;
  const int co = n0 + mi * 16 + 4 * lg;   // Cout % BN == 0: always a whole group of four inside Cout
  const u32x2 o = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
  if (valid) *reinterpret_cast<u32x2*>((bf16_t*)p.y + ((long)b * p.HW + pix) * p.ldy + co) = o;
  if (p.stats) {   // uniform
    const f32x4 sv = valid ? f32x4{bflo(o[0]), bfhi(o[0]), bflo(o[1]), bfhi(o[1])} : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = row16_sum(sv[r]), c2 = row16_sum(sv[r] * sv[r]);   // over the 16 pixels of the tile (DPP)
      if (l15 == 0) {
        const int m = mi * 16 + 4 * lg + r;
        red[(ni * 2 + 0) * BN + m] = a;
        red[(ni * 2 + 1) * BN + m] = c2;
      }
    }
    __syncthreads();
    if (tid < 2 * BN) {
      const int which = tid / BN, m = tid - which * BN;
      const float tot = red[(0 * 2 + which) * BN + m] + red[(1 * 2 + which) * BN + m] + red[(2 * 2 + which) * BN + m] + red[(3 * 2 + which) * BN + m];
      const long rep = (blockIdx.x + blockIdx.z) % p.nrep;
      atomicAdd(p.stats + rep * p.rep_stride + ((long)grp * 2 + which) * p.stats_ld + n0 + m, (double)tot);
    }
  }
}

template <int KB, bool RELU>
int launch_point_kb(const PointArgs& a, int B, size_t lds, hipStream_t s) {
  auto kern = conv_point_kernel<KB, RELU>;
  static bool attr_set = false;  // per instantiation
  if (lds > 64 * 1024 && !attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_point: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  dim3 grid(sdhip_cdiv(a.HW, kPointPix), a.Cout / kPointBN, B);
  hipLaunchKernelGGL(kern, grid, dim3(kPointWaves * 64), lds, s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

// fills the LDS layout of `a` from its Cin
int launch_point(PointArgs& a, int B, hipStream_t s) {
  const int nk = sdhip_cdiv(a.Cin, 32);
  const int kb = sdhip_cdiv(nk, kPointWaves);
  a.tab_off = (nk < kPointWaves ? nk : kPointWaves) * kPointWaves * 64 * (int)sizeof(f32x4);
  a.tab_cs = (a.Cin + 63) & ~63;
  const size_t lds = (size_t)a.tab_off + 2 * (size_t)a.tab_cs * sizeof(float) + kPointPix / 16 * 2 * kPointBN * sizeof(float);
  return sdhip_by_flag(a.in_relu != 0, [&](auto R) {
    switch (kb) {
      case 1: return launch_point_kb<1, R()>(a, B, lds, s);
      case 2: return launch_point_kb<2, R()>(a, B, lds, s);
      case 3: return launch_point_kb<3, R()>(a, B, lds, s);
      default: return launch_point_kb<4, R()>(a, B, lds, s);
    }
  });
}

}  // namespace
