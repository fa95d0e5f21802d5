// 3x3 (stride 1, dilation 1, pad 1) convolution with an input prologue into 32 output channels on small maps, bf16, for
// gfx950: the conv2 ("growth" convolution, 128 -> 32 with norm2 + ReLU on load) of the DenseNet dense layers.
//
// conv_fast.h cannot stage these layers by LDS-DMA (the prologue has to touch every element), so it walks a chain of
// dependent global round trips: the finalize table, the halo through registers (needs the table), then one stage per
// (64-channel chunk, tap group), each a barrier with a weight round trip behind it.  Here, as in conv_point.h, the number
// of barriers and of dependent round trips per workgroup depends neither on Cin nor on the taps:
//   - a workgroup owns a 4 x 16 pixel tile of one image x all 32 output channels; 8 waves (512 threads);
//   - the reduction, 9 taps x NK = Cin / 32 k-steps, is split over the waves: wave w takes the (tap, k-step) units
//     w, w + 8, ... (at most KB = ceil(9 NK / 8)) and forms the whole 64 x 32 partial tile over them;
//   - EVERY global load is issued before anything waits: the raw 6 x 18 halo pixels (16 bytes per lane and load, a lane of a
//     padding pixel loads nothing), the wave's weight fragments (16 bytes per lane straight from the 'fwd' packing
//     [Cin / 64][9][32][64]) and the statistics / coefficient rows of the table.  None depends on the table;
//   - barrier 1 publishes the table (pin_finalize of conv_point.h, or a copy of the given rows of the workgroup's group);
//     the prologue runs in registers and the halo goes to LDS once.  relu(shift) is not zero: a padding pixel is zeroed
//     AFTER the prologue;
//   - barrier 2; the MFMAs: pixel fragments from the LDS halo with the tap shift as a row offset, weights from registers.
//     Halo image: [64-channel chunk][pixel row = hy * 18 + hx][128 bytes] with conv_fast.h's chunk key (row & 6): a fragment
//     read touches 16 consecutive rows and is conflict-free for every tap shift;
//   - barrier 3 (the halo is dead), the partial tiles go to LDS over it, barrier 4, and wave t sums the 16 x 16 tile t of
//     all waves in wave order (no LDS atomics: the same inputs give the same y bits), rounds once, stores 8 bytes per lane;
//   - statistics of the STORED values as in conv_point.h: row16_sum, the four pixel tiles through LDS in f32, one f64
//     atomic per value into replica (blockIdx.x + blockIdx.z) % nrep.
// LDS: 64 KiB of partial tiles (over the halo, <= 54 KiB) + the table (8 Cin bytes) + 1 KiB: two workgroups per CU.
#pragma once
#include "conv_point.h"

namespace {

struct GrowArgs {
  const void* x; const void* wp; void* y;
  const float* in_scale; const float* in_shift; double* stats;
  int H, W, Cin, ldx, ldy, tiles_w;
  int in_relu, bpg;                    // bpg: images per statistics group
  int stats_ld, nrep; long rep_stride;
  // consumer-side BatchNorm finalize: the fields of FastArgs under the same names (pin_finalize reads them)
  const double* pin_stats; int pin_ld, pin_nrep, pin_groups;
  const float* pin_gamma; const float* pin_beta;
  float* pin_scale; float* pin_shift; float* pin_mean; float* pin_invstd; float* pin_rmean; float* pin_rvar;
  float pin_eps, pin_momentum; double pin_count;
  const double* pend_stats; double* pin_fold; int pend_ld, pend_nrep, pend_c0, pend_n;
};

constexpr int kGrowWaves = 8, kGrowBN = 32, kGrowTH = 4, kGrowTW = 16;
constexpr int kGrowIW = kGrowTW + 2, kGrowHalo = (kGrowTH + 2) * kGrowIW;   // halo pixels of a tile
constexpr int kGrowPartBytes = kGrowWaves * kGrowTH * kGrowTW * kGrowBN * 4;   // the partial tiles: 64 KiB
constexpr int kGrowMaxWG = 512;    // the dispatch's upper limit on the grid: two workgroups on each of 256 CUs, resident at once
constexpr int kGrowMaxMap = 2048;  // ... and on the pixels of one image: the largest map measured faster (32x64; 64x128 is not)

template <int NK, bool RELU>
__global__ __launch_bounds__(512, NK <= 4 ? 4 : 2) void conv_grow_kernel(const GrowArgs p) {
  constexpr int NW = kGrowWaves, NT = NW * 64, BN = kGrowBN, NT_CO = BN / 16, NT_PIX = kGrowTH;
  constexpr int CIN = 32 * NK, U = 9 * NK, KB = (U + NW - 1) / NW;   // units (tap, k-step); per wave at most KB
  constexpr int CPP = 4 * NK, NCH = kGrowHalo * CPP, HL = (NCH + NT - 1) / NT;   // 16-byte pieces per pixel, per halo, per lane
  constexpr int QB = kGrowHalo * 128;   // bytes of one 64-channel chunk of the halo image
  static_assert(NT_CO * NT_PIX == NW, "one 16 x 16 output tile per wave in the reduction");
  static_assert(U >= NW && ((NK + 1) / 2) * QB <= kGrowPartBytes, "every wave works; the halo fits under the partial tiles");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f32x4* const part = reinterpret_cast<f32x4*>(smem);                      // [wave][tile][lane], over the halo image
  float* const ptab_sc = reinterpret_cast<float*>(smem + kGrowPartBytes);
  float* const ptab_sh = ptab_sc + CIN;
  float* const red = ptab_sh + CIN;                                        // [NT_PIX][2][BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z;
  const int grp = b < p.bpg ? 0 : b / p.bpg;
  const int ty = blockIdx.x / p.tiles_w;
  const int oh0 = ty * kGrowTH, ow0 = (blockIdx.x - ty * p.tiles_w) * kGrowTW;
  const bf16_t* const xb = (const bf16_t*)p.x + (long)b * p.H * p.W * p.ldx;
  const bf16_t* const wpk = (const bf16_t*)p.wp;

  // ---- every load of the wave, before anything waits ----
  // halo: piece i = tid + j * NT is channels [8 cc, + 8) of halo pixel hp, i = hp * CPP + cc (a pixel's pieces on
  // neighbouring lanes).  Padding pixels (outside the image) and pieces past the halo load nothing.
  u32x4 hx[HL];
  bool hin[HL];
#pragma unroll
  for (int j = 0; j < HL; ++j) {
    const int i = tid + j * NT;
    const int hp = i / CPP, cc = i - hp * CPP;
    const int hy = hp / kGrowIW, hw = hp - hy * kGrowIW;
    const int gh = oh0 - 1 + hy, gw = ow0 - 1 + hw;
    hin[j] = i < NCH && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W;
    hx[j] = u32x4{0u, 0u, 0u, 0u};
    if (hin[j]) hx[j] = *reinterpret_cast<const u32x4*>(xb + (gh * p.W + gw) * p.ldx + cc * 8);
  }
  // weights: unit u = t * NK + ks; packed [Cin / 64][9][32][64], lane (l15, lg) holds channels [8 lg, + 8) of the k-step
  u32x4 wf[KB][NT_CO];
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const int u = wave + j * NW;
    if (u < U) {   // uniform
      const int t = u / NK, ks = u - t * NK;
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi)
        wf[j][mi] = *reinterpret_cast<const u32x4*>(wpk + (((ks >> 1) * 9 + t) * BN + mi * 16 + l15) * 64 + (ks & 1) * 32 + 8 * lg);
    }
  }

  // ---- the coefficient table of this workgroup's statistics group ----
  if (p.pin_stats) {   // uniform
    pin_finalize<NT>(p, grp, tid, blockIdx.x == 0 && blockIdx.z == 0, ptab_sc, ptab_sh);
  } else {
    for (int c = tid * 4; c < CIN; c += NT * 4) {
      *reinterpret_cast<f32x4*>(ptab_sc + c) = *reinterpret_cast<const f32x4*>(p.in_scale + (long)grp * CIN + c);
      *reinterpret_cast<f32x4*>(ptab_sh + c) = *reinterpret_cast<const f32x4*>(p.in_shift + (long)grp * CIN + c);
    }
  }
  __syncthreads();

  // ---- prologue in registers, the halo to LDS once.  One dword = two channels: one packed fma with the table's (even,
  //      odd) entries, two max, one packed conversion; a padding pixel is zero AFTER it ----
#pragma unroll
  for (int j = 0; j < HL; ++j) {
    const int i = tid + j * NT;
    if (i < NCH) {
      const int hp = i / CPP, cc = i - hp * CPP;
      const int ch = cc * 8;
      const f32x4 sc0 = *reinterpret_cast<const f32x4*>(ptab_sc + ch), sc1 = *reinterpret_cast<const f32x4*>(ptab_sc + ch + 4);
      const f32x4 sh0 = *reinterpret_cast<const f32x4*>(ptab_sh + ch), sh1 = *reinterpret_cast<const f32x4*>(ptab_sh + ch + 4);
      const f32x2 sc2[4] = {f32x2{sc0[0], sc0[1]}, f32x2{sc0[2], sc0[3]}, f32x2{sc1[0], sc1[1]}, f32x2{sc1[2], sc1[3]}};
      const f32x2 sh2[4] = {f32x2{sh0[0], sh0[1]}, f32x2{sh0[2], sh0[3]}, f32x2{sh1[0], sh1[1]}, f32x2{sh1[2], sh1[3]}};
      const u32x4 raw = hx[j];
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f32x2 z = __builtin_elementwise_fma(f32x2{bflo(raw[e]), bfhi(raw[e])}, sc2[e], sh2[e]);
        if constexpr (RELU) z = f32x2{fmaxf(z[0], 0.f), fmaxf(z[1], 0.f)};
        o[e] = __builtin_bit_cast(unsigned int, __builtin_convertvector(z, bf16x2_t));   // RNE, one v_cvt_pk_bf16_f32
      }
      if (!hin[j]) o = u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(smem + (cc >> 3) * QB + LdsRow<2>::off(hp, cc & 7)) = o;
    }
  }
  __syncthreads();

  // ---- MFMAs: pixel tile ni is tile row ni; tap (ky, kx) shifts its 16 halo rows by ky * 18 + kx ----
  f32x4 acc[NT_CO][NT_PIX];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT_PIX; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const int u = wave + j * NW;
    if (u < U) {   // uniform
      const int t = u / NK, ks = u - t * NK;
      const int ky = t / 3, kx = t - ky * 3;
      const unsigned char* const hq = smem + (ks >> 1) * QB;
      const int row0 = ky * kGrowIW + kx + l15, c = (ks & 1) * 4 + lg;
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) {
        const u32x4 bfrag = *reinterpret_cast<const u32x4*>(hq + LdsRow<2>::off(row0 + ni * kGrowIW, c));
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi) Mma<bf16_t>::run(acc[mi][ni], wf[j][mi], bfrag);
      }
    }
  }
  __syncthreads();   // every wave is done with the halo: the partial tiles go over it
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni)
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) part[(wave * NW + ni * NT_CO + mi) * 64 + lane] = acc[mi][ni];
  __syncthreads();

  // ---- reduction in wave order: this wave owns tile (ni, mi) = (wave / NT_CO, wave % NT_CO), MFMA result layout ----
  const int ni = wave / NT_CO, mi = wave % NT_CO;
  f32x4 v = part[wave * 64 + lane];
#pragma unroll
  for (int w = 1; w < NW; ++w) v += part[(w * NW + wave) * 64 + lane];

  // ---- epilogue: round, store, statistics of the stored values ----
  const int oh = oh0 + ni, ow = ow0 + l15;
  const bool valid = oh < p.H && ow < p.W;
  const int co = mi * 16 + 4 * lg;
  const u32x2 o = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
  if (valid) *reinterpret_cast<u32x2*>((bf16_t*)p.y + (((long)b * p.H + oh) * p.W + ow) * p.ldy + co) = o;
  if (p.stats) {   // uniform
    const f32x4 sv = valid ? f32x4{bflo(o[0]), bfhi(o[0]), bflo(o[1]), bfhi(o[1])} : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = row16_sum(sv[r]), c2 = row16_sum(sv[r] * sv[r]);   // over the 16 pixels of the tile row (DPP)
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
      atomicAdd(p.stats + rep * p.rep_stride + ((long)grp * 2 + which) * p.stats_ld + m, (double)tot);
    }
  }
}

constexpr size_t kGrowLds(int Cin) { return (size_t)kGrowPartBytes + 2 * (size_t)Cin * sizeof(float) + kGrowTH * 2 * kGrowBN * sizeof(float); }

template <int NK, bool RELU>
int launch_grow_nk(const GrowArgs& a, int B, hipStream_t s) {
  auto kern = conv_grow_kernel<NK, RELU>;
  static bool attr_set = false;  // per instantiation
  if (!attr_set) {   // always above 64 KiB
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_grow: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  dim3 grid(a.tiles_w * sdhip_cdiv(a.H, kGrowTH), 1, B);
  hipLaunchKernelGGL(kern, grid, dim3(kGrowWaves * 64), kGrowLds(32 * NK), s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

// Cin = 32 NK, 2 <= NK <= 8
int launch_grow(const GrowArgs& a, int B, hipStream_t s) {
  return sdhip_by_flag(a.in_relu != 0, [&](auto R) {
    switch (a.Cin / 32) {
      case 2: return launch_grow_nk<2, R()>(a, B, s);
      case 3: return launch_grow_nk<3, R()>(a, B, s);
      case 4: return launch_grow_nk<4, R()>(a, B, s);
      case 5: return launch_grow_nk<5, R()>(a, B, s);
      case 6: return launch_grow_nk<6, R()>(a, B, s);
      case 7: return launch_grow_nk<7, R()>(a, B, s);
      default: return launch_grow_nk<8, R()>(a, B, s);
    }
  });
}

}  // namespace
