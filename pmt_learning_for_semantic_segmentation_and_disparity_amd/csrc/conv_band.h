// Persistent K x K convolution for the full-resolution 5x5 layers (Conv2DownUp, models/dsnet_t2.py:80-117 of the reference;
// the ten launches that lead the training step's profile) and the 3x3 layers with <= 32 input channels: bf16, stride 1, no
// dilation, <= 64 input and output channels.
//
// What the tap-group pipeline of conv_fast.h cannot do inside its 80 KiB (two workgroups per CU): keep more than one tap
// of 64x64 weights per stage next to a 64-channel halo tile — 25 stages of 32 MFMAs per wave, a barrier and a DMA drain
// between each.  This kernel owns the whole CU instead (one 512-thread workgroup, ~144 KiB of LDS) and is persistent:
//
//   tile    16 x 32 output pixels x all output channels; wave w computes pixel rows 2w, 2w+1 (4 MFMA pixel tiles) times
//           BN output channels, exactly the register tile of conv_fast.h
//   chunk   (tile, 32-channel half of the input): its halo image, (16+K-1) x 40 rows of 64 bytes, is 50 KiB, so TWO fit:
//           the halo of chunk c+1 streams in by LDS-DMA, a couple of rounds per stage, while chunk c is computed
//   stage   one kernel ROW of a chunk: K taps x BN rows of 64 bytes of weights (20 KiB), double-buffered; K * 4 * BN/16
//           MFMAs per wave between two barriers (80 for 5x5 / 64 channels, against 32).  3x3: the whole kernel is one stage and
//           its nine taps of weights stay resident (BandCfg::WRES), so the stage loop issues halo DMA only
//
// Every fragment address is  buffer + wave row + compile-time constant + one of K per-lane registers:  with the halo
// row pitch (40) and the 16-pixel column step multiples of 8 rows, the swizzle key of a pixel depends on
// (kw + lane) only, so the inner loop carries no address arithmetic at all.
//
// LDS-DMA bookkeeping (the DMA is inline asm, invisible to the compiler's wait-count pass): the weights of the next
// stage are issued first after a barrier, the halo rounds of the next chunk after them; `s_waitcnt vmcnt(n)` with
// n = the halo instructions issued since then waits for exactly the weights; at a tile boundary n = the epilogue's
// stores (vmcnt retires loads, stores and LDS-DMA together, in issue order).
//
// conv_band_bx_kernel is the same kernel with the BatchNorm-backward sums of sdhip_conv2d_fwd_bnbwd (mode 0) in its epilogue
// (BandBxArgs); both kernels compile the one body of conv_band_body.h.
#pragma once
#include <type_traits>
#include "conv_fast.h"

namespace {

struct BandArgs {
  const void* x; const void* wp; void* y;
  const float* bias; double* stats;
  int B, H, W, Ho, Wo, pad_t, pad_l;
  int Cin, ldx, Cout, Mpad, ldy;
  int bpg, act, stats_ld, nrep;
  const void* res; int ldres;              // y = result + res (same geometry as y; res == y: accumulate in place); nullptr: off
  long rep_stride;
  int tiles_w, tiles_hw, ntiles, tpw;      // tiles per output row / per image / in total / per workgroup
  unsigned magic_hw, magic_tw;             // div_magic(tiles_hw), div_magic(tiles_w)
  int D, Do, pad_d;                        // volumes (KD = 3): input / output depth, front padding; B counts batch entries then
  unsigned magic_do;                       // div_magic(Do)
  int dbg;                                 // diagnostic bits (SDHIP_TUNE_BAND_DBG): 1 no halo prefetch, 2 no weight DMA, 4 no MFMA, 8 no stores
};
// The BatchNorm-backward-sums launches (VAR & 8, sdhip_conv2d_fwd_bnbwd mode 0; the semantics of FastArgs::bx): u = bx has the
// geometry of y and pixel stride ldbx, z = fmaf(u, bsc[group][c], bsh[group][c]), gm = the STORED y where z > 0 else 0, and the
// statistics slots receive sum(gm * u) and sum(gm) instead of sum(y), sum(y^2).  A kernel of their own with arguments of their
// own: the plain launches keep their kernarg block, and with it their code, to the byte.
struct BandBxArgs : BandArgs {
  const void* bx; const float* bsc; const float* bsh; int ldbx;
};

template <int I, int N, typename F> __device__ __forceinline__ void band_static_for(F&& f) {   // f(integral_constant<I>) ... <N-1>
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); band_static_for<I + 1, N>(f); }
}
template <int N> __device__ __forceinline__ void band_wait() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }

template <int K, int BN, int NW = 8, int KD = 1>
struct BandCfg {
  static constexpr int RPR = NW * 16;                    // LDS rows (64 bytes) one DMA round of the workgroup fills
  static constexpr int RPW = 16 / NW;                    // output pixel rows per wave
  static constexpr int TH = 16, TW = 32;
  static constexpr int IH = TH + K - 1, IW = TW + K - 1, IWp = (IW + 7) & ~7;
  static constexpr int HROWS = IH * IWp;                 // halo rows (64 bytes each) of one chunk
  static constexpr int HR = (HROWS + RPR - 1) / RPR;     // LDS-DMA rounds (NW x 64 lanes x 16 bytes = RPR rows) per halo image
  static constexpr int HB = HROWS * 64;
  // A stage = RS kernel rows.  5x5: one row per stage, the weights of the next stage double-buffered.  3x3 (<= 32 input
  // channels only): the whole kernel is ONE stage per chunk and its 9 taps of weights (<= 37 KB) stay RESIDENT — every
  // chunk of every tile uses the same ones — so the stage loop issues halo DMA only.
  static constexpr int RS = K == 3 ? 3 : 1;
  static constexpr int NSTG = K / RS;                    // stages per chunk
  static constexpr bool WRES = NSTG == 1 && KD == 1;     // weights resident (host: single channel half); KD = 3: every depth tap is a chunk with weights of its own, streamed like the 5x5 stages
  static constexpr int TPS = RS * K;                     // taps per stage
  static constexpr int WROWS = TPS * BN;
  static constexpr int WR = (WROWS + RPR - 1) / RPR;
  static constexpr int WB = WROWS * 64;
  static constexpr int NWB = WRES ? 1 : 2;               // weight buffers
  static constexpr int WRS = WRES ? 0 : WR;              // weight DMA slots per stage
  // halo rounds of the next chunk issued per stage: spread over stages 0 .. NSTG-2, or all in the only stage
  static constexpr int HPS = NSTG == 1 ? HR : (HR + NSTG - 2) / (NSTG - 1);
  static constexpr int RED = NW * 2 * BN * 4;            // statistics scratch: [NW waves][2][BN] floats
  static constexpr int SPT = (WRS + HPS + TPS - 1) / TPS;   // DMA slots per tap
  static constexpr size_t LDS = 2 * HB + NWB * WB + RED;
  static_assert(HROWS % 16 == 0 && WROWS % 16 == 0, "a wave's 16 rows of a DMA round are either all inside or all outside the image");
  static_assert(NSTG == 1 || HPS * (NSTG - 1) >= HR, "halo rounds must fit the stages of one chunk");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

// One LDS-DMA instruction through a buffer resource: lane address = base + soff + voff; a lane whose voff is not below
// the resource's num_records fetches zeros (padding, dead channels) — no zero page, no 64-bit address arithmetic.
typedef __attribute__((ext_vector_type(4))) int band_rsrc_t;
constexpr int kBandOob = 0x7fffff00;           // num_records of every resource and the voff of a padding lane
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void band_dma(int voff, band_rsrc_t rsrc, unsigned lds_wave_base, int soff) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
               : : "v"(voff), "s"(rsrc), "s"(lds_wave_base), "s"(soff) : "memory", "m0");
}
#pragma clang diagnostic pop
__device__ __forceinline__ band_rsrc_t band_rsrc(const void* base) {
  const unsigned long long a = (unsigned long long)base;
  band_rsrc_t r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
  r[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));   // stride 0: raw buffer
  r[2] = kBandOob;
  r[3] = 0x00020000;
  return r;
}

// (the body: conv_band_body.h, included once per argument block)
template <int K, int BN, int VAR, int NW, int KD = 1>
__global__ __launch_bounds__(NW * 64) void conv_band_kernel(const BandArgs p) {
#include "conv_band_body.h"
}

// VAR & 8: the BatchNorm-backward-sums form
template <int K, int BN, int VAR, int NW, int KD = 1>
__global__ __launch_bounds__(NW * 64) void conv_band_bx_kernel(const BandBxArgs p) {
  static_assert((VAR & 8) != 0 && KD == 1, "the BatchNorm-backward epilogue: 2-D form only");
#include "conv_band_body.h"
}

inline bool band_ok(int ntiles) { return ntiles >= 192 && ntiles < 65536; }
// the BatchNorm-backward-sums forms that exist: all but 5x5 with more than 32 output channels AND an addend (that kernel spills)
inline bool band_bx_form_ok(int k, int Mpad, bool addend) { return !(k == 5 && Mpad > 32 && addend); }

template <int K, int BN, int VAR, int NW = 8, int KD = 1>
int launch_band_bn(const BandArgs& a, int grid, hipStream_t s) {
  auto kern = conv_band_kernel<K, BN, VAR, NW, KD>;
  static bool attr_set = false;   // per instantiation
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_band: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  const size_t lds = BandCfg<K, BN, NW, KD>::LDS;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

template <int K, int BN, int VAR, int NW = 8>
int launch_band_bx_bn(const BandBxArgs& a, int grid, hipStream_t s) {
  auto kern = conv_band_bx_kernel<K, BN, VAR, NW>;
  static bool attr_set = false;   // per instantiation
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_band: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  constexpr size_t lds = BandCfg<K, BN, NW, 1>::LDS + 2 * BN * sizeof(float);   // + scale / shift of the current group
  static_assert(lds <= 160 * 1024, "LDS budget of the BatchNorm-backward form");
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

// tiles, their division constants and tiles per workgroup; returns the grid
template <int KD>
int band_tiling(BandArgs& a) {
  const int tiles_h = sdhip_cdiv(a.Ho, 16);
  a.tiles_w = sdhip_cdiv(a.Wo, 32);
  a.tiles_hw = tiles_h * a.tiles_w;
  a.ntiles = a.tiles_hw * a.B * (KD > 1 ? a.Do : 1);
  a.magic_do = (KD > 1 && a.Do > 1) ? (unsigned)(0x100000000ULL / (unsigned)a.Do) + 1u : 0u;
  a.magic_hw = a.tiles_hw > 1 ? (unsigned)(0x100000000ULL / (unsigned)a.tiles_hw) + 1u : 0u;
  a.magic_tw = a.tiles_w > 1 ? (unsigned)(0x100000000ULL / (unsigned)a.tiles_w) + 1u : 0u;
  a.tpw = sdhip_cdiv(a.ntiles, 256);
  return sdhip_cdiv(a.ntiles, a.tpw);
}

template <int K, int KD = 1>
int launch_band(BandArgs& a, hipStream_t s) {
  const int grid = band_tiling<KD>(a);
  a.dbg = sdhip_diag().tune_band_dbg;
  // VAR 5 = DMA slot ahead of the fragment reads + one read per two MFMAs (sched_group_barrier): 207 -> 201 us against the
  // other orders; 4 waves (one per SIMD, 64 x 128 register tiles) measured 265 us — the partner wave's cover is worth more
  // than the quarter of LDS reads saved.  VAR 128: diagnostic build that honours SDHIP_TUNE_BAND_DBG.
  a.dbg &= 0xff;
  if constexpr (K == 5) {
    if (a.Mpad > 32) return a.dbg ? launch_band_bn<K, 64, 128 + 5>(a, grid, s) : launch_band_bn<K, 64, 5>(a, grid, s);
  } else if constexpr (KD > 1) {
    return launch_band_bn<K, 32, 5, 8, KD>(a, grid, s);      // (host: <= 32 channels on both sides)
  } else {
    if (a.Mpad > 32) return launch_band_bn<K, 64, 5>(a, grid, s);
  }
  return launch_band_bn<K, 32, 5>(a, grid, s);
}

// the BatchNorm-backward-sums form (2-D): the same variant of the stage loop, the epilogue of BandBxArgs
template <int K>
int launch_band_bx(BandBxArgs& a, hipStream_t s) {
  const int grid = band_tiling<1>(a);
  a.dbg = 0;
  // VAR & 16: with an addend — a flag, so that the epilogue carries no branch per store.  (5x5, 64 output channels, addend:
  // not built — host, band_bx_form_ok: it is the one form that spills, 2 registers)
  if (!band_bx_form_ok(K, a.Mpad, a.res != nullptr))
    SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv_band: the BatchNorm-backward form with an addend is not built for %dx%d with more than 32 output channels", K, K);
  SDHIP_CHOSE(kFwdBand, K, 1, 1);
  if constexpr (K == 5) {
    if (a.Mpad > 32) return launch_band_bx_bn<K, 64, 5 + 8>(a, grid, s);
  } else {
    if (a.Mpad > 32) return a.res ? launch_band_bx_bn<K, 64, 5 + 8 + 16>(a, grid, s) : launch_band_bx_bn<K, 64, 5 + 8>(a, grid, s);
  }
  return a.res ? launch_band_bx_bn<K, 32, 5 + 8 + 16>(a, grid, s) : launch_band_bx_bn<K, 32, 5 + 8>(a, grid, s);
}

}  // namespace
