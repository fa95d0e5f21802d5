// 3x3 (stride 1, dilation 1, pad 1) convolution 64 -> 64 on mid-size maps, bf16, for gfx950: the decoder blocks on the
// 1/4-resolution maps (Conv2DownUp6 / 7 / 9 / 10), forward and data gradient.
//
// conv_fast.h gives these layers its 4 x 16 tile: every workgroup streams the whole 9 x 64 x 64 weight set (73.7 KB) for 64
// output pixels, and the launch is bound by what a CU's load path sustains.  Here a CU loads the weights ONCE:
//   - a workgroup owns an 8 x 32 pixel tile of one image x all 64 output channels; 8 waves (512 threads); wave w owns tile
//     row w: two 16-pixel MFMA tiles x four output-channel tiles, 32 accumulator registers;
//   - everything goes global -> LDS by LDS-DMA in conv_fast.h's image format (128-byte rows, chunk slot c ^ (row & 6), halo
//     row pitch 40, zero source for padding), so its conflict-free fragment reads carry over: the 10 x 40 halo rows (7 load
//     rounds of 64 rows) and the nine taps of the unchanged 'fwd' / 'dgrad' packing [1][9][64][64] (one round per tap);
//   - ALL of it is issued at kernel start, halo first, then the weights in tap order, behind the epilogue's operand loads (BX
//     launches: u, the addend, scale / shift — plain loads into registers).  The DMA retires in issue order, so the waits
//     are counted: vmcnt(6) + barrier publishes the halo and kernel row 0, which multiplies while rows 1 and 2 arrive;
//     vmcnt(3) + barrier, vmcnt(0) + barrier.  No plain load stands between the DMA issue and the last MFMA;
//   - the reduction order per output element is conv_fast.h's (tap-major, then the two 32-channel k-steps of the 128-byte
//     row) with the same MFMA instruction: the y bits are those of the halo-tile kernel;
//   - epilogues as in conv_fast.h (D[cout][pixel], 4 channels per lane, 8-byte stores): plain; statistics of the stored
//     values (row16_sum, the 8 waves through LDS, one f64 atomic per channel into replica (blockIdx.x + blockIdx.z) % nrep);
//     BatchNorm-backward sums of sdhip_conv2d_fwd_bnbwd mode 0 with the optional addend.
// LDS: 56 KiB halo + 72 KiB weights = 128 KiB: one workgroup per CU.
#pragma once
#include "conv_fast.h"

namespace {

struct MidArgs {
  const void* x; const void* wp; void* y; double* stats;
  int H, W, ldx, ldy, tiles_w;
  int bpg;                              // images per statistics group
  int stats_ld, nrep; long rep_stride;
  // BX launches (FastArgs::bx, bx_mode 0): u = bx, z = u * bsc + bsh; res: y = result + res (or nullptr)
  const void* bx; const float* bsc; const float* bsh; int ldbx;
  const void* res; int ldres;
};

constexpr int kMidWaves = 8, kMidBN = 64, kMidTH = 8, kMidTW = 32;
constexpr int kMidIH = kMidTH + 2, kMidIWp = 40;                  // halo rows; halo row pitch: 34 pixels rounded up to 8
constexpr int kMidHaloRounds = (kMidIH * kMidIWp + 63) / 64;      // load rounds of 512 lanes x 16 bytes = 64 LDS rows
constexpr int kMidHaloBytes = kMidHaloRounds * 8192, kMidLds = kMidHaloBytes + 9 * 8192;
// the dispatch's limits: what was measured faster (tools/gpu_conv3x3_mid.py, 8 images)
constexpr int kMidMinMap = 8192, kMidMaxMap = 8192;   // pixels of one image: 64 x 128
constexpr int kMidMaxWG = 256;                        // one workgroup on each of 256 CUs, resident at once

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// the DMA retires in issue order: at most N of the wave's own are still in flight, then every wave's are visible
template <int N> __device__ __forceinline__ void mid_wait_publish() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" : : "n"(N) : "memory");
}
#pragma clang diagnostic pop

template <bool BX, bool RES>
__global__ __launch_bounds__(512) void conv_mid_kernel(const MidArgs p) {
  constexpr int BN = kMidBN, NT_CO = BN / 16, NT_PIX = kMidTW / 16, IWp = kMidIWp, RB = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned char* const halo = smem;
  const unsigned char* const wl = smem + kMidHaloBytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z;
  const int grp = b < p.bpg ? 0 : b / p.bpg;
  const int ty = blockIdx.x / p.tiles_w;
  const int oh0 = ty * kMidTH, ow0 = (blockIdx.x - ty * p.tiles_w) * kMidTW;
  const bf16_t* const xb = (const bf16_t*)p.x + (long)b * p.H * p.W * p.ldx;
  const bf16_t* const wpk = (const bf16_t*)p.wp;

  // this lane's output pixels: tile row `wave`, columns l15 and 16 + l15; its channels 16 mi + 4 lg .. + 3
  const int oh = oh0 + wave;
  bool valid[NT_PIX];
  long pix[NT_PIX], pixc[NT_PIX];   // pixc: clamped into the image, for loads that must not branch
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni) {
    const int ow = ow0 + ni * 16 + l15;
    valid[ni] = oh < p.H && ow < p.W;
    pix[ni] = ((long)b * p.H + oh) * p.W + ow;
    pixc[ni] = ((long)b * p.H + min(oh, p.H - 1)) * p.W + min(ow, p.W - 1);
  }

  // ---- the epilogue's operands, into registers, in front of the DMA.  Straight-line: a pixel past the image loads the
  //      image's nearest pixel (its sums get gm = 0); a branch here costs a register copy behind a full wait ----
  u32x2 uu[NT_CO][NT_PIX], rr[NT_CO][NT_PIX];
  f32x4 sc[NT_CO], sh[NT_CO];
  if constexpr (BX) {
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) {
      const int co = mi * 16 + 4 * lg;
      sc[mi] = *reinterpret_cast<const f32x4*>(p.bsc + (long)grp * BN + co);
      sh[mi] = *reinterpret_cast<const f32x4*>(p.bsh + (long)grp * BN + co);
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) {
        uu[mi][ni] = *reinterpret_cast<const u32x2*>((const bf16_t*)p.bx + pixc[ni] * p.ldbx + co);
        if constexpr (RES) rr[mi][ni] = *reinterpret_cast<const u32x2*>((const bf16_t*)p.res + pixc[ni] * p.ldres + co);
      }
    }
  }

  // ---- every DMA of the kernel: lane tid fills bytes [(j * 512 + tid) * 16, + 16) of an image in round j, i.e. physical
  //      chunk slot tid & 7 of row j * 64 + (tid >> 3); it fetches logical chunk slot ^ key(row), the same in every round ----
  {
    const int rsub = tid >> 3;
    const int c_l = (tid & 7) ^ (rsub & 6);
    unsigned lds = __builtin_amdgcn_readfirstlane(lds_addr(smem) + wave * 1024);
#pragma unroll
    for (int j = 0; j < kMidHaloRounds; ++j) {
      const int row = rsub + j * 64;
      const int ih = row / IWp, iw = row - ih * IWp;
      const int gh = oh0 - 1 + ih, gw = ow0 - 1 + iw;
      const bool in = ih < kMidIH && iw < kMidTW + 2 && gh >= 0 && gh < p.H && gw >= 0 && gw < p.W;
      glds16(in ? (const void*)(xb + (gh * p.W + gw) * p.ldx + c_l * 8) : (const void*)sdhip_zero16, lds);
      lds += 8192;
    }
    const bf16_t* wsrc = wpk + rsub * 64 + c_l * 8;   // packed [9][64][64]: row (tap, m) = rsub of round `tap`
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      glds16(wsrc + t * (BN * 64), lds);
      lds += 8192;
    }
  }

  f32x4 acc[NT_CO][NT_PIX];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT_PIX; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- fragment addressing of conv_fast.h: pixel tiles 0 / 1 of tile row `wave` are 16 halo rows apart (one swizzle key) ----
  const int prow0 = wave * IWp + l15;
  const int lg4 = lg << 4;
  const int a_base = LdsRow<2>::off(l15, lg);
  auto kernel_row = [&](int ky) {   // taps (ky, 0..2), each its two k-steps: conv_fast.h's order per accumulator
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int row = prow0 + ky * IWp + kx;
      const int b_addr = row * RB + (lg4 ^ ((row & 6) << 4));
      const int a_addr = a_base + (ky * 3 + kx) * (BN * RB);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        u32x4 af[NT_CO], bf[NT_PIX];
        const unsigned char* ab = wl + (a_addr ^ (ks << 6));
        const unsigned char* bb = halo + (b_addr ^ (ks << 6));
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi) af[mi] = *reinterpret_cast<const u32x4*>(ab + mi * (16 * RB));
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni) bf[ni] = *reinterpret_cast<const u32x4*>(bb + ni * (16 * RB));
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni) Mma<bf16_t>::run(acc[mi][ni], af[mi], bf[ni]);
      }
    }
  };
  mid_wait_publish<6>();   // the halo and taps 0 .. 2
  kernel_row(0);
  mid_wait_publish<3>();   // taps 3 .. 5
  kernel_row(1);
  mid_wait_publish<0>();   // taps 6 .. 8
  kernel_row(2);

  // ---- epilogue: round once, store, sums over the stored values ----
  float s1[NT_CO][4], s2[NT_CO][4];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[mi][r] = 0.f; s2[mi][r] = 0.f; }
  bf16_t* const yb = (bf16_t*)p.y;
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni) {
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) {
      const int co = mi * 16 + 4 * lg;
      f32x4 v = acc[mi][ni];
      if constexpr (RES) v += f32x4{bflo(rr[mi][ni][0]), bfhi(rr[mi][ni][0]), bflo(rr[mi][ni][1]), bfhi(rr[mi][ni][1])};
      const u32x2 o = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      if (valid[ni]) *reinterpret_cast<u32x2*>(yb + pix[ni] * p.ldy + co) = o;
      const f32x4 g = valid[ni] ? f32x4{bflo(o[0]), bfhi(o[0]), bflo(o[1]), bfhi(o[1])} : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (BX) {
        const float u4[4] = {bflo(uu[mi][ni][0]), bfhi(uu[mi][ni][0]), bflo(uu[mi][ni][1]), bfhi(uu[mi][ni][1])};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gm = fmaf(u4[r], sc[mi][r], sh[mi][r]) > 0.f ? g[r] : 0.f;
          s1[mi][r] = fmaf(gm, u4[r], s1[mi][r]);
          s2[mi][r] += gm;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) { s1[mi][r] += g[r]; s2[mi][r] = fmaf(g[r], g[r], s2[mi][r]); }
      }
    }
  }

  if (p.stats) {  // uniform
    __syncthreads();  // all fragment reads done: LDS is reused for the cross-wave reduction
    float* red = reinterpret_cast<float*>(smem);  // [8 waves][2][BN]
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = row16_sum(s1[mi][r]), c2 = row16_sum(s2[mi][r]);   // over the 16 pixels of the MFMA tile (DPP)
        if (l15 == 0) {
          const int m = mi * 16 + 4 * lg + r;
          red[(wave * 2 + 0) * BN + m] = a;
          red[(wave * 2 + 1) * BN + m] = c2;
        }
      }
    }
    __syncthreads();
    if (tid < 2 * BN) {
      const int which = tid / BN, m = tid - which * BN;
      float tot = red[which * BN + m];
#pragma unroll
      for (int w = 1; w < kMidWaves; ++w) tot += red[(w * 2 + which) * BN + m];
      const long rep = (blockIdx.x + blockIdx.z) % p.nrep;
      atomicAdd(p.stats + rep * p.rep_stride + ((long)grp * 2 + which) * p.stats_ld + m, (double)tot);
    }
  }
}

template <bool BX, bool RES>
int launch_mid_bx(const MidArgs& a, int B, hipStream_t s) {
  auto kern = conv_mid_kernel<BX, RES>;
  static bool attr_set = false;  // per instantiation
  if (!attr_set) {   // always above 64 KiB
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_mid: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  dim3 grid(a.tiles_w * sdhip_cdiv(a.H, kMidTH), 1, B);
  hipLaunchKernelGGL(kern, grid, dim3(kMidWaves * 64), kMidLds, s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

int launch_mid(const MidArgs& a, int B, hipStream_t s) {
  if (!a.bx) return launch_mid_bx<false, false>(a, B, s);
  return a.res ? launch_mid_bx<true, true>(a, B, s) : launch_mid_bx<true, false>(a, B, s);
}

}  // namespace
