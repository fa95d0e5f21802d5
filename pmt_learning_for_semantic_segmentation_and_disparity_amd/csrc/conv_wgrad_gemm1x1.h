// Weight gradient of a 1x1 / stride-1 / unpadded convolution with a BatchNorm(+ReLU) prologue on X, bf16, written as a
// GEMM over pixels for gfx950 (the DenseNet bottlenecks Cin -> 128 and the transitions):
//
//   dW[m][k] = sum over pixels of dY[pix][m] * Xhat[pix][k],   Xhat = bf16(relu?(fma(X, scale_g, shift_g)))
//
// conv_wgrad_fast.h's workgroup is built for 9..25 taps; with one tap it multiplies a 64 x 64 output block, does 8 MFMAs
// per wave between two barriers and re-stages dY once per 64 input channels.  Here ONE 512-thread workgroup owns
// 128 output channels x up to 256 input channels (four 64-channel chunks):
//  * waves = 2 output halves x 4 input chunks; a wave holds 4 x 4 MFMA tiles (64 accumulator registers) and per 32-pixel
//    k-step issues 16 MFMAs for 8 transposing fragment reads (4 of dY, 4 of Xhat);
//  * the K loop runs over SLABS of 64 pixels of one image (a slab never crosses an image, so a slab has one statistics
//    group; the pixels past the end of the image are zeroed in BOTH operands AFTER the prologue: relu(shift) != 0);
//  * dY is staged once per 256 input channels, X once per 128 output channels;
//  * staging keeps the discipline of conv_wgrad_fast.h's register path: plain register loads two slabs ahead in two
//    register sets (exact vmcnt waits placed by the compiler), one barrier per slab, two LDS stages.
// LDS stage = six [64 pixels][64 channels] images of 128-byte rows with WRow's swizzle (four chunks of Xhat, two halves of
// dY); consecutive images start 8192 + 128 bytes apart, so that the two images a 16-lane group of a staging store writes
// (same pixel row, neighbouring chunks) fall into different halves of the banks.  Every wave reads its fragments from one
// Xhat image and one dY image with the byte offsets of the unpacked kernel (conflict-free, see WRow).
// A staging lane owns the same 8 input channels in every slab: 16 prologue coefficients in registers.
// The workgroup sweeps a strided share of the slabs and flushes once with f32 atomics into the packed gradient
// [nq][1][Mpad][64]; only real (m, k) entries are flushed.  Chunks past Cin are neither staged nor multiplied.
//
// Registers (hipcc 7.2, gfx950; tools/kernel_regs.py conv_wgrad wgrad_gemm1x1): 224 VGPRs stand-alone, 212 grouped, no AGPRs,
// no scratch — 64 accumulators, 2 x 24 staging, 16 coefficients, 32 fragments.  One workgroup per CU (2 x 48.75 KB of LDS;
// 8 waves = 2 per SIMD, 256 registers each).
// Measured (MI355X, both towers as one batch of 16 images, tools/gpu_wgrad1x1.py blocks: a block's layers as one grouped call,
// against the kernels this one replaces): block 1 (64x128 maps) 223 -> 128 us, block 2 (32x64) 231 -> 122, block 3 (16x32)
// 284 -> 128, block 4 (8x16) 69 -> 43, transitions 55 / 58 / 54 -> 53 / 57 / 48: no map size is left on the old kernels.
#pragma once
#include "conv_wgrad_fast.h"

namespace {

constexpr int kWg1Slab = 64;                 // pixels per stage
constexpr int kWg1Img = 8192 + 128;          // bytes between two LDS images of a stage
constexpr int kWg1Stage = 6 * kWg1Img;       // Xhat chunks 0..3, dY halves 0..1

// (bx, gdx, by): slab share bx of gdx, by = (128-output block, group of four input chunks) — as in wgrad_fast_body.
// WgfArgs: nq = groups of four chunks, nq_tot = 64-channel chunks; Cout % 128 == 0, Cin % 8 == 0, D == Do == kd == 1.
__device__ __forceinline__ void wgrad_gemm1x1_body(const WgfArgs& p, const int bx, const int gdx, const int by) {
  typedef bf16_t T;
  constexpr int V = 8, CK = 64, SLAB = kWg1Slab, IMG = kWg1Img, STAGE = kWg1Stage;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int ciq = wave & 3, coh = wave >> 2;           // input chunk / output half of this wave
  const int qg = by % p.nq, mb = by / p.nq;
  const int m0 = mb * 128, q0 = qg * 4;
  const int nch = min(4, p.nq_tot - q0);               // chunks this workgroup owns
  const int HW = p.H * p.W;
  const int spi = (HW + SLAB - 1) / SLAB;              // slabs per image
  const int nslab = p.B * spi;

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- fragment addresses inside an image (see wgrad_fast_body): the same for the dY tiles mi and the Xhat tiles ni ----
  const int p4 = lane & 3, r4 = l15 >> 2;
  const int sub = (p4 & 1) << 3;
  const int pa = 8 * lg + r4;
  int f_lo[4], f_hi[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = 2 * t + (p4 >> 1);
    f_lo[t] = WRow::off(pa, c) + sub;
    f_hi[t] = WRow::off(pa + 4, c) + sub;
  }
  const int a_img = (4 + coh) * IMG, b_img = ciq * IMG;

  // ---- staging roles: X lane = (8 channels cx of chunk jx, rows rx0 + 16 i), dY lane = (8 channels cy of half hy, rows ry0 + 32 i).
  //      WRow's key repeats every 16 rows: the rounds of a lane differ by a constant byte offset. ----
  const int cx = tid & 7, jx = (tid >> 3) & 3, rx0 = tid >> 5;
  const int cy = tid & 7, hy = (tid >> 3) & 1, ry0 = tid >> 4;
  const int chx = (q0 + jx) * CK + cx * V;             // first input channel of the lane
  const bool livex = jx < nch;                         // the chunk exists (its image is read by a wave)
  const bool okx = livex && chx < p.Cin;               // Cin % 8 == 0: the lane's 8 channels are inside or outside together
  const int chy = m0 + hy * CK + cy * V;               // < Cout (Cout % 128 == 0)
  const int xdst = jx * IMG + WRow::off(rx0, cx);
  const int ydst = (4 + hy) * IMG + WRow::off(ry0, cy);

  float psc[V], psf[V];
  int cur_grp = -1;

  // slab walk without divisions in the loop: (image, slab of the image) of the NEXT slab to load advance by gdx slabs
  int n_img = bx / spi, n_sl = bx - n_img * spi;
  const int step_img = gdx / spi, step_sl = gdx - step_img * spi;

  struct RegSet { u32x4 x[4]; u32x4 y[2]; int npx, grp; };
  RegSet ra, rb;
  auto load = [&](RegSet& r) {
    const int img = n_img, pix0 = n_sl * SLAB;
    n_sl += step_sl; if (n_sl >= spi) { n_sl -= spi; ++n_img; }
    n_img += step_img;
    r.npx = min(SLAB, HW - pix0);                      // real pixels of the slab (uniform)
    r.grp = img >= p.bpg ? img / p.bpg : 0;
    const T* xb = (const T*)p.x + ((long)img * HW + pix0) * p.ldx + chx;
    const T* yb = (const T*)p.dy + ((long)img * HW + pix0) * p.lddy + chy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = rx0 + 16 * i;
      const T* src = (okx && row < r.npx) ? xb + row * p.ldx : (const T*)sdhip_zero16;
      r.x[i] = *reinterpret_cast<const u32x4*>(src);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = ry0 + 32 * i;
      const T* src = row < r.npx ? yb + row * p.lddy : (const T*)sdhip_zero16;
      r.y[i] = *reinterpret_cast<const u32x4*>(src);
    }
  };
  auto store = [&](const RegSet& r, unsigned char* buf) {   // prologue on X, rows past the image zeroed, both operands into LDS
    if (p.in_scale && r.grp != cur_grp) {               // uniform; the group changes a few times per sweep at most
      cur_grp = r.grp;
      const float* sc = p.in_scale + cur_grp * p.Cin + (okx ? chx : 0);
      const float* sf = p.in_shift + cur_grp * p.Cin + (okx ? chx : 0);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        psc[e] = okx ? sc[e] : 0.f;
        psf[e] = okx ? sf[e] : 0.f;
      }
    }
    if (livex) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = okx && rx0 + 16 * i < r.npx;
        u32x4 raw = u32x4{0u, 0u, 0u, 0u};
        if (in) {
          raw = r.x[i];
          if (p.in_scale) {
            float f[V];
            Chunk<T>::unpack(raw, f);
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float v = fmaf(f[e], psc[e], psf[e]);
              f[e] = p.in_relu ? fmaxf(v, 0.f) : v;
            }
            raw = Chunk<T>::pack(f);
          }
        }
        *reinterpret_cast<u32x4*>(buf + xdst + i * (16 * 128)) = raw;
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool in = ry0 + 32 * i < r.npx;
      *reinterpret_cast<u32x4*>(buf + ydst + i * (32 * 128)) = in ? r.y[i] : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto compute = [&](const unsigned char* buf) {
    if (ciq >= nch) return;                              // wave-uniform: no such chunk
#pragma unroll
    for (int ks = 0; ks < SLAB / 32; ++ks) {
      const unsigned char* ab = buf + a_img + ks * (32 * 128);
      const unsigned char* bb = buf + b_img + ks * (32 * 128);
      u32x4 af[4], bf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) af[t] = tr_pair(ab + f_lo[t], ab + f_hi[t]);
#pragma unroll
      for (int t = 0; t < 4; ++t) bf[t] = tr_pair(bb + f_lo[t], bb + f_hi[t]);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) Mma<T>::run(acc[mi][ni], af[mi], bf[ni]);
    }
  };

  // ---- sweep (the two-register-set pipeline of wgrad_fast_body) ----
  const int ntl = bx < nslab ? (nslab - bx + gdx - 1) / gdx : 0;   // this workgroup's slabs
  if (ntl > 0) load(ra);
  if (ntl > 1) load(rb);
  for (int it = 0; it < ntl; it += 2) {
    store(ra, smem);
    __syncthreads();                      // slab visible; everybody has finished slab it-2 in this stage (see slab it-1's barrier)
    if (it + 2 < ntl) load(ra);
    compute(smem);
    if (it + 1 < ntl) {                   // uniform
      store(rb, smem + STAGE);
      __syncthreads();
      if (it + 3 < ntl) load(rb);
      compute(smem + STAGE);
    }
  }

  // ---- flush: f32 atomics into [nq_tot][1][Mpad][64]; the channel tail of the last chunk stays zero ----
  if (ntl > 0 && ciq < nch) {             // wave-uniform
    const int q = q0 + ciq;
    float* dst = p.dwp + (long)q * p.Mpad * CK;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int kc = ni * 16 + l15;
      if (q * CK + kc < p.Cin) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + coh * CK + mi * 16 + 4 * lg + r;
            atomicAdd(dst + (long)m * CK + kc, acc[mi][ni][r]);
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(512) void wgrad_gemm1x1_kernel(const WgfArgs p) {
  wgrad_gemm1x1_body(p, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

__global__ __launch_bounds__(512) void wgrad_gemm1x1_group_kernel(const WgfGroup g) {
  const int b = (int)blockIdx.x;
  int i = 0;
  while (i + 1 < g.n && b >= g.wg0[i + 1]) ++i;
  const int local = b - g.wg0[i];
  const int gx = g.gx[i];
  const int by = local / gx;
  wgrad_gemm1x1_body(g.L[i], local - by * gx, gx, by);
}

// Does the layer run on this kernel (wg_fast has checked bf16, 16-byte pixels on both operands and 31-bit image offsets)?
inline bool wgrad_gemm1x1_ok(const WgfArgs& f, int T) {
  return T == 1 && f.kd == 1 && f.D == 1 && f.Do == 1 && f.stride == 1 && f.pad_t == 0 && f.pad_l == 0 && f.Ho == f.H && f.Wo == f.W &&
         f.Cout % 128 == 0 && f.Cin >= 96 && f.Cin % 8 == 0 && f.in_scale && !f.dbias;
}

// `f` as wg_fast fills it (nq = 64-channel chunks).  The plan joins launch_wgf_group like any other: ntiles counts slabs.
inline int plan_wg1(const WgfArgs& f, WgfPlan& pl) {
  WgfArgs a = f;
  a.nq_tot = f.nq; a.nq = sdhip_cdiv(f.nq, 4);
  a.tpb = 1; a.ntg = 1; a.qb = 0; a.qsh = 0;
  const size_t lds = 2 * (size_t)kWg1Stage;
  SDHIP_CHOSE(kWgGemm1x1);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)wgrad_gemm1x1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)wgrad_gemm1x1_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv2d_wgrad: cannot raise dynamic LDS limit");
    attr_set = true;
  }
  const int gy = (a.Cout / 128) * a.nq;
  const int ntiles = a.B * sdhip_cdiv((long)a.H * a.W, kWg1Slab);
  // Cost model (the balance of plan_wgf): a slab of a workgroup moves 64 pixels x (128 + 64 nch) channels; the closing
  // atomics of a workgroup are its 128 x (Cin / nq) real entries at the chip-wide atomic rate.
  // Calibration (tools/gpu_wgrad1x1.py blocks, SDHIP_TUNE_WG1_TILE scales t_tile_us): 256 -> 128 at 16x64x128 alone (2048
  // slabs) took 70.7 / 58.0 / 52.9 / 52.7 / 57.8 us with 64 / 91 / 128 / 181 / 256 shares; a fit T = a / gx + b gx gives
  // 1.8 us per slab and 0.17 us of flush per workgroup on that HBM-bound map — both about twice the constants below, so
  // their RATIO, which is all the share count depends on, stands.  The grouped blocks do not react to the scale at all
  // (sum over the tower 600 / 582 / 579 / 579 / 584 us at x0.25 / 0.5 / 1 / 2 / 4): the constants stay as derived.
  const int nch = a.nq_tot < 4 ? a.nq_tot : 4;
  const double t_tile_us = (0.20 + 0.15 * nch) * sdhip_diag().tune_wg1_tile;
  const double flush_us = 128.0 * ((double)a.Cin / a.nq) * 4 / (sdhip_diag().tune_atomic_tbs * 1e6);
  int gx = (int)(sqrt((double)ntiles * t_tile_us / flush_us) + 0.5);
  if (gx > sdhip_cdiv(256, gy)) gx = sdhip_cdiv(256, gy);
  if (gx > sdhip_cdiv(ntiles, 2)) gx = sdhip_cdiv(ntiles, 2);
  if (gx < 1) gx = 1;
  pl.single = (const void*)wgrad_gemm1x1_kernel; pl.group = (const void*)wgrad_gemm1x1_group_kernel;
  pl.lds = lds; pl.ntiles = ntiles; pl.gy = gy; pl.gx = gx; pl.occ = 1;
  pl.t_tile_us = t_tile_us; pl.flush_us = flush_us; pl.a = a;
  return SDHIP_OK;
}

}  // namespace
