// Direct 2-D convolution, forward / data-gradient form, for gfx950 (MI355X).
//
// Replaces ATen/cuDNN under `conv2dSame` (models/torch_model.py:236-281), the
// stride-1 `ConvTranspose2dSame` (models/torch_model.py:284-349, run as a
// correlation with flipped, transposed weights), the plain `nn.Conv2d`s of the
// DenseNet towers (models/densenet.py:25-93,218-245) and ASPP (models/aspp.py:7-32),
// and — with dgrad-packed weights — their input gradients.
//
// One 256-thread workgroup computes a TH x TW tile of output pixels for up to BN
// output channels of one image.  Per 128-byte channel chunk of the input it stages
// the halo tile ((TH-1)s+(kh-1)d+1) x ((TW-1)s+(kw-1)d+1) pixels ONCE in LDS and
// then walks all kh*kw taps over it (im2col-free; every input byte is read from
// HBM/L2 once per chunk), with the tap weights staged next to it.  Optional fused
// prologue (per-channel affine + ReLU on the input = the BatchNorm+ReLU that
// precedes the conv) and epilogue (bias, activation, accumulate, per-channel
// sum / sum-of-squares for the BatchNorm that follows).
#include "conv_common.h"
#include "conv_fast.h"
#include "conv_point.h"
#include "conv_grow.h"
#include "conv_mid.h"
#include "conv_band.h"
#include "conv_gemm.h"
#include "conv_thin.h"

namespace {

struct FwdArgs {
  const void* x; const void* wp; void* y;
  const float* bias; const float* in_scale; const float* in_shift; double* stats;
  ConvGeom g;
  int Cin, ldx, Cout, Mpad, ldy;
  int in_relu, groups, act, accumulate;
  int tg, vec_in, vec_out, stats_ld, nrep, pf_halo, sh, per_tap;
  long rep_stride;
};

template <typename T, int TH, int TW, int BN>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const FwdArgs p) {
  constexpr int V = Chunk<T>::N;
  constexpr int CK = 8 * V;
  constexpr int TWT = TW / 16;             // pixel tiles per tile row
  constexpr int NPT = TH * TWT;            // pixel tiles per workgroup
  constexpr int NT_PIX = NPT / 4;          // per wave
  constexpr int NT_CO = BN / 16;
  static_assert(NPT % 4 == 0 && NT_PIX >= 1, "tile must give every wave at least one 16-pixel MFMA tile");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const ConvGeom& g = p.g;
  const int tiles_w = (g.Wo + TW - 1) / TW;
  const int oh0 = (blockIdx.x / tiles_w) * TH, ow0 = (blockIdx.x % tiles_w) * TW;
  const int n0 = blockIdx.y * BN;
  const int b = blockIdx.z / g.Do, dz = blockIdx.z - b * g.Do;   // image = (batch, output depth slice)
  const int grp = p.groups > 1 ? b / (g.B / p.groups) : 0;
  const int s = g.stride, d = g.dil;
  // per_tap (strongly dilated kernels, e.g. ASPP's 3x3 dil 6/12): the halo tile would be mostly holes, so every tap stages
  // just the shifted TH x TW tile instead and is treated as a 1x1 convolution.
  const int IH = (TH - 1) * s + (p.per_tap ? 0 : (g.kh - 1) * d) + 1, IW = (TW - 1) * s + (p.per_tap ? 0 : (g.kw - 1) * d) + 1;
  const int ih0 = oh0 * s - g.pad_t, iw0 = ow0 * s - g.pad_l;
  const int Tn = g.kh * g.kw;
  const int nq = (p.Cin + CK - 1) / CK;     // channel chunks per depth tap; the chunk loop runs over kd*nq "chunks"
  const int nqq = g.kd * nq;
  const int mvalid = min(BN, p.Mpad - n0);  // multiple of 16
  // LDS: [halo (x2 when its loads are register-prefetched)] [weights stage buffer 0] [weights stage buffer 1]
  const int halo_bytes = (IH * IW * 128 + 15) & ~15;
  const int wbuf_bytes = p.tg * BN * 128;
  unsigned char* halo0 = smem;
  unsigned char* wl0 = smem + halo_bytes * (((TH * TW <= 64) && p.pf_halo) ? 2 : 1);

  f32x4 acc[NT_CO][NT_PIX];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT_PIX; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  int pbase[NT_PIX];  // halo pixel index of this lane's output pixel for tap (0,0)
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni) {
    const int pt = wave * NT_PIX + ni;
    pbase[ni] = ((pt / TWT) * s) * IW + ((pt % TWT) * 16 + l15) * s;
  }

  const T* xb0 = (const T*)p.x + (long)b * g.D * g.H * g.W * p.ldx;   // depth slice 0 of batch b
  const T* wpk = (const T*)p.wp;
  const int ntg = (Tn + p.tg - 1) / p.tg;
  const int S = nqq * ntg;   // pipeline stages: (depth tap, channel chunk, tap group)
  // chunk qq = (kdi, q): input depth slice din = dz*sd + kdi - pad_d (a slice outside the volume is zero padding)
  auto slice_of = [&](int qq) { return dz * g.sd + qq / nq - g.pad_d; };
  auto slice_ok = [&](int qq) { const int din = slice_of(qq); return din >= 0 && din < g.D; };
  auto xb_of = [&](int qq) { return xb0 + (long)slice_of(qq) * g.H * g.W * p.ldx; };

  // Software pipeline: the global loads of stage s+1 (its tap-group weights and, at a chunk boundary, its halo tile)
  // are issued into registers BEFORE the MFMAs of stage s and committed to the other LDS buffer after them, so the
  // L2/HBM latency hides behind the matrix work and a stage costs one barrier.
  // PF (small 4x16 tiles only): the halo tile is register-prefetched and double-buffered too; the large 8x32 tiles
  // stage their halo with a plain copy at chunk boundaries and spend the registers on accumulators instead.
  constexpr bool PF = (TH * TW <= 64);
  constexpr int HPF = PF ? 4 : 1, WPF = 4;   // 16-byte loads per lane kept in flight for the halo / the weights
  u32x4 rh[HPF], rw[WPF];
  const bool pf_halo = PF && p.pf_halo;

  // Per-lane staging plan, computed ONCE (it does not depend on the stage): where each of this lane's 16-byte loads
  // comes from (relative to the stage base) and where it lands in LDS.  p.sh is constant for the launch: 8 chunks per
  // 128-byte row, or 4 when the whole reduction fits one half row (Cin <= CK/2).
  const int sh = p.sh;
  const unsigned magic_iw = div_magic(IW);
  int h_src[HPF], h_lds[HPF], h_ch[HPF];   // halo: element offset inside the image (or -1), LDS byte offset, channel offset
  if (pf_halo) {
    const int total = (IH * IW) << sh;
#pragma unroll
    for (int j = 0; j < HPF; ++j) {
      const int i = tid + j * 256;
      h_src[j] = -1; h_lds[j] = -1; h_ch[j] = 0;
      if (i < total) {
        const int pix = i >> sh, c = i & ((1 << sh) - 1);
        const int ih = fast_div(pix, IW, magic_iw), iw = pix - ih * IW;
        const int gh = ih0 + ih, gw = iw0 + iw;
        h_lds[j] = lds_off(pix, c);
        h_ch[j] = c * V;
        if (gh >= 0 && gh < g.H && gw >= 0 && gw < g.W) h_src[j] = (gh * g.W + gw) * p.ldx + c * V;
      }
    }
  }
  int w_src[WPF], w_lds[WPF], w_tl[WPF];   // weights: element offset inside the stage's packed block, LDS offset, tap
  {
    const unsigned magic_m = div_magic(mvalid);
#pragma unroll
    for (int j = 0; j < WPF; ++j) {
      const int i = tid + j * 256;
      const int row = i >> sh, c = i & ((1 << sh) - 1);
      const int tl = fast_div(row, mvalid, magic_m), m = row - tl * mvalid;
      w_tl[j] = tl;
      w_src[j] = (tl * p.Mpad + m) * CK + c * V;
      w_lds[j] = lds_off(tl * BN + m, c);
    }
  }

  auto halo_issue = [&](int qq) {   // vector path only (host guarantees vec_in when pf_halo)
    const int q = qq % nq;
    const bool ok = slice_ok(qq);
    const T* xb = xb_of(qq);
#pragma unroll
    for (int j = 0; j < HPF; ++j) {
      rh[j] = u32x4{0u, 0u, 0u, 0u};
      if (ok && h_src[j] >= 0 && q * CK + h_ch[j] < p.Cin)
        rh[j] = *reinterpret_cast<const u32x4*>(xb + h_src[j] + q * CK);
    }
  };
  auto halo_commit = [&](int qq, unsigned char* dst) {
    const int q = qq % nq;
    const bool ok = slice_ok(qq);
#pragma unroll
    for (int j = 0; j < HPF; ++j) {
      if (h_lds[j] >= 0) {
        u32x4 raw = rh[j];
        if (p.in_scale && ok && h_src[j] >= 0) {
          const int ch0 = q * CK + h_ch[j];
          if (ch0 < p.Cin) {   // zero padding (spatial or channel) stays zero
            float f[V];
            Chunk<T>::unpack(raw, f);
            const float* sc = p.in_scale + grp * p.Cin + ch0;
            const float* sf = p.in_shift + grp * p.Cin + ch0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float v = fmaf(f[e], sc[e], sf[e]);
              f[e] = p.in_relu ? fmaxf(v, 0.f) : v;
            }
            raw = Chunk<T>::pack(f);
          }
        }
        *reinterpret_cast<u32x4*>(dst + h_lds[j]) = raw;
      }
    }
  };
  auto halo_sync_stage = [&](int qq, unsigned char* dst) {   // big halo tiles: plain staged copy (4 loads in flight)
    const int q = qq % nq;
    StageSrc ss;
    ss.base = xb_of(qq); ss.H = slice_ok(qq) ? g.H : 0; ss.W = g.W; ss.ld = p.ldx; ss.C = p.Cin;
    ss.h0 = ih0; ss.w0 = iw0; ss.IH = IH; ss.IW = IW;
    ss.scale = p.in_scale ? p.in_scale + grp * p.Cin : nullptr;
    ss.shift = p.in_scale ? p.in_shift + grp * p.Cin : nullptr;
    ss.relu = p.in_relu; ss.vec = p.vec_in; ss.magic_iw = magic_iw;
    stage_tile<T, 4>(dst, ss, q, sh, tid);
  };
  auto w_issue = [&](int qq, int t0) {   // packed weights are [kd][nq][T][Mpad][CK]: chunk index qq as is
    const int nt = min(p.tg, Tn - t0);
    const T* base = wpk + ((long)(qq * Tn + t0) * p.Mpad + n0) * CK;
#pragma unroll
    for (int j = 0; j < WPF; ++j)
      if (w_tl[j] < nt) rw[j] = *reinterpret_cast<const u32x4*>(base + w_src[j]);
  };
  auto w_commit = [&](int q, int t0, unsigned char* dst) {
    const int nt = min(p.tg, Tn - t0);
#pragma unroll
    for (int j = 0; j < WPF; ++j)
      if (w_tl[j] < nt) *reinterpret_cast<u32x4*>(dst + w_lds[j]) = rw[j];
  };
  // Fragment addressing.  lds_off(row, c) = row*128 + ((c ^ s(row)) << 4) with s(row) = (row>>1)&7 and c = 4*ks + lg, i.e.
  // row*128 + ((ks<<6) ^ (lg<<4) ^ (s(row)<<4)).  For the weight rows s() does not depend on the tap (tap stride BN*128 is
  // a multiple of 16 rows), so everything but the k-step bit is hoisted out of the tap loop.
  int a_off[NT_CO];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi) {
    const int row = mi * 16 + l15;
    a_off[mi] = row * 128 + ((lg << 4) ^ (((row >> 1) & 7) << 4));
  }
  auto compute = [&](int qq, int t0, const unsigned char* halo, const unsigned char* wl) {
    const int cq = min(CK, p.Cin - (qq % nq) * CK);
    const bool two = (cq + CK / 2 - 1) / (CK / 2) == 2;   // second 64-byte k-step present (wave-uniform)
    const int nt = min(p.tg, Tn - t0);
    int khi = t0 / g.kw, kwi = t0 - khi * g.kw;
    for (int tl = 0; tl < nt; ++tl) {
      const int toff = p.per_tap ? 0 : (khi * d) * IW + kwi * d;
      if (++kwi == g.kw) { kwi = 0; ++khi; }
      const unsigned char* wt = wl + tl * (BN * 128);
      int b_off[NT_PIX];
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) {
        const int row = pbase[ni] + toff;
        b_off[ni] = row * 128 + ((lg << 4) ^ (((row >> 1) & 7) << 4));
      }
      // both k-steps' fragments are requested up front: the second k-step's LDS latency hides behind the first's MFMAs
      u32x4 af0[NT_CO], bf0[NT_PIX], af1[NT_CO], bf1[NT_PIX];
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi)
        if (mi * 16 < mvalid) af0[mi] = *reinterpret_cast<const u32x4*>(wt + a_off[mi]);
#pragma unroll
      for (int ni = 0; ni < NT_PIX; ++ni) bf0[ni] = *reinterpret_cast<const u32x4*>(halo + b_off[ni]);
      if (two) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
          if (mi * 16 < mvalid) af1[mi] = *reinterpret_cast<const u32x4*>(wt + (a_off[mi] ^ 64));
#pragma unroll
        for (int ni = 0; ni < NT_PIX; ++ni) bf1[ni] = *reinterpret_cast<const u32x4*>(halo + (b_off[ni] ^ 64));
      }
#pragma unroll
      for (int mi = 0; mi < NT_CO; ++mi)
        if (mi * 16 < mvalid) {
#pragma unroll
          for (int ni = 0; ni < NT_PIX; ++ni) Mma<T>::run(acc[mi][ni], af0[mi], bf0[ni]);
        }
      if (two) {
#pragma unroll
        for (int mi = 0; mi < NT_CO; ++mi)
          if (mi * 16 < mvalid) {
#pragma unroll
            for (int ni = 0; ni < NT_PIX; ++ni) Mma<T>::run(acc[mi][ni], af1[mi], bf1[ni]);
          }
      }
    }
  };

  if (p.per_tap) {   // one stage per (chunk, tap): shifted tile + that tap's weights, no prefetch (rare, small layers)
    for (int st = 0; st < nqq * Tn; ++st) {
      const int q = st / Tn, t = st - q * Tn;   // q runs over (depth tap, channel chunk)
      const int khi = t / g.kw, kwi = t - khi * g.kw;
      __syncthreads();
      StageSrc ss;
      ss.base = xb_of(q); ss.H = slice_ok(q) ? g.H : 0; ss.W = g.W; ss.ld = p.ldx; ss.C = p.Cin;
      ss.h0 = ih0 + khi * d; ss.w0 = iw0 + kwi * d; ss.IH = IH; ss.IW = IW;
      ss.scale = p.in_scale ? p.in_scale + grp * p.Cin : nullptr;
      ss.shift = p.in_scale ? p.in_shift + grp * p.Cin : nullptr;
      ss.relu = p.in_relu; ss.vec = p.vec_in; ss.magic_iw = magic_iw;
      stage_tile<T, 4>(halo0, ss, q % nq, sh, tid);
      w_issue(q, t);
      w_commit(q, t, wl0);
      __syncthreads();
      compute(q, t, halo0, wl0);
    }
  } else {
  // prologue: stage 0
  if (pf_halo) halo_issue(0); else halo_sync_stage(0, halo0);
  w_issue(0, 0);
  for (int st = 0; st < S; ++st) {
    const int q = st / ntg, t0 = (st - q * ntg) * p.tg;
    unsigned char* halo = halo0 + ((pf_halo && (q & 1)) ? halo_bytes : 0);
    unsigned char* wl = wl0 + (st & 1) * wbuf_bytes;
    if (pf_halo && t0 == 0) halo_commit(q, halo);
    w_commit(q, t0, wl);
    __syncthreads();                      // stage st is visible; every wave has finished stage st-1
    const int sn = st + 1;
    int qn = 0, t0n = 0;
    if (sn < S) {
      qn = sn / ntg; t0n = (sn - qn * ntg) * p.tg;
      if (pf_halo && t0n == 0) halo_issue(qn);
      w_issue(qn, t0n);
    }
    compute(q, t0, halo, wl);
    if (!pf_halo && sn < S && t0n == 0) {   // chunk boundary with a single (large) halo buffer
      __syncthreads();
      halo_sync_stage(qn, halo0);
    }
  }
  }

  // ---- epilogue: bias / activation / accumulate / store / BN statistics ----
  float s1[NT_CO][4], s2[NT_CO][4];
#pragma unroll
  for (int mi = 0; mi < NT_CO; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[mi][r] = 0.f; s2[mi][r] = 0.f; }

  T* yb = (T*)p.y + (long)blockIdx.z * g.Ho * g.Wo * p.ldy;
#pragma unroll
  for (int ni = 0; ni < NT_PIX; ++ni) {
    const int pt = wave * NT_PIX + ni;
    const int oh = oh0 + pt / TWT, ow = ow0 + (pt % TWT) * 16 + l15;
    const bool valid = oh < g.Ho && ow < g.Wo;
    T* dst = yb + ((long)oh * g.Wo + ow) * p.ldy;
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) {
      if (mi * 16 >= mvalid) continue;
      const int co = n0 + mi * 16 + 4 * lg;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[mi][ni][r];
        if (p.bias && co + r < p.Cout) x += p.bias[co + r];
        if (p.act == 1) x = fmaxf(x, 0.f);
        else if (p.act == 2) x = 1.f / (1.f + __expf(-x));
        v[r] = x;
      }
      if (!valid) continue;
      if (p.vec_out && co + 3 < p.Cout) {
        if constexpr (sizeof(T) == 4) {
          f32x4* d4 = reinterpret_cast<f32x4*>(dst + co);
          f32x4 o = f32x4{v[0], v[1], v[2], v[3]};
          if (p.accumulate) o += *d4;
          *d4 = o;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = o[r];
        } else {
          u32x2* d2 = reinterpret_cast<u32x2*>(dst + co);
          if (p.accumulate) {
            const u32x2 old = *d2;
            v[0] += bflo(old[0]); v[1] += bfhi(old[0]); v[2] += bflo(old[1]); v[3] += bfhi(old[1]);
          }
          const u32x2 o = u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *d2 = o;
          v[0] = bflo(o[0]); v[1] = bfhi(o[0]); v[2] = bflo(o[1]); v[3] = bfhi(o[1]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (co + r < p.Cout) {
            if (p.accumulate) v[r] += Elem<T>::ld(dst + co + r);
            Elem<T>::st(dst + co + r, v[r]);
            v[r] = Elem<T>::rnd(v[r]);
          } else {
            v[r] = 0.f;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) { s1[mi][r] += v[r]; s2[mi][r] = fmaf(v[r], v[r], s2[mi][r]); }
    }
  }

  if (p.stats) {  // uniform
    __syncthreads();  // all fragment reads done: LDS is reused for the cross-wave reduction
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][2][BN]
#pragma unroll
    for (int mi = 0; mi < NT_CO; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float a = s1[mi][r], c2 = s2[mi][r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c2 += __shfl_xor(c2, o, 64); }
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
      if (n0 + m < p.Cout) {
        const float tot = red[(0 * 2 + which) * BN + m] + red[(1 * 2 + which) * BN + m] +
                          red[(2 * 2 + which) * BN + m] + red[(3 * 2 + which) * BN + m];
        atomicAdd(p.stats + (long)((blockIdx.x + blockIdx.z) % p.nrep) * p.rep_stride + ((long)grp * 2 + which) * p.stats_ld + n0 + m, (double)tot);
      }
    }
  }
}

template <typename T, int TH, int TW, int BN>
int launch(const FwdArgs& a, size_t lds, hipStream_t s) {
  auto kern = conv_fwd_kernel<T, TH, TW, BN>;
  static size_t attr_set = 0;  // per instantiation
  if (lds > 64 * 1024 && lds > attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      SDHIP_FAIL(SDHIP_ERR_LAUNCH, "conv_fwd: cannot raise dynamic LDS limit");
    attr_set = 160 * 1024;
  }
  const ConvGeom& g = a.g;
  dim3 grid(sdhip_cdiv(g.Ho, TH) * sdhip_cdiv(g.Wo, TW), sdhip_cdiv(a.Mpad, BN), g.B * g.Do);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}

template <typename T, int TH, int TW>
int launch_bn(const FwdArgs& a, int bn, size_t lds, hipStream_t s) {
  SDHIP_CHOSE(kFwdGeneric, TH, TW, a.per_tap, a.pf_halo);
  switch (bn) {
    case 16: return launch<T, TH, TW, 16>(a, lds, s);
    case 32: return launch<T, TH, TW, 32>(a, lds, s);
    case 64: return launch<T, TH, TW, 64>(a, lds, s);
    default: return launch<T, TH, TW, 128>(a, lds, s);
  }
}

size_t halo_bytes_of(const ConvGeom& g, int th, int tw, int per_tap) {
  const int eh = per_tap ? 0 : (g.kh - 1) * g.dil, ew = per_tap ? 0 : (g.kw - 1) * g.dil;
  const int IH = (th - 1) * g.stride + eh + 1, IW = (tw - 1) * g.stride + ew + 1;
  return ((size_t)IH * IW * 128 + 15) & ~(size_t)15;
}

// ---- host-side dispatch ---------------------------------------------------------

// consumer-side BatchNorm finalize of the input prologue (sdhip_conv2d_fwd_bnpro; FastArgs::pin_*)
struct ProStats {
  const double* stats; int ld, nrep;
  const float* gamma; const float* beta;
  float* scale; float* shift; float* mean; float* invstd; float* rmean; float* rvar;
  float eps, momentum; double count;
  const double* pend; double* fold; int pend_ld, pend_nrep, pend_c0, pend_n;
};

// One call of any of the extern "C" entry points below (never a kernel parameter).  The defaults are the plain
// convolution: an entry point sets the operands and, of the variant fields, only those that make it differ.
struct ConvCall {
  const void* x = nullptr; const void* wp = nullptr; void* y = nullptr;
  const float* bias = nullptr; const float* in_scale = nullptr; const float* in_shift = nullptr;
  double* stats = nullptr; int stats_ld = 0, stats_nrep = 1;
  ConvGeom g{};
  int Cin = 0, ldx = 0, Cout = 0, ldy = 0;
  int in_relu = 0, groups = 1, act = 0, accumulate = 0;
  int dtype = SDHIP_F32;
  hipStream_t stream = nullptr;
  // ---- variants ----
  int omul = 1, ooz = 0, ooy = 0, oox = 0;       // _phase: interleaved output (FastArgs::omul)
  const void* bx = nullptr; int ldbx = 0;        // _bnbwd: BatchNorm-backward epilogue (FastArgs::bx)
  const float* bsc = nullptr; const float* bsh = nullptr; int bx_mode = 0;
  const void* addend = nullptr; int ldadd = 0;   // _add, _bnbwd: y = conv(x) + addend
  const ProStats* ps = nullptr;                  // _bnpro
  bool plain() const { return !ps && !bx && !addend && omul == 1; }    // no variant: every kernel family may take it
  bool flat() const { return g.kd == 1 && g.D == 1 && g.Do == 1; }     // no depth axis
};

ConvGeom geom2d(int B, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int dil, int pad_t, int pad_l) {
  return ConvGeom{B, H, W, Ho, Wo, kh, kw, stride, dil, pad_t, pad_l, 1, 1, 1, 1, 0};
}

// the fields every entry point sets, in the order every entry point receives them
ConvCall conv_call(const void* x, const void* wpacked, void* y, const ConvGeom& g, int Cin, int ldx, int Cout, int ldy, int dtype, void* stream) {
  ConvCall c;
  c.x = x; c.wp = wpacked; c.y = y; c.g = g;
  c.Cin = Cin; c.ldx = ldx; c.Cout = Cout; c.ldy = ldy;
  c.dtype = dtype; c.stream = (hipStream_t)stream;
  return c;
}

// the consumer-side BatchNorm finalize of a call, if it has one, into the pin_* / pend_* fields every kernel family that
// takes it (fast, point, grow) carries under these names
template <typename Args>
void set_pin(Args& f, const ConvCall& c) {
  const ProStats* ps = c.ps;
  if (!ps) return;
  f.pin_stats = ps->stats; f.pin_ld = ps->ld; f.pin_nrep = ps->nrep; f.pin_groups = c.groups; f.pin_gamma = ps->gamma; f.pin_beta = ps->beta;
  f.pin_scale = ps->scale; f.pin_shift = ps->shift; f.pin_mean = ps->mean; f.pin_invstd = ps->invstd; f.pin_rmean = ps->rmean; f.pin_rvar = ps->rvar;
  f.pin_eps = ps->eps; f.pin_momentum = ps->momentum; f.pin_count = ps->count;
  f.pend_stats = ps->pend; f.pin_fold = ps->fold; f.pend_ld = ps->pend_ld; f.pend_nrep = ps->pend_nrep; f.pend_c0 = ps->pend_c0; f.pend_n = ps->pend ? ps->pend_n : 0;
}

// What the paths share, computed once per call.
struct ConvPlan {
  int V, es, Mpad;                       // elements per 16 bytes, element size, Cout rounded up to 16
  int stats_ld, nrep; long rep_stride;   // normalised statistics layout
  int vec_in, vec_out;
  int T, bn; bool big;                   // taps; output channels per workgroup; 8x32 (or 4x16) pixel tiles
  int rows, chunks_per_row, per_tap_any;
};

constexpr size_t kLdsMax = 160 * 1024, kLdsSoft = 80 * 1024;   // kLdsSoft: two workgroups per CU

ConvPlan conv_plan(const ConvCall& c) {
  const ConvGeom& g = c.g;
  const SdhipDiag& dg = sdhip_diag();
  ConvPlan d;
  d.V = c.dtype == SDHIP_BF16 ? 8 : 4;
  d.es = conv_esize(c.dtype);
  d.Mpad = (c.Cout + 15) & ~15;
  d.stats_ld = c.stats_ld > 0 ? c.stats_ld : c.Cout;
  d.nrep = c.stats_nrep > 0 ? c.stats_nrep : 1;
  d.rep_stride = (long)c.groups * 2 * d.stats_ld;
  d.vec_in = (c.ldx % d.V == 0) && (((uintptr_t)c.x & 15) == 0);   // channel tails are masked in stage_tile
  d.vec_out = (c.ldy % 4 == 0) && (((uintptr_t)c.y % (4 * d.es)) == 0);
  // output channels per workgroup: the widest block that wastes at most a quarter of its MFMA rows on padding
  int bn = 16;
  for (int cand = 128; cand >= 32; cand >>= 1)
    if ((long)sdhip_cdiv(d.Mpad, cand) * cand * 4 <= (long)d.Mpad * 5) { bn = cand; break; }
  // short reductions (1x1 over <= 128 channels ...) are bound by staging the input tile, not by MFMA rows: one pass
  if ((long)g.kh * g.kw * g.kd * c.Cin <= 128 && d.Mpad <= 128) bn = d.Mpad > 64 ? 128 : (d.Mpad > 32 ? 64 : (d.Mpad > 16 ? 32 : 16));
  d.T = g.kh * g.kw;
  const long blocks_big = (long)sdhip_cdiv(g.Ho, 8) * sdhip_cdiv(g.Wo, 32) * g.B * g.Do * sdhip_cdiv(d.Mpad, bn);
  d.big = (blocks_big >= dg.tune_big && g.Wo >= 24) || dg.conv_big;
  // stride-2 volumes (hourglass conv1 / conv3 and the adjoint of conv5 / conv6, stackhourglass.py:13-29): the 8x32 tile's halo is
  // 17 x 72 rows per depth tap — 78 KB single-buffered, one workgroup per CU, staging and arithmetic in turn (0.26 PFLOP/s);
  // the 4x16 tile's 9 x 40 rows double-buffer and leave room for a second workgroup
  if (g.stride == 2 && g.kd > 1 && !dg.conv_big && dg.tune_s2_small) d.big = false;
  if (!d.big) {
    // small feature maps (DenseNet blocks 2-4, pooled pyramids): the launch cannot fill 256 CUs with pixel tiles alone,
    // so split the output channels over more workgroups (the input tile is re-read from L2, the serial
    // chunk-by-chunk latency chain per workgroup gets shorter and more of them overlap per CU).
    const long px_blocks = (long)sdhip_cdiv(g.Ho, 4) * sdhip_cdiv(g.Wo, 16) * g.B * g.Do;
    while (bn > 32 && px_blocks * sdhip_cdiv(d.Mpad, bn) < dg.tune_split) bn >>= 1;
  }
  d.bn = bn;
  d.rows = d.Mpad < bn ? d.Mpad : bn;
  d.chunks_per_row = c.Cin <= 8 * d.V / 2 ? 4 : 8;   // the whole reduction fits one half row of 8 * V channels
  d.per_tap_any = (g.kh > 1 || g.kw > 1) && g.dil >= 4 && g.kd == 1;
  return d;
}

// Each path below holds its own predicate and the filling of its kernel's argument struct, and returns the launch's
// status or kNotTaken.  conv2d_fwd_impl calls them in order.

// ---- thin path (conv_thin.h): <= 8 input channels -> 1 output channel on the vector ALUs ----
int path_thin(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  if (!(c.plain() && c.Cout == 1 && c.Cin <= d.V && d.vec_in && g.stride == 1 && c.flat() && !c.in_scale && !c.accumulate &&
        d.T <= kThinMaxT && g.Ho == g.H + 2 * g.pad_t - g.dil * (g.kh - 1) && g.Wo == g.W + 2 * g.pad_l - g.dil * (g.kw - 1) &&
        g.pad_t >= 0 && g.pad_l >= 0 && !sdhip_diag().conv_no_thin))
    return kNotTaken;
  SDHIP_CHOSE(kFwdThin);
  ThinArgs t{};
  t.x = c.x; t.wp = c.wp; t.y = c.y; t.bias = c.bias; t.stats = c.stats;
  set_extent(t, g);
  t.kh = g.kh; t.kw = g.kw; t.dil = g.dil;
  t.Cin = c.Cin; t.ldx = c.ldx; t.ldy = c.ldy; t.Mpad = d.Mpad; t.act = c.act; t.bpg = g.B / c.groups;
  t.stats_ld = d.stats_ld; t.nrep = d.nrep; t.rep_stride = d.rep_stride;
  dim3 grid(sdhip_cdiv(g.Wo, 256), g.Ho, g.B);
  if (c.dtype == SDHIP_BF16) hipLaunchKernelGGL(conv_thin_fwd_kernel<bf16_t>, grid, dim3(256), 0, c.stream, t);
  else hipLaunchKernelGGL(conv_thin_fwd_kernel<float>, grid, dim3(256), 0, c.stream, t);
  SDHIP_LAUNCH_CHECK_AS("conv2d_fwd_impl");
  return SDHIP_OK;
}

// ---- 16..64 input channels into ONE output map (conv_thin.h): taps as the MFMA rows, fixed-order sum over taps ----
int path_fanin(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  if (!(c.plain() && c.dtype == SDHIP_BF16 && fanin_ok(c.Cin, c.Cout, g.kh, g.kw, g.stride, g.dil, g.kd, g.sd, c.ldx, c.x) && !c.in_scale &&
        !c.accumulate && !c.stats && (long)g.H * g.W * c.ldx < (1L << 31) && !sdhip_diag().conv_no_thin))
    return kNotTaken;
  FaninArgs t{};
  t.x = c.x; t.wp = c.wp; t.y = c.y; t.bias = c.bias;
  set_extent(t, g);
  t.kh = g.kh; t.kw = g.kw;
  t.D = g.D; t.Do = g.Do; t.pad_d = g.pad_d;
  t.Cin = c.Cin; t.ldx = c.ldx; t.ldy = c.ldy; t.Mpad = d.Mpad; t.act = c.act;
  t.dpw = 1; t.zsegs = g.Do; t.npxp = 0; t.pitch = 0;
  return launch_fanin(t, g.kd, c.stream);   // kNotTaken: not launchable (LDS / grid limits) -> the kernels below
}

// ---- one input channel fanned out to <= 64 output channels (conv_thin.h): taps as the MFMA reduction axis ----
int path_fanout(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  if (!(c.plain() && c.dtype == SDHIP_BF16 && fanout_ok(c.Cin, c.Cout, d.T, g.stride, g.kd, g.sd, c.ldy, c.y) && !c.in_scale &&
        !c.accumulate && !c.stats && !c.bias && c.act == 0 && (g.kh - 1) * g.dil <= 31 && (g.kw - 1) * g.dil <= 31 &&
        (long)sdhip_cdiv(g.Ho, 8) * sdhip_cdiv(g.Wo, 32) < (1L << 31) && g.B <= 65535 && !sdhip_diag().conv_no_thin))
    return kNotTaken;
  FanArgs t{};
  t.x = c.x; t.wp = c.wp; t.y = c.y;
  set_extent(t, g);
  t.kh = g.kh; t.kw = g.kw; t.dil = g.dil;
  t.ldx = c.ldx; t.Cout = c.Cout; t.Mpad = d.Mpad; t.ldy = c.ldy;
  t.D = g.D; t.Do = g.Do; t.kd = g.kd; t.pad_d = g.pad_d; t.dpw = 1; t.zsegs = g.Do;
  return launch_fanout(t, c.stream);
}

// ---- 1x1 as a streaming GEMM (conv_gemm.h): bf16, plain stride-1 1x1 over whole images ----
int path_gemm(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const SdhipDiag& dg = sdhip_diag();
  if (!(c.plain() && c.dtype == SDHIP_BF16 && g.kh == 1 && g.kw == 1 && c.flat() && g.stride == 1 && g.pad_t == 0 && g.pad_l == 0 &&
        g.Ho == g.H && g.Wo == g.W && !c.accumulate && !dg.conv_generic && !dg.conv_no_gemm))
    return kNotTaken;
  GemmArgs a{};
  a.seg[0] = GemmSeg{c.x, c.ldx, c.Cin, 0};
  a.seg[1] = GemmSeg{nullptr, 0, 0, 0};
  a.nseg = 1;
  a.wp = c.wp; a.y = c.y; a.bias = c.bias; a.in_scale = c.in_scale; a.in_shift = c.in_shift; a.stats = c.stats;
  a.ldy = c.ldy; a.Cout = c.Cout; a.Mpad = d.Mpad; a.K = c.Cin; a.in_relu = c.in_relu; a.act = c.act;
  a.M = (long)g.B * g.H * g.W; a.H = g.H; a.W = g.W; a.ppg = a.M / c.groups;
  a.stats_ld = d.stats_ld; a.nrep = d.nrep; a.rep_stride = d.rep_stride;
  if (!gemm1x1_ok(a, (c.in_scale || c.stats) ? c.groups : 1)) return kNotTaken;
  // launch_gemm's own decline (the prologue table does not fit LDS) cannot fire behind gemm1x1_ok: K <= 1024 with a prologue
  static_assert(gemm_lds_bytes(128, 3, 1024 / 64, true) <= 160 * 1024 && gemm_lds_bytes(128, 3, 4096 / 64, false) <= 160 * 1024, "gemm1x1_ok bounds the LDS of every launch");
  SDHIP_CHOSE(kFwdGemm);
  return launch_gemm_any(a, c.stream);
}

// ---- persistent whole-CU kernel (conv_band.h), bf16, weights resident in LDS.  What its 2-D and 3-D forms share: ----
bool band_common_ok(const ConvCall& c) {
  const ConvGeom& g = c.g;
  // BatchNorm-backward sums (bx, mode 0): an epilogue of the 2-D form (conv_band_bx_kernel); the one launch that takes an addend
  // AND statistics — they are sums over the stored y, addend included.  SDHIP_CONV_NO_BAND_BX sends such calls on (A/B, tests)
  const bool bx_ok = !c.bx || (c.bx_mode == 0 && c.flat() && c.stats && !c.accumulate && !c.bias && c.act == 0 && c.Cout % 4 == 0 &&
                               c.ldbx % 8 == 0 && ((uintptr_t)c.bx & 15) == 0 && !sdhip_diag().conv_no_band_bx);
  return !c.ps && bx_ok && c.omul == 1 && c.dtype == SDHIP_BF16 && g.stride == 1 && g.dil == 1 && !c.in_scale &&
         !((c.accumulate || c.addend) && c.stats && !c.bx) && !(c.accumulate && c.addend) &&
         (!c.addend || (c.ldadd % 8 == 0 && ((uintptr_t)c.addend & 15) == 0)) && c.Cin % 8 == 0 &&
         c.ldx % 8 == 0 && ((uintptr_t)c.x & 15) == 0 && c.ldy % 8 == 0 && ((uintptr_t)c.y & 15) == 0 &&
         (long)g.B * g.D * g.H * g.W * c.ldx * 2 < (long)kBandOob && band_ok(sdhip_cdiv(g.Ho, 16) * sdhip_cdiv(g.Wo, 32) * g.B * g.Do) &&
         !sdhip_diag().conv_generic && !sdhip_diag().conv_no_band;
}

BandArgs band_args(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  BandArgs f{};
  f.x = c.x; f.wp = c.wp; f.y = c.y; f.bias = c.bias; f.stats = c.stats;
  set_extent(f, g);
  f.D = g.D; f.Do = g.Do; f.pad_d = g.pad_d;
  f.Cin = c.Cin; f.ldx = c.ldx; f.Cout = c.Cout; f.Mpad = d.Mpad; f.ldy = c.ldy;
  f.bpg = (g.B / c.groups) * g.Do; f.act = c.act; f.stats_ld = d.stats_ld; f.nrep = d.nrep; f.rep_stride = d.rep_stride;
  f.res = c.addend ? c.addend : (c.accumulate ? c.y : nullptr); f.ldres = c.addend ? c.ldadd : c.ldy;
  return f;
}

// the full-resolution 5x5 layers (<= 64 channels either side) and the 3x3 layers with <= 32 input channels
int path_band2d(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const bool band5 = g.kh == 5 && g.kw == 5 && (c.Cin <= 32 || c.Cin == 64);
  const bool band3 = g.kh == 3 && g.kw == 3 && c.Cin <= 32 && !sdhip_diag().conv_no_band3;
  if (!((band5 || band3) && c.flat() && d.Mpad <= 64 && d.Mpad >= 32 && band_common_ok(c))) return kNotTaken;
  if (c.bx && !band_bx_form_ok(g.kh, d.Mpad, c.addend != nullptr)) return kNotTaken;
  if (c.bx) {
    BandBxArgs f{};
    static_cast<BandArgs&>(f) = band_args(c, d);
    f.pad_d = 0;
    f.bx = c.bx; f.bsc = c.bsc; f.bsh = c.bsh; f.ldbx = c.ldbx;
    return band5 ? launch_band_bx<5>(f, c.stream) : launch_band_bx<3>(f, c.stream);
  }
  SDHIP_CHOSE(kFwdBand, g.kh, 1, 0);
  BandArgs f = band_args(c, d);
  f.pad_d = 0;   // no depth axis: whatever the caller passed for it
  return band5 ? launch_band<5>(f, c.stream) : launch_band<3>(f, c.stream);
}

// the same kernel over volumes: 3x3x3, <= 32 channels on both sides (PSMNet's 32 -> 32 stack, stackhourglass.py:59-102):
// every depth tap is a chunk of its tile (its own input slice and 3x3 weights), z runs fastest over a workgroup's tiles
int path_band3d(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  if (!(g.kh == 3 && g.kw == 3 && g.kd == 3 && g.sd == 1 && c.Cin <= 32 && d.Mpad == 32 && !c.bx && band_common_ok(c) && !sdhip_diag().conv_no_band3))
    return kNotTaken;
  SDHIP_CHOSE(kFwdBand, 3, 3, 0);
  BandArgs f = band_args(c, d);
  return launch_band<3, 3>(f, c.stream);
}

// ---- pointwise split-K kernel (conv_point.h): bf16 1x1 with an input prologue (given, or the consumer-side BatchNorm
//      finalize) over >= 128 channels on the small maps where the tower is a latency chain (<= 32768 pixels, the
//      TUNE_PRO_MAX_PIX range of densenet.py).  The rest of the predicate is what was measured (tools/gpu_conv1x1_small.py,
//      16 images): dense blocks 3 and 4 (16x32 and 8x16 maps, 512 and 128 workgroups) are faster on it; block 2 and
//      transition 2 (32x64 maps, 2048 and 4096 workgroups) and transition 3 (512 output channels: the pixel tile is re-read
//      once per 32 of them) are bound by load throughput, not latency, and faster on the halo-tile kernel.  So: maps of at
//      most kPointMaxMap pixels, a grid that is resident at once (<= 2 workgroups on each of 256 CUs), <= 256 outputs.
//      A given prologue WITHOUT a statistics epilogue is an inference call: it keeps the halo-tile kernel, whose summation
//      order the eval-mode goldens were checked against (two of their caps sit within one change of f32 summation order) ----
int path_point(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const SdhipDiag& dg = sdhip_diag();
  if (!(c.dtype == SDHIP_BF16 && !c.bx && !c.addend && c.omul == 1 && (c.ps || (c.in_scale && c.stats)) && !c.bias && c.act == 0 && !c.accumulate &&
        g.kh == 1 && g.kw == 1 && c.flat() && g.stride == 1 && g.pad_t == 0 && g.pad_l == 0 && g.Ho == g.H && g.Wo == g.W &&
        c.Cin >= 128 && c.Cin <= kPinMaxC && c.Cin % 8 == 0 && c.Cout % kPointBN == 0 && c.Cout <= 256 && (long)g.B * g.H * g.W <= 32768 && (long)g.H * g.W <= kPointMaxMap &&
        (long)g.B * sdhip_cdiv((long)g.H * g.W, kPointPix) * (c.Cout / kPointBN) <= kPointMaxWG &&
        d.vec_in && d.vec_out && (long)g.H * g.W * c.ldx < (1L << 31) && !dg.conv_generic && !dg.conv_no_point))
    return kNotTaken;
  SDHIP_CHOSE(kFwdPoint);
  PointArgs f{};
  f.x = c.x; f.wp = c.wp; f.y = c.y; f.in_scale = c.in_scale; f.in_shift = c.in_shift; f.stats = c.stats;
  f.HW = g.H * g.W; f.Cin = c.Cin; f.ldx = c.ldx; f.Cout = c.Cout; f.Mpad = d.Mpad; f.ldy = c.ldy;
  f.in_relu = c.in_relu; f.bpg = g.B / c.groups;
  f.stats_ld = d.stats_ld; f.nrep = d.nrep; f.rep_stride = d.rep_stride;
  set_pin(f, c);
  return launch_point(f, g.B, c.stream);
}

// ---- 3x3 split-K kernel (conv_grow.h): bf16 3x3 / stride 1 / pad 1 with an input prologue (given together with a
//      statistics epilogue, or the consumer-side BatchNorm finalize) from 64 .. 256 channels into exactly 32: the conv2 of
//      the DenseNet dense layers.  The map and grid limits are what was measured (tools/gpu_conv3x3_small.py, 16 images):
//      see kGrowMaxMap / kGrowMaxWG and DESIGN.md §4.  A given prologue WITHOUT a statistics epilogue is an inference call
//      and keeps the halo-tile kernel, for the reason written above path_point ----
int path_grow(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const SdhipDiag& dg = sdhip_diag();
  if (!(c.dtype == SDHIP_BF16 && !c.bx && !c.addend && c.omul == 1 && (c.ps || (c.in_scale && c.stats)) && !c.bias && c.act == 0 && !c.accumulate &&
        g.kh == 3 && g.kw == 3 && c.flat() && g.stride == 1 && g.dil == 1 && g.pad_t == 1 && g.pad_l == 1 && g.Ho == g.H && g.Wo == g.W &&
        c.Cin % 32 == 0 && c.Cin >= 64 && c.Cin <= 256 && c.Cout == kGrowBN && (long)g.H * g.W <= kGrowMaxMap &&
        (long)g.B * sdhip_cdiv(g.H, kGrowTH) * sdhip_cdiv(g.W, kGrowTW) <= kGrowMaxWG &&
        d.vec_in && d.vec_out && (long)g.H * g.W * c.ldx < (1L << 31) && !dg.conv_generic && !dg.conv_no_grow))
    return kNotTaken;
  SDHIP_CHOSE(kFwdGrow);
  GrowArgs f{};
  f.x = c.x; f.wp = c.wp; f.y = c.y; f.in_scale = c.in_scale; f.in_shift = c.in_shift; f.stats = c.stats;
  f.H = g.H; f.W = g.W; f.Cin = c.Cin; f.ldx = c.ldx; f.ldy = c.ldy; f.tiles_w = sdhip_cdiv(g.W, kGrowTW);
  f.in_relu = c.in_relu; f.bpg = g.B / c.groups;
  f.stats_ld = d.stats_ld; f.nrep = d.nrep; f.rep_stride = d.rep_stride;
  set_pin(f, c);
  return launch_grow(f, g.B, c.stream);
}

// ---- whole-weight-set kernel (conv_mid.h): bf16 3x3 / stride 1 / pad 1, 64 -> 64, no prologue, bias, activation or
//      accumulation: the decoder blocks on the 1/4-resolution maps, forward (plain or with the statistics epilogue) and data
//      gradient (the BatchNorm-backward epilogue of sdhip_conv2d_fwd_bnbwd mode 0, with or without its addend).  Same y bits
//      as the halo-tile kernel.  The map and grid limits are what was measured faster (tools/gpu_conv3x3_mid.py, 8 images):
//      see kMidMinMap / kMidMaxMap / kMidMaxWG and DESIGN.md section 4; SDHIP_TUNE_MID_* replace them (tests) ----
int path_mid(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const SdhipDiag& dg = sdhip_diag();
  const long min_map = dg.tune_mid_min_map > 0 ? dg.tune_mid_min_map : kMidMinMap, max_map = dg.tune_mid_max_map > 0 ? dg.tune_mid_max_map : kMidMaxMap;
  const long max_wg = dg.tune_mid_max_wg > 0 ? dg.tune_mid_max_wg : kMidMaxWG;
  if (!(c.dtype == SDHIP_BF16 && g.kh == 3 && g.kw == 3 && c.flat() && g.stride == 1 && g.dil == 1 && g.pad_t == 1 && g.pad_l == 1 &&
        g.Ho == g.H && g.Wo == g.W && c.Cin == kMidBN && c.Cout == kMidBN && !c.in_scale && !c.ps && !c.bias && c.act == 0 && !c.accumulate &&
        c.omul == 1 && (c.bx ? c.bx_mode == 0 : !c.addend) && (long)g.H * g.W >= min_map && (long)g.H * g.W <= max_map &&
        (long)g.B * sdhip_cdiv(g.H, kMidTH) * sdhip_cdiv(g.W, kMidTW) <= max_wg &&
        d.vec_in && d.vec_out && (long)g.H * g.W * c.ldx < (1L << 31) && !dg.conv_generic && !dg.conv_no_mid))
    return kNotTaken;
  SDHIP_CHOSE(kFwdMid);
  MidArgs f{};
  f.x = c.x; f.wp = c.wp; f.y = c.y; f.stats = c.stats;
  f.H = g.H; f.W = g.W; f.ldx = c.ldx; f.ldy = c.ldy; f.tiles_w = sdhip_cdiv(g.W, kMidTW);
  f.bpg = g.B / c.groups;
  f.stats_ld = d.stats_ld; f.nrep = d.nrep; f.rep_stride = d.rep_stride;
  f.bx = c.bx; f.bsc = c.bsc; f.bsh = c.bsh; f.ldbx = c.ldbx;
  f.res = c.bx ? c.addend : nullptr; f.ldres = c.ldadd;
  return launch_mid(f, g.B, c.stream);
}

// ---- fast path (conv_fast.h): 16-byte-aligned pixels on both sides, halo-tile mode.  It takes every variant (phase
//      output, BatchNorm-backward epilogue, consumer-side BatchNorm finalize) ----
int path_fast(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  if (!(!d.per_tap_any && d.vec_in && d.vec_out && (long)g.H * g.W * c.ldx < (1L << 31) && !sdhip_diag().conv_generic)) return kNotTaken;
  const int tune_ksoft_small = 80, tune_ksoft_big = 80;
  const int CKh = 8 * d.V, T = d.T, bn = d.bn;
  const int ks = d.chunks_per_row == 4 ? 1 : 2;
  const int rb = 64 * ks, px_per_round = 256 / (4 * ks);
  FastArgs f{};
  f.x = c.x; f.wp = c.wp; f.y = c.y; f.bias = c.bias; f.in_scale = c.in_scale; f.in_shift = c.in_shift; f.stats = c.stats;
  set_extent(f, g);
  f.kh = g.kh; f.kw = g.kw; f.stride = g.stride; f.dil = g.dil;
  f.D = g.D; f.Do = g.Do; f.kd = g.kd; f.sd = g.sd; f.pad_d = g.pad_d;
  f.Cin = c.Cin; f.ldx = c.ldx; f.Cout = c.Cout; f.Mpad = d.Mpad; f.ldy = c.ldy;
  f.in_relu = c.in_relu; f.bpg = g.B / c.groups; f.act = c.act; f.accumulate = c.accumulate;
  f.stats_ld = d.stats_ld; f.nrep = d.nrep; f.rep_stride = d.rep_stride; f.tail = (c.Cin % d.V) != 0;
  f.omul = c.omul; f.ooz = c.ooz; f.ooy = c.ooy; f.oox = c.oox;
  f.bx = c.bx; f.ldbx = c.ldbx; f.bsc = c.bsc; f.bsh = c.bsh;
  f.res = c.bx ? c.addend : nullptr; f.ldres = c.ldadd; f.bx_mode = c.bx_mode; f.bx_groups = c.groups;
  f.dma = !c.in_scale && !f.tail && !c.ps;
  set_pin(f, c);
  bool fbig = d.big;   // this path's own copy: the generic path starts from d.big again
  for (int attempt = 0; attempt < 2; ++attempt) {
    const int th = fbig ? 8 : 4, tw = fbig ? 32 : 16;
    const int IH = (th - 1) * g.stride + (g.kh - 1) * g.dil + 1, IW = (tw - 1) * g.stride + (g.kw - 1) * g.dil + 1;
    const int IWp = (IW + 7) & ~7;
    const int hrows = ((IH * IWp + px_per_round - 1) / px_per_round) * px_per_round;   // whole load rounds
    const int nqq_f = g.kd * (ks == 2 ? sdhip_cdiv(c.Cin, CKh) : 1);
    const size_t hb = (size_t)hrows * rb * ((fbig || nqq_f == 1) ? 1 : 2);   // small tiles double-buffer the halo across chunks
    if (!fbig && hrows > ((f.dma && ks == 1) ? 6 : 5) * px_per_round) { fbig = true; continue; }   // small-tile halo prefetch plan: 5 / 6 rounds (conv_fast.h HPF)
    auto wbuf = [&](int tgv) { return (size_t)(((tgv * bn + px_per_round - 1) / px_per_round) * px_per_round) * rb; };
    int tg = T;
    const size_t ksoft_f = (size_t)(fbig ? tune_ksoft_big : tune_ksoft_small) * 1024;
    size_t lds;
    if (nqq_f == 1 && hb + wbuf(T) <= ksoft_f) {
      lds = hb + wbuf(T);              // the whole kernel is ONE stage: all taps resident, no second weight buffer
    } else {
      while (tg > 1 && hb + 2 * wbuf(tg) > ksoft_f) --tg;
      lds = hb + 2 * wbuf(tg);
    }
    if (lds < 4096) lds = 4096;
    f.pin_off = 0; f.pin_cs = 0;
    if (c.ps) { f.pin_off = (int)lds; f.pin_cs = (c.Cin + 63) & ~63; lds += 2 * (size_t)f.pin_cs * sizeof(float); }   // the finalize table sits behind everything else
    if (lds > kLdsMax) { if (!fbig) break; fbig = false; continue; }
    f.tg = tg;
    f.magic_iwp = IWp > 1 ? (unsigned)(0x100000000ULL / (unsigned)IWp) + 1u : 0u;
    f.tiles_w = sdhip_cdiv(g.Wo, tw);
    f.magic_tw = f.tiles_w > 1 ? (unsigned)(0x100000000ULL / (unsigned)f.tiles_w) + 1u : 0u;
    f.ntg = sdhip_cdiv(T, tg);
    if ((long)f.tiles_w * sdhip_cdiv(g.Ho, th) >= 65536) break;   // fast_div range: general kernel for gigantic images
    return c.dtype == SDHIP_BF16 ? launch_fast_any<bf16_t>(f, fbig, ks, bn, lds, c.stream) : launch_fast_any<float>(f, fbig, ks, bn, lds, c.stream);
  }
  return kNotTaken;
}

// ---- general kernel (this file): any layout, per-tap mode for strongly dilated kernels.  The last path: never kNotTaken ----
int path_generic(const ConvCall& c, const ConvPlan& d) {
  const ConvGeom& g = c.g;
  const int bn = d.bn;
  FwdArgs a{};
  a.x = c.x; a.wp = c.wp; a.y = c.y; a.bias = c.bias; a.in_scale = c.in_scale; a.in_shift = c.in_shift; a.stats = c.stats;
  a.g = g;
  a.Cin = c.Cin; a.ldx = c.ldx; a.Cout = c.Cout; a.Mpad = d.Mpad; a.ldy = c.ldy;
  a.in_relu = c.in_relu; a.groups = c.groups; a.act = c.act; a.accumulate = c.accumulate;
  a.vec_in = d.vec_in; a.vec_out = d.vec_out;
  a.stats_ld = d.stats_ld; a.nrep = d.nrep; a.rep_stride = d.rep_stride;
  bool big = d.big;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const int th = big ? 8 : 4, tw = big ? 32 : 16;
    const int per_tap = d.per_tap_any;   // halo would be >= 4x the tile in each direction's holes
    const size_t halo = halo_bytes_of(g, th, tw, per_tap);
    const long halo_loads = (long)(halo / 128) * d.chunks_per_row;
    // register-prefetched (double-buffered) halo: small tiles, at most 4 loads per lane, vector loads only
    const int pf = !per_tap && !big && d.vec_in && (c.Cin % d.V == 0) && halo_loads <= 4 * 256 && 2 * halo + 2 * (size_t)bn * 128 <= kLdsSoft;
    // weights: at most 4 loads per lane per stage => tg*rows*chunks_per_row <= 1024
    int tg = per_tap ? 1 : 1024 / (d.rows * d.chunks_per_row);
    if (tg < 1) tg = 1;
    if (tg > d.T) tg = d.T;
    const size_t hb = halo * (pf ? 2 : 1);
    while (tg > 1 && hb + 2 * (size_t)tg * bn * 128 > kLdsSoft) --tg;
    size_t lds = hb + 2 * (size_t)tg * bn * 128;
    if (lds < 4096) lds = 4096;   // stats reduction scratch
    if (lds > kLdsMax) {
      if (big) { big = false; continue; }
      SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd: halo tile of a %dx%d kernel with dilation %d does not fit LDS", g.kh, g.kw, g.dil);
    }
    a.tg = tg; a.pf_halo = pf; a.sh = d.chunks_per_row == 4 ? 2 : 3; a.per_tap = per_tap;
    if (c.dtype == SDHIP_BF16)
      return big ? launch_bn<bf16_t, 8, 32>(a, bn, lds, c.stream) : launch_bn<bf16_t, 4, 16>(a, bn, lds, c.stream);
    return big ? launch_bn<float, 8, 32>(a, bn, lds, c.stream) : launch_bn<float, 4, 16>(a, bn, lds, c.stream);
  }
  SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd: no tile configuration fits");
}

int conv2d_fwd_dispatch(const ConvCall& c) {
  const ConvGeom& g = c.g;
  SDHIP_CHECK_ARG(c.x && c.wp && c.y, "conv2d_fwd: null pointer");
  SDHIP_CHECK_ARG(c.dtype == SDHIP_F32 || c.dtype == SDHIP_BF16, "conv2d_fwd: unknown dtype %d", c.dtype);
  SDHIP_CHECK_ARG(g.B > 0 && g.H > 0 && g.W > 0 && c.Cin > 0 && c.Cout > 0 && g.Ho > 0 && g.Wo > 0, "conv2d_fwd: empty tensor");
  SDHIP_CHECK_ARG(c.ldx >= c.Cin && c.ldy >= c.Cout, "conv2d_fwd: pixel stride smaller than channel count");
  SDHIP_CHECK_ARG(g.kh >= 1 && g.kw >= 1 && g.stride >= 1 && g.dil >= 1, "conv2d_fwd: bad kernel geometry");
  SDHIP_CHECK_ARG(c.groups >= 1 && g.B % c.groups == 0, "conv2d_fwd: batch %d not divisible by %d stat groups", g.B, c.groups);
  SDHIP_CHECK_ARG((c.in_scale == nullptr) == (c.in_shift == nullptr), "conv2d_fwd: in_scale/in_shift must come together");
  SDHIP_CHECK_ARG(((uintptr_t)c.wp & 15) == 0, "conv2d_fwd: packed weights must be 16-byte aligned");
  SDHIP_CHECK_ARG(g.D >= 1 && g.Do >= 1 && g.kd >= 1 && g.sd >= 1 && (long)g.B * g.Do <= 65535, "conv2d_fwd: bad depth geometry");
  const ConvPlan d = conv_plan(c);
  int rc;
  for (auto path : {path_thin, path_fanin, path_fanout, path_gemm, path_band2d, path_band3d})
    if ((rc = path(c, d)) != kNotTaken) return rc;
  if (c.addend && !c.bx) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd_add: only the persistent 5x5 kernel adds a second tensor in its epilogue (bf16, <= 64 channels, >= 192 tiles of 16x32)");
  if ((rc = path_point(c, d)) != kNotTaken) return rc;
  if ((rc = path_grow(c, d)) != kNotTaken) return rc;
  if ((rc = path_mid(c, d)) != kNotTaken) return rc;
  if ((rc = path_fast(c, d)) != kNotTaken) return rc;
  if (c.omul != 1) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd_phase: interleaved output needs the aligned fast path (ldx %% 8, ldy %% 4)");
  if (c.ps) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd_bnpro: needs the aligned fast path (ldx %% 8, ldy %% 4, halo tile within LDS)");
  if (c.bx) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd_bnbwd: needs the aligned fast path (ldx %% 8, ldy %% 4, halo tile within LDS)");
  return path_generic(c, d);
}

int conv2d_fwd_impl(const ConvCall& c) {
  return sdhip_path_exit(conv2d_fwd_dispatch(c));
}

}  // namespace

// 1x1 convolution over the channel concatenation of up to two tensors, either of which may be a nearest-neighbour
// upsampled map (see include/sdhip.h).  bf16 only: the f32 parity path materialises the concatenation.
extern "C" int sdhip_conv1x1_cat_fwd(const void* x0, int ld0, int c0, int us0, const void* x1, int ld1, int c1, int us1,
                                     const void* wpacked, void* y, int ldy, const float* bias,
                                     int B, int H, int W, int Cout, int act, int dtype, void* stream) {
  SDHIP_CHECK_ARG(x0 && wpacked && y && c0 > 0 && B > 0 && H > 0 && W > 0 && Cout > 0, "conv1x1_cat_fwd: bad arguments");
  SDHIP_CHECK_ARG(dtype == SDHIP_BF16, "conv1x1_cat_fwd: bf16 only");
  SDHIP_CHECK_ARG((x1 == nullptr) == (c1 == 0) && us0 >= 0 && us1 >= 0 && us0 < 8 && us1 < 8, "conv1x1_cat_fwd: bad second segment");
  GemmArgs g{};
  g.seg[0] = GemmSeg{x0, ld0, c0, us0};
  g.seg[1] = GemmSeg{x1, ld1, c1, us1};
  g.nseg = x1 ? 2 : 1;
  g.wp = wpacked; g.y = y; g.bias = bias;
  g.ldy = ldy; g.Cout = Cout; g.Mpad = (Cout + 15) & ~15; g.K = c0 + c1; g.act = act;
  g.M = (long)B * H * W; g.H = H; g.W = W; g.ppg = g.M;
  g.stats_ld = Cout; g.nrep = 1; g.rep_stride = 0;
  if (!gemm1x1_ok(g, 1, true)) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv1x1_cat_fwd: operands not 16-byte aligned / grid not divisible by the upsampling factor");
  return launch_gemm_any(g, (hipStream_t)stream);
}

extern "C" int sdhip_conv2d_fwd(const void* x, const void* wpacked, void* y,
                                const float* bias, const float* in_scale, const float* in_shift,
                                double* stats, int stats_ld, int stats_nrep,
                                int B, int H, int W, int Cin, int ldx,
                                int Ho, int Wo, int Cout, int ldy,
                                int kh, int kw, int stride, int dil, int pad_t, int pad_l,
                                int D, int Do, int kd, int sd, int pad_d,
                                int in_relu, int groups, int act, int accumulate,
                                int dtype, void* stream) {
  sdhip_path_enter();
  ConvCall c = conv_call(x, wpacked, y, ConvGeom{B, H, W, Ho, Wo, kh, kw, stride, dil, pad_t, pad_l, D, Do, kd, sd, pad_d},
                         Cin, ldx, Cout, ldy, dtype, stream);
  c.bias = bias; c.in_scale = in_scale; c.in_shift = in_shift;
  c.stats = stats; c.stats_ld = stats_ld; c.stats_nrep = stats_nrep;
  c.in_relu = in_relu; c.groups = groups; c.act = act; c.accumulate = accumulate;
  return conv2d_fwd_impl(c);
}

// y = conv(relu(BatchNorm_train(x))) with the BatchNorm finalized inside the launch (see include/sdhip.h).
extern "C" int sdhip_conv2d_fwd_bnpro(const void* x, const void* wpacked, void* y, double* out_stats, int out_stats_ld, int out_stats_nrep,
                                      double* in_stats, int in_stats_ld, int in_stats_nrep,
                                      const double* pend_stats, int pend_ld, int pend_nrep, int pend_c0, int pend_n,
                                      const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float* scale_out, float* shift_out, float* mean_out,
                                      float* invstd_out, double count, float eps, float momentum,
                                      int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                                      int kh, int kw, int pad_t, int pad_l, int groups, int dtype, void* stream) {
  sdhip_path_enter();
  SDHIP_CHECK_ARG(in_stats && scale_out && shift_out && mean_out && invstd_out && count >= 1. && in_stats_nrep >= 1 && in_stats_ld >= Cin,
                  "conv2d_fwd_bnpro: statistics / output vectors missing");
  SDHIP_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "conv2d_fwd_bnpro: running_mean / running_var come together");
  if (Cin > kPinMaxC || in_stats_nrep > 4 || (pend_stats && pend_nrep > 4)) {
    sdhip_path_exit(SDHIP_ERR_UNSUPPORTED);
    SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "conv2d_fwd_bnpro: at most %d input channels and 4 statistics replicas", kPinMaxC);
  }
  SDHIP_CHECK_ARG(!pend_stats || (pend_n > 0 && pend_c0 >= 0 && pend_c0 + pend_n <= Cin && pend_ld >= pend_n && pend_nrep >= 1 && in_stats_nrep == 1),
                  "conv2d_fwd_bnpro: bad pending-statistics slice (folding needs single-replica slab statistics)");
  ProStats ps{in_stats, in_stats_ld, in_stats_nrep, gamma, beta, scale_out, shift_out, mean_out, invstd_out, running_mean, running_var,
              eps, momentum, count, pend_stats, in_stats, pend_ld, pend_nrep, pend_c0, pend_n};
  ConvCall c = conv_call(x, wpacked, y, geom2d(B, H, W, Ho, Wo, kh, kw, 1, 1, pad_t, pad_l), Cin, ldx, Cout, ldy, dtype, stream);
  c.stats = out_stats; c.stats_ld = out_stats_ld; c.stats_nrep = out_stats_nrep;
  c.in_relu = 1; c.groups = groups;
  c.ps = &ps;
  return conv2d_fwd_impl(c);
}

// y = conv(x) + addend (see include/sdhip.h).
extern "C" int sdhip_conv2d_fwd_add(const void* x, const void* wpacked, void* y, const void* addend, int ldadd,
                                    int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                                    int kh, int kw, int pad_t, int pad_l, int dtype, void* stream) {
  sdhip_path_enter();
  SDHIP_CHECK_ARG(addend && ldadd >= Cout, "conv2d_fwd_add: addend missing / pixel stride smaller than Cout");
  ConvCall c = conv_call(x, wpacked, y, geom2d(B, H, W, Ho, Wo, kh, kw, 1, 1, pad_t, pad_l), Cin, ldx, Cout, ldy, dtype, stream);
  c.addend = addend; c.ldadd = ldadd;
  return conv2d_fwd_impl(c);
}

// Data gradient of a stride-1 convolution whose input was relu(BatchNorm(u)): y = the gradient w.r.t. that input, and the
// epilogue also takes the two reductions of the BatchNorm backward over it (see include/sdhip.h).
extern "C" int sdhip_conv2d_fwd_bnbwd(const void* x, const void* wpacked, void* y, double* sums, int sums_ld, int sums_nrep,
                                      const void* u, int ldu, const float* scale, const float* shift, const void* addend, int ldadd,
                                      int B, int H, int W, int Cin, int ldx, int Ho, int Wo, int Cout, int ldy,
                                      int kh, int kw, int dil, int pad_t, int pad_l, int groups, int mode, int dtype, void* stream) {
  sdhip_path_enter();
  SDHIP_CHECK_ARG(mode == 0 || (mode == 1 && addend), "conv2d_fwd_bnbwd: mode 1 (apply) needs the tensor the result is added to");
  SDHIP_CHECK_ARG(dtype == SDHIP_BF16, "conv2d_fwd_bnbwd: bf16 only");
  SDHIP_CHECK_ARG(sums && u && scale && shift && ldu >= Cout && Cout % 4 == 0 && ldu % 4 == 0 && ((uintptr_t)u & 7) == 0 &&
                  ((uintptr_t)scale & 15) == 0 && ((uintptr_t)shift & 15) == 0,
                  "conv2d_fwd_bnbwd: sums / u / scale / shift missing or misaligned (Cout %% 4, ldu %% 4)");
  SDHIP_CHECK_ARG(!addend || (ldadd >= Cout && ldadd % 4 == 0 && ((uintptr_t)addend & 7) == 0), "conv2d_fwd_bnbwd: addend misaligned");
  ConvCall c = conv_call(x, wpacked, y, geom2d(B, H, W, Ho, Wo, kh, kw, 1, dil, pad_t, pad_l), Cin, ldx, Cout, ldy, dtype, stream);
  c.stats = sums; c.stats_ld = sums_ld; c.stats_nrep = sums_nrep;
  c.groups = groups;
  c.bx = u; c.ldbx = ldu; c.bsc = scale; c.bsh = shift; c.bx_mode = mode;
  c.addend = addend; c.ldadd = ldadd;
  return conv2d_fwd_impl(c);
}

// One sub-pixel phase of a stride-2 transposed convolution (see include/sdhip.h): a stride-1 correlation whose outputs are
// written to every second voxel of a volume twice as large in each of depth / height / width.
extern "C" int sdhip_conv2d_fwd_phase(const void* x, const void* wpacked, void* y, double* stats, int stats_ld, int stats_nrep,
                                      int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int kh, int kw,
                                      int D, int kd, int groups, int off_d, int off_h, int off_w, int dtype, void* stream) {
  sdhip_path_enter();
  SDHIP_CHECK_ARG(off_d >= 0 && off_d < 2 && off_h >= 0 && off_h < 2 && off_w >= 0 && off_w < 2, "conv2d_fwd_phase: phase offsets are 0 or 1");
  ConvCall c = conv_call(x, wpacked, y, ConvGeom{B, H, W, H, W, kh, kw, 1, 1, 0, 0, D, D, kd, 1, 0}, Cin, ldx, Cout, ldy, dtype, stream);
  c.stats = stats; c.stats_ld = stats_ld; c.stats_nrep = stats_nrep;
  c.groups = groups;
  c.omul = 2; c.ooz = off_d; c.ooy = off_h; c.oox = off_w;
  return conv2d_fwd_impl(c);
}

