// The pooled pyramids of piramidNet2 (models/dsnet_t2.py:2037-2081) for gfx950:
//   cat([x] + [bilinear_up(map_j) for j]) written as ONE slab by one launch, and the gradients of all maps by two.
// The arithmetic is that of resample.hip's resize_fwd / resize_bwd_axis (resample_common.h holds what the two files share);
// what changes is who writes what: a thread owns a 16-byte unit of a slab row, consecutive threads own consecutive units of
// the same pixel, so a row of the slab leaves as whole lines instead of 64-byte pieces of six separate launches.
// The branch tables travel by value in the kernel arguments (<= kPyrMax entries): nothing is copied to the device, a
// captured step stays a chain of kernel nodes.
#include "resample_common.h"

namespace {

constexpr int kPyrMax = 8;

// table lookup by a lane-dependent index: selects over kernel-argument values instead of an indexed (scratch) array
template <typename V>
__device__ __forceinline__ V pick(const V (&t)[kPyrMax], int j) {
  V v = t[0];
#pragma unroll
  for (int k = 1; k < kPyrMax; ++k) v = j == k ? t[k] : v;
  return v;
}

// r = h0l * (w0l * a + lw * b) + lh * (w0l * c + lw * d) with the roundings of resize_fwd's vector instantiations.  The slab
// has to carry the bits of resize_fwd + copies, and "the same expression" does not give them: the compiler contracts that
// expression differently per element of a unit (its packed-f32 pairing leaves the last two elements over).  In the code
// objects of resize_fwd<float, true> and resize_fwd<bf16_t, true> elements 0 .. N-3 are three fused multiply-adds
// (fma(h0l, fma(w0l, a, lw * b), lh * fma(w0l, c, lw * d))), element N-2 is not fused at all, and element N-1 fuses the
// two inner sums only.  Written out here with contraction off; tests/test_pyramid.py compares the bits.
template <int N>
__device__ __forceinline__ void blend_as_resize_fwd(const float* a, const float* b, const float* c, const float* d,
                                                    float h0l, float lh, float w0l, float lw, float* r) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < N; ++e) {
    float P, Q;
    if (e == N - 2) { P = w0l * a[e] + lw * b[e]; Q = w0l * c[e] + lw * d[e]; }
    else { P = __builtin_fmaf(w0l, a[e], lw * b[e]); Q = __builtin_fmaf(w0l, c[e], lw * d[e]); }
    r[e] = e < N - 2 ? __builtin_fmaf(h0l, P, lh * Q) : h0l * P + lh * Q;
  }
}

// ---------------------------------------------------------------- forward: y = [x | up(map_0) | ... | up(map_{n-1})]
struct UpcatMaps {
  const void* p[kPyrMax];
  int h[kPyrMax], w[kPyrMax], ld[kPyrMax];
  float sh[kPyrMax], sw[kPyrMax];        // make_axis(h, H, 1, 0).scale, make_axis(w, W, 1, 0).scale
};

template <typename T>
__global__ __launch_bounds__(256) void pyramid_upcat_fwd(const T* __restrict__ x, int ldx, T* __restrict__ y, Img out,
                                                         int C, int Cb, const UpcatMaps m) {
  using U = Unit<T, true>;
  constexpr int N = U::N;
  const int units = out.C / N, xu = C / N, bu = Cb / N;
  const long npix = (long)out.B * out.H * out.W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x;; i += (long)gridDim.x * 256) {
    long pix; int c0;
    if (!item<N>(i, npix, units, pix, c0)) break;
    const int u = c0 / N;
    float r[N];
    if (u < xu) {
      U::load(x + pix * ldx + c0, r);
    } else {
      const int j = (u - xu) / bu;
      const int cb = (u - xu - j * bu) * N;
      const int hj = pick(m.h, j), wj = pick(m.w, j), ldj = pick(m.ld, j);
      const Axis ah{hj, out.H, pick(m.sh, j), 1}, aw{wj, out.W, pick(m.sw, j), 1};
      const int ow = (int)(pix % out.W), oh = (int)((pix / out.W) % out.H);
      const long b = pix / ((long)out.W * out.H);
      const T* xb = static_cast<const T*>(pick(m.p, j)) + b * hj * wj * ldj + cb;
      int h0, h1, w0, w1; float lh, lw;
      linear_src(ah, oh, h0, h1, lh);
      linear_src(aw, ow, w0, w1, lw);
      float a[N], bb[N], c[N], d[N];
      U::load(xb + ((long)h0 * wj + w0) * ldj, a);
      U::load(xb + ((long)h0 * wj + w1) * ldj, bb);
      U::load(xb + ((long)h1 * wj + w0) * ldj, c);
      U::load(xb + ((long)h1 * wj + w1) * ldj, d);
      blend_as_resize_fwd<N>(a, bb, c, d, 1.f - lh, lh, 1.f - lw, lw, r);
    }
    U::store(y + pix * out.ld + c0, r);
  }
}

// ---------------------------------------------------------------- backward: one axis of the separable gather, all branches
// Job j is resize_bwd_axis on branch j: layout [outer][axis = in -> out][inner pixels][C], `split` lanes per item.  A
// branch owns the virtual workgroups [blk0[j], blk0[j+1]) (entries from n on hold the total), each of 256 / split items;
// the grid is capped and walks the virtual workgroups, so the branch and its split are uniform over a workgroup.
struct AxisJobs {
  const void* src[kPyrMax];
  void* dst[kPyrMax];
  long outer[kPyrMax];
  int lds[kPyrMax], ldd[kPyrMax], inner[kPyrMax], in[kPyrMax], split[kPyrMax];
  float scale[kPyrMax];
  int blk0[kPyrMax + 1];
  int out, C;
};

template <typename T, bool VEC, typename TO>
__global__ __launch_bounds__(256) void pyramid_bwd_axis(const AxisJobs J) {
  constexpr int N = Unit<T, VEC>::N;
  const int units = J.C / N;
  for (int vb = blockIdx.x; vb < J.blk0[kPyrMax]; vb += gridDim.x) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < kPyrMax; ++k) j = vb >= J.blk0[k] ? k : j;
    const Axis a{pick(J.in, j), J.out, pick(J.scale, j), 1};
    const int split = pick(J.split, j), inner = pick(J.inner, j), ldg = pick(J.lds, j), ldx = pick(J.ldd, j);
    const T* gy = static_cast<const T*>(pick(J.src, j));
    TO* gx = static_cast<TO*>(pick(J.dst, j));
    int first = J.blk0[0];
#pragma unroll
    for (int k = 1; k < kPyrMax; ++k) first = j == k ? J.blk0[k] : first;
    const long npix = pick(J.outer, j) * a.in * inner;
    const int sub = threadIdx.x & (split - 1);
    const long it = (long)(vb - first) * (256 / split) + threadIdx.x / split;
    long pix; int c0;
    if (!item<N>(it, npix, units, pix, c0)) continue;      // uniform over the lanes of an item
    const int r = (int)(pix % inner);
    const int i = (int)((pix / inner) % a.in);
    const long o = pix / ((long)inner * a.in);
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    int lo, hi;
    bwd_window(a, i, lo, hi);
    for (int d = lo + sub; d <= hi; d += split) {
      const float wgt = bwd_weight(a, d, i);
      if (wgt != 0.f) {
        float g[N];
        Unit<T, VEC>::load(gy + ((o * a.out + d) * inner + r) * ldg + c0, g);
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = fmaf(wgt, g[e], acc[e]);
      }
    }
    for (int o2 = split >> 1; o2 > 0; o2 >>= 1)
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += __shfl_xor(acc[e], o2, 64);
    if (sub != 0) continue;
    TO* dst = gx + pix * ldx + c0;
    if constexpr (sizeof(TO) == sizeof(T)) {
      Unit<T, VEC>::store(reinterpret_cast<T*>(dst), acc);
    } else {  // f32 intermediate between the two passes of a bf16 tensor
#pragma unroll
      for (int e = 0; e < N; ++e) Elem<TO>::st(dst + e, acc[e]);
    }
  }
}

// virtual workgroups of the jobs filled so far (items[j] of units-per-pixel `units`, J.split[j] lanes each); false: too many
bool plan_blocks(AxisJobs& J, int n, const long* npix, int units) {
  long total = 0;
  for (int j = 0; j <= kPyrMax; ++j) {
    J.blk0[j] = (int)total;
    if (j < n) total += (npix[j] * units + 256 / J.split[j] - 1) / (256 / J.split[j]);
    if (total > 0x7fffffffL) return false;
  }
  return true;
}

inline dim3 grid_of_blocks(int vb) { return dim3((unsigned)(vb > 4096 ? 4096 : vb < 1 ? 1 : vb)); }

int check_maps(const char* who, const SdhipPyrMap* maps, int n, int B, int H, int W, int C, int Cb, int ld, int dtype) {
  SDHIP_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && Cb > 0, "%s: bad shape B=%d H=%d W=%d C=%d Cb=%d", who, B, H, W, C, Cb);
  SDHIP_CHECK_ARG(maps && n >= 1 && n <= kPyrMax, "%s: 1..%d branch maps (got %d)", who, kPyrMax, n);
  SDHIP_CHECK_ARG((long)C + (long)n * Cb <= ld, "%s: slab stride %d is below C + n * Cb = %ld", who, ld, (long)C + (long)n * Cb);
  for (int j = 0; j < n; ++j)
    SDHIP_CHECK_ARG(maps[j].p && maps[j].h > 0 && maps[j].w > 0 && maps[j].ld >= Cb, "%s: bad map %d (h=%d w=%d ld=%d)", who, j,
                    maps[j].h, maps[j].w, maps[j].ld);
  SDHIP_CHECK_DTYPE(who, dtype);
  return 0;
}

}  // namespace

extern "C" int sdhip_pyramid_upcat_fwd(const void* x, int ldx, const SdhipPyrMap* maps, int n, void* y, int ldy,
                                       int B, int H, int W, int C, int Cb, int dtype, void* stream) {
  if (int rc = check_maps("pyramid_upcat_fwd", maps, n, B, H, W, C, Cb, ldy, dtype)) return rc;
  SDHIP_CHECK_ARG(x && y && ldx >= C, "pyramid_upcat_fwd: bad pointers");
  const int Ct = C + n * Cb;
  UpcatMaps m = UpcatMaps();
  for (int j = 0; j < n; ++j) {
    m.p[j] = maps[j].p; m.h[j] = maps[j].h; m.w[j] = maps[j].w; m.ld[j] = maps[j].ld;
    m.sh[j] = make_axis(maps[j].h, H, 1, 0.f).scale;
    m.sw[j] = make_axis(maps[j].w, W, 1, 0.f).scale;
  }
  const Img out{B, H, W, Ct, ldy};
  const long np = (long)B * H * W;
  return sdhip_by_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    constexpr int N = Chunk<T>::N;
    bool vec = Cb % N == 0 && sdhip_vec_ok<T>(C, {ldx, ldy}, {x, y});
    for (int j = 0; j < n; ++j) vec = vec && sdhip_vec_ok<T>(Cb, {maps[j].ld}, {maps[j].p});
    if (!vec) SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "pyramid_upcat_fwd: layout is not a whole number of 16-byte units");
    hipLaunchKernelGGL((pyramid_upcat_fwd<T>), grid_for(np * (Ct / N)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (T*)y,
                       out, C, Cb, m);
    SDHIP_LAUNCH_CHECK_AS("sdhip_pyramid_upcat_fwd");
    return SDHIP_OK;
  });
}

extern "C" int sdhip_pyramid_upcat_bwd(const void* gy, int ldg, const SdhipPyrMap* gmaps, int n, float* tmp,
                                       int B, int H, int W, int C, int Cb, int dtype, void* stream) {
  if (int rc = check_maps("pyramid_upcat_bwd", gmaps, n, B, H, W, C, Cb, ldg, dtype)) return rc;
  SDHIP_CHECK_ARG(gy && tmp, "pyramid_upcat_bwd: bad pointers");
  hipStream_t s = (hipStream_t)stream;
  return sdhip_by_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    constexpr bool f32 = std::is_same<T, float>::value;
    constexpr int N = Chunk<T>::N;
    if (!(Cb % N == 0 && sdhip_vec_ok<T>(C, {ldg}, {gy, tmp})))
      SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "pyramid_upcat_bwd: layout is not a whole number of 16-byte units");
    // pass 1 along W: [outer = B*H][axis = w_j][inner = 1][Cb], slab gradient in place -> f32 tmp_j (ld = Cb)
    // pass 2 along H: [outer = B][axis = h_j][inner = w_j][Cb], tmp_j -> gradient of map j
    AxisJobs J1 = AxisJobs(), J2 = AxisJobs();
    long np1[kPyrMax], np2[kPyrMax], off = 0;
    bool vec2 = f32;
    for (int j = 0; j < n; ++j) {
      const int h = gmaps[j].h, w = gmaps[j].w;
      const Axis ah = make_axis(h, H, 1, 0.f), aw = make_axis(w, W, 1, 0.f);
      J1.src[j] = (const T*)gy + C + (long)j * Cb; J1.lds[j] = ldg;
      J1.dst[j] = tmp + off; J1.ldd[j] = Cb;
      J1.outer[j] = (long)B * H; J1.inner[j] = 1; J1.in[j] = w; J1.scale[j] = aw.scale; J1.split[j] = bwd_lanes(aw);
      J2.src[j] = tmp + off; J2.lds[j] = Cb;
      J2.dst[j] = gmaps[j].p; J2.ldd[j] = gmaps[j].ld;
      J2.outer[j] = B; J2.inner[j] = w; J2.in[j] = h; J2.scale[j] = ah.scale; J2.split[j] = bwd_lanes(ah);
      np1[j] = (long)B * H * w; np2[j] = (long)B * h * w;
      off += np1[j] * Cb;
      vec2 = vec2 && sdhip_vec_ok<T>(Cb, {gmaps[j].ld}, {gmaps[j].p});
    }
    for (int j = n; j < kPyrMax; ++j) { J1.split[j] = J2.split[j] = 1; J1.inner[j] = J2.inner[j] = 1; J1.in[j] = J2.in[j] = 1; }
    J1.out = W; J2.out = H; J1.C = J2.C = Cb;
    // the second pass of a bf16 tensor reads f32 and writes bf16 with scalar units, as sdhip_resize_bwd does
    const int units2 = vec2 ? Cb / N : Cb;
    if (!plan_blocks(J1, n, np1, Cb / N) || !plan_blocks(J2, n, np2, units2))
      SDHIP_FAIL(SDHIP_ERR_UNSUPPORTED, "pyramid_upcat_bwd: too many work items");
    hipLaunchKernelGGL((pyramid_bwd_axis<T, true, float>), grid_of_blocks(J1.blk0[kPyrMax]), dim3(256), 0, s, J1);
    if constexpr (f32) {
      sdhip_by_flag(vec2, [&](auto V) {
        hipLaunchKernelGGL((pyramid_bwd_axis<float, V(), T>), grid_of_blocks(J2.blk0[kPyrMax]), dim3(256), 0, s, J2);
      });
    } else {
      hipLaunchKernelGGL((pyramid_bwd_axis<float, false, T>), grid_of_blocks(J2.blk0[kPyrMax]), dim3(256), 0, s, J2);
    }
    SDHIP_LAUNCH_CHECK_AS("sdhip_pyramid_upcat_bwd");
    return SDHIP_OK;
  });
}
