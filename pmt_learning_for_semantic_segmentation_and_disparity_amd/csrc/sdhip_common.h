// sdhip — shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels.
// Everything here is wave64 / MFMA specific; there is no other backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <initializer_list>
#include <type_traits>

#include "../../include/sdhip.h"

#define SDHIP_WAVE 64

typedef unsigned short bf16_t;  // raw bf16 bits (storage type)

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// ---- error plumbing (thread-local last error, never abort) -----------------
void sdhip_set_error(const char* fmt, ...);
#define SDHIP_FAIL(code, ...) do { sdhip_set_error(__VA_ARGS__); return (code); } while (0)
#define SDHIP_CHECK_ARG(cond, ...) do { if (!(cond)) SDHIP_FAIL(SDHIP_ERR_ARG, __VA_ARGS__); } while (0)
// `who` names the launch in the message: a dispatch split into per-path functions keeps reporting under one name
#define SDHIP_LAUNCH_CHECK_AS(who) do { hipError_t e__ = hipGetLastError(); \
    if (e__ != hipSuccess) SDHIP_FAIL(SDHIP_ERR_LAUNCH, "%s: launch failed: %s", (who), hipGetErrorString(e__)); } while (0)
#define SDHIP_LAUNCH_CHECK() SDHIP_LAUNCH_CHECK_AS(__func__)

// ---- diagnostic / tuning switches (runtime.hip): environment read once at library load ----
struct SdhipDiag {
  bool conv_generic, conv_big, conv_no_thin, conv_no_gemm, conv_no_band, conv_no_band3, conv_no_band_bx, wgrad_generic, wgrad_no_pack, wgrad_force_pack, wgrad_no_half, thin_wgrad_reg, corr_no_tiled, wgrad_no_half32, wgrad_split2d, wgrad_no_gemm, conv_no_point, conv_no_grow, conv_no_mid;
  int tune_s2_small;
  int tune_big, tune_split, tune_thin_blocks, tune_fused_blocks, tune_gemm_dbg, tune_band_dbg;
  int tune_mid_min_map, tune_mid_max_map, tune_mid_max_wg;   // > 0: replace kMidMinMap / kMidMaxMap / kMidMaxWG of conv_mid.h
  double tune_atomic_tbs, tune_wg1_tile;
};
const SdhipDiag& sdhip_diag();

// ---- bf16 <-> f32 ------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16_t v) { return __builtin_bit_cast(float, ((unsigned int)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }  // RNE, NaN-safe (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned int pack2bf(float lo, float hi) {
  return (unsigned int)f2bf(lo) | ((unsigned int)f2bf(hi) << 16);
}
__device__ __forceinline__ float bflo(unsigned int u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bfhi(unsigned int u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int kPer16B = 4;
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
  static __device__ __forceinline__ float rnd(float v) { return v; }
};
template <> struct Elem<bf16_t> {
  static constexpr int kPer16B = 8;
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
  static __device__ __forceinline__ float rnd(float v) { return bf2f(f2bf(v)); }
};

// unpack a 16-byte chunk into floats (4 for f32, 8 for bf16) and back
template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int N = 4;
  // NB: bit_cast the WHOLE vector; __builtin_bit_cast on a vector-element lvalue (u[i]) reads element 0 (hipcc 7.2).
  static __device__ __forceinline__ void unpack(const u32x4& u, float* f) {
    const f32x4 v = __builtin_bit_cast(f32x4, u);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i];
  }
  static __device__ __forceinline__ u32x4 pack(const float* f) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = f[i];
    return __builtin_bit_cast(u32x4, v);
  }
};
template <> struct Chunk<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const u32x4& u, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bflo(u[i]); f[2 * i + 1] = bfhi(u[i]); }
  }
  static __device__ __forceinline__ u32x4 pack(const float* f) {
    u32x4 u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = pack2bf(f[2 * i], f[2 * i + 1]);
    return u;
  }
};

// ---- wave64 reductions (DPP-free, shuffle based) --------------------------
// one loop for every summand type __shfl_xor takes (in use: float, and metrics.hip's long and double)
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- reductions of a workgroup (one wave per 64 threads; `sh` / `red` hold one value per wave) ------------------------
// block reduce of one float, result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
  return r;
}
// Ordered tail of a 256-thread workgroup, the first half of the "slot fold" (loss_common.h has the second): every wave sums
// its 64 lanes, the four wave sums are added in wave order, always in this association, so the f64 partial a workgroup
// stores in its slot has the same bits on every run.  For thread 0 (any thread may read it); one barrier.
template <typename T> __device__ __forceinline__ T block_tail(T v, T* red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // wave_sum written out: nested, the callers are scheduled differently
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// one "unit" of a row-wise elementwise kernel: a 16-byte chunk (VEC) or a single element
template <typename T, bool VEC> struct Unit {
  static constexpr int N = VEC ? Chunk<T>::N : 1;
  static __device__ __forceinline__ void load(const T* p, float* f) {
    if constexpr (VEC) Chunk<T>::unpack(*reinterpret_cast<const u32x4*>(p), f);
    else f[0] = Elem<T>::ld(p);
  }
  static __device__ __forceinline__ void store(T* p, const float* f) {
    if constexpr (VEC) *reinterpret_cast<u32x4*>(p) = Chunk<T>::pack(f);
    else Elem<T>::st(p, f[0]);
  }
  // issue and use apart: raw() only loads (16 bytes, or one element); unpack() converts, once every load of a trip is on
  // its way.  load() converts where it loads, so each guarded load of a trip waits for its own data.
  using Raw = std::conditional_t<VEC, u32x4, T>;
  static __device__ __forceinline__ Raw raw(const T* p) {
    if constexpr (VEC) return *reinterpret_cast<const u32x4*>(p);
    else return *p;
  }
  static __device__ __forceinline__ void unpack(const Raw& r, float* f) {
    if constexpr (VEC) Chunk<T>::unpack(r, f);
    else f[0] = Elem<T>::ld(&r);
  }
};

// ---- hard activations of MobileNetV3 (models/mobilenetv3.py:44-61): act codes SDHIP_ACT_HSWISH / SDHIP_ACT_HSIGMOID ----
// h_sigmoid = relu6(x + 3) / 6, h_swish = x * h_sigmoid(x).  The derivatives are torch's composite of those ops: relu6' is
// 0 at both kinks (hardtanh_backward masks x + 3 <= 0 and x + 3 >= 6), so h_swish'(-3) = 0 and h_swish'(3) = 1.
__device__ __forceinline__ float hsig_f(float v) { return fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f; }
__device__ __forceinline__ float act_hs(float v, int act) { return act == SDHIP_ACT_HSWISH ? v * hsig_f(v) : hsig_f(v); }
__device__ __forceinline__ float act_hs_d(float v, int act) {
  const float t = v + 3.f;
  const float m = (t > 0.f && t < 6.f) ? 1.f / 6.f : 0.f;
  return act == SDHIP_ACT_HSWISH ? hsig_f(v) + v * m : m;
}

static inline int sdhip_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- host dispatch: runtime dtype / bool -> template argument -----------------------------------------------------
// An entry point writes its launch once, inside generic lambdas:
//   sdhip_by_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type;
//     sdhip_by_flag(vec, [&](auto V) { hipLaunchKernelGGL((kernel<T, V()>), grid, block, lds, s, (const T*)x, ...); }); });
// Only what is nested gets instantiated: a flag that one dtype never takes is dispatched inside an `if constexpr` on T.
// The dtype must have passed SDHIP_CHECK_DTYPE before.
template <typename T> struct SdhipType { using type = T; };
template <typename F> inline auto sdhip_by_dtype(int dtype, F&& f) {
  return dtype == SDHIP_F32 ? f(SdhipType<float>{}) : f(SdhipType<bf16_t>{});
}
template <typename F> inline auto sdhip_by_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

#define SDHIP_CHECK_DTYPE(who, dtype) \
  SDHIP_CHECK_ARG((dtype) == SDHIP_F32 || (dtype) == SDHIP_BF16, "%s: unknown dtype %d", who, (int)(dtype))

// may rows of C channels be moved as 16-byte chunks: C and every pixel stride a whole number of chunks, every non-null
// pointer 16-byte aligned.  (A kernel that masks its own channel tail passes a C that always divides, e.g. 0.)
template <typename T>
inline bool sdhip_vec_ok(int C, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs) {
  const int n = Chunk<T>::N;
  if (C % n) return false;
  for (int l : lds) if (l % n) return false;
  for (const void* p : ptrs) if (p && ((uintptr_t)p & 15)) return false;
  return true;
}

// ---- zero fill as a KERNEL ------------------------------------------------------------------------------------------
// hipMemsetAsync becomes a memset node when the training step is captured into a hipGraph, and on ROCm 7.2 such a node
// was observed to stop clearing its 512-byte target once unrelated allocations had been made between two replays (the
// Lovasz class counters then accumulated from replay to replay: tests/diag/gpu_lovasz_graph.py).  Everything the
// library clears on a stream is therefore cleared by this kernel: a captured step consists of kernel nodes only.
namespace {
__global__ __launch_bounds__(256) void sdhip_zero_kernel(unsigned char* __restrict__ p, size_t bytes) {
  // any alignment, any length: byte head up to the first 16-byte boundary, 16-byte body, byte tail (a 2-byte-aligned bf16
  // buffer with an odd element count must not fall back to a memset node either)
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  size_t head = (size_t)((16 - (((uintptr_t)p) & 15)) & 15);
  if (head > bytes) head = bytes;
  const size_t n16 = (bytes - head) >> 4;
  const size_t tail0 = head + (n16 << 4);
  u32x4* p16 = reinterpret_cast<u32x4*>(p + head);
  for (size_t j = i; j < n16; j += stride) p16[j] = u32x4{0u, 0u, 0u, 0u};
  if (i < head) p[i] = 0;
  if (tail0 + i < bytes && i < 16) p[tail0 + i] = 0;
}
inline hipError_t sdhip_zero_async(void* ptr, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  size_t blocks = (bytes / 16 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sdhip_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (unsigned char*)ptr, bytes);
  return hipGetLastError();
}
}  // namespace
