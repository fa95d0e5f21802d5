// Eval-mode BatchNorm folded into the packed convolution weights, for gfx950 (MI355X).
//
// With running statistics, conv -> BatchNorm -> activation (convbn / deconvbn of models/dsnet_t2.py:16-77 under model.eval(),
// torch_implementation.py:450-582) is ONE convolution with weights W(m,k,t) * scale[m], the bias shift[m] and the activation
// epilogue every forward kernel already has.  This file packs such weights for a whole network in one launch
// (sdhip_conv_pack_fold_batch, the eval counterpart of sdhip_conv_pack_batch) and, for the BatchNorms that are not folded,
// writes their scale / shift tables in the same launch.  Gather-bound like the plain pack kernel; no atomics.
#include "conv_common.h"

namespace {

constexpr int kFoldBlocks = 64;    // workgroups per row, as sdhip_conv_pack_batch (surplus workgroups of small rows exit at once)
constexpr int kFoldCols = 16;      // int64 columns of a row (include/sdhip.h)

// scale / shift of channel c: exactly the f32 arithmetic of the eval branch of bn_finalize_kernel (bn_act.hip)
struct FoldBN {
  const float* gamma; const float* beta; const float* rmean; const float* rvar; const float* cbias; float eps;
  __device__ __forceinline__ float scale(unsigned c) const {
    const float gm = gamma ? gamma[c] : 1.f;
    const float inv = 1.f / sqrtf(rvar[c] + eps);
    return gm * inv;
  }
  __device__ __forceinline__ float shift(unsigned c) const {
    const float gm = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
    const float inv = 1.f / sqrtf(rvar[c] + eps);
    float sh = bt - rmean[c] * gm * inv;
    if (cbias) sh += cbias[c] * (gm * inv);
    return sh;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void pack_fold_batch_kernel(const long* __restrict__ desc) {
  constexpr int CK = 8 * Chunk<T>::N;
  const long* d = desc + (long)blockIdx.y * kFoldCols;
  FoldBN bn;
  bn.gamma = reinterpret_cast<const float*>(d[10]);
  bn.beta = reinterpret_cast<const float*>(d[11]);
  bn.rmean = reinterpret_cast<const float*>(d[12]);
  bn.rvar = reinterpret_cast<const float*>(d[13]);
  bn.cbias = reinterpret_cast<const float*>(d[15]);
  bn.eps = __builtin_bit_cast(float, (unsigned int)(d[14] & 0xffffffffL));
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
  if (d[0] == 1) {   // table row: scale / shift [groups][C] of a BatchNorm that stays a separate pass
    float* scale = reinterpret_cast<float*>(d[2]);
    float* shift = reinterpret_cast<float*>(d[3]);
    const unsigned C = (unsigned)d[4], G = (unsigned)d[5];
    for (unsigned c = tid; c < C; c += nthr) {
      const float sc = bn.scale(c), sh = bn.shift(c);
      for (unsigned g = 0; g < G; ++g) { scale[g * C + c] = sc; shift[g * C + c] = sh; }
    }
    return;
  }
  const float* src = reinterpret_cast<const float*>(d[1]);
  T* dst = reinterpret_cast<T*>(d[2]);
  float* bias_out = reinterpret_cast<float*>(d[3]);
  const int M = (int)d[4], K = (int)d[5], Tn = (int)d[6], flip = (int)d[9];
  const long sm = d[7], sk = d[8];
  const int Mpad = (M + 15) & ~15;
  for (unsigned m = tid; m < (unsigned)M; m += nthr) bias_out[m] = bn.shift(m);
  // 32-bit index arithmetic and the [q][t][m][c] walk of pack_batch_kernel (conv_wgrad.hip); the pad rows m >= M and the channel
  // tail k >= K are written as zeros, and nothing per-channel is read for them
  const unsigned total = (unsigned)((K + CK - 1) / CK) * Tn * Mpad * CK;
  const unsigned per_q = (unsigned)Tn * Mpad;
  for (unsigned i = tid; i < total; i += nthr) {
    const unsigned c = i % CK;
    const unsigned r = i / CK;
    const unsigned q = r / per_q, rr = r - q * per_q;
    const unsigned t = rr / Mpad, m = rr - t * Mpad;
    const unsigned k = q * CK + c;
    float v = 0.f;
    if (m < (unsigned)M && k < (unsigned)K)
      v = src[(long)m * sm + (long)k * sk + (flip ? Tn - 1 - (int)t : (int)t)] * bn.scale(m);   // f32 product, rounded once by st
    Elem<T>::st(dst + i, v);
  }
}

}  // namespace

extern "C" int sdhip_conv_pack_fold_batch(const long* desc, int ndesc, int dtype, void* stream) {
  SDHIP_CHECK_ARG(desc && ndesc > 0, "conv_pack_fold_batch: bad arguments");
  SDHIP_CHECK_DTYPE("conv_pack_fold_batch", dtype);
  sdhip_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pack_fold_batch_kernel<T>, dim3(kFoldBlocks, ndesc), dim3(256), 0, (hipStream_t)stream, desc);
  });
  SDHIP_LAUNCH_CHECK();
  return SDHIP_OK;
}
