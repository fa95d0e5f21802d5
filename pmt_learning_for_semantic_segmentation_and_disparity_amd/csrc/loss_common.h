// Host-side plumbing the loss and gate operators share (segloss / dispsmooth / edge / warp / multitask), and the one
// kernel they share: the slot fold.
//
// Slot fold: how a scalar loss term is summed without float atomics.  Every workgroup of the term's main kernel reduces
// its elements to ONE f64 partial (block_tail in sdhip_common.h: lanes by xor-shuffle, the four waves in wave order) and
// STORES it in a workspace slot of its own.  slot_fold_kernel, one workgroup on the same stream, then adds the slots in
// slot order (thread i the slots i, i + 256, ...), the 256 thread sums in thread order, and does loss[0] += scale * total.
// Which elements a workgroup and a thread own depends on the problem size alone, never on a stride or an alignment, so a
// term's value has the same bits on every run and for every layout of its inputs.
#pragma once
#include "sdhip_common.h"

namespace {

__global__ __launch_bounds__(256) void slot_fold_kernel(const double* __restrict__ slots, long n, double scale,
                                                        double* __restrict__ loss) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) acc += slots[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += sh[i];
    loss[0] += scale * tot;                        // stream order makes this the only writer
  }
}

// `who` is the entry point's __func__, as SDHIP_LAUNCH_CHECK() reports it
inline int sdhip_slot_fold(const char* who, const double* slots, long n, double scale, double* loss, hipStream_t s) {
  hipLaunchKernelGGL(slot_fold_kernel, dim3(1), dim3(256), 0, s, slots, n, scale, loss);
  SDHIP_LAUNCH_CHECK_AS(who);
  return SDHIP_OK;
}

// grid of a grid-stride streaming kernel: one 256-thread workgroup per 256 items, 1 .. 2048 of them
inline dim3 stream_grid(long items) {
  long b = (items + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

// lanes side by side on one pixel's `units` chunks: the power of two >= min(units, 64)
inline int lane_group(int units) {
  int G = 1;
  while (G < units && G < 64) G <<= 1;
  return G;
}

// an image read through (batch, channel, pixel) strides
#define SDHIP_CHECK_IMAGE_STRIDES(who, bs, cs, ps)                                                                                  \
  SDHIP_CHECK_ARG((bs) >= 1 && (cs) >= 1 && (ps) >= 1, "%s: image strides %ld / %ld / %ld (batch, channel, pixel) must be positive", who, \
                  (long)(bs), (long)(cs), (long)(ps))

// a workspace of f64 / u64 slots
#define SDHIP_CHECK_WORKSPACE(who, ptr, bytes, need)                                                                                \
  SDHIP_CHECK_ARG((bytes) >= (need) && (((uintptr_t)(ptr)) & 7) == 0, "%s: workspace of %ld bytes (8-byte aligned), %ld needed", who, \
                  (long)(bytes), (long)(need))

}  // namespace
