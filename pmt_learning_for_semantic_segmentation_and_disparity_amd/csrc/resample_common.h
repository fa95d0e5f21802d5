// What resample.hip and pyramid.hip share: the NHWC item decomposition, ATen's area_pixel_* index maths of the resize
// kernels, the candidate window and lanes-per-item rule of the resize backward, and the capped grid.
#pragma once
#include "sdhip_common.h"

namespace {

struct Img { int B, H, W, C, ld; };

// flat work item -> (pixel, channel unit)
template <int N>
__device__ __forceinline__ bool item(long i, long npix, int units, long& pix, int& c0) {
  if (i >= npix * units) return false;
  pix = i / units;
  c0 = (int)(i - pix * units) * N;
  return true;
}

struct Axis { int in, out; float scale; int mode; };  // mode 0 nearest, 1 bilinear (align_corners=False), 2 bilinear (True)

__device__ __forceinline__ int nearest_src(const Axis& a, int d) {
  const int s = (int)floorf((float)d * a.scale);
  return s < a.in - 1 ? s : a.in - 1;
}
__device__ __forceinline__ void linear_src(const Axis& a, int d, int& i0, int& i1, float& l1) {
  float s;
  if (a.mode == 2) s = (float)d * a.scale;
  else { s = ((float)d + 0.5f) * a.scale - 0.5f; if (s < 0.f) s = 0.f; }
  i0 = (int)s;
  if (i0 > a.in - 1) i0 = a.in - 1;
  i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  if (l1 < 0.f) l1 = 0.f;
  if (l1 > 1.f) l1 = 1.f;
}

// destination candidates [lo, hi] of source index i in the gather backward: source coordinate within [i-1, i+1) (+-2
// destinations of slack).  align_corners=False samples at (d + 0.5) * scale - 0.5, so its window is shifted by
// 0.5 * inv - 0.5 destinations: without the shift an upsampling by more than ~4x missed the destinations between
// (i+1) * inv and (i+1.5) * inv (x32: 7 % of the gradient dropped)
__device__ __forceinline__ void bwd_window(const Axis& a, int i, int& lo, int& hi) {
  const float inv = a.scale > 0.f ? 1.f / a.scale : 0.f;
  const float shift = a.mode == 1 ? 0.5f * inv - 0.5f : 0.f;
  lo = (int)floorf(((float)i - 1.f) * inv + shift) - 2;
  hi = (int)ceilf(((float)i + 1.f) * inv + shift) + 2;
  if (a.scale <= 0.f) { lo = 0; hi = a.out - 1; }
  if (lo < 0) lo = 0;
  if (hi > a.out - 1) hi = a.out - 1;
}

// weight with which destination d of the axis contributes to source index i
__device__ __forceinline__ float bwd_weight(const Axis& a, int d, int i) {
  float wgt = 0.f;
  if (a.mode == 0) {
    wgt = nearest_src(a, d) == i ? 1.f : 0.f;
  } else {
    int i0, i1; float l1;
    linear_src(a, d, i0, i1, l1);
    if (i0 == i) wgt += 1.f - l1;
    if (i1 == i) wgt += l1;
  }
  return wgt;
}

inline dim3 grid_for(long items) {
  long b = (items + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return dim3((unsigned)b);
}

inline Axis make_axis(int in, int out, int mode, float scale_override) {
  Axis a; a.in = in; a.out = out; a.mode = mode;
  if (mode == 2) a.scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  else a.scale = scale_override > 0.f ? scale_override : (float)in / (float)out;
  return a;
}

// lanes that share one item of the gather backward: candidates per item ~ 2 / scale + 5 (see bwd_window)
inline int bwd_lanes(const Axis& a) {
  const float span = a.scale > 0.f ? 2.f / a.scale + 5.f : (float)a.out;
  return span >= 32.f ? 16 : span >= 12.f ? 4 : 1;
}

}  // namespace
