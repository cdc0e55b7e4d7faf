// The per-pixel sampling of the segmentation augmentation kernels (seg_aug.hip, seg_elastic.hip): from a Q16 source
// coordinate (X, Y) to the image's bilinear value and the mask's nearest value.
//   mask:   ix = (X + 32768) >> 16, iy likewise; outside the image: mask_fill
//   image:  x0 = X >> 16, fx = (X & 0xFFFF) / 65536, likewise y0, fy;
//           (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11); a tap outside reads image_fill
// Every tap is bounds-tested before its address is formed: nothing outside a source plane is ever read.
#pragma once
#include "common.h"

namespace dlmpi {

// the four bilinear taps of one output pixel: `o` is the in-plane offset of tap (y0, x0) -- possibly of a
// pixel outside the plane, which is why it is only ever added to a pointer under the tap's bit of `ok`
// (1: p00, 2: p01, 4: p10, 8: p11)
struct SegTaps {
  int o;
  unsigned ok;
  float fx, fy;
};
__device__ __forceinline__ SegTaps seg_taps(int64_t X, int64_t Y, int H, int W) {
  const int64_t x0 = X >> 16, y0 = Y >> 16;
  SegTaps t;
  t.fx = (float)(int)(X & 0xFFFF) * (1.f / 65536.f);
  t.fy = (float)(int)(Y & 0xFFFF) * (1.f / 65536.f);
  t.o = 0;
  t.ok = 0;
  if (x0 >= -1 && x0 < W && y0 >= -1 && y0 < H) {   // some tap may lie inside; all four fit an int now
    const int xi = (int)x0, yi = (int)y0;
    const unsigned l = xi >= 0, r = xi + 1 < W, u = yi >= 0, d = yi + 1 < H;
    t.ok = (u & l) | ((u & r) << 1) | ((d & l) << 2) | ((d & r) << 3);
    t.o = yi * W + xi;
  }
  return t;
}
__device__ __forceinline__ float seg_bilinear(const float* __restrict__ plane, const SegTaps& t, int W, float fill) {
  // every product and sum rounded on its own, as the reference does: which ones the compiler fuses would
  // otherwise differ between the two instantiations, and with it the last bit between the two store paths
#pragma clang fp contract(off)
  const float p00 = (t.ok & 1u) ? plane[t.o] : fill;
  const float p01 = (t.ok & 2u) ? plane[t.o + 1] : fill;
  const float p10 = (t.ok & 4u) ? plane[t.o + W] : fill;
  const float p11 = (t.ok & 8u) ? plane[t.o + W + 1] : fill;
  const float top = (1.f - t.fx) * p00 + t.fx * p01;
  const float bot = (1.f - t.fx) * p10 + t.fx * p11;
  return (1.f - t.fy) * top + t.fy * bot;
}
template <typename MT>
__device__ __forceinline__ MT seg_nearest(const MT* __restrict__ plane, int64_t X, int64_t Y, int H, int W, MT fill) {
  const int64_t ix = (X + 32768) >> 16, iy = (Y + 32768) >> 16;
  if (ix < 0 || ix >= W || iy < 0 || iy >= H) return fill;
  return plane[(int)iy * W + (int)ix];
}

}  // namespace dlmpi
