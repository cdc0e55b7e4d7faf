// Segmentation augmentation on the device (data/seg_aug.py, data/device.py:DeviceSegDataset): ONE kernel per
// batch gathers image / mask pairs by a device index vector and resamples both through each sample's inverse
// affine map -- flip, rotation, isotropic scale, translation, and crop / zoom when the output size differs from
// the source's -- bilinear for the image, nearest for the mask.
//
// The map of dataset sample d is row d of an int32 [N][6] table in Q16, (a, b, c, d, e, f) with
// x_src = a x + b y + c and y_src = d x + e y + f, which the host draws once per epoch.  All coordinate
// arithmetic is integer (int64) and identical in the torch reference (seg_aug_reference), so the mask is
// bit-exact and the image differs by the fp32 rounding of its three lerps only:
//   mask:   ix = (X + 32768) >> 16, iy likewise; outside the image: mask_fill
//   image:  x0 = X >> 16, fx = (X & 0xFFFF) / 65536, likewise y0, fy;
//           (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11); a tap outside reads image_fill
// Every tap is bounds-tested before its address is formed: nothing outside a source plane is ever read.
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

// One thread owns V consecutive output columns (b, y, x .. x + V - 1), all C channels and the mask; the
// coordinates advance along the row by adding a and d.  V = 4: Wo % 4 == 0 and 16-byte aligned outputs, 16-byte
// stores; V = 1: any shape and alignment.  images [N][C][H][W] fp32, masks [N][H][W] MT (float | int64),
// out [B][C][Ho][Wo] fp32, out_mask [B][Ho][Wo] MT.  H * W and B * Ho * Wo fit an int (checked by the launcher).
template <typename MT, int V>
__global__ __launch_bounds__(256) void seg_aug_batch_kernel(const float* __restrict__ images,
                                                            const MT* __restrict__ masks,
                                                            const int64_t* __restrict__ idx,
                                                            const int* __restrict__ table, int B, int C, int H,
                                                            int W, int Ho, int Wo, float image_fill, MT mask_fill,
                                                            float* __restrict__ out, MT* __restrict__ out_mask) {
  const int Wq = Wo / V;
  const int64_t total = (int64_t)B * Ho * Wq, HW = (int64_t)H * W, HWo = (int64_t)Ho * Wo;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    // total fits 31 bits (the launcher checks B * Ho * Wo): 32-bit divisions
    const uint32_t r = (uint32_t)i / (uint32_t)Wq;
    const int x = (int)((uint32_t)i - r * (uint32_t)Wq) * V;
    const int b = (int)(r / (uint32_t)Ho);
    const int y = (int)(r - (uint32_t)b * (uint32_t)Ho);
    const int64_t s = idx[b];
    const int* m = table + s * 6;
    const int64_t a = m[0], d = m[3];
    int64_t X = a * x + (int64_t)m[1] * y + m[2];
    int64_t Y = d * x + (int64_t)m[4] * y + m[5];
    const MT* mplane = masks + s * HW;
    SegTaps t[V];
    MT mv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      t[j] = seg_taps(X, Y, H, W);
      mv[j] = seg_nearest(mplane, X, Y, H, W, mask_fill);
      X += a;
      Y += d;
    }
    const int64_t po = (int64_t)y * Wo + x;
    MT* om = out_mask + b * HWo + po;
    if constexpr (V == 4) {
      if constexpr (sizeof(MT) == 4) {
        *reinterpret_cast<f32x4*>(om) = f32x4{(float)mv[0], (float)mv[1], (float)mv[2], (float)mv[3]};
      } else {
        typedef long long i64x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<i64x2*>(om) = i64x2{(long long)mv[0], (long long)mv[1]};
        *reinterpret_cast<i64x2*>(om + 2) = i64x2{(long long)mv[2], (long long)mv[3]};
      }
    } else {
      om[0] = mv[0];
    }
    const float* plane = images + s * C * HW;
    float* o = out + (int64_t)b * C * HWo + po;
    for (int c = 0; c < C; ++c, plane += HW, o += HWo) {
      float v[V];
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = seg_bilinear(plane, t[j], W, image_fill);
      if constexpr (V == 4)
        *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      else
        o[0] = v[0];
    }
  }
}

// blocks of one grid sweep (the kernel strides over the rest)
static constexpr int kSegAugBlocks = 2048;

template <typename MT>
static hipError_t launch_seg_aug(const float* images, const MT* masks, const int64_t* idx, const int* table, int B,
                                 int C, int H, int W, int Ho, int Wo, float image_fill, MT mask_fill, float* out,
                                 MT* out_mask, hipStream_t s) {
  const bool vec = Wo % 4 == 0 && (((uintptr_t)out | (uintptr_t)out_mask) & 15u) == 0;
  const int64_t work = (int64_t)B * Ho * (vec ? Wo / 4 : Wo);
  int64_t blocks = (work + 255) / 256;
  if (blocks > kSegAugBlocks) blocks = kSegAugBlocks;
  if (vec)
    hipLaunchKernelGGL((seg_aug_batch_kernel<MT, 4>), dim3((unsigned)blocks), dim3(256), 0, s, images, masks, idx,
                       table, B, C, H, W, Ho, Wo, image_fill, mask_fill, out, out_mask);
  else
    hipLaunchKernelGGL((seg_aug_batch_kernel<MT, 1>), dim3((unsigned)blocks), dim3(256), 0, s, images, masks, idx,
                       table, B, C, H, W, Ho, Wo, image_fill, mask_fill, out, out_mask);
  return hipGetLastError();
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" hipError_t dlmpi_seg_aug_batch(const float* images, const void* masks, int mask_i64, const int64_t* idx,
                                          const int* table, int B, int C, int H, int W, int Ho, int Wo,
                                          float image_fill, float mask_fill_f, int64_t mask_fill_i, float* out,
                                          void* out_mask, hipStream_t s) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (int64_t)H * W > INT32_MAX ||
      (int64_t)B * Ho * Wo > INT32_MAX || !images || !masks || !idx || !table || !out || !out_mask)
    return hipErrorInvalidValue;
  if (mask_i64)
    return launch_seg_aug<int64_t>(images, (const int64_t*)masks, idx, table, B, C, H, W, Ho, Wo, image_fill,
                                   mask_fill_i, out, (int64_t*)out_mask, s);
  return launch_seg_aug<float>(images, (const float*)masks, idx, table, B, C, H, W, Ho, Wo, image_fill, mask_fill_f,
                               out, (float*)out_mask, s);
}
