// Device-resident input pipeline (data/device.py): the whole training set lives in HBM (CIFAR-10
// is 150 MB of uint8; 288 GB per MI355X) and every batch is assembled by ONE kernel from a device
// index vector -- gather + RandomCrop(32, padding=4) + RandomHorizontalFlip + ToTensor + Normalize
// of the reference's CIFAR transform (/root/reference/pytorch/resnet/main.py:82-87) -- instead of
// per-sample host transforms in DataLoader worker processes and a host->device copy per step.
//
// Augmentation randomness is a counter-based hash of (seed, epoch, dataset index): reproducible,
// independent of batch size, rank layout and worker count, and identical in the torch reference
// (data/device.py:_aug_params).
#include "common.h"

namespace dlmpi {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// Where output pixel (y, x) of dataset image d comes from: RandomCrop of the zero-padded image at the
// hashed offset, then the horizontal flip of the crop.  `in` false: the pixel lies in the padding.
struct SrcPixel {
  const uint8_t* px;
  bool in;
};
__device__ __forceinline__ SrcPixel source_pixel(const uint8_t* __restrict__ data, int64_t d, int y, int x, int H,
                                                 int W, int C, int pad, int augment, uint32_t seed, uint32_t epoch) {
  int oi = pad, oj = pad, flip = 0;
  if (augment) {
    const uint32_t h = fmix32(seed * 0x9E3779B1u + epoch * 0x85EBCA77u + (uint32_t)d);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    oi = (int)(h % span);
    oj = (int)((h >> 8) % span);
    flip = (int)((h >> 16) & 1u);
  }
  const int sy = y + oi - pad;
  const int sx = (flip ? W - 1 - x : x) + oj - pad;
  const bool in = (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W;
  return {data + ((d * H + (in ? sy : 0)) * W + (in ? sx : 0)) * C, in};
}
__device__ __forceinline__ float normalised(const SrcPixel& s, int c, float mean, float sd) {
  const float v = s.in ? (float)s.px[c] / 255.f : 0.f;
  return (v - mean) / sd;
}

// mixup / CutMix of a sample with its partner B - 1 - b (data/mix.py): one lam and one box per batch
struct MixArgs {
  int kind;   // 0 none, 1 mixup, 2 CutMix
  float lam;
  int y0, y1, x0, x1;
};
__device__ __forceinline__ bool in_box(const MixArgs& m, int y, int x) {
  return y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1;
}
// the mixed value of a sample's own u and its partner's v at (y, x)
__device__ __forceinline__ float mix_value(const MixArgs& m, int y, int x, float u, float v) {
  if (m.kind == 1) return m.lam * u + (1.f - m.lam) * v;
  return in_box(m, y, x) ? v : u;
}

// One thread per output pixel (b, y, x), all C channels.  data: [Nds][H][W][C] uint8 (HWC);
// out: [B][C][H][W] fp32 normalised; out_labels[b] = labels[idx[b]].
__global__ __launch_bounds__(256) void image_batch_kernel(const uint8_t* __restrict__ data,
                                                          const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ idx, int B, int H, int W,
                                                          int C, int pad, int augment, uint32_t seed, uint32_t epoch,
                                                          float m0, float m1, float m2, float s0, float s1, float s2,
                                                          float* __restrict__ out, int64_t* __restrict__ out_labels) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t t = i / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const int64_t d = idx[b];
    const SrcPixel src = source_pixel(data, d, y, x, H, W, C, pad, augment, seed, epoch);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= C) break;
      out[(((int64_t)b * C + c) * H + y) * W + x] = normalised(src, c, mean[c], sd[c]);
    }
    if (x == 0 && y == 0 && out_labels) out_labels[b] = labels[d];
  }
}

// The same batch, mixed: the thread of an output pixel gathers its own source pixel and, where the mix needs
// it, the partner's (each with its own crop / flip), so "augment, then mix" stays one kernel.  Also writes
// labels_b[b] = labels[idx[B - 1 - b]] and lam_out[0].  The middle sample of an odd batch is its own partner
// and is not blended.
__global__ __launch_bounds__(256) void image_batch_mix_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ labels, const int64_t* __restrict__ idx, int B,
    int H, int W, int C, int pad, int augment, uint32_t seed, uint32_t epoch, float m0, float m1, float m2, float s0,
    float s1, float s2, MixArgs mix, float* __restrict__ out, int64_t* __restrict__ out_labels,
    int64_t* __restrict__ labels_b, float* __restrict__ lam_out) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t t = i / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const int pb = B - 1 - b;
    const int64_t d = idx[b], dp = idx[pb];
    const SrcPixel own = source_pixel(data, d, y, x, H, W, C, pad, augment, seed, epoch);
    const bool blend = pb != b && (mix.kind == 1 || (mix.kind == 2 && in_box(mix, y, x)));
    SrcPixel other = own;
    if (blend) other = source_pixel(data, dp, y, x, H, W, C, pad, augment, seed, epoch);
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= C) break;
      float v = normalised(own, c, mean[c], sd[c]);
      if (blend) v = mix_value(mix, y, x, v, normalised(other, c, mean[c], sd[c]));
      out[(((int64_t)b * C + c) * H + y) * W + x] = v;
    }
    if (x == 0 && y == 0) {
      out_labels[b] = labels[d];
      labels_b[b] = labels[dp];
      if (b == 0) lam_out[0] = mix.lam;
    }
  }
}

// In-place mix of any fp32 [B][C][H][W] batch: one thread owns V consecutive elements of sample b < B / 2 and
// the same elements of its partner B - 1 - b, reads both and writes both, so no other thread touches them.
// Block 0 also writes labels_b[b] = labels[B - 1 - b] and lam_out[0].
template <int V>
__global__ __launch_bounds__(256) void mix_batch_kernel(float* __restrict__ xb, const int64_t* __restrict__ labels,
                                                        int B, int64_t CHW, int H, int W, MixArgs mix,
                                                        int64_t* __restrict__ labels_b, float* __restrict__ lam_out) {
  if (blockIdx.x == 0) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) labels_b[b] = labels[B - 1 - b];
    if (threadIdx.x == 0) lam_out[0] = mix.lam;
  }
  if (mix.kind == 0) return;
  const int64_t per = CHW / V, total = (int64_t)(B / 2) * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per, r = (i % per) * V;
    float* pu = xb + b * CHW + r;
    float* pv = xb + (B - 1 - b) * CHW + r;
    float u[V], v[V];
    if constexpr (V == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(pu), c = *reinterpret_cast<const f32x4*>(pv);
#pragma unroll
      for (int j = 0; j < 4; ++j) { u[j] = a[j]; v[j] = c[j]; }
    } else {
      u[0] = *pu;
      v[0] = *pv;
    }
    float nu[V], nv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t p = (r + j) % ((int64_t)H * W);
      const int y = (int)(p / W), x = (int)(p % W);
      nu[j] = mix_value(mix, y, x, u[j], v[j]);
      nv[j] = mix_value(mix, y, x, v[j], u[j]);
    }
    if constexpr (V == 4) {
      *reinterpret_cast<f32x4*>(pu) = f32x4{nu[0], nu[1], nu[2], nu[3]};
      *reinterpret_cast<f32x4*>(pv) = f32x4{nv[0], nv[1], nv[2], nv[3]};
    } else {
      *pu = nu[0];
      *pv = nv[0];
    }
  }
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" hipError_t dlmpi_image_batch(const uint8_t* data, const int64_t* labels, const int64_t* idx, int B, int H,
                                        int W, int C, int pad, int augment, uint32_t seed, uint32_t epoch,
                                        const float* mean3, const float* std3, float* out, int64_t* out_labels,
                                        hipStream_t s) {
  if (C < 1 || C > 3 || B <= 0) return B == 0 ? hipSuccess : hipErrorInvalidValue;
  int64_t blocks = ((int64_t)B * H * W + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(image_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, data, labels, idx, B, H, W, C, pad,
                     augment, seed, epoch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out, out_labels);
  return hipGetLastError();
}

// blocks of one grid sweep of the in-place mix (the kernel strides over the rest)
static constexpr int kMixBlocks = 2048;

extern "C" hipError_t dlmpi_image_batch_mix(const uint8_t* data, const int64_t* labels, const int64_t* idx, int B,
                                            int H, int W, int C, int pad, int augment, uint32_t seed, uint32_t epoch,
                                            const float* mean3, const float* std3, int kind, float lam, int y0, int y1,
                                            int x0, int x1, float* out, int64_t* out_labels, int64_t* labels_b,
                                            float* lam_out, hipStream_t s) {
  if (C < 1 || C > 3 || B <= 0 || kind < 0 || kind > 2 || !out_labels || !labels_b || !lam_out)
    return hipErrorInvalidValue;
  int64_t blocks = ((int64_t)B * H * W + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const MixArgs mix{kind, lam, y0, y1, x0, x1};
  hipLaunchKernelGGL(image_batch_mix_kernel, dim3((unsigned)blocks), dim3(256), 0, s, data, labels, idx, B, H, W, C,
                     pad, augment, seed, epoch, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], mix, out,
                     out_labels, labels_b, lam_out);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_mix_batch(float* x, const int64_t* labels, int B, int C, int H, int W, int kind, float lam,
                                      int y0, int y1, int x0, int x1, int64_t* labels_b, float* lam_out,
                                      hipStream_t s) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || kind < 0 || kind > 2) return hipErrorInvalidValue;
  const int64_t CHW = (int64_t)C * H * W;
  const bool vec = CHW % 4 == 0 && ((uintptr_t)x & 15u) == 0;
  const int64_t work = kind == 0 ? 1 : (int64_t)(B / 2) * (vec ? CHW / 4 : CHW);
  int64_t blocks = (work + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > kMixBlocks) blocks = kMixBlocks;
  const MixArgs mix{kind, lam, y0, y1, x0, x1};
  if (vec)
    hipLaunchKernelGGL((mix_batch_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, s, x, labels, B, CHW, H, W, mix,
                       labels_b, lam_out);
  else
    hipLaunchKernelGGL((mix_batch_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, s, x, labels, B, CHW, H, W, mix,
                       labels_b, lam_out);
  return hipGetLastError();
}
