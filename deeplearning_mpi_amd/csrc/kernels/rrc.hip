// RandomResizedCrop of the device-resident classification pipeline (data/rrc.py, data/device.py): ONE kernel per
// batch gathers uint8 HWC images by a device index vector, crops each to its box, resizes the box to Ho x Wo with
// the anti-aliased bilinear (tent) filter, flips, normalises and writes fp32 NCHW, and gathers the labels.
//
// The box of dataset sample d is row d of an int32 [N][5] table (top, left, h, w, flip) that the host draws once
// per epoch.  Per axis (n source, m output pixels), as in the torch reference rrc_reference:
//   scale = n / m, support = max(scale, 1), centre_i = scale (i + 0.5)
//   lo_i = max(0, floor(centre_i - support + 0.5)), hi_i = min(n, floor(centre_i + support + 0.5)), both in exact
//   integer arithmetic over the denominator 2 m
//   t_j = max(0, 1 - |j - centre_i + 0.5| / support) for j in [lo_i, hi_i), divided by their sum (fp32)
// The resize runs on u8 / 255.f, rows first (x), then columns (y); then (v - mean_c) / std_c, the two expressions
// of image_batch_kernel, so an identity box (weights 1 and 0) gives that kernel's bits.
//
// A block owns one sample and a tile of 32 rows x 32 V columns.  The weights of its columns and rows do not depend
// on the pixel: they are computed once per block into LDS (at most kRrcTaps per output pixel and axis; the binding
// refuses a box with h / Ho or w / Wo above kRrcMaxScale), next to the 256 values u8 / 255.f.  Every tap lies in
// [0, n) of its box and the binding has checked that every box of the table lies inside the image, so nothing
// outside a source image is ever read.
#include "common.h"

namespace dlmpi {

constexpr int kRrcTaps = 32;        // taps per output pixel and axis held in LDS
constexpr int kRrcMaxScale = 15;    // 2 * scale + 1 <= 31 taps
constexpr int kRrcTX = 32, kRrcTY = 8, kRrcRows = 32;

// The taps of output pixel i of an axis with n source and m output pixels: first tap *lo, count *cnt, and the
// normalised weights at w[k * stride].  Every operation rounded on its own, as the reference does.
__device__ __forceinline__ void rrc_axis(int n, int m, int i, int* lo, int* cnt, float* w, int stride) {
#pragma clang fp contract(off)
  const int64_t c2 = (int64_t)n * (2 * i + 1), s2 = 2 * (int64_t)(n > m ? n : m);
  const int64_t a = c2 - s2 + m, e = (c2 + s2 + m) / (2 * (int64_t)m);
  const int l = a <= 0 ? 0 : (int)(a / (2 * (int64_t)m));
  const int h = e < n ? (int)e : n;
  int c = h - l;
  if (c > kRrcTaps) c = kRrcTaps;   // never taken: the binding bounds n / m
  const float scale = (float)n / (float)m, support = fmaxf(scale, 1.f), centre = scale * ((float)i + 0.5f);
  float sum = 0.f;
  for (int k = 0; k < c; ++k) {
    const float t = fmaxf(0.f, 1.f - fabsf(((float)(l + k) - centre) + 0.5f) / support);
    w[k * stride] = t;
    sum += t;
  }
  for (int k = 0; k < c; ++k) w[k * stride] = w[k * stride] / sum;
  *lo = l;
  *cnt = c;
}

// Thread (tx, ty) of a 32 x 8 block produces output columns x0 + tx V .. + V - 1 of rows y0 + ty + 8 r, all C
// channels of each pixel, so the channels of a source pixel are read together; the sums are explicit fused
// multiply-adds in tap order, so both instantiations give the same bits.  V = 4: Wo % 4 == 0 and a 16-byte
// aligned output, 16-byte stores; V = 1: any shape and alignment.  data [N][H][W][C] uint8, C = 1 or 3;
// out [B][C][Ho][Wo] fp32; out_labels[b] = labels[idx[b]].  grid (ceil(Wo / 32 V), ceil(Ho / 32), B).
template <int V, int C>
__global__ __launch_bounds__(256) void image_rrc_batch_kernel(const uint8_t* __restrict__ data,
                                                              const int64_t* __restrict__ labels,
                                                              const int64_t* __restrict__ idx,
                                                              const int* __restrict__ table, int H, int W, int Ho,
                                                              int Wo, float m0, float m1, float m2, float s0,
                                                              float s1, float s2, float* __restrict__ out,
                                                              int64_t* __restrict__ out_labels) {
  constexpr int TW = kRrcTX * V;
  __shared__ float wx[kRrcTaps][TW];        // tap-major: the threads of a row read neighbouring words
  __shared__ float wy[kRrcTaps][kRrcRows];
  __shared__ int xlo[TW], xn[TW], ylo[kRrcRows], yn[kRrcRows];
  __shared__ float unit[256];               // u8 / 255.f

  const int b = blockIdx.z, bx0 = blockIdx.x * TW, by0 = blockIdx.y * kRrcRows;
  const int64_t d = idx[b];
  const int* box = table + d * 5;
  const int top = box[0], left = box[1], h = box[2], w = box[3], flip = box[4];

  unit[threadIdx.x] = (float)threadIdx.x / 255.f;
  for (int e = threadIdx.x; e < TW + kRrcRows; e += blockDim.x) {
    if (e < TW) {
      const int x = bx0 + e;
      xn[e] = 0;
      if (x < Wo) rrc_axis(w, Wo, flip ? Wo - 1 - x : x, &xlo[e], &xn[e], &wx[0][e], TW);
    } else {
      const int r = e - TW, y = by0 + r;
      yn[r] = 0;
      if (y < Ho) rrc_axis(h, Ho, y, &ylo[r], &yn[r], &wy[0][r], kRrcRows);
    }
  }
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) out_labels[b] = labels[d];
  __syncthreads();

  const int tx = threadIdx.x % kRrcTX, ty = threadIdx.x / kRrcTX;
  const int x0 = bx0 + tx * V;
  if (x0 >= Wo) return;   // (V = 4: Wo % 4 == 0, so the thread's four columns are in or out together)
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const uint8_t* src = data + ((d * H + top) * (int64_t)W + left) * C;
  const int64_t HWo = (int64_t)Ho * Wo;
  for (int r = ty; r < kRrcRows; r += kRrcTY) {
    const int y = by0 + r;
    if (y >= Ho) break;
    const int ly = ylo[r], ny = yn[r];
    float v[C][V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int col = tx * V + j, lx = xlo[col], nx = xn[col];
      float acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 0.f;
      const uint8_t* row = src + ((int64_t)ly * W + lx) * C;
      for (int ky = 0; ky < ny; ++ky, row += (int64_t)W * C) {
        float racc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) racc[c] = 0.f;
        for (int kx = 0; kx < nx; ++kx) {
          const float wgt = wx[kx][col];
#pragma unroll
          for (int c = 0; c < C; ++c) racc[c] = __builtin_fmaf(wgt, unit[row[kx * C + c]], racc[c]);
        }
        const float wv = wy[ky][r];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __builtin_fmaf(wv, racc[c], acc[c]);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = (acc[c] - mean[c]) / sd[c];
    }
    float* o = out + (int64_t)b * C * HWo + (int64_t)y * Wo + x0;
#pragma unroll
    for (int c = 0; c < C; ++c, o += HWo) {
      if constexpr (V == 4)
        *reinterpret_cast<f32x4*>(o) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
      else
        o[0] = v[c][0];
    }
  }
}

template <int V, int C>
static hipError_t launch_rrc(const uint8_t* data, const int64_t* labels, const int64_t* idx, const int* table, int B,
                             int H, int W, int Ho, int Wo, const float* mean3, const float* std3, float* out,
                             int64_t* out_labels, hipStream_t s) {
  const dim3 grid((unsigned)((Wo + kRrcTX * V - 1) / (kRrcTX * V)), (unsigned)((Ho + kRrcRows - 1) / kRrcRows),
                  (unsigned)B);
  hipLaunchKernelGGL((image_rrc_batch_kernel<V, C>), grid, dim3(kRrcTX * kRrcTY), 0, s, data, labels, idx, table, H,
                     W, Ho, Wo, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out, out_labels);
  return hipGetLastError();
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_rrc_max_scale() { return kRrcMaxScale; }

extern "C" hipError_t dlmpi_image_rrc_batch(const uint8_t* data, const int64_t* labels, const int64_t* idx,
                                            const int* table, int B, int H, int W, int C, int Ho, int Wo,
                                            const float* mean3, const float* std3, float* out, int64_t* out_labels,
                                            hipStream_t s) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (C != 1 && C != 3) ||
      (int64_t)Ho > 65535 * (int64_t)kRrcRows || !data || !labels || !idx || !table || !out || !out_labels)
    return hipErrorInvalidValue;
  const bool vec = Wo % 4 == 0 && ((uintptr_t)out & 15u) == 0;
  if (C == 3)
    return vec ? launch_rrc<4, 3>(data, labels, idx, table, B, H, W, Ho, Wo, mean3, std3, out, out_labels, s)
               : launch_rrc<1, 3>(data, labels, idx, table, B, H, W, Ho, Wo, mean3, std3, out, out_labels, s);
  return vec ? launch_rrc<4, 1>(data, labels, idx, table, B, H, W, Ho, Wo, mean3, std3, out, out_labels, s)
             : launch_rrc<1, 1>(data, labels, idx, table, B, H, W, Ho, Wo, mean3, std3, out, out_labels, s);
}
