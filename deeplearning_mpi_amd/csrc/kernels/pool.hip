// Pooling / layout / resampling kernels (NHWC, 8 channels per thread; every kernel is templated on
// the activation storage type T: uint16_t = bf16, float = the fp32 precision path).
// Replace ATen MaxPool2d (ResNet stem 3x3/s2/p1, UNet 2x2/s2: /root/reference/pytorch/unet/model.py:25),
// AdaptiveAvgPool2d(1) (ResNet head), the host-side NCHW fp32 -> NHWC bf16 input conversion, and
// nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (model.py:39-40).
#include "rowreduce.h"

namespace dlmpi {

// grid of the elementwise kernels here: ew_blocks with this cap
static inline dim3 pool_grid(int64_t total) { return dim3(ew_blocks(total, 16384)); }

// Max pool forward; idx stores the winning window position (kh*k + kw) per channel, first max
// in scan order wins (torch semantics).  Padding never wins: a window whose in-image taps are all -inf
// reports its first in-image tap (the launcher refuses 2 * pad > k, so every window has one).
// scale/shift (optional): the pooled input is relu(x * scale + shift) rounded to bf16, i.e. the
// training-mode BN-apply + ReLU of the ResNet stem fused into the pool -- the stem's BN output is
// never written or re-read (identical values and argmax to pooling the materialised bf16 tensor).
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, int N, int H, int W, int C, int ldx, int xoff,
                                   int k, int stride, int pad, T* __restrict__ y, uint8_t* __restrict__ idx,
                                   int OH, int OW, const float* __restrict__ scale, const float* __restrict__ shift,
                                   FastDiv fdCC, FastDiv fdOW, FastDiv fdOH) {
  const int CC = C >> 3;
  const int64_t total = (int64_t)N * OH * OW * CC;   // < 2^31 (launcher): 32-bit magic divisions
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t ui = (uint32_t)i;
    const uint32_t upix = fdiv(ui, fdCC);
    const int cc = (int)(ui - upix * CC);
    const int64_t pix = upix;
    const uint32_t t2 = fdiv(upix, fdOW);
    const int ow = (int)(upix - t2 * OW);
    const uint32_t n_ = fdiv(t2, fdOH);
    const int oh = (int)(t2 - n_ * OH);
    const int n = (int)n_;
    float best[8], sc[8], sh[8];
    uint8_t bi[8];
    // the first in-image tap in scan order: what a window with no value above -inf reports (torch)
    const uint8_t first = (uint8_t)(max(pad - oh * stride, 0) * k + max(pad - ow * stride, 0));
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = first; }
    if (scale) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { sc[e] = scale[cc * 8 + e]; sh[e] = shift[cc * 8 + e]; }
    }
    for (int kh = 0; kh < k; ++kh) {
      const int ih = oh * stride - pad + kh;
      if ((unsigned)ih >= (unsigned)H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int iw = ow * stride - pad + kw;
        if ((unsigned)iw >= (unsigned)W) continue;
        float v[8];
        load8(x + (((int64_t)n * H + ih) * W + iw) * ldx + xoff + cc * 8, v);
        if (scale) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = stored<T>(fmaxf(v[e] * sc[e] + sh[e], 0.f));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (v[e] > best[e] || (v[e] != v[e] && best[e] == best[e])) { best[e] = v[e]; bi[e] = (uint8_t)(kh * k + kw); }
      }
    }
    store8(y + pix * C + cc * 8, best);
    uint64_t packed = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) packed |= (uint64_t)bi[e] << (8 * e);
    *reinterpret_cast<uint64_t*>(idx + pix * C + cc * 8) = packed;
  }
}

// Max pool forward with a compile-time K x K window and stride S (the ResNet stem's 3x3/s2, the UNet's
// 2x2/s2): every tap's load is issued before the first compare (out-of-image taps read a clamped
// in-image address and are masked to -inf, which never wins), instead of one dependent round trip per
// tap of the runtime-k loop (182 -> ~100 us for the ResNet-50 bs-256 stem pool).  Same scan order and
// compares as maxpool_fwd_kernel: identical values and indices.
//
// ys (with scale / shift, K == S: every input pixel in exactly one window): the applied values
// relu(fma(x, scale, shift)) -- bn_apply_kernel's arithmetic, bit-identical -- are also stored to ys, so
// a BN-apply whose output is both kept and pooled (the UNet encoder skip) needs one pass, not two.
template <int K, int S, typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_fixed_kernel(const T* __restrict__ x, int N, int H, int W, int C,
                                                                int ldx, int xoff, int pad, T* __restrict__ y,
                                                                uint8_t* __restrict__ idx, int OH, int OW,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift, FastDiv fdCC,
                                                                FastDiv fdOW, FastDiv fdOH, T* __restrict__ ys,
                                                                int ldys, int ysoff) {
  const int CC = C >> 3;
  const int64_t total = (int64_t)N * OH * OW * CC;   // < 2^31 (launcher)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t ui = (uint32_t)i;
    const uint32_t upix = fdiv(ui, fdCC);
    const int cc = (int)(ui - upix * CC);
    const uint32_t t2 = fdiv(upix, fdOW);
    const int ow = (int)(upix - t2 * OW);
    const uint32_t n_ = fdiv(t2, fdOH);
    const int oh = (int)(t2 - n_ * OH);
    typename Vec8<T>::type raw[K][K];
    bool ok[K][K];
#pragma unroll
    for (int kh = 0; kh < K; ++kh)
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int ih = oh * S - pad + kh, iw = ow * S - pad + kw;
        ok[kh][kw] = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        const int ihc = min(max(ih, 0), H - 1), iwc = min(max(iw, 0), W - 1);
        raw[kh][kw] = raw8(x + (((int64_t)n_ * H + ihc) * W + iwc) * ldx + xoff + cc * 8);
      }
    float best[8], sc[8], sh[8];
    uint8_t bi[8];
    const uint8_t first = (uint8_t)(max(pad - oh * S, 0) * K + max(pad - ow * S, 0));   // as in maxpool_fwd_kernel
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = first; }
    if (scale) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { sc[e] = scale[cc * 8 + e]; sh[e] = shift[cc * 8 + e]; }
    }
#pragma unroll
    for (int kh = 0; kh < K; ++kh)
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        if (!ok[kh][kw]) continue;
        float v[8];
        unpack8(raw[kh][kw], v);
        if (scale) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = stored<T>(fmaxf(__builtin_fmaf(v[e], sc[e], sh[e]), 0.f));
          if (ys) {
            const int ih = oh * S - pad + kh, iw = ow * S - pad + kw;
            store8(ys + (((int64_t)n_ * H + ih) * W + iw) * ldys + ysoff + cc * 8, v);
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (v[e] > best[e] || (v[e] != v[e] && best[e] == best[e])) { best[e] = v[e]; bi[e] = (uint8_t)(kh * K + kw); }
      }
    store8(y + (int64_t)upix * C + cc * 8, best);
    uint64_t packed = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) packed |= (uint64_t)bi[e] << (8 * e);
    *reinterpret_cast<uint64_t*>(idx + (int64_t)upix * C + cc * 8) = packed;
  }
}

// Max pool backward as a gather (no atomics): each input pixel sums the gradients of the windows
// that selected it; optionally adds a second gradient source (UNet skip-concat slice).
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, int N, int H,
                                   int W, int C, int k, int stride, int pad, int OH, int OW,
                                   const T* __restrict__ add, int ldadd, int addoff, T* __restrict__ dx,
                                   int lddx, int dxoff, FastDiv fdCC, FastDiv fdW, FastDiv fdH) {
  const int CC = C >> 3;
  const int64_t total = (int64_t)N * H * W * CC;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int cc, iw, ih, n;
    int64_t pix;
    if (total < (1ll << 31)) {   // 32-bit fast division (the 64-bit divisions dominated this kernel)
      const uint32_t q = fdiv((uint32_t)i, fdCC);
      cc = (int)((uint32_t)i - q * CC);
      pix = q;
      const uint32_t t2 = fdiv(q, fdW);
      iw = (int)(q - t2 * W);
      const uint32_t nn = fdiv(t2, fdH);
      ih = (int)(t2 - nn * H);
      n = (int)nn;
    } else {
      cc = (int)(i % CC);
      pix = i / CC;
      iw = (int)(pix % W);
      const int64_t t2 = pix / W;
      ih = (int)(t2 % H);
      n = (int)(t2 / H);
    }
    float g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (add) load8(add + pix * ldadd + addoff + cc * 8, g);
    // windows oh with oh*stride - pad <= ih <= oh*stride - pad + k - 1
    int oh_lo = ih + pad - k + 1;
    oh_lo = oh_lo <= 0 ? 0 : (oh_lo + stride - 1) / stride;
    const int oh_hi = min((ih + pad) / stride, OH - 1);
    int ow_lo = iw + pad - k + 1;
    ow_lo = ow_lo <= 0 ? 0 : (ow_lo + stride - 1) / stride;
    const int ow_hi = min((iw + pad) / stride, OW - 1);
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const uint8_t want = (uint8_t)((ih - (oh * stride - pad)) * k + (iw - (ow * stride - pad)));
        const int64_t op = ((int64_t)n * OH + oh) * OW + ow;
        const uint64_t id = *reinterpret_cast<const uint64_t*>(idx + op * C + cc * 8);
        float d[8];
        load8(dy + op * C + cc * 8, d);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (((id >> (8 * e)) & 0xff) == want) g[e] += d[e];
      }
    }
    store8(dx + pix * lddx + dxoff + cc * 8, g);
  }
}

// Max-pool backward (gather, no atomics) fused with the BN-backward statistics of the BN+ReLU
// that produced the pool input (the ResNet stem): dx = [z*scale + shift > 0] * sum of the window
// gradients that selected the element, written as the masked gradient dyr, and per-block partials
// {sum dyr, sum dyr*z} for the fused finalize (raw_z).  Replaces maxpool_bwd + bn_bwd_reduce and
// the mask read of bn_bwd_apply.  `add` (optional): a second gradient of the pool input summed in
// before the mask (the UNet encoder output also feeds the decoder's skip concat).
// NWIN > 0: at most NWIN x NWIN windows hold an input pixel (ceil(k / stride): 2 for the ResNet
// stem's 3x3/s2, 1 for the UNet's 2x2/s2); the candidate loop is unrolled with predication so all
// window loads (index + gradient) are in flight at once instead of one dependent round trip per
// window.  Same summation order as the generic loop (oh, then ow, ascending) -> identical results.
template <int NWIN, typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_bn_kernel(const T* __restrict__ dy,
                                                             const uint8_t* __restrict__ idx, int N, int H, int W,
                                                             int C, int k, int stride, int pad, int OH, int OW,
                                                             FastDiv fdW, FastDiv fdH, const T* __restrict__ z,
                                                             const float* __restrict__ msc,
                                                             const float* __restrict__ msh,
                                                             const T* __restrict__ add, int ldadd, int addoff,
                                                             T* __restrict__ dx, float* __restrict__ partial) {
  const RowMap rm = rowmap(C);
  float acc[2][8] = {};
  const int64_t M = (int64_t)N * H * W;
  if (rm.active) {
    const int c0 = rm.cc * 8;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = msc[c0 + e]; sh[e] = msh[c0 + e]; }
    for (int64_t row = (int64_t)blockIdx.x * rm.RPB + rm.rr; row < M; row += (int64_t)gridDim.x * rm.RPB) {
      const uint32_t pix = (uint32_t)row;
      const uint32_t t2 = fdiv(pix, fdW);
      const int iw = (int)(pix - t2 * W);
      const uint32_t n = fdiv(t2, fdH);
      const int ih = (int)(t2 - n * H);
      float g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int oh_lo = ih + pad - k + 1;
      oh_lo = oh_lo <= 0 ? 0 : (oh_lo + stride - 1) / stride;
      const int oh_hi = min((ih + pad) / stride, OH - 1);
      int ow_lo = iw + pad - k + 1;
      ow_lo = ow_lo <= 0 ? 0 : (ow_lo + stride - 1) / stride;
      const int ow_hi = min((iw + pad) / stride, OW - 1);
      if constexpr (NWIN > 0) {
        uint64_t id[NWIN * NWIN];
        typename Vec8<T>::type dv[NWIN * NWIN];
#pragma unroll
        for (int a = 0; a < NWIN; ++a)
#pragma unroll
          for (int b = 0; b < NWIN; ++b) {
            const bool ok = oh_lo + a <= oh_hi && ow_lo + b <= ow_hi;
            const int64_t op = ok ? ((int64_t)n * OH + oh_lo + a) * OW + ow_lo + b : 0;   // 0: a valid address
            id[a * NWIN + b] = *reinterpret_cast<const uint64_t*>(idx + op * C + c0);
            dv[a * NWIN + b] = raw8(dy + op * C + c0);
          }
#pragma unroll
        for (int a = 0; a < NWIN; ++a)
#pragma unroll
          for (int b = 0; b < NWIN; ++b) {
            const bool ok = oh_lo + a <= oh_hi && ow_lo + b <= ow_hi;
            const int want = ok ? (ih - ((oh_lo + a) * stride - pad)) * k + (iw - ((ow_lo + b) * stride - pad)) : 256;
            float d[8];
            unpack8(dv[a * NWIN + b], d);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if ((int)((id[a * NWIN + b] >> (8 * e)) & 0xff) == want) g[e] += d[e];
          }
      } else {
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
          for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            const uint8_t want = (uint8_t)((ih - (oh * stride - pad)) * k + (iw - (ow * stride - pad)));
            const int64_t op = ((int64_t)n * OH + oh) * OW + ow;
            const uint64_t id = *reinterpret_cast<const uint64_t*>(idx + op * C + c0);
            float d[8];
            load8(dy + op * C + c0, d);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (((id >> (8 * e)) & 0xff) == want) g[e] += d[e];
          }
        }
      }
      if (add) {   // second gradient source of the pool input (UNet: its skip-concat slice)
        float a2[8];
        load8(add + row * ldadd + addoff + c0, a2);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] += a2[e];
      }
      float zz[8];
      load8(z + row * C + c0, zz);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = zz[e] * sc[e] + sh[e] > 0.f ? g[e] : 0.f;
      store8(dx + row * C + c0, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // statistics of the stored gradient
        const float r = stored<T>(g[e]);
        acc[0][e] += r;
        acc[1][e] += r * zz[e];
      }
    }
  }
  block_combine<2>(acc, rm, C, partial);
}

// Global average pool [N][HW][C] -> [N][C]
template <typename T>
__global__ void avgpool_fwd_kernel(const T* __restrict__ x, int N, int HW, int C, T* __restrict__ y) {
  const int CC = C >> 3;
  const int64_t total = (int64_t)N * CC;
  const float inv = 1.f / (float)HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cc = (int)(i % CC);
    const int n = (int)(i / CC);
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < HW; ++p) {
      float v[8];
      load8(x + ((int64_t)n * HW + p) * C + cc * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] *= inv;
    store8(y + (int64_t)n * C + cc * 8, s);
  }
}

template <typename T>
__global__ void avgpool_bwd_kernel(const T* __restrict__ dy, int N, int HW, int C, T* __restrict__ dx) {
  const int CC = C >> 3;
  const int64_t total = (int64_t)N * HW * CC;
  const float inv = 1.f / (float)HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cc = (int)(i % CC);
    const int64_t pix = i / CC;
    const int n = (int)(pix / HW);
    float v[8];
    load8(dy + (int64_t)n * C + cc * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= inv;
    store8(dx + pix * C + cc * 8, v);
  }
}

// NCHW fp32 -> NHWC T with channel zero-padding to Cpad (multiple of 8).
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, int N, int C, int H, int W, int Cpad,
                                    T* __restrict__ y) {
  const int CC = Cpad >> 3;
  const int64_t HW = (int64_t)H * W;
  const int64_t total = (int64_t)N * HW * CC;
  if (total < (1ll << 31) && N * HW * C < (1ll << 31)) {   // 32-bit index math (no 64-bit divisions)
    const uint32_t ut = (uint32_t)total, uCC = CC, uHW = (uint32_t)HW;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ut; i += gridDim.x * blockDim.x) {
      const uint32_t pix = i / uCC;
      const int cc = (int)(i - pix * uCC);
      const uint32_t n = pix / uHW, hw = pix - n * uHW;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = cc * 8 + e;
        v[e] = c < C ? x[(n * (uint32_t)C + c) * uHW + hw] : 0.f;
      }
      store8(y + (int64_t)pix * Cpad + cc * 8, v);
    }
    return;
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = i / CC;   // cc-major inner loop keeps reads of one channel plane coalesced
    const int cc = (int)(i - pix * CC);
    const int64_t n = pix / HW, hw = pix - n * HW;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = cc * 8 + e;
      v[e] = c < C ? x[(n * C + c) * HW + hw] : 0.f;
    }
    store8(y + pix * Cpad + cc * 8, v);
  }
}

// 2x2 space-to-depth of a zero-padded fp32 NCHW image into bf16 NHWC (the strided-stem layout,
// models/engine.py:S2DConvUnit): y[n][u][v][(vh*2 + vw)*CS + c] = x[n][c][2u+vh-pad][2v+vw-pad]
// (zero outside the image and for c >= C).  One thread = 8 output channels of one pixel.
template <typename T>
__global__ void s2d_nchw_kernel(const float* __restrict__ x, int N, int C, int H, int W, int pad, int U, int V, int CS,
                                T* __restrict__ y) {
  const int CT = 4 * CS, CC = CT >> 3;
  const int64_t total = (int64_t)N * U * V * CC;
  if (total < (1ll << 31)) {
    // 32-bit index math (the 64-bit divisions of the general loop dominated it: 90 us at ResNet-50
    // bs 256, 2.9 TB/s); one thread per (pixel, 8-channel group), the same loads and values
    const uint32_t ut = (uint32_t)total, uCC = CC, uV = V, uU = U;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ut; i += gridDim.x * blockDim.x) {
      const uint32_t pix = i / uCC;
      const int g = (int)(i - pix * uCC);
      const uint32_t t = pix / uV;
      const int v = (int)(pix - t * uV);
      const uint32_t n = t / uU;
      const int u = (int)(t - n * uU);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = g * 8 + e, slot = j / CS, c = j - slot * CS;
        const int h = 2 * u + (slot >> 1) - pad, w = 2 * v + (slot & 1) - pad;
        o[e] = (c < C && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
                   ? x[(int64_t)(((int)n * C + c) * H + h) * W + w]
                   : 0.f;
      }
      store8(y + (int64_t)pix * CT + g * 8, o);
    }
    return;
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = i / CC;
    const int g = (int)(i - pix * CC);
    const int v = (int)(pix % V);
    const int64_t t = pix / V;
    const int u = (int)(t % U);
    const int64_t n = t / U;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = g * 8 + e, slot = j / CS, c = j - slot * CS;
      const int h = 2 * u + (slot >> 1) - pad, w = 2 * v + (slot & 1) - pad;
      o[e] = (c < C && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? x[((n * C + c) * H + h) * W + w]
                                                                               : 0.f;
    }
    store8(y + pix * CT + g * 8, o);
  }
}

// Bilinear x2 upsample, align_corners=True: src = o * (in-1)/(out-1).
template <typename T>
__global__ void upsample2x_fwd_kernel(const T* __restrict__ x, int N, int H, int W, int C, int ldx, int xoff,
                                      T* __restrict__ y, int ldy, int yoff) {
  const int OH = 2 * H, OW = 2 * W, CC = C >> 3;
  const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  const int64_t total = (int64_t)N * OH * OW * CC;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cc = (int)(i % CC);
    const int64_t pix = i / CC;
    const int ow = (int)(pix % OW);
    const int64_t t2 = pix / OW;
    const int oh = (int)(t2 % OH);
    const int n = (int)(t2 / OH);
    const float fh = oh * sh, fw = ow * sw;
    const int h0 = (int)fh, w0 = (int)fw;
    const int h1 = min(h0 + 1, H - 1), w1 = min(w0 + 1, W - 1);
    const float lh = fh - h0, lw = fw - w0;
    float a[8], b[8], c[8], d[8], o[8];
    const int64_t base = (int64_t)n * H;
    load8(x + ((base + h0) * W + w0) * ldx + xoff + cc * 8, a);
    load8(x + ((base + h0) * W + w1) * ldx + xoff + cc * 8, b);
    load8(x + ((base + h1) * W + w0) * ldx + xoff + cc * 8, c);
    load8(x + ((base + h1) * W + w1) * ldx + xoff + cc * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = (1.f - lh) * ((1.f - lw) * a[e] + lw * b[e]) + lh * ((1.f - lw) * c[e] + lw * d[e]);
    store8(y + pix * ldy + yoff + cc * 8, o);
  }
}

// Bilinear x2 backward as a GATHER (deterministic, no atomics): input pixel (h, w) sums, in
// ascending (oh, ow) order, the output gradients whose interpolation footprint contains it, with the
// forward's own weights (same fh = oh * sh, h0 = (int) fh, lh = fh - h0 arithmetic).  An output row
// oh touches input rows h0(oh) and h1(oh) = min(h0 + 1, H - 1) with h0 = floor(oh * sh) monotone in
// oh, so h receives from h0 in {h - 1, h}: oh in [(h - 1) / sh, (h + 1) / sh), widened by one row
// each side against rounding (sh = (H-1)/(2H-1) < 1/2: at most ~2/sh + 3 candidate rows).
__device__ __forceinline__ void bilin_rows(int o, float s, int n_in, int& i0, int& i1, float& l) {
  const float f = o * s;
  i0 = (int)f;
  i1 = min(i0 + 1, n_in - 1);
  l = f - i0;
}

template <typename T>
__global__ void upsample2x_bwd_kernel(const T* __restrict__ dy, int N, int H, int W, int C, int lddy, int dyoff,
                                      T* __restrict__ dx) {
  const int OH = 2 * H, OW = 2 * W, CC = C >> 3;
  const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  const int64_t total = (int64_t)N * H * W * CC;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int cc = (int)(i % CC);
    const int64_t pix = i / CC;
    const int w = (int)(pix % W);
    const int64_t t2 = pix / W;
    const int h = (int)(t2 % H);
    const int n = (int)(t2 / H);
    int oh_lo = 0, oh_hi = OH - 1, ow_lo = 0, ow_hi = OW - 1;
    if (sh > 0.f) {
      oh_lo = max(0, (int)floorf((h - 1) / sh) - 1);
      oh_hi = min(OH - 1, (int)((h + 1) / sh) + 1);
    }
    if (sw > 0.f) {
      ow_lo = max(0, (int)floorf((w - 1) / sw) - 1);
      ow_hi = min(OW - 1, (int)((w + 1) / sw) + 1);
    }
    float g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      int h0, h1;
      float lh;
      bilin_rows(oh, sh, H, h0, h1, lh);
      const float wh = (h0 == h ? 1.f - lh : 0.f) + (h1 == h ? lh : 0.f);
      if (h0 != h && h1 != h) continue;
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        int w0, w1;
        float lw;
        bilin_rows(ow, sw, W, w0, w1, lw);
        if (w0 != w && w1 != w) continue;
        const float ww = (w0 == w ? 1.f - lw : 0.f) + (w1 == w ? lw : 0.f);
        float d[8];
        load8(dy + (((int64_t)n * OH + oh) * OW + ow) * lddy + dyoff + cc * 8, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] += wh * ww * d[e];
      }
    }
    store8(dx + pix * C + cc * 8, g);
  }
}

}  // namespace dlmpi

using namespace dlmpi;

// f32: 1 = fp32 activations (the fp32 precision path), 0 = bf16 (uint16_t storage)
extern "C" hipError_t dlmpi_maxpool_fwd(const void* x, int N, int H, int W, int C, int ldx, int xoff, int k,
                                        int stride, int pad, void* y, uint8_t* idx, int OH, int OW,
                                        const float* scale, const float* shift, void* ys, int ldys, int ysoff,
                                        int f32, hipStream_t s) {
  if (C < 8 || C % 8) return hipErrorInvalidValue;
  // idx is one byte per element (k * k - 1 <= 255); 2 * pad > k would leave a window wholly in padding
  if (k < 1 || k > 16 || stride < 1 || pad < 0 || 2 * pad > k) return hipErrorInvalidValue;
  // ys: K == S, no padding, the windows tile the input exactly, an applied input (scale / shift)
  if (ys && (!scale || !shift || k != 2 || stride != 2 || pad != 0 || H != 2 * OH || W != 2 * OW || ldys % 8 ||
             ysoff % 8))
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)N * OH * OW * (C / 8);
  if (total >= (1ll << 31)) return hipErrorInvalidValue;
  const FastDiv a = make_fastdiv(C / 8), b = make_fastdiv(OW), c = make_fastdiv(OH);
  const dim3 g = pool_grid(total);
#define LAUNCH_MPF(K_, S_)                                                                                        \
  WITH_T(f32, hipLaunchKernelGGL((maxpool_fwd_fixed_kernel<K_, S_, T>), g, dim3(256), 0, s, (const T*)x, N, H, W, C, \
                                 ldx, xoff, pad, (T*)y, idx, OH, OW, scale, shift, a, b, c, (T*)ys, ldys, ysoff))
  if (k == 3 && stride == 2 && H > 0 && W > 0) LAUNCH_MPF(3, 2);
  else if (k == 2 && stride == 2 && H > 0 && W > 0) LAUNCH_MPF(2, 2);
  else
    WITH_T(f32, hipLaunchKernelGGL(maxpool_fwd_kernel<T>, g, dim3(256), 0, s, (const T*)x, N, H, W, C, ldx, xoff, k,
                                   stride, pad, (T*)y, idx, OH, OW, scale, shift, a, b, c));
#undef LAUNCH_MPF
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_maxpool_bwd(const void* dy, const uint8_t* idx, int N, int H, int W, int C, int k,
                                        int stride, int pad, int OH, int OW, const void* add, int ldadd,
                                        int addoff, void* dx, int lddx, int dxoff, int f32, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  const int64_t total = (int64_t)N * H * W * (C / 8);
  WITH_T(f32, hipLaunchKernelGGL(maxpool_bwd_kernel<T>, pool_grid(total), dim3(256), 0, s, (const T*)dy, idx, N, H, W,
                                 C, k, stride, pad, OH, OW, (const T*)add, ldadd, addoff, (T*)dx, lddx, dxoff,
                                 make_fastdiv(C / 8), make_fastdiv(W), make_fastdiv(H)));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_maxpool_bwd_bn(const void* dy, const uint8_t* idx, int N, int H, int W, int C, int k,
                                           int stride, int pad, int OH, int OW, const void* z, const float* mscale,
                                           const float* mshift, const void* add, int ldadd, int addoff,
                                           void* dx, float* partial, int nblk, int f32, hipStream_t s) {
  if (C % 8 || C > 2048 || (int64_t)N * H * W >= (1ll << 31)) return hipErrorInvalidValue;
  const int nw = (k + stride - 1) / stride;
#define LAUNCH_MPB(NW)                                                                                              \
  WITH_T(f32, hipLaunchKernelGGL((maxpool_bwd_bn_kernel<NW, T>), dim3(nblk), dim3(256), 0, s, (const T*)dy, idx, N, H, \
                                 W, C, k, stride, pad, OH, OW, make_fastdiv(W), make_fastdiv(H), (const T*)z, mscale, \
                                 mshift, (const T*)add, ldadd, addoff, (T*)dx, partial))
  // fixed window extents for the 2x2/s2 and 3x3/s2 pools; NW 0: the general window loop
  if (nw == 1) LAUNCH_MPB(1);
  else if (nw == 2) LAUNCH_MPB(2);
  else LAUNCH_MPB(0);
#undef LAUNCH_MPB
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_avgpool_fwd(const void* x, int N, int HW, int C, void* y, int f32, hipStream_t s) {
  if (C < 8 || C % 8 || HW < 1) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(avgpool_fwd_kernel<T>, pool_grid((int64_t)N * (C / 8)), dim3(256), 0, s, (const T*)x,
                                 N, HW, C, (T*)y));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_avgpool_bwd(const void* dy, int N, int HW, int C, void* dx, int f32, hipStream_t s) {
  if (C < 8 || C % 8 || HW < 1) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(avgpool_bwd_kernel<T>, pool_grid((int64_t)N * HW * (C / 8)), dim3(256), 0, s,
                                 (const T*)dy, N, HW, C, (T*)dx));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_nchw_to_nhwc(const float* x, int N, int C, int H, int W, int Cpad, void* y, int f32,
                                         hipStream_t s) {
  if (Cpad % 8 || Cpad < C) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, pool_grid((int64_t)N * H * W * (Cpad / 8)), dim3(256), 0, s,
                                 x, N, C, H, W, Cpad, (T*)y));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_s2d_nchw(const float* x, int N, int C, int H, int W, int pad, int U, int V, int CS,
                                     void* y, int f32, hipStream_t s) {
  if ((4 * CS) % 8 || C > CS) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(s2d_nchw_kernel<T>, pool_grid((int64_t)N * U * V * (CS / 2)), dim3(256), 0, s, x, N,
                                 C, H, W, pad, U, V, CS, (T*)y));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_upsample2x_fwd(const void* x, int N, int H, int W, int C, int ldx, int xoff, void* y,
                                           int ldy, int yoff, int f32, hipStream_t s) {
  if (C < 8 || C % 8 || H < 1 || W < 1) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(upsample2x_fwd_kernel<T>, pool_grid((int64_t)N * 4 * H * W * (C / 8)), dim3(256), 0,
                                 s, (const T*)x, N, H, W, C, ldx, xoff, (T*)y, ldy, yoff));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_upsample2x_bwd(const void* dy, int N, int H, int W, int C, int lddy, int dyoff, void* dx,
                                           int f32, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(upsample2x_bwd_kernel<T>, pool_grid((int64_t)N * H * W * (C / 8)), dim3(256), 0, s,
                                 (const T*)dy, N, H, W, C, lddy, dyoff, (T*)dx));
  return hipGetLastError();
}
