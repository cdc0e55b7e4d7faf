// 1x1 convolution with at most 4 output channels -- the UNet head, Conv2d(64, n_classes, 1) with
// n_classes = 1 for the binary masks (/root/reference/pytorch/unet/model.py:68, train.py:160) --
// as a streaming dot product:  y[m][k] = sum_c x[m][c] * w[k][c] + b[k].
//
// Through the GEMM it was a 128 x 64 tile per 128 rows with 63 of 64 output columns discarded
// (244 us for the 16 x 512^2 x 64 input = 2.2 TB/s).  Here L = C / 8 lanes share a row (16 B each,
// so one wave instruction reads 64 / L whole rows = 1 KB contiguous), each lane forms its 8-channel
// partial dot for every output channel in fp32 (weights in registers), and the L partials are
// combined by a fixed xor-shuffle tree; the first lane of the row adds the bias and stores.  Four
// row groups per wave are in flight per iteration.  The result differs from the MFMA path only in
// the fp32 summation order.
// psc / psh (optional): the input is a deferred BN-apply + ReLU of x -- bf16(relu(fma(x, psc, psh))),
// bn_apply_kernel's arithmetic, so identical to reading the stored BN output -- computed on the fly.
//
// Below it, the head's data gradients into the BN+ReLU output it reads.
#include "rowreduce.h"

namespace dlmpi {

template <int L, int KV, typename TO>
__global__ __launch_bounds__(256) void head1x1_kernel(const uint16_t* __restrict__ x, int ldx, int xoff, int64_t M,
                                                      const uint16_t* __restrict__ w, int ldw,
                                                      const float* __restrict__ bias, TO* __restrict__ y, int ldy,
                                                      int yoff, const float* __restrict__ psc,
                                                      const float* __restrict__ psh) {
  constexpr int RPW = 64 / L;   // rows per wave instruction
  constexpr int U = 4;          // row groups in flight per wave
  const int lane = threadIdx.x & 63;
  const int sub = lane % L, rw = lane / L;
  float wv[KV][8], b[KV];
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    load8(w + (int64_t)k * ldw + sub * 8, wv[k]);
    b[k] = bias ? bias[k] : 0.f;
  }
  float ps[8], ph[8];
  if (psc)
#pragma unroll
    for (int e = 0; e < 8; ++e) { ps[e] = psc[sub * 8 + e]; ph[e] = psh[sub * 8 + e]; }
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * 4 * RPW * U;
  for (int64_t base = wave * RPW * U; base < M; base += step) {
    float v[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = base + u * RPW + rw;
      if (row < M) load8(x + row * ldx + xoff + sub * 8, v[u]);
      else
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
      if (psc)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u][e] = bf2f(f2bf(fmaxf(__builtin_fmaf(v[u][e], ps[e], ph[e]), 0.f)));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = base + u * RPW + rw;
#pragma unroll
      for (int k = 0; k < KV; ++k) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = __builtin_fmaf(v[u][e], wv[k][e], s);
#pragma unroll
        for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (sub == 0 && row < M) store1(y + row * ldy + yoff + k, s + b[k]);
      }
    }
  }
}

// Data gradient of a 1x1 convolution with ONE output channel (the UNet head, reference
// model.py:68) into the gradient of the BN+ReLU output below it: dx[m, c] = dy[m] * w[c] -- an
// outer product, so a streaming kernel instead of a GEMM tile with 63 of 64 reduction lanes zero
// -- masked by [z*scale + shift > 0], stored, and the BN-backward partials {sum dx, sum dx*z} per
// block.  The bf16 x bf16 product is exact in fp32, as in the GEMM path: identical dx.
template <typename T>
__global__ __launch_bounds__(256) void outer_dgrad_bn_kernel(const T* __restrict__ dy, int lddy, int64_t M,
                                                             int C, const T* __restrict__ w, int ldw,
                                                             const T* __restrict__ z,
                                                             const float* __restrict__ msc,
                                                             const float* __restrict__ msh,
                                                             T* __restrict__ dx, float* __restrict__ partial) {
  const RowMap rm = rowmap(C);
  float acc[2][8] = {};
  if (rm.active) {
    const int c0 = rm.cc * 8;
    float wv[8], sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wv[e] = load1(w + (int64_t)(c0 + e) * ldw);
      sc[e] = msc[c0 + e];
      sh[e] = msh[c0 + e];
    }
    for (int64_t row = (int64_t)blockIdx.x * rm.RPB + rm.rr; row < M; row += (int64_t)gridDim.x * rm.RPB) {
      const float d = load1(dy + row * lddy);
      float zz[8], g[8];
      load8(z + row * C + c0, zz);
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = zz[e] * sc[e] + sh[e] > 0.f ? d * wv[e] : 0.f;
      store8(dx + row * C + c0, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float r = stored<T>(g[e]);
        acc[0][e] += r;
        acc[1][e] += r * zz[e];
      }
    }
  }
  block_combine<2>(acc, rm, C, partial);
}

// The same for a 1x1 convolution with K = 2..4 output channels (the multi-class UNet head):
// dx[m, c] = [z*scale + shift > 0] * sum_k dl[m, k] * w[c, k], summed in fp32 in ascending k.  The GEMM
// path pads the reduction from K to 8; here a row costs K broadcast loads of dl beside the z read and
// the dx write.  Same row map, partial layout [blocks][2][C] and finalize as the K = 1 kernel.
template <int K, typename T>
__global__ __launch_bounds__(256) void head_dgrad_bn_kernel(const T* __restrict__ dl, int lddl, int64_t M, int C,
                                                            const T* __restrict__ w, int ldw,
                                                            const T* __restrict__ z,
                                                            const float* __restrict__ msc,
                                                            const float* __restrict__ msh,
                                                            T* __restrict__ dx, float* __restrict__ partial) {
  const RowMap rm = rowmap(C);
  float acc[2][8] = {};
  if (rm.active) {
    const int c0 = rm.cc * 8;
    float wv[K][8], sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int k = 0; k < K; ++k) wv[k][e] = load1(w + (int64_t)(c0 + e) * ldw + k);
      sc[e] = msc[c0 + e];
      sh[e] = msh[c0 + e];
    }
    for (int64_t row = (int64_t)blockIdx.x * rm.RPB + rm.rr; row < M; row += (int64_t)gridDim.x * rm.RPB) {
      float d[K];
#pragma unroll
      for (int k = 0; k < K; ++k) d[k] = load1(dl + row * lddl + k);
      float zz[8], g[8];
      load8(z + row * C + c0, zz);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float a = d[0] * wv[0][e];
#pragma unroll
        for (int k = 1; k < K; ++k) a += d[k] * wv[k][e];
        g[e] = zz[e] * sc[e] + sh[e] > 0.f ? a : 0.f;
      }
      store8(dx + row * C + c0, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float r = stored<T>(g[e]);
        acc[0][e] += r;
        acc[1][e] += r * zz[e];
      }
    }
  }
  block_combine<2>(acc, rm, C, partial);
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_head1x1_ok(int C, int kv) {
  return kv >= 1 && kv <= 4 && (C == 16 || C == 32 || C == 64 || C == 128 || C == 256 || C == 512);
}

extern "C" hipError_t dlmpi_head1x1(const void* x, int ldx, int xoff, int64_t M, int C, const void* w, int ldw,
                                    const float* bias, void* y, int ldy, int yoff, int kv, int y_f32,
                                    const float* psc, const float* psh, hipStream_t s) {
  if ((psc == nullptr) != (psh == nullptr)) return hipErrorInvalidValue;
  if (!dlmpi_head1x1_ok(C, kv) || M <= 0 || ldx % 8 || xoff % 8 || ldw % 8) return hipErrorInvalidValue;
  const int L = C / 8;
  const int64_t rows_per_block = 4LL * (64 / L) * 4;
  const unsigned nblk = (unsigned)std::min<int64_t>((M + rows_per_block - 1) / rows_per_block, 4096);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const uint16_t* wp = static_cast<const uint16_t*>(w);
#define HEAD_KV(L_, KV_)                                                                                        \
  WITH_T(y_f32, hipLaunchKernelGGL((head1x1_kernel<L_, KV_, T>), dim3(nblk), dim3(256), 0, s, xp, ldx, xoff, M, wp, \
                                   ldw, bias, (T*)y, ldy, yoff, psc, psh))
#define HEAD_L(L_)                        \
  do {                                    \
    if (kv == 1) HEAD_KV(L_, 1);          \
    else if (kv == 2) HEAD_KV(L_, 2);     \
    else if (kv == 3) HEAD_KV(L_, 3);     \
    else HEAD_KV(L_, 4);                  \
  } while (0)
  switch (L) {
    case 2: HEAD_L(2); break;
    case 4: HEAD_L(4); break;
    case 8: HEAD_L(8); break;
    case 16: HEAD_L(16); break;
    case 32: HEAD_L(32); break;
    default: HEAD_L(64); break;
  }
#undef HEAD_L
#undef HEAD_KV
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_outer_dgrad_bn(const void* dy, int lddy, int64_t M, int C, const void* w, int ldw,
                                           const void* z, const float* mscale, const float* mshift, void* dx,
                                           float* partial, int nblk, int f32, hipStream_t s) {
  if (C % 8 || C > 2048 || M <= 0) return hipErrorInvalidValue;
  WITH_T(f32, hipLaunchKernelGGL(outer_dgrad_bn_kernel<T>, dim3(nblk), dim3(256), 0, s, (const T*)dy, lddy, M, C,
                                 (const T*)w, ldw, (const T*)z, mscale, mshift, (T*)dx, partial));
  return hipGetLastError();
}

// dl [M][lddl] (columns 0..K-1 read), w [C][ldw] (w[c][k] = the head weight of class k, channel c)
extern "C" hipError_t dlmpi_head_dgrad_bn(const void* dl, int lddl, int K, int64_t M, int C, const void* w, int ldw,
                                          const void* z, const float* mscale, const float* mshift, void* dx,
                                          float* partial, int nblk, int f32, hipStream_t s) {
  if (C % 8 || C > 2048 || M <= 0 || K < 2 || K > 4 || lddl < K || ldw < K || nblk < 1) return hipErrorInvalidValue;
#define HEAD_DGRAD(K_)                                                                                            \
  WITH_T(f32, hipLaunchKernelGGL((head_dgrad_bn_kernel<K_, T>), dim3(nblk), dim3(256), 0, s, (const T*)dl, lddl, M, \
                                 C, (const T*)w, ldw, (const T*)z, mscale, mshift, (T*)dx, partial))
  if (K == 2) HEAD_DGRAD(2);
  else if (K == 3) HEAD_DGRAD(3);
  else HEAD_DGRAD(4);
#undef HEAD_DGRAD
  return hipGetLastError();
}
