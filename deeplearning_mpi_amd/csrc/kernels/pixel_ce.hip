// Multi-class segmentation: pixel-wise softmax cross-entropy (forward / backward), exact
// per-sample / per-class segmentation counts, and the NHWC pad-cast of a channels-last loss gradient.
//
// The loss kernels are bandwidth-bound over M = N*H*W pixels and K (2..256, tuned for <= 32)
// classes: every lane owns pixels, not classes (loss.hip's one-block-per-row kernel is built for
// 256 x 1000 classification logits).  Logits are fp32 and addressed by (sample, class, pixel)
// element strides, so the engine's NHWC buffer viewed as [N, K, H, W] (class stride 1) and plain
// NCHW (class stride H*W) both run in place; dlogits is written in the same strides.
// Labels are int64 [N*H*W]; a label equal to ignore_index or outside [0, K) is ignored.  With a
// per-class weight w the loss is sum w[t] nll / sum w[t] over the kept pixels (torch semantics;
// all pixels ignored -> 0 / 0 = NaN, gradient exactly zero).
// Reductions are two-stage with a fixed order, no float atomics: the same bits on every run.
// The softmax arithmetic, the addressing, the block reduction and the tile copy are pixel_softmax.h's,
// shared with the fused CE + Dice kernels of seg_dice.hip.
#include "pixel_softmax.h"

namespace dlmpi {

constexpr int kPixBlocksMax = 2048;

// lse[m] = logsumexp_k x[m][k]; partial[blk] = {sum w[t] (lse - x[t]), sum w[t]} over the block's kept pixels
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void pixel_ce_fwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                           int64_t HW, int64_t M,
                                                           const int64_t* __restrict__ labels, int64_t ignore_index,
                                                           const float* __restrict__ weight,
                                                           float* __restrict__ lse, float* __restrict__ partial) {
  __shared__ float shf[8];
  float ce[2] = {0.f, 0.f};   // {sum w nll, sum w}
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const float* x = logits + n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    float l, xt = 0.f;
    if constexpr (KC > 0) {
      float v[KC];
      pix_load<KC, VEC>(x, st.sk, v);
      const PixSoftmax r = pix_softmax_reg<KC>(v, lab);
      l = r.mx + __logf(r.s);
      xt = r.xt;
    } else {
      l = pix_online_lse(x, st.sk, K);
      if (keep) xt = x[lab * st.sk];
    }
    lse[m] = l;
    if (keep) pix_ce_add(ce, weight, lab, l, xt);
  }
  pix_ce_block_store(ce, shf, partial + 2 * blockIdx.x);
}

// Class-last ([M][K] contiguous) logits with K > 4.  A lane that walks its own pixel's K floats makes
// every load of the wave touch 64 cache lines (4 bytes used of each), and the lines are evicted before
// the next class reads them (K = 21: several times slower than a plain read of the same bytes,
// benchmarks/multiclass_bench.py times both through dlmpi_set_pixel_tiles).  So a block
// stages P pixels (P * K contiguous floats, 16-byte loads: tiles start 16-byte aligned here, phase 0) in
// LDS and each of the first P threads reduces its row from there (pix_row_lse).
__global__ __launch_bounds__(256) void pixel_ce_fwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                                int64_t M, const int64_t* __restrict__ labels,
                                                                int64_t ignore_index,
                                                                const float* __restrict__ weight,
                                                                float* __restrict__ lse,
                                                                float* __restrict__ partial) {
  extern __shared__ __align__(16) float tile[];
  __shared__ float shf[8];
  float ce[2] = {0.f, 0.f};
  const int64_t ntiles = (M + P - 1) / P;
  const int k0 = threadIdx.x % K;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m0 = t * P;
    const int np = (int)(M - m0 < P ? M - m0 : P);
    pix_tile_copy<true>(tile, const_cast<float*>(logits + m0 * K), np * K, 0);
    __syncthreads();
    if ((int)threadIdx.x < np) {
      const float* row = tile + threadIdx.x * K;
      const float l = pix_row_lse(row, K, k0);
      const int64_t m = m0 + threadIdx.x;
      const int64_t lab = labels[m];
      lse[m] = l;
      if (pix_kept(lab, K, ignore_index)) pix_ce_add(ce, weight, lab, l, row[lab]);
    }
    __syncthreads();
  }
  pix_ce_block_store(ce, shf, partial + 2 * blockIdx.x);
}

// the backward through the same tiles: the row is turned into its gradient in LDS and stored with 16-byte stores
__global__ __launch_bounds__(256) void pixel_ce_bwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                                int64_t M, const int64_t* __restrict__ labels,
                                                                int64_t ignore_index,
                                                                const float* __restrict__ weight,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ go,
                                                                const float* __restrict__ den,
                                                                float* __restrict__ dlogits) {
  extern __shared__ __align__(16) float tile[];
  const float g0 = (go ? *go : 1.f) / *den;
  const int64_t ntiles = (M + P - 1) / P;
  const int k0 = threadIdx.x % K;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m0 = t * P;
    const int np = (int)(M - m0 < P ? M - m0 : P);
    const int nf = np * K;
    pix_tile_copy<true>(tile, const_cast<float*>(logits + m0 * K), nf, 0);
    __syncthreads();
    if ((int)threadIdx.x < np) {
      float* row = tile + threadIdx.x * K;
      const int64_t m = m0 + threadIdx.x;
      const int64_t lab = labels[m];
      int kk = k0;
      if (pix_kept(lab, K, ignore_index)) {
        const float g = g0 * (weight ? weight[lab] : 1.f);
        const float l = lse[m];
        for (int k = 0; k < K; ++k) {
          row[kk] = (__expf(row[kk] - l) - ((int64_t)kk == lab ? 1.f : 0.f)) * g;
          kk = pix_row_next(kk, K);
        }
      } else {
        pix_row_zero(row, K, k0);
      }
    }
    __syncthreads();
    pix_tile_copy<false>(tile, dlogits + m0 * K, nf, 0);
    __syncthreads();
  }
}

// loss = sum partial[.][0] / sum partial[.][1]; den = the denominator, kept for the backward
__global__ __launch_bounds__(256) void pixel_ce_finish_kernel(const float* __restrict__ partial, int nblk,
                                                              float* __restrict__ loss, float* __restrict__ den) {
  __shared__ double sh[2][4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    a += (double)partial[2 * i];
    b += (double)partial[2 * i + 1];
  }
  a = warp_sum_d(a);
  b = warp_sum_d(b);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = a; sh[1][wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    b = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    *loss = (float)(a / b);
    *den = (float)b;
  }
}

// dlogits[m][k] = (exp(x[m][k] - lse[m]) - [k == t]) * w[t] * go / den; exact zeros at ignored pixels
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void pixel_ce_bwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                           int64_t HW, int64_t M,
                                                           const int64_t* __restrict__ labels, int64_t ignore_index,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ go,
                                                           const float* __restrict__ den,
                                                           float* __restrict__ dlogits) {
  const float g0 = (go ? *go : 1.f) / *den;
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const int64_t off = n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    float g = 0.f;
    if (keep) g = g0 * (weight ? weight[lab] : 1.f);
    const float l = lse[m];
    if constexpr (KC > 0) {
      float v[KC];
      if (keep) {
        pix_load<KC, VEC>(logits + off, st.sk, v);
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = (__expf(v[k] - l) - ((int64_t)k == lab ? 1.f : 0.f)) * g;
      } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = 0.f;
      }
      pix_store<KC, VEC>(dlogits + off, st.sk, v);
    } else {
      if (keep) {
        for (int k = 0; k < K; ++k)
          dlogits[off + k * st.sk] = (__expf(logits[off + k * st.sk] - l) - ((int64_t)k == lab ? 1.f : 0.f)) * g;
      } else {
        for (int k = 0; k < K; ++k) dlogits[off + k * st.sk] = 0.f;
      }
    }
  }
}

// counts[n][c] = {|pred = c and target = c|, |pred = c|, |target = c|} over the kept pixels of sample n,
// pred = argmax_k (ties to the lowest index).  Integer LDS histogram per block, integer atomics into
// the zeroed output: exact in any order.
__global__ __launch_bounds__(256) void seg_counts_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                         int64_t HW, const int64_t* __restrict__ labels,
                                                         int64_t ignore_index,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned int h[256 * 3];
  for (int i = threadIdx.x; i < K * 3; i += 256) h[i] = 0u;
  __syncthreads();
  const int n = blockIdx.y;
  const float* xs = logits + (int64_t)n * st.sn;
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int64_t lab = labels[(int64_t)n * HW + p];
    if (!pix_kept(lab, K, ignore_index)) continue;
    const float* x = xs + p * st.sp;
    float bv = x[0];
    int bi = 0;
    for (int k = 1; k < K; ++k) {
      const float v = x[k * st.sk];
      if (v > bv) { bv = v; bi = k; }
    }
    if (bi == (int)lab) atomicAdd(&h[bi * 3], 1u);
    atomicAdd(&h[bi * 3 + 1], 1u);
    atomicAdd(&h[(int)lab * 3 + 2], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * 3; i += 256)
    if (h[i]) atomicAdd(&counts[(int64_t)n * K * 3 + i], (unsigned long long)h[i]);
}

// x [M][K] fp32 -> y [M][Kp] storage type, columns K..Kp-1 zero (Kp a multiple of 8)
template <typename T>
__global__ __launch_bounds__(256) void nhwc_pad_cast_kernel(const float* __restrict__ x, int64_t M, int K, int Kp,
                                                            T* __restrict__ y) {
  const int CC = Kp >> 3;
  const int64_t total = M * CC;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / CC;
    const int c0 = (int)(i - m * CC) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c0 + e < K ? x[m * K + c0 + e] : 0.f;
    store8(y + m * Kp + c0, v);
  }
}

static inline unsigned pix_blocks(int64_t M) {
  int64_t b = (M + 255) / 256;
  if (b > kPixBlocksMax) b = kPixBlocksMax;
  if (b < 1) b = 1;
  return (unsigned)b;
}
static inline unsigned ew_blocks_pix(int64_t total) {
  int64_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_pixel_ce_blocks(int64_t M) { return (int)pix_blocks(M); }

static bool pix_args_ok(int K, int64_t HW, int N) { return K >= 2 && K <= 256 && HW > 0 && N > 0; }

// 0: the lane-per-pixel kernels everywhere, here and in seg_dice.hip (A/B; pix_tile_pixels)
extern "C" void dlmpi_set_pixel_tiles(int on) { g_pix_tiles = on; }

// partial: [dlmpi_pixel_ce_blocks(N * HW)][2] floats; loss, den: one float each
extern "C" hipError_t dlmpi_pixel_ce_fwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                         int64_t HW, const int64_t* labels, int64_t ignore_index,
                                         const float* weight, float* lse, float* partial, float* loss, float* den,
                                         hipStream_t s) {
  if (!pix_args_ok(K, HW, N)) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  const unsigned nblk = pix_blocks(M);
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, nullptr, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, nullptr, K, HW, sn, sk, sp);
  if (P > 0)
    hipLaunchKernelGGL(pixel_ce_fwd_tile_kernel, dim3(nblk), dim3(256), (size_t)P * K * sizeof(float), s, logits, K, P,
                       M, labels, ignore_index, weight, lse, partial);
  else
    PIX_DISPATCH(pixel_ce_fwd_kernel, dim3(nblk), vec, logits, st, K, HW, M, labels, ignore_index, weight, lse,
                 partial);
  hipLaunchKernelGGL(pixel_ce_finish_kernel, dim3(1), dim3(256), 0, s, partial, (int)nblk, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_pixel_ce_bwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                         int64_t HW, const int64_t* labels, int64_t ignore_index,
                                         const float* weight, const float* lse, const float* go, const float* den,
                                         float* dlogits, hipStream_t s) {
  if (!pix_args_ok(K, HW, N) || !den) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, dlogits, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, dlogits, K, HW, sn, sk, sp);
  if (P > 0)
    hipLaunchKernelGGL(pixel_ce_bwd_tile_kernel, dim3(ew_blocks_pix((M + P - 1) / P * 256)), dim3(256),
                       (size_t)P * K * sizeof(float), s, logits, K, P, M, labels, ignore_index, weight, lse, go, den,
                       dlogits);
  else
    PIX_DISPATCH(pixel_ce_bwd_kernel, dim3(ew_blocks_pix(M)), vec, logits, st, K, HW, M, labels, ignore_index, weight,
                 lse, go, den, dlogits);
  return hipGetLastError();
}

// counts: int64 [N][K][3], zeroed here (on the stream)
extern "C" hipError_t dlmpi_seg_counts(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                       int64_t HW, const int64_t* labels, int64_t ignore_index, int64_t* counts,
                                       hipStream_t s) {
  if (!pix_args_ok(K, HW, N) || N > 65535) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * K * 3 * sizeof(int64_t), s);
  if (e != hipSuccess) return e;
  int64_t bx = (HW + 256 * 8 - 1) / (256 * 8);   // ~8 pixels per thread: few global atomics per block
  if (bx > 1024) bx = 1024;
  const PixStrides st{sn, sk, sp};
  hipLaunchKernelGGL(seg_counts_kernel, dim3((unsigned)bx, (unsigned)N), dim3(256), 0, s, logits, st, K, HW, labels,
                     ignore_index, reinterpret_cast<unsigned long long*>(counts));
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_nhwc_pad_cast(const float* x, int64_t M, int K, int Kp, void* y, int f32, hipStream_t s) {
  if (Kp % 8 || Kp < K || K < 1 || M <= 0) return hipErrorInvalidValue;
  const dim3 g(ew_blocks_pix(M * (Kp / 8)));
  if (f32) hipLaunchKernelGGL(nhwc_pad_cast_kernel<float>, g, dim3(256), 0, s, x, M, K, Kp, (float*)y);
  else hipLaunchKernelGGL(nhwc_pad_cast_kernel<uint16_t>, g, dim3(256), 0, s, x, M, K, Kp, (uint16_t*)y);
  return hipGetLastError();
}
