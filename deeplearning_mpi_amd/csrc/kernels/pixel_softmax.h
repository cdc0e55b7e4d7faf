// Pixel-wise softmax building blocks shared by pixel_ce.hip (cross-entropy alone) and seg_dice.hip (the
// cross-entropy with the soft Dice fused in): addressing, the per-pixel softmax in registers / online / over
// a row of an LDS tile, the fixed-order block reduction, the tile copy, and the host-side choice of kernel.
//
// The two files promise the same bits wherever they compute the same thing (a zero Dice weight is the plain
// loss, bit for bit), so the arithmetic lives here once: hipcc contracts a * b + c into an fma as written,
// and every sum below has one order.  A change here changes both families.
//
// dlmpi_set_pixel_tiles(0) (the A/B switch of benchmarks/multiclass_bench.py) turns the LDS-tile kernels off
// for both families through pix_tile_pixels; the default is on.
#pragma once
#include "common.h"

namespace dlmpi {

struct PixStrides {
  int64_t sn, sk, sp;   // element strides of sample, class, flat pixel (h * W + w)
};

__device__ __forceinline__ bool pix_kept(int64_t lab, int K, int64_t ignore_index) {
  return lab != ignore_index && lab >= 0 && lab < K;
}

// KC > 0: K known at compile time, the pixel's logits are held in registers (one pass, one load each;
// VEC: class stride 1 and an aligned base, so they are one 8 / 16 byte load).  KC == 0: any K, online
// softmax (running maximum and rescaled sum) in one pass.
template <int KC, bool VEC>
__device__ __forceinline__ void pix_load(const float* __restrict__ p, int64_t sk, float* v) {
  if constexpr (VEC && KC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else if constexpr (VEC && KC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < KC; ++k) v[k] = p[k * sk];
  }
}
template <int KC, bool VEC>
__device__ __forceinline__ void pix_store(float* __restrict__ p, int64_t sk, const float* v) {
  if constexpr (VEC && KC == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else if constexpr (VEC && KC == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < KC; ++k) p[k * sk] = v[k];
  }
}

// softmax of one pixel held in registers: v[k] becomes exp(v[k] - mx); logsumexp = mx + __logf(s)
struct PixSoftmax {
  float mx, s, xt;   // row maximum, sum_k exp(v[k] - mx), the logit of class lab (0 if lab is no class)
};
template <int KC>
__device__ __forceinline__ PixSoftmax pix_softmax_reg(float* v, int64_t lab) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < KC; ++k) mx = fmaxf(mx, v[k]);
  float s = 0.f, xt = 0.f;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    xt = (int64_t)k == lab ? v[k] : xt;
    v[k] = __expf(v[k] - mx);
    s += v[k];
  }
  return {mx, s, xt};
}

// logsumexp of x[0], x[sk], ..., x[(K - 1) sk] in one pass (online softmax)
__device__ __forceinline__ float pix_online_lse(const float* __restrict__ x, int64_t sk, int K) {
  float mx = x[0], s = 1.f;
  for (int k = 1; k < K; ++k) {
    const float xv = x[k * sk];
    if (xv > mx) {
      s = s * __expf(mx - xv) + 1.f;
      mx = xv;
    } else {
      s += __expf(xv - mx);
    }
  }
  return mx + __logf(s);
}

// A pixel's row of K floats in an LDS tile is walked from class k0 = thread % K on and around, so rows of an
// even length do not collide on LDS banks; the order is fixed per thread, hence still reproducible.
__device__ __forceinline__ int pix_row_next(int kk, int K) { return kk + 1 == K ? 0 : kk + 1; }

__device__ __forceinline__ float pix_row_lse(const float* row, int K, int k0) {
  float mx = -INFINITY;
  int kk = k0;
  for (int k = 0; k < K; ++k) {
    mx = fmaxf(mx, row[kk]);
    kk = pix_row_next(kk, K);
  }
  float s = 0.f;
  for (int k = 0; k < K; ++k) {
    s += __expf(row[kk] - mx);
    kk = pix_row_next(kk, K);
  }
  return mx + __logf(s);
}

__device__ __forceinline__ void pix_row_zero(float* row, int K, int k0) {
  int kk = k0;
  for (int k = 0; k < K; ++k) {
    row[kk] = 0.f;
    kk = pix_row_next(kk, K);
  }
}

__device__ __forceinline__ unsigned warp_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// block-wide sums (4 waves, fixed order) of NF floats and NU counts, returned to every thread;
// shf: 4 * NF floats, shu: 4 * NU counts of LDS, free again on return
template <int NF, int NU>
__device__ __forceinline__ void pix_block_sums(float* f, unsigned* u, float* shf, unsigned* shu) {
  const int wv = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const float v = warp_sum(f[i]);
    if (lead) shf[i * 4 + wv] = v;
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const unsigned v = warp_sum_u(u[i]);
    if (lead) shu[i * 4 + wv] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NF; ++i) f[i] = shf[i * 4] + shf[i * 4 + 1] + shf[i * 4 + 2] + shf[i * 4 + 3];
#pragma unroll
  for (int i = 0; i < NU; ++i) u[i] = shu[i * 4] + shu[i * 4 + 1] + shu[i * 4 + 2] + shu[i * 4 + 3];
  __syncthreads();
}

// the cross-entropy's two sums ce = {sum w nll, sum w}: a kept pixel's term (l its logsumexp, xt its label's
// logit), and the block's sums -> out[0..1] (shf: 8 floats of LDS)
__device__ __forceinline__ void pix_ce_add(float* ce, const float* __restrict__ weight, int64_t lab, float l,
                                           float xt) {
  const float w = weight ? weight[lab] : 1.f;
  ce[0] += w * (l - xt);
  ce[1] += w;
}
__device__ __forceinline__ void pix_ce_block_store(float* ce, float* shf, float* __restrict__ out) {
  pix_block_sums<2, 0>(ce, nullptr, shf, nullptr);
  if (threadIdx.x == 0) {
    out[0] = ce[0];
    out[1] = ce[1];
  }
}

// Copy of nf floats between an LDS tile and global memory by the block's 256 threads.  The global side need
// not be 16-byte aligned (a sample of odd H * W * K): the tile is kept at the source's offset ph within its
// 16 bytes (tile = 16-byte aligned LDS + ph), so there are 16-byte copies in between and single floats at
// the two ends.  ph = 0: an aligned source.
__device__ __forceinline__ int pix_tile_phase(const float* src) { return (int)(((uintptr_t)src >> 2) & 3); }

template <bool LOAD>
__device__ __forceinline__ void pix_tile_copy(float* __restrict__ tile, float* __restrict__ glob, int nf, int ph) {
  const int head = min((4 - ph) & 3, nf);
  const int body = (nf - head) & ~3;
  if ((int)threadIdx.x < head) {
    if constexpr (LOAD) tile[threadIdx.x] = glob[threadIdx.x];
    else glob[threadIdx.x] = tile[threadIdx.x];
  }
  for (int i = head + threadIdx.x * 4; i < head + body; i += 1024) {
    if constexpr (LOAD) *reinterpret_cast<f32x4*>(tile + i) = *reinterpret_cast<const f32x4*>(glob + i);
    else *reinterpret_cast<f32x4*>(glob + i) = *reinterpret_cast<const f32x4*>(tile + i);
  }
  const int i = head + body + threadIdx.x;
  if (i < nf) {
    if constexpr (LOAD) tile[i] = glob[i];
    else glob[i] = tile[i];
  }
}

// ---- host side: which kernel a launcher takes ----

// vector access of a pixel's K logits: class stride 1, pixel stride K, and every pixel K*4-byte aligned
static inline bool pix_vec_ok(const void* a, const void* b, int K, int64_t sn, int64_t sk, int64_t sp) {
  if ((K != 2 && K != 4) || sk != 1 || sp != K || sn % K) return false;
  const uintptr_t al = (uintptr_t)K * 4 - 1;
  return !((uintptr_t)a & al) && !(b && ((uintptr_t)b & al));
}

// the LDS-tile kernels: class-last contiguous [N][HW][K] logits, K > 4, 16-byte aligned bases; pixels per
// tile (0: no).  g_pix_tiles is dlmpi_set_pixel_tiles' switch (0: the lane-per-pixel kernels everywhere).
inline int g_pix_tiles = 1;

static inline int pix_tile_pixels(const void* a, const void* b, int K, int64_t HW, int64_t sn, int64_t sk,
                                  int64_t sp) {
  if (!g_pix_tiles || K <= 4 || sk != 1 || sp != K || sn != HW * K) return 0;
  if (((uintptr_t)a & 15) || (b && ((uintptr_t)b & 15))) return 0;
  return K <= 32 ? 256 : (8192 / K) & ~3;   // <= 32 KB of tile, a multiple of 4 pixels: tiles stay 16-byte aligned
}

// KER<KC, VEC> for the caller's K (and stream s): K = 2, 3, 4 in registers, vector access where VECOK, else any K
#define PIX_DISPATCH(KER, GRID, VECOK, ...)                                                           \
  do {                                                                                                \
    if (K == 2 && (VECOK)) hipLaunchKernelGGL((KER<2, true>), GRID, dim3(256), 0, s, __VA_ARGS__);    \
    else if (K == 4 && (VECOK)) hipLaunchKernelGGL((KER<4, true>), GRID, dim3(256), 0, s, __VA_ARGS__); \
    else if (K == 2) hipLaunchKernelGGL((KER<2, false>), GRID, dim3(256), 0, s, __VA_ARGS__);         \
    else if (K == 3) hipLaunchKernelGGL((KER<3, false>), GRID, dim3(256), 0, s, __VA_ARGS__);         \
    else if (K == 4) hipLaunchKernelGGL((KER<4, false>), GRID, dim3(256), 0, s, __VA_ARGS__);         \
    else hipLaunchKernelGGL((KER<0, false>), GRID, dim3(256), 0, s, __VA_ARGS__);                     \
  } while (0)

}  // namespace dlmpi
