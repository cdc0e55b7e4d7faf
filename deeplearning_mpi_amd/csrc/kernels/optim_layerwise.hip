// Layer-wise optimizers (LARS, LAMB) over the flat fp32 buffers of a ParamArena, with the step
// count, the learning-rate schedule and the skip decision on the device (a captured step replays
// a live schedule).
//
// Per-tensor quantities come from a CHUNK TABLE built once on the host (ParamArena.segments()):
// every tensor is cut, from its own start, into chunks of LW_CHUNK = 4096 elements (256 threads x
// 4 loads x 4 floats: one block iteration per chunk, the last chunk of a tensor is short).  A chunk
// is int32 {segment, length, start lo, start hi}.  Thread t of the block owns the 16-byte vectors
// t, t + 256, t + 512, t + 768 of its chunk and element e of each goes to accumulator e, so a
// chunk's partial sum is a function of the chunk alone: not of the grid size, not of where the
// tensor sits in the arena, not of its alignment (an unaligned tensor takes scalar loads into the
// same lanes and accumulators).  One fp32 partial per (quantity, chunk), no atomics; seg_finish
// adds a tensor's partials in a fixed order in fp64.  Hence bit-identical results run to run and
// between the arena path and the one-segment-per-tensor fallback.
//
//   LARS:  seg_sumsq(w, g)  -> seg_finish -> lars_update        (7 array passes; SGD momentum: 5)
//   LAMB:  lamb_moments     -> seg_finish -> lamb_update        (10 array passes; Adam: 7)
//
// The table seg_finish writes (floats): [0] lr of this update, [1] bc1, [2] bc2, [3] skip,
// [4] global gradient norm (LARS), [5] first applied update, [6..7] bc1, bc2 of the next update,
// [LW_TAB + i] trust ratio of tensor i.
// A skipped update writes only [3] (and [4]): lr, ratios, step count and every state array stay.
// Pure bandwidth: wide loads, 8 to 16 of them in flight per thread, nothing else.
#include "common.h"

namespace dlmpi {

constexpr int LW_CHUNK = 4096;
constexpr int LW_TAB = 8;
constexpr int LW_U = LW_CHUNK / (256 * 4);   // 16-byte vectors per thread and array

struct LwChunk {
  int seg, len;
  int64_t start;
  bool ok;
};
__device__ __forceinline__ LwChunk lw_chunk(const int* __restrict__ chunks, int c, int64_t n, int T) {
  const int4 d = reinterpret_cast<const int4*>(chunks)[c];
  LwChunk k;
  k.seg = d.x;
  k.len = d.y;
  k.start = (int64_t)(uint32_t)d.z | ((int64_t)d.w << 32);
  // a table that does not fit the buffers is never followed
  k.ok = d.x >= 0 && d.x < T && d.y > 0 && d.y <= LW_CHUNK && k.start >= 0 && k.start + d.y <= n;
  return k;
}

// FAST: a whole chunk of 16-byte aligned arrays.  Otherwise a vector inside the chunk is still one
// 16-byte load when the arrays allow it; the tail vector and unaligned arrays go element by element
template <bool FAST>
__device__ __forceinline__ f32x4 lw_ld(const float* __restrict__ x, int i, int len, bool vec) {
  if constexpr (FAST) return *reinterpret_cast<const f32x4*>(x + i);
  if (vec && i + 4 <= len) return *reinterpret_cast<const f32x4*>(x + i);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < len) r[e] = x[i + e];
  return r;
}
template <bool FAST>
__device__ __forceinline__ void lw_st(float* __restrict__ x, int i, int len, bool vec, const f32x4 v) {
  if constexpr (FAST) {
    *reinterpret_cast<f32x4*>(x + i) = v;
    return;
  }
  if (vec && i + 4 <= len) {
    *reinterpret_cast<f32x4*>(x + i) = v;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < len) x[i + e] = v[e];
}

// two block sums at once (as sumsq_kernel: wave butterflies, then the four wave sums through LDS)
__device__ __forceinline__ void lw_block_sum2(const float* sa, const float* sb, float* sh, float* out0,
                                              float* out1) {
  float a = (sa[0] + sa[1]) + (sa[2] + sa[3]), b = (sb[0] + sb[1]) + (sb[2] + sb[3]);
  a = warp_sum(a);
  b = warp_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = a;
    sh[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *out0 = sh[0] + sh[1] + sh[2] + sh[3];
    *out1 = sh[4] + sh[5] + sh[6] + sh[7];
  }
  __syncthreads();
}

// Adam's bias corrections of update number steps_done + 1.  The betas arrive as doubles and 1 - beta^t
// is formed in fp64: in fp32, 1 - 0.999f is already 3e-5 off, and so would be every v_hat of the
// first thousand updates.  Only seg_finish calls it (one thread): the corrections of the NEXT update
// wait in tab[6..7], so neither LAMB pass computes a power and both see the same two floats.
__device__ __forceinline__ void lw_bias_corrections(float steps_done, double b1, double b2, float& bc1, float& bc2) {
  const double t = (double)steps_done + 1.0;
  bc1 = (float)(1.0 - pow(b1, t));
  bc2 = (float)(1.0 - pow(b2, t));
}

// LAMB's update direction; both LAMB passes form it with this one expression
__device__ __forceinline__ float lamb_u(float w, float m, float v, float bc1, float sqrt_bc2, float eps, float wd) {
  const float denom = sqrtf(v) / sqrt_bc2 + eps;   // adam_elem's denominator
  return __builtin_fmaf(wd, w, (m / bc1) / denom);
}

// ------------------------------------------------------------------ LARS pass 1
template <bool FAST>
__device__ __forceinline__ void sumsq2_chunk(const float* __restrict__ a, const float* __restrict__ b, int len,
                                             bool vec, float* sa, float* sb) {
  f32x4 va[LW_U], vb[LW_U];
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    va[u] = lw_ld<FAST>(a, i, len, vec);
    vb[u] = lw_ld<FAST>(b, i, len, vec);
  }
#pragma unroll
  for (int u = 0; u < LW_U; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sa[e] = __builtin_fmaf(va[u][e], va[u][e], sa[e]);
      sb[e] = __builtin_fmaf(vb[u][e], vb[u][e], sb[e]);
    }
}

// partial[c] = sum a^2, partial[nchunks + c] = sum b^2 over chunk c
__global__ __launch_bounds__(256) void seg_sumsq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const int* __restrict__ chunks, int nchunks, int64_t n,
                                                        int T, float* __restrict__ partial) {
  __shared__ float sh[8];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const LwChunk k = lw_chunk(chunks, c, n, T);
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    if (k.ok) {
      const float *pa = a + k.start, *pb = b + k.start;
      const bool vec = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
      if (vec && k.len == LW_CHUNK) sumsq2_chunk<true>(pa, pb, k.len, vec, sa, sb);
      else sumsq2_chunk<false>(pa, pb, k.len, vec, sa, sb);
    }
    lw_block_sum2(sa, sb, sh, partial + c, partial + nchunks + c);
  }
}

// ------------------------------------------------------------------ finish
// One block of 1024.  Wave j < 15 takes tensors j, j + 15, ...; lane l adds the tensor's chunk partials
// l, l + 64, ... in increasing order in fp64 and a fixed butterfly joins the lanes: an order set by
// the chunking alone.  mode 0 LARS (partials: w^2, g^2), mode 1 LAMB (partials: w^2, u^2).
// flags bit 0: no weight decay, bit 1: no adaptation (ratio 1).  step = updates applied so far,
// advanced here unless the update is skipped.  kind 0 constant, 1 cosine, 2 polynomial.
// tab[6..7] hold the bias corrections of the next update to be applied (read by lamb_moments):
// mode 2 only primes them from the step count (first step, or a loaded state), an applied update
// moves them into tab[1..2] for lamb_update and writes the following pair.
__global__ __launch_bounds__(1024) void seg_finish_kernel(
    const float* __restrict__ partial, int nchunks, const int* __restrict__ chunk_first, const int* __restrict__ flags,
    int T, float* __restrict__ tab, float* __restrict__ step, const float* __restrict__ skip, int mode, float tc,
    float wd, float eps, double b1, double b2, int kind, float base_lr, float warmup, float total, float min_lr,
    float power) {
  __shared__ double shd[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (mode == 2) {
    if (threadIdx.x == 0) lw_bias_corrections(*step, b1, b2, tab[6], tab[7]);
    return;
  }
  bool sk = skip && *skip != 0.f;
  if (mode == 0) {   // the global gradient norm falls out of the same partials
    double s = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 1024) s += (double)partial[nchunks + i];
    s = warp_sum_d(s);
    if (lane == 0) shd[wave] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += shd[j];
    const float gnorm = (float)sqrt(tot);
    if (threadIdx.x == 0) tab[4] = gnorm;
    if (!isfinite(gnorm)) sk = true;   // a non-finite gradient: the same decision on every rank
  }
  if (sk) {
    if (threadIdx.x == 0) tab[3] = 1.f;
    return;
  }
  // Waves 0..14 sum, wave 15 does the scalar work beside them.  A wave takes its tensors in rounds
  // of 64: lane j first fetches the chunk range of the round's j-th tensor (one latency for all),
  // the partials of tensor k + 1 are in flight while tensor k is summed, and lane k keeps tensor
  // k's sums, so the fp64 square roots and the division of a whole round run side by side.
  // (One tensor after the other, each with its own chain of dependent loads, took 21 us for 161.)
  if (wave < 15) {
    for (int base = wave; base < T; base += 15 * 64) {
      const int mine = base + 15 * lane;
      int c0 = 0, c1 = 0;
      if (mine < T) {
        c0 = chunk_first[mine];
        c1 = chunk_first[mine + 1];
        c0 = c0 < 0 ? 0 : c0;
        c1 = c1 > nchunks ? nchunks : c1;
      }
      const int left = (T - base + 14) / 15;
      const int cnt = left < 64 ? left : 64;   // tensors of this round (wave-uniform)
      double myx = 0.0, myy = 0.0, nx = 0.0, ny = 0.0;
      {
        const int c = __shfl(c0, 0, 64) + lane;
        if (c < __shfl(c1, 0, 64)) {
          nx = (double)partial[c];
          ny = (double)partial[nchunks + c];
        }
      }
      for (int k = 0; k < cnt; ++k) {
        const int a0 = __shfl(c0, k, 64), a1 = __shfl(c1, k, 64);
        double x = nx, y = ny;   // chunk a0 + lane; then a0 + lane + 64, ... in increasing order
        nx = 0.0;
        ny = 0.0;
        if (k + 1 < cnt) {
          const int c = __shfl(c0, k + 1, 64) + lane;
          if (c < __shfl(c1, k + 1, 64)) {
            nx = (double)partial[c];
            ny = (double)partial[nchunks + c];
          }
        }
        for (int c = a0 + 64 + lane; c < a1; c += 64) {
          x += (double)partial[c];
          y += (double)partial[nchunks + c];
        }
        x = warp_sum_d(x);
        y = warp_sum_d(y);
        if (lane == k) {
          myx = x;
          myy = y;
        }
      }
      if (mine < T) {
        const int fl = flags[mine];
        const double wn = sqrt(myx), on = sqrt(myy);   // |w| and |g| (LARS) or |u| (LAMB)
        float r = 1.f;
        if (!(fl & 2) && wn > 0.0 && on > 0.0) {
          if (mode == 0) r = (float)((double)tc * wn / (on + ((fl & 1) ? 0.0 : (double)wd) * wn + (double)eps));
          else r = (float)(wn / on);
        }
        tab[LW_TAB + mine] = r;
      }
    }
    return;
  }
  if (lane == 0) {
    const float s = *step;
    double lr = base_lr;
    if (s < warmup) {
      lr = (double)base_lr * ((double)s + 1.0) / (double)warmup;
    } else if (kind != 0) {
      const double span = (double)total - (double)warmup;
      double q = ((double)s - (double)warmup) / (span > 1.0 ? span : 1.0);
      q = q < 1.0 ? q : 1.0;
      const double f = kind == 1 ? 0.5 * (1.0 + cos(3.14159265358979323846 * q)) : pow(1.0 - q, (double)power);
      lr = (double)min_lr + ((double)base_lr - (double)min_lr) * f;
    }
    tab[0] = (float)lr;
    tab[1] = tab[6];
    tab[2] = tab[7];
    lw_bias_corrections(s + 1.f, b1, b2, tab[6], tab[7]);
    tab[3] = 0.f;
    tab[5] = s == 0.f ? 1.f : 0.f;
    *step = s + 1.f;
  }
}

// ------------------------------------------------------------------ LARS pass 2
template <bool FAST>
__device__ __forceinline__ void lars_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           int len, bool vec, float r, float lr, float momentum, float wd, int nesterov,
                                           bool first) {
  f32x4 pv[LW_U], gv[LW_U], mv[LW_U];
  const bool use_m = momentum != 0.f;
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    pv[u] = lw_ld<FAST>(p, i, len, vec);
    gv[u] = lw_ld<FAST>(g, i, len, vec);
    if (use_m && !first) mv[u] = lw_ld<FAST>(m, i, len, vec);
  }
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    f32x4 w = pv[u], mo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = r * __builtin_fmaf(wd, w[e], gv[u][e]);
      float up = d;
      if (use_m) {
        const float me = first ? d : __builtin_fmaf(momentum, mv[u][e], d);
        mo[e] = me;
        up = nesterov ? __builtin_fmaf(momentum, me, d) : me;
      }
      w[e] = __builtin_fmaf(-lr, up, w[e]);
    }
    lw_st<FAST>(p, i, len, vec, w);
    if (use_m) lw_st<FAST>(m, i, len, vec, mo);
  }
}

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, const int* __restrict__ chunks,
                                                          int nchunks, int64_t n, const int* __restrict__ flags, int T,
                                                          const float* __restrict__ tab, float momentum, float wd,
                                                          int nesterov) {
  if (tab[3] != 0.f) return;
  const float lr = tab[0];
  const bool first = tab[5] != 0.f;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const LwChunk k = lw_chunk(chunks, c, n, T);
    if (!k.ok) continue;
    const float r = tab[LW_TAB + k.seg];
    const float wdi = (flags[k.seg] & 1) ? 0.f : wd;
    float* pp = p + k.start;
    const float* pg = g + k.start;
    float* pm = m + k.start;
    const bool vec = (((uintptr_t)pp | (uintptr_t)pg | (uintptr_t)pm) & 15) == 0;
    if (vec && k.len == LW_CHUNK) lars_chunk<true>(pp, pg, pm, k.len, vec, r, lr, momentum, wdi, nesterov, first);
    else lars_chunk<false>(pp, pg, pm, k.len, vec, r, lr, momentum, wdi, nesterov, first);
  }
}

// ------------------------------------------------------------------ LAMB pass 1
template <bool FAST>
__device__ __forceinline__ void lamb_moments_chunk(const float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int len, bool vec,
                                                   float coef, float omb1, float b2, float omb2, float eps, float wd,
                                                   float bc1,
                                                   float sqrt_bc2, float* sw, float* su) {
  f32x4 pv[LW_U], gv[LW_U], mv[LW_U], vv[LW_U];
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    pv[u] = lw_ld<FAST>(p, i, len, vec);
    gv[u] = lw_ld<FAST>(g, i, len, vec);
    mv[u] = lw_ld<FAST>(m, i, len, vec);
    vv[u] = lw_ld<FAST>(v, i, len, vec);
  }
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    f32x4 mo, vo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = gv[u][e] * coef;
      float me = mv[u][e], ve = vv[u][e];
      me += (ge - me) * omb1;             // adam_elem's recurrences, 1 - beta rounded once from fp64
      ve = ve * b2 + omb2 * ge * ge;
      mo[e] = me;
      vo[e] = ve;
      // (past the end of a short chunk w = m = v = 0: u = 0 / eps = 0 adds nothing)
      const float ue = lamb_u(pv[u][e], me, ve, bc1, sqrt_bc2, eps, wd);
      sw[e] = __builtin_fmaf(pv[u][e], pv[u][e], sw[e]);
      su[e] = __builtin_fmaf(ue, ue, su[e]);
    }
    lw_st<FAST>(m, i, len, vec, mo);
    lw_st<FAST>(v, i, len, vec, vo);
  }
}

// m, v <- Adam's recurrences; partial[c] = sum w^2, partial[nchunks + c] = sum u^2 over chunk c.
// clip = {scale, nonfinite} as for adam_kernel; step = updates applied so far (read only here)
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           const int* __restrict__ chunks, int nchunks, int64_t n,
                                                           const int* __restrict__ flags, int T,
                                                           float* __restrict__ partial, const float* __restrict__ tab,
                                                           const float* __restrict__ clip, float omb1, float b2,
                                                           float omb2, float eps, float wd) {
  __shared__ float sh[8];
  if (clip && clip[1] != 0.f) return;   // collective skip: seg_finish sees the same flag
  const float coef = clip ? clip[0] : 1.f;
  const float bc1 = tab[6], sqrt_bc2 = sqrtf(tab[7]);   // this update's bias corrections (seg_finish)
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const LwChunk k = lw_chunk(chunks, c, n, T);
    float sw[4] = {0.f, 0.f, 0.f, 0.f}, su[4] = {0.f, 0.f, 0.f, 0.f};
    if (k.ok) {
      const float wdi = (flags[k.seg] & 1) ? 0.f : wd;
      const float *pp = p + k.start, *pg = g + k.start;
      float *pm = m + k.start, *pv = v + k.start;
      const bool vec = (((uintptr_t)pp | (uintptr_t)pg | (uintptr_t)pm | (uintptr_t)pv) & 15) == 0;
      if (vec && k.len == LW_CHUNK)
        lamb_moments_chunk<true>(pp, pg, pm, pv, k.len, vec, coef, omb1, b2, omb2, eps, wdi, bc1, sqrt_bc2, sw, su);
      else
        lamb_moments_chunk<false>(pp, pg, pm, pv, k.len, vec, coef, omb1, b2, omb2, eps, wdi, bc1, sqrt_bc2, sw, su);
    }
    lw_block_sum2(sw, su, sh, partial + c, partial + nchunks + c);
  }
}

// ------------------------------------------------------------------ LAMB pass 2
template <bool FAST>
__device__ __forceinline__ void lamb_update_chunk(float* __restrict__ p, const float* __restrict__ m,
                                                  const float* __restrict__ v, int len, bool vec, float nlr, float eps,
                                                  float wd, float bc1, float sqrt_bc2) {
  f32x4 pv[LW_U], mv[LW_U], vv[LW_U];
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    pv[u] = lw_ld<FAST>(p, i, len, vec);
    mv[u] = lw_ld<FAST>(m, i, len, vec);
    vv[u] = lw_ld<FAST>(v, i, len, vec);
  }
#pragma unroll
  for (int u = 0; u < LW_U; ++u) {
    const int i = 4 * (threadIdx.x + 256 * u);
    f32x4 w = pv[u];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = __builtin_fmaf(nlr, lamb_u(w[e], mv[u][e], vv[u][e], bc1, sqrt_bc2, eps, wd), w[e]);
    lw_st<FAST>(p, i, len, vec, w);
  }
}

// w -= lr * ratio * u, u formed again from m, v, w (never stored)
__global__ __launch_bounds__(256) void lamb_update_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                          const float* __restrict__ v, const int* __restrict__ chunks,
                                                          int nchunks, int64_t n, const int* __restrict__ flags, int T,
                                                          const float* __restrict__ tab, float eps, float wd) {
  if (tab[3] != 0.f) return;
  const float lr = tab[0], bc1 = tab[1], sqrt_bc2 = sqrtf(tab[2]);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const LwChunk k = lw_chunk(chunks, c, n, T);
    if (!k.ok) continue;
    const float nlr = -(lr * tab[LW_TAB + k.seg]);
    const float wdi = (flags[k.seg] & 1) ? 0.f : wd;
    float* pp = p + k.start;
    const float *pm = m + k.start, *pv = v + k.start;
    const bool vec = (((uintptr_t)pp | (uintptr_t)pm | (uintptr_t)pv) & 15) == 0;
    if (vec && k.len == LW_CHUNK) lamb_update_chunk<true>(pp, pm, pv, k.len, vec, nlr, eps, wdi, bc1, sqrt_bc2);
    else lamb_update_chunk<false>(pp, pm, pv, k.len, vec, nlr, eps, wdi, bc1, sqrt_bc2);
  }
}

// one block per chunk: with a few chunks per block of a fixed grid, the blocks that drew one chunk
// more set the time (6334 chunks on 2048 blocks: 4 rounds for 3.1 rounds of work); results do not
// depend on the grid
static inline unsigned lw_grid(int nchunks) { return (unsigned)(nchunks < (1 << 20) ? nchunks : (1 << 20)); }

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_lw_chunk(void) { return LW_CHUNK; }
extern "C" int dlmpi_lw_tab(void) { return LW_TAB; }

extern "C" hipError_t dlmpi_seg_sumsq(const float* a, const float* b, const int* chunks, int nchunks, int64_t n, int T,
                                      float* partial, hipStream_t s) {
  if (nchunks < 1) return hipSuccess;
  hipLaunchKernelGGL(seg_sumsq_kernel, dim3(lw_grid(nchunks)), dim3(256), 0, s, a, b, chunks, nchunks, n, T, partial);
  return hipGetLastError();
}
extern "C" hipError_t dlmpi_seg_finish(const float* partial, int nchunks, const int* chunk_first, const int* flags,
                                       int T, float* tab, float* step, const float* skip, int mode, float tc, float wd,
                                       float eps, double b1, double b2, int kind, float base_lr, float warmup,
                                       float total, float min_lr, float power, hipStream_t s) {
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(1024), 0, s, partial, nchunks, chunk_first, flags, T, tab, step,
                     skip, mode, tc, wd, eps, b1, b2, kind, base_lr, warmup, total, min_lr, power);
  return hipGetLastError();
}
extern "C" hipError_t dlmpi_lars_update(float* p, const float* g, float* m, const int* chunks, int nchunks, int64_t n,
                                        const int* flags, int T, const float* tab, float momentum, float wd,
                                        int nesterov, hipStream_t s) {
  if (nchunks < 1) return hipSuccess;
  hipLaunchKernelGGL(lars_update_kernel, dim3(lw_grid(nchunks)), dim3(256), 0, s, p, g, m, chunks, nchunks, n, flags,
                     T, tab, momentum, wd, nesterov);
  return hipGetLastError();
}
extern "C" hipError_t dlmpi_lamb_moments(const float* p, const float* g, float* m, float* v, const int* chunks,
                                         int nchunks, int64_t n, const int* flags, int T, float* partial,
                                         const float* tab, const float* clip, double b1, double b2, float eps, float wd,
                                         hipStream_t s) {
  if (nchunks < 1) return hipSuccess;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(lw_grid(nchunks)), dim3(256), 0, s, p, g, m, v, chunks, nchunks, n,
                     flags, T, partial, tab, clip, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), eps, wd);
  return hipGetLastError();
}
extern "C" hipError_t dlmpi_lamb_update(float* p, const float* m, const float* v, const int* chunks, int nchunks,
                                        int64_t n, const int* flags, int T, const float* tab, float eps, float wd,
                                        hipStream_t s) {
  if (nchunks < 1) return hipSuccess;
  hipLaunchKernelGGL(lamb_update_kernel, dim3(lw_grid(nchunks)), dim3(256), 0, s, p, m, v, chunks, nchunks, n, flags,
                     T, tab, eps, wd);
  return hipGetLastError();
}
