// Segmentation: soft Dice loss fused into the pixel-wise cross-entropy / BCE passes.
//
// Multi-class (logits [N, K, H, W] addressed by (sample, class, pixel) strides as in pixel_ce.hip, labels
// int64 [N*HW], p = softmax_k x): over the kept pixels of sample n (label != ignore_index and in [0, K))
//   I[n,c] = sum p_c [y = c],  P[n,c] = sum p_c,  T[n,c] = sum [y = c],
//   dice[n,c] = (2 I + smooth) / (P + T + smooth),  L_dice = 1 - mean_{n, c in C} dice[n,c],
//   L = ce_weight * CE + dice_weight * L_dice        (C: all classes, or 1..K-1 without the background).
// Binary (logits, float targets t [N*HW], p = sigmoid x): the same with one class per sample and BCE.
//
// Three launches, the same number of passes over the logits as the cross-entropy alone:
//   forward  grid (blocks_x, N): reads each logit once, writes lse[m], per block {sum w nll, sum w} and per
//            (block, class) {I, P, T} (T an exact integer, stored as its bit pattern);
//   finish   one block: the partials summed in double in a fixed order -> loss, CE denominator, and the
//            fp32 table tab[n][c] = {A, B} of the Dice gradient d dice_weight*L_dice / d p_c =
//            A [y = c] + B, A = -2 s / U, B = s (2 I + smooth) / U^2, U = P + T + smooth,
//            s = dice_weight / (N |C|) (zeros for a class outside C);
//   backward grid (blocks_x, N): dx_k = go * (p_k (g_k - sum_j p_j g_j) + ce_weight (p_k - [k = y]) w[y] / den),
//            g_k = A [y = k] + B, exact zeros at ignored pixels, written in the strides of the logits.
// A block never spans two samples.  No float atomics, every reduction in a fixed order: the same bits on
// every run.  A weight of exactly zero leaves its term out (a NaN cross-entropy of an all-ignored batch
// does not reach a pure Dice loss).
// The softmax arithmetic, the addressing, the block reduction and the tile copy are pixel_softmax.h's,
// shared with pixel_ce.hip: a zero Dice weight is that file's loss, bit for bit.
#include "pixel_softmax.h"

namespace dlmpi {

constexpr int kDiceBlocksTotal = 2048;   // about N * blocks_x

// ------------------------------------------------------------------------------------------------
// forward, a lane per pixel.  KC = 2, 3, 4: the pixel's logits and the per-class sums in registers
// (VEC: one 8 / 16 byte load).  KC == 0: any K and any strides; the per-pixel logsumexp first (online
// softmax), then one block-reduced {I, P, T} per class that re-reads the block's pixels.
// part_ce [N][gridDim.x][2], part_d [N][gridDim.x][K][3]
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void ce_dice_fwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                          int64_t HW, const int64_t* __restrict__ labels,
                                                          int64_t ignore_index, const float* __restrict__ weight,
                                                          float* lse, float* __restrict__ part_ce,
                                                          float* __restrict__ part_d) {
  constexpr int KK = KC > 0 ? KC : 1;
  __shared__ float shf[(2 * KK + 2) * 4];
  __shared__ unsigned shu[KK * 4];
  const int n = blockIdx.y;
  const int64_t blk = (int64_t)n * gridDim.x + blockIdx.x;
  const float* xs = logits + (int64_t)n * st.sn;
  const int64_t p0 = blockIdx.x * (int64_t)256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  float f[2 * KK + 2];
  unsigned u[KK];
#pragma unroll
  for (int i = 0; i < 2 * KK + 2; ++i) f[i] = 0.f;
#pragma unroll
  for (int i = 0; i < KK; ++i) u[i] = 0u;
  float* ce = f + 2 * KK;   // {sum w nll, sum w}
  for (int64_t p = p0; p < HW; p += step) {
    const int64_t m = (int64_t)n * HW + p;
    const float* x = xs + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    float l, xt = 0.f;
    if constexpr (KC > 0) {
      float v[KC];
      pix_load<KC, VEC>(x, st.sk, v);
      const PixSoftmax r = pix_softmax_reg<KC>(v, lab);
      l = r.mx + __logf(r.s);
      xt = r.xt;
      if (keep) {
        const float inv = 1.f / r.s;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const float pk = v[k] * inv;
          const bool hit = (int64_t)k == lab;
          f[2 * k] += hit ? pk : 0.f;
          f[2 * k + 1] += pk;
          u[k] += hit ? 1u : 0u;
        }
      }
    } else {
      l = pix_online_lse(x, st.sk, K);
      if (keep) xt = x[lab * st.sk];
    }
    lse[m] = l;
    if (keep) pix_ce_add(ce, weight, lab, l, xt);
  }
  if constexpr (KC > 0) {
    pix_block_sums<2 * KC + 2, KC>(f, u, shf, shu);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        float* q = part_d + (blk * KC + k) * 3;
        q[0] = f[2 * k];
        q[1] = f[2 * k + 1];
        q[2] = __uint_as_float(u[k]);
      }
      part_ce[2 * blk] = ce[0];
      part_ce[2 * blk + 1] = ce[1];
    }
  } else {
    pix_ce_block_store(ce, shf, part_ce + 2 * blk);
    for (int c = 0; c < K; ++c) {
      float a[2] = {0.f, 0.f};
      unsigned t[1] = {0u};
      for (int64_t p = p0; p < HW; p += step) {
        const int64_t m = (int64_t)n * HW + p;
        const int64_t lab = labels[m];
        if (!pix_kept(lab, K, ignore_index)) continue;
        const float pc = __expf(xs[p * st.sp + c * st.sk] - lse[m]);   // lse[m]: this thread's own store
        a[1] += pc;
        if (lab == c) {
          a[0] += pc;
          t[0] += 1u;
        }
      }
      pix_block_sums<2, 1>(a, t, shf, shu);
      if (threadIdx.x == 0) {
        float* q = part_d + (blk * K + c) * 3;
        q[0] = a[0];
        q[1] = a[1];
        q[2] = __uint_as_float(t[0]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Class-last contiguous logits with K > 4: the LDS tiles of pixel_ce.hip, per sample.  A sample's first
// logit need not be 16-byte aligned (H * W * K odd), so the tile is kept at the source's offset within
// its 16 bytes (pix_tile_phase, pix_tile_copy).
// dynamic LDS: tile [P * K + 4] | red [768] | labs [P] | sh [8].  Thread t < np reduces pixel t's row
// (from class t % K on) and turns it into the row's softmax (zeros if ignored); then thread (g, c) =
// (t / K, t % K), g < G = 256 / K, sums class c over the pixels g, g + G, ..., and thread c < K adds the G
// group sums to its running {I, P, T} of class c: a fixed order throughout.
__global__ __launch_bounds__(256) void ce_dice_fwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                               int64_t HW, const int64_t* __restrict__ labels,
                                                               int64_t ignore_index,
                                                               const float* __restrict__ weight,
                                                               float* __restrict__ lse, float* __restrict__ part_ce,
                                                               float* __restrict__ part_d) {
  extern __shared__ __align__(16) float smem[];
  const int n = blockIdx.y;
  const int64_t blk = (int64_t)n * gridDim.x + blockIdx.x;
  const float* base = logits + (int64_t)n * HW * K;
  const int ph = pix_tile_phase(base);
  float* tile = smem + ph;
  float* red = smem + P * K + 4;
  int* labs = reinterpret_cast<int*>(red + 768);
  float* shf = reinterpret_cast<float*>(labs + P);
  const int G = 256 / K;
  const int c = threadIdx.x % K, g = threadIdx.x / K;
  float ce[2] = {0.f, 0.f};
  float accI = 0.f, accP = 0.f;
  unsigned accT = 0u;
  const int64_t ntiles = (HW + P - 1) / P;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t q0 = t * P;
    const int np = (int)(HW - q0 < P ? HW - q0 : P);
    pix_tile_copy<true>(tile, const_cast<float*>(base + q0 * K), np * K, ph);
    __syncthreads();
    if ((int)threadIdx.x < np) {
      float* row = tile + threadIdx.x * K;
      const float l = pix_row_lse(row, K, c);
      const int64_t m = (int64_t)n * HW + q0 + threadIdx.x;
      const int64_t lab = labels[m];
      lse[m] = l;
      if (pix_kept(lab, K, ignore_index)) {
        pix_ce_add(ce, weight, lab, l, row[lab]);
        int kk = c;
        for (int k = 0; k < K; ++k) {
          row[kk] = __expf(row[kk] - l);
          kk = pix_row_next(kk, K);
        }
        labs[threadIdx.x] = (int)lab;
      } else {
        pix_row_zero(row, K, c);
        labs[threadIdx.x] = -1;
      }
    }
    __syncthreads();
    if (g < G) {
      float fi = 0.f, fp = 0.f;
      unsigned ft = 0u;
      for (int p = g; p < np; p += G) {
        const float v = tile[p * K + c];
        const bool hit = labs[p] == c;
        fp += v;
        fi += hit ? v : 0.f;
        ft += hit ? 1u : 0u;
      }
      float* r = red + (g * K + c) * 3;
      r[0] = fi;
      r[1] = fp;
      r[2] = __uint_as_float(ft);
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
      for (int gg = 0; gg < G; ++gg) {
        const float* r = red + (gg * K + threadIdx.x) * 3;
        accI += r[0];
        accP += r[1];
        accT += __float_as_uint(r[2]);
      }
    }
  }
  if ((int)threadIdx.x < K) {
    float* q = part_d + (blk * K + threadIdx.x) * 3;
    q[0] = accI;
    q[1] = accP;
    q[2] = __uint_as_float(accT);
  }
  __syncthreads();
  pix_ce_block_store(ce, shf, part_ce + 2 * blk);
}

// ------------------------------------------------------------------------------------------------
// finish: LP adjacent lanes per (sample, class) pair sum that pair's gx partials (lane j takes the blocks j,
// j + LP, ... in double, then the butterfly over the LP lanes); the group's first lane writes the {A, B} row
// and adds the pair's dice to its own sum.  LP is the largest power of two with pairs * LP <= 1024 (the
// one block's 1024 threads all load at once: the launch is latency-bound), so the order of every sum is
// a function of the shapes alone.  The 1024 per-thread dice sums are added by waves, then in order by thread 0.
__global__ __launch_bounds__(1024) void ce_dice_finish_kernel(const float* __restrict__ part_ce,
                                                              const float* __restrict__ part_d, int N, int gx, int K,
                                                              int c0, float smooth, float ce_w, float dice_w,
                                                              float* __restrict__ loss, float* __restrict__ den,
                                                              float* __restrict__ tab) {
  __shared__ double sh[3][16];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double cnt = (double)N * (K - c0);
  const double s0 = (double)dice_w / cnt;
  const int64_t npairs = (int64_t)N * K;
  int LP = 64;
  while (LP > 1 && npairs * LP > 1024) LP >>= 1;
  const int sub = threadIdx.x & (LP - 1);
  const int64_t nround = (npairs * LP + 1023) / 1024;
  double dsum = 0.0;
  for (int64_t r = 0; r < nround; ++r) {   // (a whole wave stays in the shuffles: pair past the end sums nothing)
    const int64_t pair = r * (1024 / LP) + threadIdx.x / LP;
    const bool live = pair < npairs;
    const int64_t n = live ? pair / K : 0;
    const int c = live ? (int)(pair - n * K) : 0;
    double I = 0.0, Pp = 0.0, T = 0.0;
    if (live) {
      for (int b = sub; b < gx; b += LP) {
        const float* q = part_d + ((n * gx + b) * K + c) * 3;
        I += (double)q[0];
        Pp += (double)q[1];
        T += (double)__float_as_uint(q[2]);
      }
    }
    for (int o = LP >> 1; o > 0; o >>= 1) {
      I += __shfl_xor(I, o, 64);
      Pp += __shfl_xor(Pp, o, 64);
      T += __shfl_xor(T, o, 64);
    }
    if (live && sub == 0) {
      double A = 0.0, B = 0.0;
      if (c >= c0) {
        const double U = Pp + T + (double)smooth;
        const double num = 2.0 * I + (double)smooth;
        dsum += num / U;
        A = -2.0 * s0 / U;
        B = s0 * num / (U * U);
      }
      tab[2 * pair] = (float)A;
      tab[2 * pair + 1] = (float)B;
    }
  }
  dsum = warp_sum_d(dsum);
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)N * gx; i += 1024) {
    a += (double)part_ce[2 * i];
    b += (double)part_ce[2 * i + 1];
  }
  a = warp_sum_d(a);
  b = warp_sum_d(b);
  if (lane == 0) { sh[0][wv] = dsum; sh[1][wv] = a; sh[2][wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0;
    a = 0.0;
    b = 0.0;
    for (int i = 0; i < 16; ++i) { d += sh[0][i]; a += sh[1][i]; b += sh[2][i]; }
    double L = (double)dice_w * (1.0 - d / cnt);
    if (ce_w != 0.f) L += (double)ce_w * (a / b);
    *loss = (float)L;
    *den = (float)b;
  }
}

// ------------------------------------------------------------------------------------------------
// backward, a lane per pixel; the sample's {A, B} rows (times go) in registers (KC > 0) or LDS
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void ce_dice_bwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                          int64_t HW, const int64_t* __restrict__ labels,
                                                          int64_t ignore_index, const float* __restrict__ weight,
                                                          const float* __restrict__ lse,
                                                          const float* __restrict__ go,
                                                          const float* __restrict__ den,
                                                          const float* __restrict__ tab, float ce_w,
                                                          float* __restrict__ dlogits) {
  constexpr int KK = KC > 0 ? KC : 256;
  __shared__ float stab[KC > 0 ? 2 : 512];
  const int n = blockIdx.y;
  const float g0 = go ? *go : 1.f;
  const float cg = ce_w != 0.f ? ce_w * g0 / *den : 0.f;
  const float* tn = tab + (int64_t)n * K * 2;
  float tA[KC > 0 ? KC : 1], tB[KC > 0 ? KC : 1];
  if constexpr (KC > 0) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      tA[k] = tn[2 * k] * g0;
      tB[k] = tn[2 * k + 1] * g0;
    }
  } else {
    for (int i = threadIdx.x; i < 2 * K && i < 2 * KK; i += 256) stab[i] = tn[i] * g0;
    __syncthreads();
  }
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int64_t m = (int64_t)n * HW + p;
    const int64_t off = (int64_t)n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    const float l = lse[m];
    const float wc = keep ? cg * (weight ? weight[lab] : 1.f) : 0.f;
    if constexpr (KC > 0) {
      float v[KC];
      if (keep) {
        pix_load<KC, VEC>(logits + off, st.sk, v);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          v[k] = __expf(v[k] - l);
          dot += v[k] * (tB[k] + ((int64_t)k == lab ? tA[k] : 0.f));
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const bool hit = (int64_t)k == lab;
          v[k] = v[k] * (tB[k] + (hit ? tA[k] : 0.f) - dot) + (v[k] - (hit ? 1.f : 0.f)) * wc;
        }
      } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = 0.f;
      }
      pix_store<KC, VEC>(dlogits + off, st.sk, v);
    } else {
      if (keep) {
        float dot = 0.f;
        for (int k = 0; k < K; ++k) {
          const float pk = __expf(logits[off + k * st.sk] - l);
          dot += pk * (stab[2 * k + 1] + ((int64_t)k == lab ? stab[2 * k] : 0.f));
        }
        for (int k = 0; k < K; ++k) {
          const float pk = __expf(logits[off + k * st.sk] - l);
          const bool hit = (int64_t)k == lab;
          const float gk = stab[2 * k + 1] + (hit ? stab[2 * k] : 0.f);
          dlogits[off + k * st.sk] = pk * (gk - dot) + (pk - (hit ? 1.f : 0.f)) * wc;
        }
      } else {
        for (int k = 0; k < K; ++k) dlogits[off + k * st.sk] = 0.f;
      }
    }
  }
}

// the backward through the tiles of the forward: dynamic LDS tile [P * K + 4] | stab [512]
__global__ __launch_bounds__(256) void ce_dice_bwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                               int64_t HW, const int64_t* __restrict__ labels,
                                                               int64_t ignore_index,
                                                               const float* __restrict__ weight,
                                                               const float* __restrict__ lse,
                                                               const float* __restrict__ go,
                                                               const float* __restrict__ den,
                                                               const float* __restrict__ tab, float ce_w,
                                                               float* __restrict__ dlogits) {
  extern __shared__ __align__(16) float smem[];
  const int n = blockIdx.y;
  const float* base = logits + (int64_t)n * HW * K;
  float* dbase = dlogits + (int64_t)n * HW * K;
  const int ph = pix_tile_phase(base);   // dlogits: the same offset within 16 bytes (checked by the launcher)
  float* tile = smem + ph;
  float* stab = smem + P * K + 4;
  const float g0 = go ? *go : 1.f;
  const float cg = ce_w != 0.f ? ce_w * g0 / *den : 0.f;
  for (int i = threadIdx.x; i < 2 * K; i += 256) stab[i] = tab[(int64_t)n * K * 2 + i] * g0;
  const int k0 = threadIdx.x % K;
  const int64_t ntiles = (HW + P - 1) / P;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t q0 = t * P;
    const int np = (int)(HW - q0 < P ? HW - q0 : P);
    const int nf = np * K;
    pix_tile_copy<true>(tile, const_cast<float*>(base + q0 * K), nf, ph);
    __syncthreads();   // (also orders the stab stores before their first use)
    if ((int)threadIdx.x < np) {
      float* row = tile + threadIdx.x * K;
      const int64_t m = (int64_t)n * HW + q0 + threadIdx.x;
      const int64_t lab = labels[m];
      int kk = k0;
      if (pix_kept(lab, K, ignore_index)) {
        const float wc = cg * (weight ? weight[lab] : 1.f);
        const float l = lse[m];
        float dot = 0.f;
        for (int k = 0; k < K; ++k) {
          const float pk = __expf(row[kk] - l);
          row[kk] = pk;
          dot += pk * stab[2 * kk + 1];
          kk = pix_row_next(kk, K);
        }
        const float al = stab[2 * (int)lab];
        dot += row[lab] * al;
        for (int k = 0; k < K; ++k) {
          const float pk = row[kk];
          const bool hit = (int64_t)kk == lab;
          row[kk] = pk * (stab[2 * kk + 1] + (hit ? al : 0.f) - dot) + (pk - (hit ? 1.f : 0.f)) * wc;
          kk = pix_row_next(kk, K);
        }
      } else {
        pix_row_zero(row, K, k0);
      }
    }
    __syncthreads();
    pix_tile_copy<false>(tile, dbase + q0 * K, nf, ph);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// binary: contiguous logits / targets [N][HW], p = sigmoid(x);
// part [N][gridDim.x][4] = {sum bce, sum p t, sum p, sum t}
__global__ __launch_bounds__(256) void bce_dice_fwd_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ target, int64_t HW,
                                                           float* __restrict__ part) {
  __shared__ float shf[16];
  const int n = blockIdx.y;
  const float* x = logits + (int64_t)n * HW;
  const float* t = target + (int64_t)n * HW;
  float f[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const float xv = x[p], tv = t[p];
    const float e = __expf(-fabsf(xv));
    f[0] += fmaxf(xv, 0.f) - xv * tv + log1pf(e);
    const float pr = 1.f / (1.f + __expf(-xv));
    f[1] += pr * tv;
    f[2] += pr;
    f[3] += tv;
  }
  pix_block_sums<4, 0>(f, nullptr, shf, nullptr);
  if (threadIdx.x == 0) {
    float* q = part + ((int64_t)n * gridDim.x + blockIdx.x) * 4;
    q[0] = f[0]; q[1] = f[1]; q[2] = f[2]; q[3] = f[3];
  }
}

// a wave per sample; loss = bce_w * sum bce / (N HW) + dice_w * (1 - mean_n dice), tab [N][2] = {A, B}
__global__ __launch_bounds__(1024) void bce_dice_finish_kernel(const float* __restrict__ part, int N, int gx,
                                                               double count, float smooth, float bce_w, float dice_w,
                                                               float* __restrict__ loss, float* __restrict__ tab) {
  __shared__ double sh[2][16];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double s0 = (double)dice_w / (double)N;
  double dsum = 0.0, bsum = 0.0;
  for (int n = wv; n < N; n += 16) {
    double e = 0.0, I = 0.0, Pp = 0.0, T = 0.0;
    for (int b = lane; b < gx; b += 64) {
      const float* q = part + ((int64_t)n * gx + b) * 4;
      e += (double)q[0];
      I += (double)q[1];
      Pp += (double)q[2];
      T += (double)q[3];
    }
    e = warp_sum_d(e);
    I = warp_sum_d(I);
    Pp = warp_sum_d(Pp);
    T = warp_sum_d(T);
    const double U = Pp + T + (double)smooth;
    const double num = 2.0 * I + (double)smooth;
    dsum += num / U;
    bsum += e;
    if (lane == 0) {
      tab[2 * n] = (float)(-2.0 * s0 / U);
      tab[2 * n + 1] = (float)(s0 * num / (U * U));
    }
  }
  if (lane == 0) { sh[0][wv] = dsum; sh[1][wv] = bsum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0, e = 0.0;
    for (int i = 0; i < 16; ++i) { d += sh[0][i]; e += sh[1][i]; }
    double L = (double)dice_w * (1.0 - d / (double)N);
    if (bce_w != 0.f) L += (double)bce_w * (e / count);
    *loss = (float)L;
  }
}

// dx = go * (bscale (p - t) + p (1 - p) (A t + B)), bscale = bce_weight / (N HW)
__global__ __launch_bounds__(256) void bce_dice_bwd_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ target, int64_t HW,
                                                           const float* __restrict__ go,
                                                           const float* __restrict__ tab, float bscale,
                                                           float* __restrict__ dlogits) {
  const int n = blockIdx.y;
  const float g0 = go ? *go : 1.f;
  const float A = tab[2 * n] * g0, B = tab[2 * n + 1] * g0, bs = bscale * g0;
  const float* x = logits + (int64_t)n * HW;
  const float* t = target + (int64_t)n * HW;
  float* d = dlogits + (int64_t)n * HW;
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const float tv = t[p];
    const float pr = 1.f / (1.f + __expf(-x[p]));
    d[p] = bs * (pr - tv) + pr * (1.f - pr) * (A * tv + B);
  }
}

}  // namespace dlmpi

using namespace dlmpi;

// blocks_x of the 2-D grids (blocks_x, N): one block per 256 pixels of a sample, about kDiceBlocksTotal in all
extern "C" int dlmpi_seg_dice_blocks(int64_t HW, int N) {
  int64_t b = (HW + 255) / 256;
  const int64_t cap = N > 0 && N < kDiceBlocksTotal ? kDiceBlocksTotal / N : 1;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// a block's pixel count stays far below 2^24 (exact float sums of hard targets; the class counts are integers)
static bool dice_args_ok(int K, int64_t HW, int N) {
  return K >= 1 && K <= 256 && HW > 0 && N > 0 && N <= 65535 &&
         HW / dlmpi_seg_dice_blocks(HW, N) < ((int64_t)1 << 24) - 256;
}
static bool dice_weights_ok(float a, float b, float smooth) {
  return a >= 0.f && b >= 0.f && a <= 3.0e38f && b <= 3.0e38f && (a > 0.f || b > 0.f) && smooth > 0.f &&
         smooth <= 3.0e38f;
}

// gx = dlmpi_seg_dice_blocks(HW, N); part_ce [N][gx][2], part_d [N][gx][K][3], tab [N][K][2]; loss, den: one float each
extern "C" hipError_t dlmpi_pixel_ce_dice_fwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                              int64_t HW, const int64_t* labels, int64_t ignore_index,
                                              const float* weight, float ce_weight, float dice_weight, float smooth,
                                              int include_background, float* lse, float* part_ce, float* part_d,
                                              float* loss, float* den, float* tab, hipStream_t s) {
  if (K < 2 || !dice_args_ok(K, HW, N) || !dice_weights_ok(ce_weight, dice_weight, smooth))
    return hipErrorInvalidValue;
  const unsigned gx = (unsigned)dlmpi_seg_dice_blocks(HW, N);
  const dim3 grid(gx, (unsigned)N);
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, nullptr, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, nullptr, K, HW, sn, sk, sp);
  if (P > 0)
    hipLaunchKernelGGL(ce_dice_fwd_tile_kernel, grid, dim3(256), ((size_t)P * K + 4 + 768 + P + 8) * sizeof(float), s,
                       logits, K, P, HW, labels, ignore_index, weight, lse, part_ce, part_d);
  else
    PIX_DISPATCH(ce_dice_fwd_kernel, grid, vec, logits, st, K, HW, labels, ignore_index, weight, lse, part_ce, part_d);
  hipLaunchKernelGGL(ce_dice_finish_kernel, dim3(1), dim3(1024), 0, s, part_ce, part_d, N, (int)gx, K,
                     include_background ? 0 : 1, smooth, ce_weight, dice_weight, loss, den, tab);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_pixel_ce_dice_bwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                              int64_t HW, const int64_t* labels, int64_t ignore_index,
                                              const float* weight, const float* lse, const float* go,
                                              const float* den, const float* tab, float ce_weight, float* dlogits,
                                              hipStream_t s) {
  if (K < 2 || !dice_args_ok(K, HW, N) || !den || !tab || !(ce_weight >= 0.f)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)dlmpi_seg_dice_blocks(HW, N), (unsigned)N);
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, dlogits, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, dlogits, K, HW, sn, sk, sp);
  if (P > 0)
    hipLaunchKernelGGL(ce_dice_bwd_tile_kernel, grid, dim3(256), ((size_t)P * K + 4 + 512) * sizeof(float), s, logits,
                       K, P, HW, labels, ignore_index, weight, lse, go, den, tab, ce_weight, dlogits);
  else
    PIX_DISPATCH(ce_dice_bwd_kernel, grid, vec, logits, st, K, HW, labels, ignore_index, weight, lse, go, den, tab,
                 ce_weight, dlogits);
  return hipGetLastError();
}

// logits, target: contiguous [N][HW]; part [N][gx][4], tab [N][2]
extern "C" hipError_t dlmpi_bce_dice_fwd(const float* logits, const float* target, int N, int64_t HW,
                                         float bce_weight, float dice_weight, float smooth, float* part, float* loss,
                                         float* tab, hipStream_t s) {
  if (!dice_args_ok(1, HW, N) || !dice_weights_ok(bce_weight, dice_weight, smooth)) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)dlmpi_seg_dice_blocks(HW, N);
  hipLaunchKernelGGL(bce_dice_fwd_kernel, dim3(gx, (unsigned)N), dim3(256), 0, s, logits, target, HW, part);
  hipLaunchKernelGGL(bce_dice_finish_kernel, dim3(1), dim3(1024), 0, s, part, N, (int)gx, (double)N * (double)HW,
                     smooth, bce_weight, dice_weight, loss, tab);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_bce_dice_bwd(const float* logits, const float* target, int N, int64_t HW, const float* go,
                                         const float* tab, float bce_weight, float* dlogits, hipStream_t s) {
  if (!dice_args_ok(1, HW, N) || !tab || !(bce_weight >= 0.f)) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)dlmpi_seg_dice_blocks(HW, N);
  hipLaunchKernelGGL(bce_dice_bwd_kernel, dim3(gx, (unsigned)N), dim3(256), 0, s, logits, target, HW, go, tab,
                     (float)((double)bce_weight / ((double)N * (double)HW)), dlogits);
  return hipGetLastError();
}
