// Classification cross-entropy over [N][K] logits with torch's weight / ignore_index / label_smoothing
// semantics and two-label mixed targets (mixup, CutMix):
//   keep(y) = y != ignore_index and 0 <= y < K;  la = lam keep(a), lb = (1 - lam) keep(b), m = la + lb
//   q[c]    = (1 - eps) (la [a = c] + lb [b = c]) + (eps / K) m
//   D       = sum_n la w_a + lb w_b            S_n = sum_c w_c q[c]   (closed form, below)
//   loss    = sum_n sum_c w_c q[c] (lse_n - x_c) / D
//   dx[c]   = (go / D) (S_n softmax[c] - w_c q[c])
// Without labels_b: b = a and lam = 1.  lam is a device fp32 vector of 1 or N elements, trusted in [0, 1].
//
// A row belongs to one wave (kRowWaves rows per block), so a 10-class row costs 64 lanes, not a block; K = 1000
// is 16 elements per lane.  One online max / sum pass over the row; 16-byte loads over the part of a row that
// is 16-byte aligned (with K = 10 every second row starts 8 bytes off: the split is per row).  The N per-row
// terms are added by one block in a fixed order: bit-reproducible, no float atomics.
#include "common.h"

namespace dlmpi {

constexpr int kRowWaves = 4;   // rows (= waves) per block

// elements of the row before its first 16-byte boundary
__device__ __forceinline__ int row_head(const float* x, int K) {
  const int h = (int)(((16u - (uint32_t)((uintptr_t)x & 15u)) & 15u) >> 2);
  return h < K ? h : K;
}

__device__ __forceinline__ bool keep_label(int64_t y, int64_t ignore_index, int K) {
  return y != ignore_index && y >= 0 && y < (int64_t)K;
}

struct RowTarget {
  int64_t a, b;
  float la, lb;   // lam keep(a), (1 - lam) keep(b)
};
__device__ __forceinline__ RowTarget row_target(const int64_t* __restrict__ labels,
                                                const int64_t* __restrict__ labels_b,
                                                const float* __restrict__ lam, int lam_stride, int n,
                                                int64_t ignore_index, int K) {
  RowTarget t;
  t.a = labels[n];
  t.b = labels_b ? labels_b[n] : t.a;
  const float l = lam ? lam[(int64_t)n * lam_stride] : 1.f;
  t.la = keep_label(t.a, ignore_index, K) ? l : 0.f;
  t.lb = keep_label(t.b, ignore_index, K) ? 1.f - l : 0.f;
  return t;
}

// SMOOTH: the pass also accumulates sum_c w_c x_c and sum_c w_c (w = 1 without a weight vector)
template <bool HAS_W, bool SMOOTH>
__global__ __launch_bounds__(64 * kRowWaves) void cls_ce_fwd_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ labels_b, const float* __restrict__ lam, int lam_stride,
    const float* __restrict__ weight, int N, int K, int64_t ignore_index, float eps, float* __restrict__ lse,
    float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (n >= N) return;   // wave-uniform; no block-wide barrier below
  const float* x = logits + (int64_t)n * ldl;
  float m = -INFINITY, s = 0.f, wx = 0.f, ws = 0.f;
  auto one = [&](int c) {
    const float v = x[c];
    if (v > m) {
      s = s * __expf(m - v) + 1.f;
      m = v;
    } else if (v != -INFINITY) {
      s += __expf(v - m);
    }
    if (SMOOTH) {
      const float wc = HAS_W ? weight[c] : 1.f;
      wx += wc * v;
      ws += wc;
    }
  };
  const int head = row_head(x, K);
  const int nvec = (K - head) >> 2;
  const int tail = head + 4 * nvec;
  if (lane < head) one(lane);
  for (int i = lane; i < nvec; i += 64) {
    const int c = head + 4 * i;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
    const float vm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (vm > m) {
      s *= __expf(m - vm);
      m = vm;
    }
    if (m != -INFINITY) s += (__expf(v[0] - m) + __expf(v[1] - m)) + (__expf(v[2] - m) + __expf(v[3] - m));
    if (SMOOTH) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float wc = HAS_W ? weight[c + j] : 1.f;
        wx += wc * v[j];
        ws += wc;
      }
    }
  }
  if (tail + lane < K) one(tail + lane);
  const float M = warp_max(m);
  const float S = warp_sum(m == -INFINITY ? 0.f : s * __expf(m - M));
  const float l = M + __logf(S);
  if (SMOOTH) {
    wx = warp_sum(wx);
    ws = warp_sum(ws);
  }
  if (lane == 0) {
    lse[n] = l;
    const RowTarget t = row_target(labels, labels_b, lam, lam_stride, n, ignore_index, K);
    float num = 0.f, den = 0.f, srow = 0.f;
    if (t.la + t.lb != 0.f) {
      float ta = 0.f, tb = 0.f, na = 0.f, nb = 0.f;   // la w_a, lb w_b and their (lse - x) terms
      if (t.la != 0.f) {
        ta = t.la * (HAS_W ? weight[t.a] : 1.f);
        na = ta * (l - x[t.a]);
      }
      if (t.lb != 0.f) {
        tb = t.lb * (HAS_W ? weight[t.b] : 1.f);
        nb = tb * (l - x[t.b]);
      }
      den = ta + tb;
      num = (1.f - eps) * (na + nb);
      srow = (1.f - eps) * den;
      if (SMOOTH) {
        const float u = eps / (float)K * (t.la + t.lb);
        num += u * (l * ws - wx);
        srow += u * ws;
      }
    }
    rows[3 * (int64_t)n] = num;
    rows[3 * (int64_t)n + 1] = den;
    rows[3 * (int64_t)n + 2] = srow;
  }
}

// loss = sum_n num_n / sum_n den_n (NaN when nothing is kept, as torch), den[0] = sum_n den_n; one block
__global__ __launch_bounds__(256) void cls_ce_finish_kernel(const float* __restrict__ rows, int N,
                                                            float* __restrict__ loss, float* __restrict__ den) {
  __shared__ float sh[2][4];
  float a = 0.f, b = 0.f;
  for (int n = threadIdx.x; n < N; n += 256) {
    a += rows[3 * (int64_t)n];
    b += rows[3 * (int64_t)n + 1];
  }
  a = warp_sum(a);
  b = warp_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float num = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    const float d = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    *loss = num / d;
    *den = d;
  }
}

// dlogits [N][K] (contiguous) = (go / D) (S_n softmax - w q); exact zeros on rows without a kept label and when D = 0
template <bool HAS_W>
__global__ __launch_bounds__(64 * kRowWaves) void cls_ce_bwd_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ labels_b, const float* __restrict__ lam, int lam_stride,
    const float* __restrict__ weight, int N, int K, int64_t ignore_index, float eps,
    const float* __restrict__ lse, const float* __restrict__ rows, const float* __restrict__ den,
    const float* __restrict__ go, float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* x = logits + (int64_t)n * ldl;
  float* d = dlogits + (int64_t)n * K;
  const RowTarget t = row_target(labels, labels_b, lam, lam_stride, n, ignore_index, K);
  const float D = *den;
  const bool live = D != 0.f && t.la + t.lb != 0.f;
  const float g = live ? (go ? *go : 1.f) / D : 0.f;
  const float l = lse[n], srow = rows[3 * (int64_t)n + 2];
  const float qa = (1.f - eps) * t.la, qb = (1.f - eps) * t.lb, qu = eps / (float)K * (t.la + t.lb);
  auto grad = [&](int c, float v) {
    if (!live) return 0.f;
    const float q = qu + ((int64_t)c == t.a ? qa : 0.f) + ((int64_t)c == t.b ? qb : 0.f);
    return g * (srow * __expf(v - l) - (HAS_W ? weight[c] : 1.f) * q);
  };
  const int head = row_head(x, K);
  const int nvec = (K - head) >> 2;
  const int tail = head + 4 * nvec;
  const bool dvec = (((uintptr_t)(d + head)) & 15u) == 0;   // the gradient's row shares the logits' misalignment
  if (lane < head) d[lane] = grad(lane, x[lane]);
  for (int i = lane; i < nvec; i += 64) {
    const int c = head + 4 * i;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = grad(c + j, v[j]);
    if (dvec) {
      *reinterpret_cast<f32x4*>(d + c) = r;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[c + j] = r[j];
    }
  }
  if (tail + lane < K) d[tail + lane] = grad(tail + lane, x[tail + lane]);
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" hipError_t dlmpi_cls_ce_fwd(const float* logits, int ldl, const int64_t* labels, const int64_t* labels_b,
                                       const float* lam, int lam_stride, const float* weight, int N, int K,
                                       int64_t ignore_index, float eps, float* lse, float* rows, float* loss,
                                       float* den, hipStream_t s) {
  if (N < 1 || K < 1 || ldl < K) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((N + kRowWaves - 1) / kRowWaves)), block(64 * kRowWaves);
#define DLMPI_CLS_FWD(W, E)                                                                                      \
  hipLaunchKernelGGL((cls_ce_fwd_kernel<W, E>), grid, block, 0, s, logits, ldl, labels, labels_b, lam, lam_stride, \
                     weight, N, K, ignore_index, eps, lse, rows)
  if (weight) {
    if (eps > 0.f) DLMPI_CLS_FWD(true, true);
    else DLMPI_CLS_FWD(true, false);
  } else {
    if (eps > 0.f) DLMPI_CLS_FWD(false, true);
    else DLMPI_CLS_FWD(false, false);
  }
#undef DLMPI_CLS_FWD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cls_ce_finish_kernel, dim3(1), dim3(256), 0, s, rows, N, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_cls_ce_bwd(const float* logits, int ldl, const int64_t* labels, const int64_t* labels_b,
                                       const float* lam, int lam_stride, const float* weight, int N, int K,
                                       int64_t ignore_index, float eps, const float* lse, const float* rows,
                                       const float* den, const float* go, float* dlogits, hipStream_t s) {
  if (N < 1 || K < 1 || ldl < K) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((N + kRowWaves - 1) / kRowWaves)), block(64 * kRowWaves);
  if (weight)
    hipLaunchKernelGGL((cls_ce_bwd_kernel<true>), grid, block, 0, s, logits, ldl, labels, labels_b, lam, lam_stride,
                       weight, N, K, ignore_index, eps, lse, rows, den, go, dlogits);
  else
    hipLaunchKernelGGL((cls_ce_bwd_kernel<false>), grid, block, 0, s, logits, ldl, labels, labels_b, lam, lam_stride,
                       weight, N, K, ignore_index, eps, lse, rows, den, go, dlogits);
  return hipGetLastError();
}
