// Boundary (surface) loss of Kervadec et al. (MIDL 2019), alone or added to the plain pixel-wise CE / BCE: the softmax
// (sigmoid) weighted by the signed distance map phi of edt.hip, in one fused pass over the pixel_softmax.h blocks.
//
// Softmax form.  phi fp32 [N][K][HW] (plain NCHW whatever the logits' layout), p = exp(x - lse) in the arithmetic of
// pixel_ce.hip, C = the classes c0..K-1 (c0 = 0, or 1 without the background), a pixel valid when pix_kept(label):
//     B = sum over valid q, c in C of p_c(q) phi_c(q) / (n_valid |C|),      loss = ce_weight CE + boundary_weight B
// with CE the plain unweighted mean over the valid pixels (left out at ce_weight = 0); n_valid = 0 gives B = 0.
// With a_c = phi_c [c in C] boundary_weight go / (n_valid |C|) and cs = ce_weight go / n_valid:
//     dx_j = p_j (a_j - sum_c a_c p_c) + cs (p_j - [j = t]),   exact zeros at invalid pixels.
// Sigmoid form (contiguous logits, float targets and phi of M elements): p = sigmoid(x), B = sum p phi / M,
// dx = phi p (1 - p) boundary_weight go / M + bce_weight go (p - t) / M.
// boundary_weight is a host float or, where bw_dev is given, one fp32 on the device read by the kernels, so a
// replayed graph follows a schedule written between replays.
//
// Passes: fwd (per block {sum p phi, sum nll} and the valid count, fixed order, no atomics; lse per pixel), finish
// (one block, the partials in fp64 in a fixed order -> loss, den = n_valid), bwd (one pointwise pass in the logits'
// strides).  Nothing needs zeroing, no host read: three kernel nodes under capture, the same bits on every run.
#include "pixel_softmax.h"

namespace dlmpi {

static inline int bd_blocks(int64_t M) {
  const int64_t b = (M + 255) / 256;
  return (int)(b > 2048 ? 2048 : b < 1 ? 1 : b);
}
static inline unsigned bd_stream_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b > 16384 ? 16384 : b < 1 ? 1 : b);
}
__device__ __forceinline__ float bd_bce_elem(float x, float t) {   // loss.hip's bce_elem
  return fmaxf(x, 0.f) - x * t + log1pf(__expf(-fabsf(x)));
}

// part[2 b] = the block's sum over its valid pixels of sum_{c >= c0} p_c phi_c, part[2 b + 1] = of lse - x_t
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void boundary_softmax_fwd_kernel(const float* __restrict__ logits, PixStrides st,
                                                                   int K, int64_t HW, int64_t M,
                                                                   const int64_t* __restrict__ labels,
                                                                   int64_t ignore_index,
                                                                   const float* __restrict__ phi, int c0,
                                                                   float* __restrict__ lse, float* __restrict__ part,
                                                                   unsigned* __restrict__ cnt) {
  __shared__ float shf[8];
  __shared__ unsigned shu[4];
  float acc[2] = {0.f, 0.f};
  unsigned nv[1] = {0u};
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const float* x = logits + n * st.sn + p * st.sp;
    const float* ph = phi + n * K * HW + p;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    float l, xt = 0.f, dot = 0.f;
    if constexpr (KC > 0) {
      float v[KC], w[KC];
      pix_load<KC, VEC>(x, st.sk, v);
#pragma unroll
      for (int k = 0; k < KC; ++k) w[k] = v[k];
      const PixSoftmax r = pix_softmax_reg<KC>(w, lab);
      l = r.mx + __logf(r.s);
      xt = r.xt;
      if (keep) {
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (c >= c0) dot += __expf(v[c] - l) * ph[c * HW];
      }
    } else {
      l = pix_online_lse(x, st.sk, K);
      if (keep) {
        xt = x[lab * st.sk];
        for (int c = c0; c < K; ++c) dot += __expf(x[c * st.sk] - l) * ph[c * HW];
      }
    }
    lse[m] = l;
    if (keep) {
      acc[0] += dot;
      acc[1] += l - xt;
      nv[0] += 1u;
    }
  }
  pix_block_sums<2, 1>(acc, nv, shf, shu);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = acc[0];
    part[2 * blockIdx.x + 1] = acc[1];
    cnt[blockIdx.x] = nv[0];
  }
}

__global__ __launch_bounds__(256) void boundary_sigmoid_fwd_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ target,
                                                                   const float* __restrict__ phi, int64_t M,
                                                                   float* __restrict__ part) {
  __shared__ float shf[8];
  float acc[2] = {0.f, 0.f};
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const float x = logits[m];
    acc[0] += phi[m] / (1.f + __expf(-x));
    acc[1] += bd_bce_elem(x, target[m]);
  }
  pix_block_sums<2, 0>(acc, nullptr, shf, nullptr);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = acc[0];
    part[2 * blockIdx.x + 1] = acc[1];
  }
}

__device__ __forceinline__ double bd_block_sum_d(double v, double* sh) {
  v = warp_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return v;
}

// One block.  cnt null: every one of the fixed_n pixels counts (the sigmoid form).  loss = plain_weight * nll / n +
// boundary_weight * b / (n * classes), the first term left out at plain_weight = 0, the second 0 at n = 0; den = n.
__global__ __launch_bounds__(256) void boundary_finish_kernel(const float* __restrict__ part,
                                                              const unsigned* __restrict__ cnt, int nblk,
                                                              int64_t fixed_n, int classes, float plain_weight,
                                                              float bw_host, const float* __restrict__ bw_dev,
                                                              float* __restrict__ loss, float* __restrict__ den) {
  __shared__ double sh[4];
  __shared__ unsigned shu[4];
  double b = 0.0, nll = 0.0;
  unsigned u[1] = {0u};
  for (int j = threadIdx.x; j < nblk; j += 256) {
    b += (double)part[2 * j];
    nll += (double)part[2 * j + 1];
    if (cnt) u[0] += cnt[j];
  }
  b = bd_block_sum_d(b, sh);
  nll = bd_block_sum_d(nll, sh);
  pix_block_sums<0, 1>(nullptr, u, nullptr, shu);
  if (threadIdx.x == 0) {
    const double n = cnt ? (double)u[0] : (double)fixed_n;
    const float bw = bw_dev ? *bw_dev : bw_host;
    double v = n > 0.0 ? (double)bw * (b / (n * (double)classes)) : 0.0;
    if (plain_weight != 0.f) v += (double)plain_weight * (nll / n);
    *loss = (float)v;
    *den = (float)n;
  }
}

template <int KC, bool VEC>
__global__ __launch_bounds__(256) void boundary_softmax_bwd_kernel(const float* __restrict__ logits, PixStrides st,
                                                                   int K, int64_t HW, int64_t M,
                                                                   const int64_t* __restrict__ labels,
                                                                   int64_t ignore_index,
                                                                   const float* __restrict__ phi, int c0,
                                                                   const float* __restrict__ lse,
                                                                   const float* __restrict__ den,
                                                                   const float* __restrict__ go, float ce_weight,
                                                                   float bw_host, const float* __restrict__ bw_dev,
                                                                   float* __restrict__ dlogits) {
  const float gout = go ? *go : 1.f;
  const float nvalid = *den;
  const float bs = (bw_dev ? *bw_dev : bw_host) * gout / (nvalid * (float)(K - c0));
  const float cs = ce_weight != 0.f ? ce_weight * gout / nvalid : 0.f;
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const int64_t off = n * st.sn + p * st.sp;
    const float* ph = phi + n * K * HW + p;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    const float l = lse[m];
    if constexpr (KC > 0) {
      float v[KC], a[KC];
      if (keep) {
        pix_load<KC, VEC>(logits + off, st.sk, v);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          v[c] = __expf(v[c] - l);
          a[c] = c >= c0 ? ph[c * HW] * bs : 0.f;
          dot += a[c] * v[c];
        }
#pragma unroll
        for (int c = 0; c < KC; ++c) v[c] = v[c] * (a[c] - dot) + (v[c] - ((int64_t)c == lab ? 1.f : 0.f)) * cs;
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) v[c] = 0.f;
      }
      pix_store<KC, VEC>(dlogits + off, st.sk, v);
    } else {
      if (keep) {
        float dot = 0.f;
        for (int c = c0; c < K; ++c) dot += ph[c * HW] * bs * __expf(logits[off + c * st.sk] - l);
        for (int c = 0; c < K; ++c) {
          const float pc = __expf(logits[off + c * st.sk] - l);
          const float ac = c >= c0 ? ph[c * HW] * bs : 0.f;
          dlogits[off + c * st.sk] = pc * (ac - dot) + (pc - ((int64_t)c == lab ? 1.f : 0.f)) * cs;
        }
      } else {
        for (int c = 0; c < K; ++c) dlogits[off + c * st.sk] = 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(256) void boundary_sigmoid_bwd_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ target,
                                                                   const float* __restrict__ phi, int64_t M,
                                                                   const float* __restrict__ go, float bce_weight,
                                                                   float bw_host, const float* __restrict__ bw_dev,
                                                                   float* __restrict__ dlogits) {
  const float gout = go ? *go : 1.f;
  const float bs = (bw_dev ? *bw_dev : bw_host) * gout / (float)M;
  const float cs = bce_weight != 0.f ? bce_weight * gout / (float)M : 0.f;
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const float p = 1.f / (1.f + __expf(-logits[m]));
    dlogits[m] = phi[m] * (p * (1.f - p)) * bs + (p - target[m]) * cs;
  }
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_boundary_blocks(int64_t M) { return bd_blocks(M); }

// part: fp32 [2 * dlmpi_boundary_blocks(N * HW)], cnt: uint32 [dlmpi_boundary_blocks(N * HW)]
extern "C" hipError_t dlmpi_boundary_softmax_fwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                                 int64_t HW, const int64_t* labels, int64_t ignore_index,
                                                 const float* phi, int include_background, float ce_weight,
                                                 float bw_host, const float* bw_dev, float* lse, float* part,
                                                 uint32_t* cnt, float* loss, float* den, hipStream_t s) {
  if (K < 2 || K > 256 || HW < 1 || N < 1) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  const int nblk = bd_blocks(M), c0 = include_background ? 0 : 1;
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, nullptr, K, sn, sk, sp);
  PIX_DISPATCH(boundary_softmax_fwd_kernel, dim3((unsigned)nblk), vec, logits, st, K, HW, M, labels, ignore_index, phi,
               c0, lse, part, cnt);
  hipLaunchKernelGGL(boundary_finish_kernel, dim3(1), dim3(256), 0, s, part, cnt, nblk, (int64_t)0, K - c0, ce_weight,
                     bw_host, bw_dev, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_boundary_softmax_bwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                                 int64_t HW, const int64_t* labels, int64_t ignore_index,
                                                 const float* phi, int include_background, const float* lse,
                                                 const float* den, const float* go, float ce_weight, float bw_host,
                                                 const float* bw_dev, float* dlogits, hipStream_t s) {
  if (K < 2 || K > 256 || HW < 1 || N < 1 || !den) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  const int c0 = include_background ? 0 : 1;
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, dlogits, K, sn, sk, sp);
  PIX_DISPATCH(boundary_softmax_bwd_kernel, dim3(bd_stream_blocks(M)), vec, logits, st, K, HW, M, labels, ignore_index,
               phi, c0, lse, den, go, ce_weight, bw_host, bw_dev, dlogits);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_boundary_sigmoid_fwd(const float* logits, const float* target, const float* phi, int64_t M,
                                                 float bce_weight, float bw_host, const float* bw_dev, float* part,
                                                 float* loss, float* den, hipStream_t s) {
  if (M < 1) return hipErrorInvalidValue;
  const int nblk = bd_blocks(M);
  hipLaunchKernelGGL(boundary_sigmoid_fwd_kernel, dim3((unsigned)nblk), dim3(256), 0, s, logits, target, phi, M, part);
  hipLaunchKernelGGL(boundary_finish_kernel, dim3(1), dim3(256), 0, s, part, (const unsigned*)nullptr, nblk, M, 1,
                     bce_weight, bw_host, bw_dev, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_boundary_sigmoid_bwd(const float* logits, const float* target, const float* phi, int64_t M,
                                                 const float* go, float bce_weight, float bw_host, const float* bw_dev,
                                                 float* dlogits, hipStream_t s) {
  if (M < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(boundary_sigmoid_bwd_kernel, dim3(bd_stream_blocks(M)), dim3(256), 0, s, logits, target, phi, M,
                     go, bce_weight, bw_host, bw_dev, dlogits);
  return hipGetLastError();
}
