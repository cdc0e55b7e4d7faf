// Chunked row reduction shared by the BatchNorm statistics kernels (bn.hip) and the fused gradient
// producers (head.hip: outer_dgrad_bn / head_dgrad_bn, pool.hip: maxpool_bwd_bn): the row map and the
// fixed-order block combine.  Grids: dlmpi_reduce_blocks / dlmpi_fused_blocks (bn.hip).
#pragma once
#include "common.h"

namespace dlmpi {

// A block of 256 threads walks rows; thread -> (chunk of 8 channels cc, row lane rr).
struct RowMap {
  int CC, RPB, cc, rr;
  bool active;
};
__device__ __forceinline__ RowMap rowmap(int C) {
  RowMap m;
  m.CC = C >> 3;
  m.RPB = 256 / m.CC;
  m.cc = threadIdx.x % m.CC;
  m.rr = threadIdx.x / m.CC;
  m.active = m.rr < m.RPB;
  return m;
}

// Block-level combine of per-thread [8] sums over threads that share a channel chunk; writes
// partial[blk][k][C] for k < NS.
// Fixed summation order over the row lanes -> bit-reproducible partials.
template <int NS>
__device__ void block_combine(float (*acc)[8], const RowMap& rm, int C, float* partial) {
  __shared__ float buf[256 * NS * 8];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) buf[(threadIdx.x * NS + k) * 8 + e] = acc[k][e];
  __syncthreads();
  for (int i = threadIdx.x; i < NS * C; i += 256) {
    const int k = i / C, c = i - k * C, cc = c >> 3, e = c & 7;
    float s = 0.f;
    for (int r = 0; r < rm.RPB; ++r) s += buf[((r * rm.CC + cc) * NS + k) * 8 + e];
    partial[(int64_t)blockIdx.x * NS * C + i] = s;
  }
}

}  // namespace dlmpi
