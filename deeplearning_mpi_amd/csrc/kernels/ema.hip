// Weight EMA over the flat fp32 buffers of a ParamArena: e += (1 - d_t) (w - e) for the master weights
// (ParamArena.flat) and the BatchNorm running statistics (ParamArena.fbuf) in one launch, and the swap that puts
// the averaged values in the model's place for evaluation.  Like the optimizers' skips and LARS's schedule, the
// counters and the "was this optimizer update applied?" decision live on the device (state, fp32 [8]), so a step
// captured into a hipGraph keeps its warm-up, its `every` and its skips under replay:
//   state[0] n     optimizer updates seen applied        state[3] omd of the last EMA update applied
//   state[1] s     EMA updates applied                   state[4] 1 if the last call updated, else 0
//   state[2] the optimizer's device step counter as last seen          state[5..7] spare
// Everything launches on the caller's stream: no stream, event or fork of its own.
#include "common.h"

namespace dlmpi {

struct EmaDecision {
  bool applied, fire;
  float omd;
};

// Every thread of ema_update_kernel, and then the one thread of ema_advance_kernel, compute this from the same
// unmodified inputs (the grid kernel never writes the state).  skip_flag: non-zero = the optimizer skipped
// (SGD.skip_flag); counter: the optimizer's device count of applied updates, which did not move iff it skipped.
__device__ __forceinline__ EmaDecision ema_decide(const float* __restrict__ state, const float* __restrict__ skip_flag,
                                                  const float* __restrict__ counter, int every, int warmup,
                                                  double decay) {
  EmaDecision d;
  d.applied = !(skip_flag && *skip_flag != 0.f) && !(counter && *counter == state[2]);
  d.fire = d.applied && fmodf(state[0] + 1.f, (float)every) == 0.f;
  double dt = decay;
  if (warmup) {   // timm / tf.train.ExponentialMovingAverage: (1 + s) / (10 + s), from the caller's double decay
    const double s = (double)state[1], w = (1.0 + s) / (10.0 + s);
    dt = w < decay ? w : decay;
  }
  d.omd = (float)(1.0 - dt);
  return d;
}

// One element: one subtraction and one fma, contraction off, so the 16-byte loop and the element loop round alike
// (the guarantee sgd_elem / adam_elem give).
__device__ __forceinline__ float ema_elem(float e, float w, float omd) {
#pragma clang fp contract(off)
  const float d = w - e;
  return __builtin_fmaf(omd, d, e);
}

// 16-byte accesses when both arrays allow them (the arena's do), the element loop for the tail or for everything
__device__ __forceinline__ void ema_range(float* __restrict__ e, const float* __restrict__ w, int64_t n, float omd) {
  const bool vec = (((uintptr_t)e | (uintptr_t)w) & 15) == 0;
  const int64_t n4 = vec ? n >> 2 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < n4; i += stride) {
    f32x4 ev = reinterpret_cast<f32x4*>(e)[i];
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] = ema_elem(ev[k], wv[k], omd);
    reinterpret_cast<f32x4*>(e)[i] = ev;
  }
  for (int64_t t = (n4 << 2) + t0; t < n; t += stride) e[t] = ema_elem(e[t], w[t], omd);
}

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ w, int64_t n,
                                                         float* __restrict__ eb, const float* __restrict__ b,
                                                         int64_t nb, const float* __restrict__ state,
                                                         const float* __restrict__ skip_flag,
                                                         const float* __restrict__ counter, int every, int warmup,
                                                         double decay) {
  const EmaDecision d = ema_decide(state, skip_flag, counter, every, warmup, decay);
  if (!d.fire) return;
  ema_range(e, w, n, d.omd);
  if (nb > 0) ema_range(eb, b, nb, d.omd);
}

// After ema_update_kernel (same stream): the same decision once more, then the counters.  One thread, no atomics.
__global__ void ema_advance_kernel(float* __restrict__ state, const float* __restrict__ skip_flag,
                                   const float* __restrict__ counter, int every, int warmup, double decay) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const EmaDecision d = ema_decide(state, skip_flag, counter, every, warmup, decay);
  if (d.applied) state[0] += 1.f;
  if (d.fire) {
    state[1] += 1.f;
    state[3] = d.omd;
  }
  if (counter) state[2] = *counter;
  state[4] = d.fire ? 1.f : 0.f;
}

__device__ __forceinline__ void swap_range(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const int64_t n4 = vec ? n >> 2 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < n4; i += stride) {
    const f32x4 av = reinterpret_cast<f32x4*>(a)[i], bv = reinterpret_cast<f32x4*>(b)[i];
    reinterpret_cast<f32x4*>(a)[i] = bv;
    reinterpret_cast<f32x4*>(b)[i] = av;
  }
  for (int64_t t = (n4 << 2) + t0; t < n; t += stride) {
    const float av = a[t], bv = b[t];
    a[t] = bv;
    b[t] = av;
  }
}

// exchange a <-> b (n elements) and, in the same launch, a2 <-> b2 (n2 elements, may be 0)
__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n,
                                                       float* __restrict__ a2, float* __restrict__ b2, int64_t n2) {
  swap_range(a, b, n);
  if (n2 > 0) swap_range(a2, b2, n2);
}

static inline unsigned blocks_for(int64_t n) {   // as optim.hip caps its grids
  int64_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" hipError_t dlmpi_ema_update(float* e, const float* w, int64_t n, float* eb, const float* b, int64_t nb,
                                       float* state, const float* skip_flag, const float* counter, int every,
                                       int warmup, double decay, int advance, hipStream_t s) {
  const int64_t big = n > nb ? n : nb;
  hipLaunchKernelGGL(ema_update_kernel, dim3(blocks_for(big / 4 + 1)), dim3(256), 0, s, e, w, n, eb, b, nb, state,
                     skip_flag, counter, every, warmup, decay);
  // advance 0: the state stays (one launch per tensor without an arena: only the last one advances it)
  if (advance)
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, s, state, skip_flag, counter, every, warmup, decay);
  return hipGetLastError();
}
extern "C" hipError_t dlmpi_swap_f32(float* a, float* b, int64_t n, float* a2, float* b2, int64_t n2, hipStream_t s) {
  const int64_t big = n > n2 ? n : n2;
  hipLaunchKernelGGL(swap_f32_kernel, dim3(blocks_for(big / 4 + 1)), dim3(256), 0, s, a, b, n, a2, b2, n2);
  return hipGetLastError();
}
