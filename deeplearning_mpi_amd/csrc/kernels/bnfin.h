// BatchNorm finalize bodies shared by the column-reduce + finalize kernels of bn.hip (forward:
// scale / shift / saved and running statistics; backward: dgamma / dbeta and the apply coefficients).
// An in-launch finalize inside the conv epilogue was measured and removed (every conv block paid a
// drained store + ticket before retiring: ResNet-50 -0.7 %, profiles/r3_fin_in_launch_rejected).
#pragma once
#include "common.h"

namespace dlmpi {

// `k = n` next to an fp32 output: the n - 1 fp32 roundings on its path from the double sums, plus one;
// tests/test_bn_family_fp64_gpu.py holds the output to k * 2^-24 of its fp64 value (profiles/bn_tests).
__device__ __forceinline__ void fin_fwd(const FinArgs& f, int c, double s1, double s2) {
  const double mean = s1 / f.count;
  double var = s2 / f.count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)f.eps));   // k = 2: the cast
  const float g = f.gamma ? f.gamma[c] : 1.f;
  const float b = f.beta ? f.beta[c] : 0.f;
  const float sc = g * invstd;   // k = 3: invstd, the product
  f.scale[c] = sc;
  f.shift[c] = b - (float)mean * sc;   // k = 6: the mean cast, sc (2), the product, the difference
  if (f.save_mean) f.save_mean[c] = (float)mean;   // k = 2: the cast
  if (f.save_invstd) f.save_invstd[c] = invstd;
  if (f.running_mean) {
    const double unbiased = f.count > 1.0 ? var * f.count / (f.count - 1.0) : var;
    // k = 6 each: 1 - momentum, its product, the cast, its product, the sum
    f.running_mean[c] = (1.f - f.momentum) * f.running_mean[c] + f.momentum * (float)mean;
    f.running_var[c] = (1.f - f.momentum) * f.running_var[c] + f.momentum * (float)unbiased;
  }
}

// coef[0..2][C] = (k1, k2, k3) with dx = k1*dyr + k2*x + k3; dgamma/dbeta accumulate.
__device__ __forceinline__ void fin_bwd(const FinArgs& f, int c, double s1, double s2, int C) {
  // raw_z: the second sum is sum dyr*z (BN input), not sum dyr*xhat
  if (f.raw_z) s2 = (double)f.invstd[c] * (s2 - (double)f.mean[c] * s1);
  if (f.dbeta) f.dbeta[c] += (float)s1;     // k = 3: the cast, the sum
  if (f.dgamma) f.dgamma[c] += (float)s2;   // k = 3: the cast, the sum
  if (f.coef) {
    const double is = f.invstd[c];
    const double k1 = (f.gamma ? (double)f.gamma[c] : 1.0) * is;
    const double k2 = -k1 * is * s2 / f.count;
    const double k3 = -k1 * s1 / f.count - k2 * (double)f.mean[c];
    f.coef[c] = (float)k1;   // k = 2 for each coefficient: the cast (k1, k2, k3 are double)
    f.coef[C + c] = (float)k2;
    f.coef[2 * C + c] = (float)k3;
  }
}

}  // namespace dlmpi
