// The operand checks of the binders outside the convolutions (bn.cpp, pool.cpp, loss.cpp, optim.cpp, data.cpp,
// ops.cpp), written once.  Each is a few compares before anything is launched: no synchronisation, no allocation,
// and the text "<fn>: <why>" is built on the failing path only.
#pragma once
#include <torch/extension.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace dlmpi_ext {

// an optional tensor argument that is present and defined
static inline bool given(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

[[noreturn]] static inline void fail(const char* fn, const std::string& why) {
  throw std::runtime_error(std::string(fn) + ": " + why);
}

static inline const char* type_name(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return "fp32";
    case at::kBFloat16: return "bf16";
    case at::kInt: return "int32";
    case at::kLong: return "int64";
    case at::kByte: return "uint8";
    default: return c10::toString(t);
  }
}

// What keeps a tensor from being the contiguous GPU tensor of `type` a kernel takes as a bare pointer (the first
// that applies; image_rrc_batch has a text per fault, every other client only asks for none).
enum class Fault { none, host, dtype, strided };
static inline Fault layout_fault(const at::Tensor& t, at::ScalarType type) {
  if (!t.is_cuda()) return Fault::host;
  if (t.scalar_type() != type) return Fault::dtype;
  return t.is_contiguous() ? Fault::none : Fault::strided;
}

// an exact dense operand: a contiguous GPU tensor of `type` with exactly n elements
static inline void dense(const at::Tensor& t, at::ScalarType type, int64_t n, const char* fn, const char* name) {
  if (layout_fault(t, type) != Fault::none || t.numel() != n)
    fail(fn, std::string(name) + " must be a contiguous " + type_name(type) + " GPU tensor of " + std::to_string(n) +
                 " elements");
}
static inline void dense(const c10::optional<at::Tensor>& t, at::ScalarType type, int64_t n, const char* fn,
                         const char* name) {
  if (given(t)) dense(*t, type, n, fn, name);
}
// an exact-shape operand: a contiguous GPU tensor of `type` whose sizes are `shape`
static inline void shaped(const at::Tensor& t, at::ScalarType type, at::IntArrayRef shape, const char* fn,
                          const char* name) {
  if (layout_fault(t, type) == Fault::none && t.sizes() == shape) return;
  std::string want;
  for (size_t i = 0; i < shape.size(); ++i) want += (i ? ", " : "") + std::to_string(shape[i]);
  fail(fn, std::string(name) + " must be a contiguous " + type_name(type) + " [" + want + "] GPU tensor");
}

// The BN family's operands are slices of arenas: at least n elements and no contiguity rule.
// an fp32 tensor of at least n elements (a per-channel vector, the partials)
static inline void floats_ok(const at::Tensor& t, int64_t n, const char* fn, const char* name) {
  if (t.scalar_type() != at::kFloat) fail(fn, std::string(name) + " must be fp32");
  if (t.numel() < n) fail(fn, std::string(name) + " has fewer elements than the launch touches");
}
static inline void floats_ok(const c10::optional<at::Tensor>& t, int64_t n, const char* fn, const char* name) {
  if (given(t)) floats_ok(*t, n, fn, name);
}
// channels [off, off + C) of M rows of a [.][ld] buffer
static inline void slice_ok(const at::Tensor& t, int64_t M, int C, int ld, int off, const char* fn, const char* name) {
  if (off < 0 || (int64_t)off + C > ld) fail(fn, std::string(name) + ": off + C > ld");
  if (t.numel() < (M - 1) * (int64_t)ld + off + C) fail(fn, std::string(name) + ": buffer smaller than the slice");
}
static inline void slice_ok(const c10::optional<at::Tensor>& t, int64_t M, int C, int ld, int off, const char* fn,
                            const char* name) {
  if (given(t)) slice_ok(*t, M, C, ld, off, fn, name);
}

// per-channel mean / std of the image kernels, which take three floats each
struct Norm3 {
  float m3[3] = {0.f, 0.f, 0.f}, s3[3] = {1.f, 1.f, 1.f};
};
static inline Norm3 norm3(const std::vector<double>& mean, const std::vector<double>& sd, int64_t C, const char* fn) {
  if (C < 1 || C > 3 || mean.size() != (size_t)C || sd.size() != (size_t)C)
    fail(fn, "mean/std per channel, 1..3 channels");
  Norm3 n;
  for (int c = 0; c < C; ++c) { n.m3[c] = (float)mean[c]; n.s3[c] = (float)sd[c]; }
  return n;
}

}  // namespace dlmpi_ext
