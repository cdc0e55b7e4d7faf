// Tensor plumbing shared by the binding's translation units.
#pragma once
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <stdexcept>
#include <string>

#include "../kernels/dlmpi_kernels.h"
#include "checks.h"
#include "conv_plan.h"

namespace dlmpi_ext {

static inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

static inline void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("dlmpi kernel launch failed: ") + what + ": " +
                                                hipGetErrorString(e));
}

template <typename T>
static inline T* ptr(const at::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}
template <typename T>
static inline T* optr(const c10::optional<at::Tensor>& t) {
  return given(t) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

static inline void require_gpu(const at::Tensor& t, const char* name) {
  if (!t.is_cuda()) throw std::runtime_error(std::string(name) + " must be a GPU tensor");
}

// Activation storage type: bf16 (the product path) or fp32 (the fp32 precision path).  Every
// activation operand of one launch must share it; the kernels are instantiated for both.
static inline int act_f32(const at::Tensor& t, const char* what) {
  if (t.scalar_type() == at::kFloat) return 1;
  if (t.scalar_type() == at::kBFloat16) return 0;
  throw std::runtime_error(std::string(what) + ": activations must be bf16 or fp32");
}
static inline void same_type(const at::Tensor& ref, const c10::optional<at::Tensor>& t, const char* what) {
  if (given(t) && t->scalar_type() != ref.scalar_type())
    throw std::runtime_error(std::string(what) + ": operand dtype differs from the activations'");
}
static inline void same_type(const at::Tensor& ref, const at::Tensor& t, const char* what) {
  same_type(ref, c10::optional<at::Tensor>(t), what);
}

// The facts of a tensor argument the argument checks (conv_plan.h) work on; absent: numel -1.
static inline int64_t onumel(const c10::optional<at::Tensor>& t) {
  return given(t) ? (int64_t)t->numel() : -1;
}
static inline Operand operand(const at::Tensor& t, int ld, int off) { return Operand{(int64_t)t.numel(), ld, off}; }
static inline Operand operand(const c10::optional<at::Tensor>& t, int ld, int off) {
  return Operand{onumel(t), ld, off};
}
static inline void require_ok(const std::string& err) {
  if (!err.empty()) throw std::runtime_error(err);
}

static inline at::Tensor colsum_ws(const at::Tensor& like, int T, int C) {
  return at::empty({(int64_t)dlmpi_colsum_ws_doubles(T, C)}, like.options().dtype(at::kDouble));
}

// A plain int switch / flag as Python functions: `set` (int) -> None and / or `get` () -> int.
static inline void def_int(pybind11::module& m, const char* set, const char* get, int* v) {
  if (set) m.def(set, [v](int x) { *v = x; });
  if (get) m.def(get, [v]() { return *v; });
}

// the Python functions of each translation unit (ops.cpp: register_ops calls them all)
void register_conv_fwd(pybind11::module& m);
void register_conv_bwd(pybind11::module& m);
void register_bn(pybind11::module& m);
void register_pool(pybind11::module& m);
void register_loss(pybind11::module& m);
void register_optim(pybind11::module& m);
void register_data(pybind11::module& m);

// bn.cpp: the shape of the chunked row reductions (rowreduce.h rowmap), shared with the fused producers of pool.cpp
void rowmap_shape(int64_t M, int C, const char* fn);

// ---- shared by the forward and data-gradient launches (conv_fwd.cpp) ----------------------------
void finish_phase(dlmpi::ConvPhase& p, int Nimg, int C, int bm, bool f32 = false);
// one dense phase over the P x Q output grid: the whole of a forward convolution
void single_phase(dlmpi::ConvArgs& a, int P, int Q, int R, int S, int pad, int bm);
void fill_epilogue(dlmpi::ConvArgs& a, at::Tensor& y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
                   const c10::optional<at::Tensor>& res, int ldres, int resoff,
                   const c10::optional<at::Tensor>& scale, const c10::optional<at::Tensor>& shift, bool relu,
                   const c10::optional<at::Tensor>& stats);
void set_prologue(dlmpi::ConvArgs& a, int pro, const c10::optional<at::Tensor>& k0,
                  const c10::optional<at::Tensor>& k1, const c10::optional<at::Tensor>& pz, int ldpz, int pzoff);
void apply_halo(dlmpi::ConvArgs& a, int N, int bm);
bool autotune(dlmpi::ConvArgs& a, int pass, int& bm, int& bn);
dlmpi::Conv3StreamArgs conv3_args(const at::Tensor& x, int N, int H, int W, int ldx, int xoff, const at::Tensor& w,
                                  int flip, void* y, int ldy, int yoff, int th, int tw, int G);

}  // namespace dlmpi_ext
