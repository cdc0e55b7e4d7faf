// Torch binding of the gfx950 kernel library outside the convolutions (conv_fwd.cpp, conv_bwd.cpp), one file per
// family: bn.cpp, pool.cpp, loss.cpp, optim.cpp, data.cpp, and here the utilities, the stream / error helpers and
// register_ops.  Every function launches on the current HIP stream and never synchronises, so a whole training
// step can be captured into a hipGraph (the one exception, outside the step: image_rrc_batch of data.cpp).
#include "ops.h"

#include "common.h"

namespace dlmpi_ext {
namespace {

void fill_(at::Tensor t, double v) {
  dense(t, at::kFloat, t.numel(), "fill_", "t");
  check(dlmpi_fill_f32(ptr<float>(t), t.numel(), (float)v, cur_stream()), "fill");
}
// t: int64 [blocks][4] on the device (bench.py clock stamps)
void clock_stamp(at::Tensor t) {
  if (layout_fault(t, at::kLong) != Fault::none || t.dim() != 2 || t.size(1) != 4)
    fail("clock_stamp", "t must be a contiguous int64 [blocks][4] GPU tensor");
  check(dlmpi_clock_stamp(reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()), (int)t.size(0), cur_stream()),
        "clock_stamp");
}
void add_i64_(at::Tensor t, int64_t v) {
  dense(t, at::kLong, t.numel(), "add_i64_", "t");
  check(dlmpi_add_i64(ptr<int64_t>(t), t.numel(), v, cur_stream()), "add_i64");
}
// dst.view(-1)[i] (+)= src.view(-1)[idx[i]]  (idx < 0: 0), every i < idx.numel()
void gather_(at::Tensor dst, const at::Tensor& src, const at::Tensor& idx, bool accumulate) {
  if (dst.scalar_type() != src.scalar_type() || !dst.is_contiguous() || !src.is_contiguous() ||
      idx.scalar_type() != at::kLong || !idx.is_contiguous() || idx.numel() > dst.numel())
    fail("gather_", "contiguous dst/src of one dtype, int64 idx no longer than dst");
  check(dlmpi_gather(dst.data_ptr(), src.data_ptr(), ptr<int64_t>(idx), idx.numel(), (int)dst.element_size(),
                     accumulate ? 1 : 0, cur_stream()),
        "gather");
}

}  // namespace

void register_ops(pybind11::module& m) {
  register_conv_fwd(m);
  register_conv_bwd(m);
  register_bn(m);
  register_pool(m);
  register_loss(m);
  register_optim(m);
  register_data(m);
  m.def("fill_", &fill_);
  m.def("clock_stamp", &clock_stamp);
  m.def("add_i64_", &add_i64_);
  m.def("gather_", &gather_);
  m.def("set_aux_stream", [](int64_t h, int role) {
    check(dlmpi_set_aux_stream(reinterpret_cast<hipStream_t>(h), role), "set_aux_stream");
  });
  // bounded spin kernel on the current stream (tests: delays a collective to expose missing fences)
  m.def("delay_ms", [](double ms) { check(dlmpi_delay(ms, cur_stream()), "delay_ms"); });
  // reads and resets HIP's per-thread sticky error (a failed hipGraph capture leaves
  // hipErrorStreamCaptureInvalidated behind, which the next checked launch would report)
  m.def("clear_hip_error", []() { return (int)hipGetLastError(); });
  // raw HIP streams (not torch pool streams: one that a failed capture leaves in capture mode is
  // simply abandoned, never handed out again)
  m.def("create_stream", []() {
    hipStream_t s = nullptr;
    check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags");
    return reinterpret_cast<int64_t>(s);
  });
  m.def("stream_capturing", [](int64_t h) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(reinterpret_cast<hipStream_t>(h), &st);
    (void)hipGetLastError();
    return e != hipSuccess || st != hipStreamCaptureStatusNone;
  });
}

}  // namespace dlmpi_ext
