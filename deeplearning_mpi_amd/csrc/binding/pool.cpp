// Torch binding of pooling, the layout / cast kernels and the fused gradient producers of the layer below a pool or
// a UNet head (kernels/pool.hip, head.hip, cast.hip, pixel_ce.hip's pad-cast).  The pool, up-sampling, layout and
// cast binders check dtypes only: their shapes are the caller's (NativeBackend).
#include "common.h"

namespace dlmpi_ext {
namespace {

// the fused gradient producers (head.hip, pool.hip; row map of rowreduce.h): z and dx dense [M][C] of the activation
// type, mscale / mshift per channel; -> their grid (partials [blocks][2][C])
int fused_producer(int64_t M, int C, const at::Tensor& z, const at::Tensor& mscale, const at::Tensor& mshift,
                   const at::Tensor& dx, const char* what) {
  rowmap_shape(M, C, what);
  slice_ok(z, M, C, C, 0, what, "z");
  slice_ok(dx, M, C, C, 0, what, "dx");
  floats_ok(mscale, C, what, "mscale");
  floats_ok(mshift, C, what, "mshift");
  return dlmpi_fused_blocks(M, C);
}

// ys (optional): also store the applied input relu(x * scale + shift) there (2x2 / s2 windows only)
void maxpool_fwd(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, int k, int stride, int pad,
                 at::Tensor y, at::Tensor idx, int OH, int OW, const c10::optional<at::Tensor>& scale,
                 const c10::optional<at::Tensor>& shift, const c10::optional<at::Tensor>& ys, int ldys, int ysoff) {
  same_type(x, y, "maxpool_fwd y");
  same_type(x, ys, "maxpool_fwd ys");
  check(dlmpi_maxpool_fwd(x.data_ptr(), N, H, W, C, ldx, xoff, k, stride, pad, y.data_ptr(), ptr<uint8_t>(idx), OH, OW,
                          optr<float>(scale), optr<float>(shift), given(ys) ? ys->data_ptr() : nullptr, ldys,
                          ysoff, act_f32(x, "maxpool_fwd"), cur_stream()),
        "maxpool_fwd");
}
void maxpool_bwd(const at::Tensor& dy, const at::Tensor& idx, int N, int H, int W, int C, int k, int stride, int pad,
                 int OH, int OW, const c10::optional<at::Tensor>& add, int ldadd, int addoff, at::Tensor dx, int lddx,
                 int dxoff) {
  same_type(dy, add, "maxpool_bwd add");
  same_type(dy, dx, "maxpool_bwd dx");
  check(dlmpi_maxpool_bwd(dy.data_ptr(), ptr<uint8_t>(idx), N, H, W, C, k, stride, pad, OH, OW, optr<uint16_t>(add),
                          ldadd, addoff, dx.data_ptr(), lddx, dxoff, act_f32(dy, "maxpool_bwd"), cur_stream()),
        "maxpool_bwd");
}
// data gradient of a 1x1 convolution with one output channel (UNet head) fused with the BN backward of
// the layer below; returns the partials [nblk][2][C] for bn_bwd_finalize_fused
at::Tensor outer_dgrad_bn(const at::Tensor& dy, int lddy, int64_t M, int C, const at::Tensor& w, int ldw,
                          const at::Tensor& z, const at::Tensor& mscale, const at::Tensor& mshift, at::Tensor dx) {
  require_gpu(dy, "dy");
  const int nblk = fused_producer(M, C, z, mscale, mshift, dx, "outer_dgrad_bn");
  at::Tensor part = at::empty({nblk, 2, C}, dy.options().dtype(at::kFloat));
  same_type(dy, w, "outer_dgrad_bn w");
  same_type(dy, z, "outer_dgrad_bn z");
  same_type(dy, dx, "outer_dgrad_bn dx");
  check(dlmpi_outer_dgrad_bn(dy.data_ptr(), lddy, M, C, w.data_ptr(), ldw, z.data_ptr(), ptr<float>(mscale),
                             ptr<float>(mshift), dx.data_ptr(), ptr<float>(part), nblk, act_f32(dy, "outer_dgrad_bn"),
                             cur_stream()),
        "outer_dgrad_bn");
  return part;
}
// the same for a 1x1 convolution with K = 2..4 output channels (the multi-class UNet head): dl [M][lddl],
// w [C][ldw] with the K class weights of a channel first in its row
at::Tensor head_dgrad_bn(const at::Tensor& dl, int lddl, int K, int64_t M, int C, const at::Tensor& w, int ldw,
                         const at::Tensor& z, const at::Tensor& mscale, const at::Tensor& mshift, at::Tensor dx) {
  require_gpu(dl, "dl");
  if (K < 2 || K > 4 || lddl < K || ldw < K) fail("head_dgrad_bn", "2 <= K <= 4, lddl / ldw >= K");
  const int nblk = fused_producer(M, C, z, mscale, mshift, dx, "head_dgrad_bn");
  same_type(dl, w, "head_dgrad_bn w");
  same_type(dl, z, "head_dgrad_bn z");
  same_type(dl, dx, "head_dgrad_bn dx");
  if (dl.numel() < (M - 1) * lddl + K || w.numel() < (int64_t)(C - 1) * ldw + K || !dl.is_contiguous() ||
      !w.is_contiguous() || !z.is_contiguous() || !dx.is_contiguous())
    fail("head_dgrad_bn", "operand sizes");
  at::Tensor part = at::empty({nblk, 2, C}, dl.options().dtype(at::kFloat));
  check(dlmpi_head_dgrad_bn(dl.data_ptr(), lddl, K, M, C, w.data_ptr(), ldw, z.data_ptr(), ptr<float>(mscale),
                            ptr<float>(mshift), dx.data_ptr(), ptr<float>(part), nblk, act_f32(dl, "head_dgrad_bn"),
                            cur_stream()),
        "head_dgrad_bn");
  g_ran.head_dgrad = 1;
  return part;
}
// max-pool backward fused with the BN-backward statistics of the producing BN+ReLU (mask from z);
// returns the partials [nblk][2][C] for bn_bwd_finalize_fused
at::Tensor maxpool_bwd_bn(const at::Tensor& dy, const at::Tensor& idx, int N, int H, int W, int C, int k, int stride,
                          int pad, int OH, int OW, const at::Tensor& z, const at::Tensor& mscale,
                          const at::Tensor& mshift, const c10::optional<at::Tensor>& add, int ldadd, int addoff,
                          at::Tensor dx) {
  const int64_t M = (int64_t)N * H * W, MO = (int64_t)N * OH * OW;
  const int nblk = fused_producer(M, C, z, mscale, mshift, dx, "maxpool_bwd_bn");
  slice_ok(add, M, C, ldadd, addoff, "maxpool_bwd_bn", "add");
  slice_ok(dy, MO, C, C, 0, "maxpool_bwd_bn", "dy");
  slice_ok(idx, MO, C, C, 0, "maxpool_bwd_bn", "idx");
  at::Tensor part = at::empty({nblk, 2, C}, dy.options().dtype(at::kFloat));
  same_type(dy, z, "maxpool_bwd_bn z");
  same_type(dy, add, "maxpool_bwd_bn add");
  same_type(dy, dx, "maxpool_bwd_bn dx");
  check(dlmpi_maxpool_bwd_bn(dy.data_ptr(), ptr<uint8_t>(idx), N, H, W, C, k, stride, pad, OH, OW, z.data_ptr(),
                             ptr<float>(mscale), ptr<float>(mshift), optr<uint16_t>(add), ldadd, addoff, dx.data_ptr(),
                             ptr<float>(part), nblk, act_f32(dy, "maxpool_bwd_bn"), cur_stream()),
        "maxpool_bwd_bn");
  return part;
}
void avgpool_fwd(const at::Tensor& x, int N, int HW, int C, at::Tensor y) {
  same_type(x, y, "avgpool_fwd y");
  check(dlmpi_avgpool_fwd(x.data_ptr(), N, HW, C, y.data_ptr(), act_f32(x, "avgpool_fwd"), cur_stream()), "avgpool_fwd");
}
void avgpool_bwd(const at::Tensor& dy, int N, int HW, int C, at::Tensor dx) {
  same_type(dy, dx, "avgpool_bwd dx");
  check(dlmpi_avgpool_bwd(dy.data_ptr(), N, HW, C, dx.data_ptr(), act_f32(dy, "avgpool_bwd"), cur_stream()),
        "avgpool_bwd");
}
void nchw_to_nhwc(const at::Tensor& x, int N, int C, int H, int W, int Cpad, at::Tensor y) {
  check(dlmpi_nchw_to_nhwc(ptr<float>(x), N, C, H, W, Cpad, y.data_ptr(), act_f32(y, "nchw_to_nhwc"), cur_stream()),
        "nchw_to_nhwc");
}
void s2d_nchw(const at::Tensor& x, int N, int C, int H, int W, int pad, int U, int V, int CS, at::Tensor y) {
  check(dlmpi_s2d_nchw(ptr<float>(x), N, C, H, W, pad, U, V, CS, y.data_ptr(), act_f32(y, "s2d_nchw"), cur_stream()),
        "s2d_nchw");
}
void upsample2x_fwd(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, at::Tensor y, int ldy,
                    int yoff) {
  same_type(x, y, "upsample2x_fwd y");
  check(dlmpi_upsample2x_fwd(x.data_ptr(), N, H, W, C, ldx, xoff, y.data_ptr(), ldy, yoff, act_f32(x, "upsample2x_fwd"),
                             cur_stream()),
        "upsample2x_fwd");
}
void upsample2x_bwd(const at::Tensor& dy, int N, int H, int W, int C, int lddy, int dyoff, at::Tensor dx) {
  same_type(dy, dx, "upsample2x_bwd dx");
  check(dlmpi_upsample2x_bwd(dy.data_ptr(), N, H, W, C, lddy, dyoff, dx.data_ptr(), act_f32(dy, "upsample2x_bwd"),
                             cur_stream()),
        "upsample2x_bwd");
}

// entries: int64 tensor [n][16] on the host: src_ptr, dst_ptr, d0..d3, v0..v3, s0..s3, start
// f32: the destinations are fp32 compute copies (fp32 precision path), else bf16
void cast_weights(const at::Tensor& entries_dev, const at::Tensor& block_map_dev, bool f32) {
  check(dlmpi_cast_weights(reinterpret_cast<const CastEntry*>(entries_dev.data_ptr()), block_map_dev.data_ptr(),
                           (int)(block_map_dev.numel() / 4), f32 ? 1 : 0, cur_stream()),
        "cast_weights");
}
// channels-last loss gradient x [M][K] fp32 -> y [M][Kp] activations, zero-padded
void nhwc_pad_cast(const at::Tensor& x, int64_t M, int K, int Kp, at::Tensor y) {
  dense(x, at::kFloat, M * K, "nhwc_pad_cast", "x");
  const int f32 = act_f32(y, "nhwc_pad_cast");
  dense(y, f32 ? at::kFloat : at::kBFloat16, M * Kp, "nhwc_pad_cast", "y");
  check(dlmpi_nhwc_pad_cast(ptr<float>(x), M, K, Kp, y.data_ptr(), f32, cur_stream()), "nhwc_pad_cast");
}
}  // namespace

void register_pool(pybind11::module& m) {
  namespace py = pybind11;
  m.def("maxpool_fwd", &maxpool_fwd, py::arg("x"), py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"),
        py::arg("ldx"), py::arg("xoff"), py::arg("k"), py::arg("stride"), py::arg("pad"), py::arg("y"), py::arg("idx"),
        py::arg("OH"), py::arg("OW"), py::arg("scale"), py::arg("shift"), py::arg("ys") = py::none(),
        py::arg("ldys") = 0, py::arg("ysoff") = 0);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("maxpool_bwd_bn", &maxpool_bwd_bn);
  m.def("outer_dgrad_bn", &outer_dgrad_bn);
  m.def("head_dgrad_bn", &head_dgrad_bn);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("upsample2x_fwd", &upsample2x_fwd);
  m.def("upsample2x_bwd", &upsample2x_bwd);
  m.def("nchw_to_nhwc", &nchw_to_nhwc);
  m.def("s2d_nchw", &s2d_nchw);
  m.def("nhwc_pad_cast", &nhwc_pad_cast);
  m.def("cast_weights", &cast_weights);
  m.attr("CAST_ENTRY_BYTES") = (int)sizeof(CastEntry);
}

}  // namespace dlmpi_ext
