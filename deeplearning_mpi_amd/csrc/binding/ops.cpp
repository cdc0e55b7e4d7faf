// Torch binding of the gfx950 kernel library outside the convolutions (conv_fwd.cpp, conv_bwd.cpp):
// batch norm, pooling / layout, losses, optimisers, utilities and the device-resident input pipeline.
// Every function launches on the current HIP stream and never synchronises, so a whole training
// step can be captured into a hipGraph (the one exception, outside the step: image_rrc_batch reads a crop
// table back the first time it sees it).
#include "ops.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

namespace dlmpi_ext {

// --------------------------------- batch norm ----------------------------------------------
// Argument checks of the BatchNorm family: a few integer compares per call, before anything is
// launched (no synchronisation, no allocation).  The kernels index by M, C, ld and off alone, so
// whatever passes here stays inside every operand.
namespace {

[[noreturn]] void bn_fail(const char* what, const std::string& why) {
  throw std::runtime_error(std::string(what) + ": " + why);
}

// the chunked row reductions (rowreduce.h rowmap): 256 / (C / 8) row lanes per block
void rowmap_shape(int64_t M, int C, const char* what) {
  if (C < 8 || C % 8 || C > 2048) bn_fail(what, "C must be a multiple of 8 in [8, 2048]");
  if (M < 1) bn_fail(what, "M < 1");
}
// the elementwise kernels: one thread per 8 channels
void ew_shape(int64_t M, int C, const char* what) {
  if (C < 8 || C % 8) bn_fail(what, "C must be a positive multiple of 8");
  if (M < 1) bn_fail(what, "M < 1");
}
// channels [off, off + C) of M rows of a [.][ld] buffer
void slice_ok(const at::Tensor& t, int64_t M, int C, int ld, int off, const char* what, const char* name) {
  if (off < 0 || (int64_t)off + C > ld) bn_fail(what, std::string(name) + ": off + C > ld");
  if (t.numel() < (M - 1) * (int64_t)ld + off + C) bn_fail(what, std::string(name) + ": buffer smaller than the slice");
}
void slice_ok(const c10::optional<at::Tensor>& t, int64_t M, int C, int ld, int off, const char* what,
              const char* name) {
  if (t.has_value() && t->defined()) slice_ok(*t, M, C, ld, off, what, name);
}
// an fp32 tensor of at least n elements (a per-channel vector, the partials)
void floats_ok(const at::Tensor& t, int64_t n, const char* what, const char* name) {
  if (t.scalar_type() != at::kFloat) bn_fail(what, std::string(name) + " must be fp32");
  if (t.numel() < n) bn_fail(what, std::string(name) + " has fewer elements than the launch touches");
}
void floats_ok(const c10::optional<at::Tensor>& t, int64_t n, const char* what, const char* name) {
  if (t.has_value() && t->defined()) floats_ok(*t, n, what, name);
}
bool given(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

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

// the column reduce + finalize over partial [T][ns][C]
void colsum_shape(const at::Tensor& partial, int T, int ns, int C, double count, const char* what) {
  if (T < 1 || C < 1) bn_fail(what, "needs at least one partial row and one channel");
  if (!(count >= 1.0)) bn_fail(what, "count < 1");
  floats_ok(partial, (int64_t)T * ns * C, what, "partial");
}

}  // namespace

void bn_finalize(const at::Tensor& partial, int ntiles, int C, double count, const c10::optional<at::Tensor>& gamma,
                 const c10::optional<at::Tensor>& beta, const c10::optional<at::Tensor>& running_mean,
                 const c10::optional<at::Tensor>& running_var, double momentum, double eps, at::Tensor scale,
                 at::Tensor shift, const c10::optional<at::Tensor>& save_mean,
                 const c10::optional<at::Tensor>& save_invstd) {
  colsum_shape(partial, ntiles, 2, C, count, "bn_finalize");
  floats_ok(gamma, C, "bn_finalize", "gamma");
  floats_ok(beta, C, "bn_finalize", "beta");
  if (given(running_mean) != given(running_var)) bn_fail("bn_finalize", "running_mean / running_var come together");
  floats_ok(running_mean, C, "bn_finalize", "running_mean");
  floats_ok(running_var, C, "bn_finalize", "running_var");
  floats_ok(scale, C, "bn_finalize", "scale");
  floats_ok(shift, C, "bn_finalize", "shift");
  floats_ok(save_mean, C, "bn_finalize", "save_mean");
  floats_ok(save_invstd, C, "bn_finalize", "save_invstd");
  at::Tensor ws = colsum_ws(partial, ntiles, C);
  check(dlmpi_bn_finalize(ptr<float>(partial), ntiles, C, count, optr<float>(gamma), optr<float>(beta),
                          optr<float>(running_mean), optr<float>(running_var), (float)momentum, (float)eps,
                          ptr<float>(scale), ptr<float>(shift), optr<float>(save_mean), optr<float>(save_invstd),
                          ptr<double>(ws), cur_stream()),
        "bn_finalize");
}

int reduce_blocks(int64_t M, int C) {
  rowmap_shape(M, C, "reduce_blocks");
  return dlmpi_reduce_blocks(M, C);
}

void bn_stats(const at::Tensor& x, int64_t M, int C, int ldx, int xoff, at::Tensor partial, int nblk) {
  rowmap_shape(M, C, "bn_stats");
  if (nblk < 1) bn_fail("bn_stats", "nblk < 1");
  slice_ok(x, M, C, ldx, xoff, "bn_stats", "x");
  floats_ok(partial, (int64_t)nblk * 2 * C, "bn_stats", "partial");
  check(dlmpi_bn_stats(x.data_ptr(), M, C, ldx, xoff, ptr<float>(partial), nblk, act_f32(x, "bn_stats"), cur_stream()),
        "bn_stats");
}

void bn_apply(const at::Tensor& x, int ldx, int xoff, int64_t M, int C, const at::Tensor& scale,
              const at::Tensor& shift, const c10::optional<at::Tensor>& res, int ldres, int resoff, bool relu,
              at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& mbits,
              const c10::optional<at::Tensor>& rscale, const c10::optional<at::Tensor>& rshift) {
  ew_shape(M, C, "bn_apply");
  if (mbits && mbits->numel() != M * (C / 8)) throw std::runtime_error("bn_apply: mask bits must be [M][C/8]");
  if (rscale.has_value() != rshift.has_value() || (rscale && !res))
    throw std::runtime_error("bn_apply: rscale / rshift come together, with a residual");
  if (rscale && (rscale->numel() < C || rshift->numel() < C)) throw std::runtime_error("bn_apply: rscale / rshift < C");
  slice_ok(x, M, C, ldx, xoff, "bn_apply", "x");
  slice_ok(res, M, C, ldres, resoff, "bn_apply", "res");
  slice_ok(y, M, C, ldy, yoff, "bn_apply", "y");
  floats_ok(scale, C, "bn_apply", "scale");
  floats_ok(shift, C, "bn_apply", "shift");
  floats_ok(rscale, C, "bn_apply", "rscale");
  floats_ok(rshift, C, "bn_apply", "rshift");
  same_type(x, y, "bn_apply y");
  same_type(x, res, "bn_apply res");
  check(dlmpi_bn_apply2(x.data_ptr(), ldx, xoff, M, C, ptr<float>(scale), ptr<float>(shift), optr<uint16_t>(res), ldres,
                        resoff, optr<float>(rscale), optr<float>(rshift), relu ? 1 : 0, y.data_ptr(), ldy, yoff,
                        optr<uint8_t>(mbits), act_f32(x, "bn_apply"), cur_stream()),
        "bn_apply");
}

void bn_bwd_reduce(const at::Tensor& dy, int lddy, int dyoff, const c10::optional<at::Tensor>& ymask, int ldym,
                   int ymoff, const c10::optional<at::Tensor>& x, int ldx, int xoff, int64_t M, int C,
                   const c10::optional<at::Tensor>& mean, const c10::optional<at::Tensor>& invstd, at::Tensor partial,
                   int nblk) {
  rowmap_shape(M, C, "bn_bwd_reduce");
  if (nblk < 1) bn_fail("bn_bwd_reduce", "nblk < 1");
  if (given(x) && !(given(mean) && given(invstd))) bn_fail("bn_bwd_reduce", "x needs mean and invstd");
  slice_ok(dy, M, C, lddy, dyoff, "bn_bwd_reduce", "dy");
  slice_ok(ymask, M, C, ldym, ymoff, "bn_bwd_reduce", "ymask");
  slice_ok(x, M, C, ldx, xoff, "bn_bwd_reduce", "x");
  floats_ok(mean, C, "bn_bwd_reduce", "mean");
  floats_ok(invstd, C, "bn_bwd_reduce", "invstd");
  floats_ok(partial, (int64_t)nblk * 2 * C, "bn_bwd_reduce", "partial");
  same_type(dy, ymask, "bn_bwd_reduce ymask");
  same_type(dy, x, "bn_bwd_reduce x");
  check(dlmpi_bn_bwd_reduce(dy.data_ptr(), lddy, dyoff, optr<uint16_t>(ymask), ldym, ymoff, optr<uint16_t>(x), ldx,
                            xoff, M, C, optr<float>(mean), optr<float>(invstd), ptr<float>(partial), nblk,
                            act_f32(dy, "bn_bwd_reduce"), cur_stream()),
        "bn_bwd_reduce");
}

// the per-channel operands of both backward finalizes (fin_bwd reads mean and invstd for coef and for raw_z)
static void bwd_fin_vectors(int C, bool raw_z, const c10::optional<at::Tensor>& gamma,
                            const c10::optional<at::Tensor>& mean, const c10::optional<at::Tensor>& invstd,
                            const c10::optional<at::Tensor>& dgamma, const c10::optional<at::Tensor>& dbeta,
                            const c10::optional<at::Tensor>& coef, const char* what) {
  if ((given(coef) || raw_z) && !(given(mean) && given(invstd))) bn_fail(what, "coef needs mean and invstd");
  floats_ok(gamma, C, what, "gamma");
  floats_ok(mean, C, what, "mean");
  floats_ok(invstd, C, what, "invstd");
  floats_ok(dgamma, C, what, "dgamma");
  floats_ok(dbeta, C, what, "dbeta");
  floats_ok(coef, 3 * (int64_t)C, what, "coef");
}

void bn_bwd_finalize(const at::Tensor& partial, int nblk, int C, double count, const c10::optional<at::Tensor>& gamma,
                     const c10::optional<at::Tensor>& mean, const c10::optional<at::Tensor>& invstd,
                     const c10::optional<at::Tensor>& dgamma, const c10::optional<at::Tensor>& dbeta,
                     const c10::optional<at::Tensor>& coef) {
  colsum_shape(partial, nblk, 2, C, count, "bn_bwd_finalize");
  bwd_fin_vectors(C, false, gamma, mean, invstd, dgamma, dbeta, coef, "bn_bwd_finalize");
  at::Tensor ws = colsum_ws(partial, nblk, C);
  check(dlmpi_bn_bwd_finalize(ptr<float>(partial), nblk, C, count, optr<float>(gamma), optr<float>(mean),
                              optr<float>(invstd), optr<float>(dgamma), optr<float>(dbeta), optr<float>(coef),
                              ptr<double>(ws), cur_stream()),
        "bn_bwd_finalize");
}

// Finalize from the fused dgrad-epilogue partials [tiles][ns][C] (rows 0 and k2 = {sum dyr, sum dyr*z}).
void bn_bwd_finalize_fused(const at::Tensor& partial, int k2, int C, double count,
                           const c10::optional<at::Tensor>& gamma, const at::Tensor& mean, const at::Tensor& invstd,
                           const c10::optional<at::Tensor>& dgamma, const c10::optional<at::Tensor>& dbeta,
                           const c10::optional<at::Tensor>& coef) {
  if (partial.dim() != 3) throw std::runtime_error("bn_bwd_finalize_fused: partial must be [tiles][ns][C]");
  const int T = (int)partial.size(0), ns = (int)partial.size(1);
  if (partial.size(2) != C) throw std::runtime_error("bn_bwd_finalize_fused: channel mismatch");
  if (ns < 2 || ns > 3 || k2 < 1 || k2 >= ns) bn_fail("bn_bwd_finalize_fused", "ns in {2, 3} and 1 <= k2 < ns");
  colsum_shape(partial, T, ns, C, count, "bn_bwd_finalize_fused");
  bwd_fin_vectors(C, true, gamma, mean, invstd, dgamma, dbeta, coef, "bn_bwd_finalize_fused");
  at::Tensor ws = colsum_ws(partial, T, C);
  check(dlmpi_bn_bwd_finalize_ex(ptr<float>(partial), T, ns, k2, 1, C, count, optr<float>(gamma), ptr<float>(mean),
                                 ptr<float>(invstd), optr<float>(dgamma), optr<float>(dbeta), optr<float>(coef),
                                 ptr<double>(ws), cur_stream()),
        "bn_bwd_finalize_fused");
}

void bn_bwd_apply(const at::Tensor& dy, int lddy, int dyoff, const c10::optional<at::Tensor>& ymask, int ldym,
                  int ymoff, const at::Tensor& x, int ldx, int xoff, int64_t M, int C, const at::Tensor& coef,
                  at::Tensor dx, const c10::optional<at::Tensor>& dyr_out) {
  ew_shape(M, C, "bn_bwd_apply");
  slice_ok(dy, M, C, lddy, dyoff, "bn_bwd_apply", "dy");
  slice_ok(ymask, M, C, ldym, ymoff, "bn_bwd_apply", "ymask");
  slice_ok(x, M, C, ldx, xoff, "bn_bwd_apply", "x");
  slice_ok(dx, M, C, C, 0, "bn_bwd_apply", "dx");
  slice_ok(dyr_out, M, C, C, 0, "bn_bwd_apply", "dyr_out");
  floats_ok(coef, 3 * (int64_t)C, "bn_bwd_apply", "coef");
  same_type(dy, ymask, "bn_bwd_apply ymask");
  same_type(dy, x, "bn_bwd_apply x");
  same_type(dy, dx, "bn_bwd_apply dx");
  same_type(dy, dyr_out, "bn_bwd_apply dyr_out");
  check(dlmpi_bn_bwd_apply(dy.data_ptr(), lddy, dyoff, optr<uint16_t>(ymask), ldym, ymoff, x.data_ptr(), ldx, xoff, M,
                           C, ptr<float>(coef), dx.data_ptr(), optr<uint16_t>(dyr_out), act_f32(dy, "bn_bwd_apply"),
                           cur_stream()),
        "bn_bwd_apply");
}

// w2 [C][2K] = {wT * coef[0], wT * coef[1]}, b [C] = wT . coef[2]: the dual 1x1 data gradient (bn.hip)
void dual_dgrad_weights(const at::Tensor& wT, int C, int K, const at::Tensor& coef, at::Tensor w2, at::Tensor b) {
  same_type(wT, w2, "dual_dgrad_weights w2");
  if (C < 1 || K < 1 || wT.numel() < (int64_t)C * K || w2.numel() < (int64_t)C * 2 * K ||
      coef.numel() < 3 * (int64_t)K || b.numel() < C || b.scalar_type() != at::kFloat ||
      coef.scalar_type() != at::kFloat)
    throw std::runtime_error("dual_dgrad_weights: shapes / dtypes");
  check(dlmpi_dual_dgrad_weights(wT.data_ptr(), C, K, ptr<float>(coef), w2.data_ptr(), ptr<float>(b),
                                 act_f32(wT, "dual_dgrad_weights"), cur_stream()),
        "dual_dgrad_weights");
}

void channel_sum(const at::Tensor& x, int64_t M, int C, int ldx, int xoff, at::Tensor out_acc) {
  rowmap_shape(M, C, "channel_sum");
  slice_ok(x, M, C, ldx, xoff, "channel_sum", "x");
  floats_ok(out_acc, C, "channel_sum", "out_acc");
  const int nblk = dlmpi_reduce_blocks(M, C);
  at::Tensor partial = at::empty({(int64_t)nblk * 2 * C}, x.options().dtype(at::kFloat));
  at::Tensor ws = colsum_ws(partial, nblk, C);
  check(dlmpi_channel_sum(x.data_ptr(), M, C, ldx, xoff, ptr<float>(out_acc), ptr<float>(partial), nblk,
                          ptr<double>(ws), act_f32(x, "channel_sum"), cur_stream()),
        "channel_sum");
}

// --------------------------------- pooling / layout ----------------------------------------
// ys (optional): also store the applied input relu(x * scale + shift) there (2x2 / s2 windows only)
void maxpool_fwd(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, int k, int stride, int pad,
                 at::Tensor y, at::Tensor idx, int OH, int OW, const c10::optional<at::Tensor>& scale,
                 const c10::optional<at::Tensor>& shift, const c10::optional<at::Tensor>& ys, int ldys, int ysoff) {
  same_type(x, y, "maxpool_fwd y");
  same_type(x, ys, "maxpool_fwd ys");
  check(dlmpi_maxpool_fwd(x.data_ptr(), N, H, W, C, ldx, xoff, k, stride, pad, y.data_ptr(), ptr<uint8_t>(idx), OH, OW,
                          optr<float>(scale), optr<float>(shift), ys.has_value() ? ys->data_ptr() : nullptr, ldys,
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
  if (K < 2 || K > 4 || lddl < K || ldw < K) throw std::runtime_error("head_dgrad_bn: 2 <= K <= 4, lddl / ldw >= K");
  const int nblk = fused_producer(M, C, z, mscale, mshift, dx, "head_dgrad_bn");
  same_type(dl, w, "head_dgrad_bn w");
  same_type(dl, z, "head_dgrad_bn z");
  same_type(dl, dx, "head_dgrad_bn dx");
  if (dl.numel() < (M - 1) * lddl + K || w.numel() < (int64_t)(C - 1) * ldw + K || !dl.is_contiguous() ||
      !w.is_contiguous() || !z.is_contiguous() || !dx.is_contiguous())
    throw std::runtime_error("head_dgrad_bn: operand sizes");
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

// --------------------------------- losses / eval -------------------------------------------
void softmax_ce_fwd(const at::Tensor& logits, int ldl, const at::Tensor& labels, int N, int K, at::Tensor loss_rows,
                    at::Tensor lse, at::Tensor loss) {
  check(dlmpi_softmax_ce_fwd(ptr<float>(logits), ldl, ptr<int64_t>(labels), N, K, ptr<float>(loss_rows),
                             ptr<float>(lse), cur_stream()),
        "softmax_ce_fwd");
  check(dlmpi_sum_f32(ptr<float>(loss_rows), N, ptr<float>(loss), 1.f / (float)N, cur_stream()), "sum");
}
void softmax_ce_bwd(const at::Tensor& logits, int ldl, const at::Tensor& labels, const at::Tensor& lse, int N, int K,
                    int ldd, const c10::optional<at::Tensor>& go, double scale, at::Tensor dlogits) {
  check(dlmpi_softmax_ce_bwd(ptr<float>(logits), ldl, ptr<int64_t>(labels), ptr<float>(lse), N, K, ldd,
                             optr<float>(go), (float)scale, ptr<float>(dlogits), cur_stream()),
        "softmax_ce_bwd");
}
void bce_fwd(const at::Tensor& logits, int ldl, const at::Tensor& target, int64_t M, at::Tensor loss) {
  int nblk = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (M + 4095) / 4096));
  at::Tensor partial = at::empty({nblk}, logits.options().dtype(at::kFloat));
  check(dlmpi_bce_fwd(ptr<float>(logits), ldl, ptr<float>(target), M, ptr<float>(partial), nblk, cur_stream()),
        "bce_fwd");
  check(dlmpi_sum_f32(ptr<float>(partial), nblk, ptr<float>(loss), 1.f / (float)M, cur_stream()), "sum");
}
void bce_bwd(const at::Tensor& logits, int ldl, const at::Tensor& target, int64_t M,
             const c10::optional<at::Tensor>& go, double scale, at::Tensor dlogits) {
  check(dlmpi_bce_bwd(ptr<float>(logits), ldl, ptr<float>(target), M, optr<float>(go), (float)scale,
                      ptr<float>(dlogits), cur_stream()),
        "bce_bwd");
}
void argmax_correct(const at::Tensor& logits, int ldl, const at::Tensor& labels, int N, int K, at::Tensor correct) {
  check(dlmpi_argmax_correct(ptr<float>(logits), ldl, ptr<int64_t>(labels), N, K, ptr<int>(correct), cur_stream()),
        "argmax_correct");
}
void dice(const at::Tensor& logits, int ldl, const at::Tensor& target, int N, int64_t HW, at::Tensor out) {
  check(dlmpi_dice(ptr<float>(logits), ldl, ptr<float>(target), N, HW, ptr<float>(out), cur_stream()), "dice");
}

// Pixel-wise losses / counts (pixel_ce.hip, seg_dice.hip): t is addressed as n*sn + k*sk + p*sp over N x K x HW; every
// address must lie inside its storage, the labels are int64 [N*HW].
static void pix_check(const at::Tensor& t, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                      const at::Tensor& labels, const char* what) {
  require_gpu(t, what);
  if (t.scalar_type() != at::kFloat || N < 1 || K < 2 || K > 256 || HW < 1 || sn < 0 || sk < 0 || sp < 0)
    throw std::runtime_error(std::string(what) + ": fp32 logits, 2 <= K <= 256, non-negative strides");
  const int64_t last = (N - 1) * sn + (K - 1) * sk + (HW - 1) * sp;
  const int64_t avail = (int64_t)(t.storage().nbytes() / sizeof(float)) - t.storage_offset();
  if (last >= avail) throw std::runtime_error(std::string(what) + ": strides reach outside the tensor's storage");
  if (labels.scalar_type() != at::kLong || !labels.is_contiguous() || labels.numel() != (int64_t)N * HW ||
      !labels.is_cuda())
    throw std::runtime_error(std::string(what) + ": labels must be contiguous int64 [N*HW] on the GPU");
}
static void f32_numel(const at::Tensor& t, int64_t n, const char* what) {
  if (t.scalar_type() != at::kFloat || !t.is_contiguous() || t.numel() != n || !t.is_cuda())
    throw std::runtime_error(std::string(what) + ": contiguous fp32 GPU tensor of " + std::to_string(n) + " elements");
}
// Classification cross-entropy with weight / ignore_index / label smoothing / mixed targets (cls_ce.hip).
// The argument rules work on integers alone, so they are tested without a GPU (cls_ce_check): absent operands
// have numel -1; dlogits_numel -1 is the forward.  Returns "" or "<fn>: <the rule>".
std::string check_cls_ce_args(const std::string& fn, int64_t N, int64_t K, int64_t ldl, int64_t logits_numel,
                              bool logits_f32, int64_t labels_numel, bool labels_i64, int64_t labels_b_numel,
                              bool labels_b_i64, int64_t lam_numel, bool lam_f32, int64_t weight_numel,
                              bool weight_f32, double eps, int64_t lse_numel, int64_t rows_numel, int64_t den_numel,
                              int64_t dlogits_numel, int64_t go_numel) {
  auto bad = [&](const std::string& why) { return fn + ": " + why; };
  if (N < 1 || N > (1 << 30)) return bad("N must be >= 1 (and below 2^30)");
  if (K < 1 || K > (1 << 30)) return bad("K must be >= 1 (and below 2^30)");
  if (!logits_f32) return bad("logits must be fp32");
  if (ldl < K || ldl > (1 << 30)) return bad("the row stride of the logits must be >= K");
  if (logits_numel < (N - 1) * ldl + K) return bad("logits shorter than N rows of K");
  if (!labels_i64 || (labels_b_numel >= 0 && !labels_b_i64)) return bad("labels must be int64");
  if (labels_numel != N) return bad("labels must have N elements");
  if ((labels_b_numel >= 0) != (lam_numel >= 0)) return bad("labels_b and lam come together");
  if (labels_b_numel >= 0 && labels_b_numel != N) return bad("labels_b must have N elements");
  if (lam_numel >= 0 && !lam_f32) return bad("lam must be fp32");
  if (lam_numel >= 0 && lam_numel != 1 && lam_numel != N) return bad("lam must have 1 or N elements");
  if (weight_numel >= 0 && !weight_f32) return bad("weight must be fp32");
  if (weight_numel >= 0 && weight_numel != K) return bad("weight must have K elements");
  if (!std::isfinite(eps)) return bad("label_smoothing must be finite");
  if (eps < 0 || eps >= 1) return bad("label_smoothing must lie in [0, 1)");
  if (lse_numel != N) return bad("lse must have N elements");
  if (rows_numel != 3 * N) return bad("rows must have 3 N elements");
  if (den_numel != 1) return bad("den must have 1 element");
  if (dlogits_numel >= 0 && dlogits_numel != N * K) return bad("dlogits must have N K elements");
  if (go_numel >= 0 && go_numel != 1) return bad("go must have 1 element");
  return "";
}
static bool is_f32(const c10::optional<at::Tensor>& t) { return !given(t) || t->scalar_type() == at::kFloat; }
static bool is_i64(const c10::optional<at::Tensor>& t) { return !given(t) || t->scalar_type() == at::kLong; }
static void cls_ce_operands(const char* fn, std::initializer_list<const at::Tensor*> ts,
                            std::initializer_list<const c10::optional<at::Tensor>*> os) {
  auto ok = [&](const at::Tensor& t) {
    if (!t.is_cuda() || !t.is_contiguous())
      throw std::runtime_error(std::string(fn) + ": every operand must be a contiguous GPU tensor");
  };
  for (const at::Tensor* t : ts) ok(*t);
  for (const c10::optional<at::Tensor>* o : os)
    if (given(*o)) ok(**o);
}
void cls_ce_fwd(const at::Tensor& logits, int64_t ldl, const at::Tensor& labels,
                const c10::optional<at::Tensor>& labels_b, const c10::optional<at::Tensor>& lam,
                const c10::optional<at::Tensor>& weight, int64_t N, int64_t K, int64_t ignore_index, double eps,
                at::Tensor lse, at::Tensor rows, at::Tensor loss, at::Tensor den) {
  require_ok(check_cls_ce_args("cls_ce_fwd", N, K, ldl, logits.numel(), is_f32(logits), labels.numel(), is_i64(labels),
                               onumel(labels_b), is_i64(labels_b), onumel(lam), is_f32(lam), onumel(weight),
                               is_f32(weight), eps, lse.numel(), rows.numel(), den.numel(), -1, -1));
  cls_ce_operands("cls_ce_fwd", {&labels, &lse, &rows, &loss, &den}, {&labels_b, &lam, &weight});
  require_gpu(logits, "cls_ce_fwd logits");
  f32_numel(lse, N, "cls_ce_fwd lse");
  f32_numel(rows, 3 * N, "cls_ce_fwd rows");
  f32_numel(loss, 1, "cls_ce_fwd loss");
  f32_numel(den, 1, "cls_ce_fwd den");
  check(dlmpi_cls_ce_fwd(ptr<float>(logits), (int)ldl, ptr<int64_t>(labels), optr<int64_t>(labels_b), optr<float>(lam),
                         given(lam) && lam->numel() > 1 ? 1 : 0, optr<float>(weight), (int)N, (int)K, ignore_index,
                         (float)eps, ptr<float>(lse), ptr<float>(rows), ptr<float>(loss), ptr<float>(den),
                         cur_stream()),
        "cls_ce_fwd");
}
void cls_ce_bwd(const at::Tensor& logits, int64_t ldl, const at::Tensor& labels,
                const c10::optional<at::Tensor>& labels_b, const c10::optional<at::Tensor>& lam,
                const c10::optional<at::Tensor>& weight, int64_t N, int64_t K, int64_t ignore_index, double eps,
                const at::Tensor& lse, const at::Tensor& rows, const at::Tensor& den,
                const c10::optional<at::Tensor>& go, at::Tensor dlogits) {
  require_ok(check_cls_ce_args("cls_ce_bwd", N, K, ldl, logits.numel(), is_f32(logits), labels.numel(), is_i64(labels),
                               onumel(labels_b), is_i64(labels_b), onumel(lam), is_f32(lam), onumel(weight),
                               is_f32(weight), eps, lse.numel(), rows.numel(), den.numel(), dlogits.numel(),
                               onumel(go)));
  cls_ce_operands("cls_ce_bwd", {&labels, &lse, &rows, &den, &dlogits}, {&labels_b, &lam, &weight, &go});
  require_gpu(logits, "cls_ce_bwd logits");
  f32_numel(lse, N, "cls_ce_bwd lse");
  f32_numel(rows, 3 * N, "cls_ce_bwd rows");
  f32_numel(den, 1, "cls_ce_bwd den");
  f32_numel(dlogits, N * K, "cls_ce_bwd dlogits");
  if (given(go)) f32_numel(*go, 1, "cls_ce_bwd go");
  check(dlmpi_cls_ce_bwd(ptr<float>(logits), (int)ldl, ptr<int64_t>(labels), optr<int64_t>(labels_b), optr<float>(lam),
                         given(lam) && lam->numel() > 1 ? 1 : 0, optr<float>(weight), (int)N, (int)K, ignore_index,
                         (float)eps, ptr<float>(lse), ptr<float>(rows), ptr<float>(den), optr<float>(go),
                         ptr<float>(dlogits), cur_stream()),
        "cls_ce_bwd");
}

// The preambles of the four pixel-loss binders (fn: the binder's name, kept in the error texts).  tab: the fused
// loss's Dice table [N][K][2], null for the cross-entropy alone; loss: null when the backward's preamble calls.
static void pix_fwd_check(const std::string& fn, const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N,
                          int K, int64_t HW, const at::Tensor& labels, const c10::optional<at::Tensor>& weight,
                          const at::Tensor& lse, const at::Tensor& den, const at::Tensor* tab, const at::Tensor* loss) {
  pix_check(logits, sn, sk, sp, N, K, HW, labels, fn.c_str());
  if (weight && weight->defined() &&
      (weight->scalar_type() != at::kFloat || !weight->is_contiguous() || weight->numel() != K || !weight->is_cuda()))
    throw std::runtime_error(fn + ": weight must be contiguous fp32 [K] on the GPU");
  f32_numel(lse, (int64_t)N * HW, (fn + " lse").c_str());
  f32_numel(den, 1, (fn + " den").c_str());
  if (tab) f32_numel(*tab, (int64_t)N * K * 2, (fn + " tab").c_str());
  if (loss) f32_numel(*loss, 1, (fn + " loss").c_str());
}
static void pix_bwd_check(const std::string& fn, const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N,
                          int K, int64_t HW, const at::Tensor& labels, const c10::optional<at::Tensor>& weight,
                          const at::Tensor& lse, const at::Tensor& den, const at::Tensor* tab,
                          const at::Tensor& dlogits, const c10::optional<at::Tensor>& go) {
  pix_fwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, tab, nullptr);
  pix_check(dlogits, sn, sk, sp, N, K, HW, labels, (fn + " dlogits").c_str());
  if (go && go->defined()) f32_numel(*go, 1, (fn + " go").c_str());
}

void pixel_ce_fwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                  const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                  at::Tensor lse, at::Tensor loss, at::Tensor den) {
  pix_fwd_check("pixel_ce_fwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, nullptr, &loss);
  at::Tensor partial = at::empty({dlmpi_pixel_ce_blocks((int64_t)N * HW), 2}, logits.options());
  check(dlmpi_pixel_ce_fwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                           optr<float>(weight), ptr<float>(lse), ptr<float>(partial), ptr<float>(loss),
                           ptr<float>(den), cur_stream()),
        "pixel_ce_fwd");
}
void pixel_ce_bwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                  const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                  const at::Tensor& lse, const c10::optional<at::Tensor>& go, const at::Tensor& den,
                  at::Tensor dlogits) {
  pix_bwd_check("pixel_ce_bwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, nullptr, dlogits, go);
  check(dlmpi_pixel_ce_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                           optr<float>(weight), ptr<float>(lse), optr<float>(go), ptr<float>(den),
                           ptr<float>(dlogits), cur_stream()),
        "pixel_ce_bwd");
}
void seg_counts(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                const at::Tensor& labels, int64_t ignore_index, at::Tensor counts) {
  pix_check(logits, sn, sk, sp, N, K, HW, labels, "seg_counts");
  if (counts.scalar_type() != at::kLong || !counts.is_contiguous() || counts.numel() != (int64_t)N * K * 3 ||
      !counts.is_cuda())
    throw std::runtime_error("seg_counts: counts must be contiguous int64 [N][K][3] on the GPU");
  check(dlmpi_seg_counts(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                         ptr<int64_t>(counts), cur_stream()),
        "seg_counts");
}
// Soft Dice fused into the pixel CE / BCE passes (seg_dice.hip).  The weights are checked here, host-side:
// finite, >= 0, not both 0, smooth > 0; the partial buffers are allocated here as pixel_ce_fwd's.
static void dice_weight_check(double a, double b, double smooth, const char* what) {
  if (!std::isfinite(a) || !std::isfinite(b) || a < 0 || b < 0 || (a == 0 && b == 0))
    throw std::runtime_error(std::string(what) + ": the two loss weights must be finite, >= 0 and not both 0");
  if (!std::isfinite(smooth) || !(smooth > 0)) throw std::runtime_error(std::string(what) + ": smooth must be > 0");
}
void pixel_ce_dice_fwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                       const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                       double ce_weight, double dice_weight, double smooth, bool include_background, at::Tensor lse,
                       at::Tensor loss, at::Tensor den, at::Tensor tab) {
  pix_fwd_check("pixel_ce_dice_fwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, &tab, &loss);
  dice_weight_check(ce_weight, dice_weight, smooth, "pixel_ce_dice_fwd");
  const int64_t gx = dlmpi_seg_dice_blocks(HW, N);
  at::Tensor part_ce = at::empty({N, gx, 2}, logits.options());
  at::Tensor part_d = at::empty({N, gx, K, 3}, logits.options());
  check(dlmpi_pixel_ce_dice_fwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                optr<float>(weight), (float)ce_weight, (float)dice_weight, (float)smooth,
                                include_background ? 1 : 0, ptr<float>(lse), ptr<float>(part_ce), ptr<float>(part_d),
                                ptr<float>(loss), ptr<float>(den), ptr<float>(tab), cur_stream()),
        "pixel_ce_dice_fwd");
}
void pixel_ce_dice_bwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                       const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                       const at::Tensor& lse, const c10::optional<at::Tensor>& go, const at::Tensor& den,
                       const at::Tensor& tab, double ce_weight, at::Tensor dlogits) {
  pix_bwd_check("pixel_ce_dice_bwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, &tab, dlogits, go);
  if (!std::isfinite(ce_weight) || ce_weight < 0) throw std::runtime_error("pixel_ce_dice_bwd: ce_weight");
  check(dlmpi_pixel_ce_dice_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                optr<float>(weight), ptr<float>(lse), optr<float>(go), ptr<float>(den),
                                ptr<float>(tab), (float)ce_weight, ptr<float>(dlogits), cur_stream()),
        "pixel_ce_dice_bwd");
}
// logits, target: contiguous fp32 [N][HW]
void bce_dice_fwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW, double bce_weight,
                  double dice_weight, double smooth, at::Tensor loss, at::Tensor tab) {
  if (N < 1 || HW < 1) throw std::runtime_error("bce_dice_fwd: N, HW >= 1");
  f32_numel(logits, (int64_t)N * HW, "bce_dice_fwd logits");
  f32_numel(target, (int64_t)N * HW, "bce_dice_fwd target");
  dice_weight_check(bce_weight, dice_weight, smooth, "bce_dice_fwd");
  f32_numel(loss, 1, "bce_dice_fwd loss");
  f32_numel(tab, (int64_t)N * 2, "bce_dice_fwd tab");
  at::Tensor part = at::empty({N, (int64_t)dlmpi_seg_dice_blocks(HW, N), 4}, logits.options());
  check(dlmpi_bce_dice_fwd(ptr<float>(logits), ptr<float>(target), N, HW, (float)bce_weight, (float)dice_weight,
                           (float)smooth, ptr<float>(part), ptr<float>(loss), ptr<float>(tab), cur_stream()),
        "bce_dice_fwd");
}
void bce_dice_bwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW,
                  const c10::optional<at::Tensor>& go, const at::Tensor& tab, double bce_weight, at::Tensor dlogits) {
  if (N < 1 || HW < 1) throw std::runtime_error("bce_dice_bwd: N, HW >= 1");
  f32_numel(logits, (int64_t)N * HW, "bce_dice_bwd logits");
  f32_numel(target, (int64_t)N * HW, "bce_dice_bwd target");
  f32_numel(dlogits, (int64_t)N * HW, "bce_dice_bwd dlogits");
  f32_numel(tab, (int64_t)N * 2, "bce_dice_bwd tab");
  if (!std::isfinite(bce_weight) || bce_weight < 0) throw std::runtime_error("bce_dice_bwd: bce_weight");
  if (go && go->defined()) f32_numel(*go, 1, "bce_dice_bwd go");
  check(dlmpi_bce_dice_bwd(ptr<float>(logits), ptr<float>(target), N, HW, optr<float>(go), ptr<float>(tab),
                           (float)bce_weight, ptr<float>(dlogits), cur_stream()),
        "bce_dice_bwd");
}
// channels-last loss gradient x [M][K] fp32 -> y [M][Kp] activations, zero-padded
void nhwc_pad_cast(const at::Tensor& x, int64_t M, int K, int Kp, at::Tensor y) {
  f32_numel(x, M * K, "nhwc_pad_cast x");
  require_gpu(y, "y");
  if (!y.is_contiguous() || y.numel() != M * Kp) throw std::runtime_error("nhwc_pad_cast: y must be contiguous [M][Kp]");
  check(dlmpi_nhwc_pad_cast(ptr<float>(x), M, K, Kp, y.data_ptr(), act_f32(y, "nhwc_pad_cast"), cur_stream()),
        "nhwc_pad_cast");
}

// --------------------------------- optimizers ----------------------------------------------
void sgd_step(at::Tensor p, const at::Tensor& g, at::Tensor m, double lr, double momentum, double dampening,
              double wd, bool nesterov, bool first, const c10::optional<at::Tensor>& skip_flag) {
  check(dlmpi_sgd(ptr<float>(p), ptr<float>(g), ptr<float>(m), p.numel(), (float)lr, (float)momentum,
                  (float)dampening, (float)wd, nesterov ? 1 : 0, first ? 1 : 0, optr<float>(skip_flag), cur_stream()),
        "sgd");
}
void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, double lr, double b1, double b2,
               double eps, double wd, bool adamw, double bc1, double bc2, const c10::optional<at::Tensor>& clip,
               const c10::optional<at::Tensor>& tstep, bool clip_writeback) {
  check(dlmpi_adam(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<float>(v), p.numel(), (float)lr, (float)b1,
                   (float)b2, (float)eps, (float)wd, adamw ? 1 : 0, (float)bc1, (float)bc2, optr<float>(clip),
                   optr<float>(tstep), clip_writeback ? 1 : 0, cur_stream()),   // tstep advanced in place unless skipped
        "adam");
}
// total L2 norm of a flat fp32 buffer -> norm_out[0]; coef_out = {min(1, max_norm/(norm+1e-6)), nonfinite}
void grad_norm(const at::Tensor& g, double max_norm, at::Tensor norm_out, at::Tensor coef_out) {
  const int nblk = 1024;
  at::Tensor partial = at::empty({nblk}, g.options().dtype(at::kFloat));
  check(dlmpi_sumsq(ptr<float>(g), g.numel(), ptr<float>(partial), nblk, cur_stream()), "sumsq");
  if (coef_out.numel() < 2) throw std::runtime_error("grad_norm: coef_out needs 2 (or 4) floats");
  check(dlmpi_clip_coef(ptr<float>(partial), nblk, (float)max_norm, ptr<float>(norm_out), ptr<float>(coef_out),
                        (int)std::min<int64_t>(4, coef_out.numel()), cur_stream()),
        "clip_coef");
}
void scale_(at::Tensor x, const at::Tensor& coef) {
  check(dlmpi_scale_f32(ptr<float>(x), x.numel(), ptr<float>(coef), cur_stream()), "scale");
}

// ---- layer-wise optimizers: segment / chunk tables of ParamArena.segments() (dlmpi_kernels.h) ----
struct LwTables {
  int nchunks, T;
};
static void i32_gpu(const at::Tensor& t, int64_t n, const char* what) {
  if (t.scalar_type() != at::kInt || !t.is_contiguous() || t.numel() != n || !t.is_cuda())
    throw std::runtime_error(std::string(what) + ": contiguous int32 GPU tensor of " + std::to_string(n) + " elements");
}
// extent = the largest start + length of the chunk table (known to the host that built it)
static LwTables lw_tables(const at::Tensor& chunks, const at::Tensor& flags, int64_t extent, int64_t n,
                          const char* what) {
  if (chunks.dim() != 2 || chunks.size(1) != 4) throw std::runtime_error(std::string(what) + ": chunks must be [n][4]");
  if (chunks.size(0) > (1 << 30)) throw std::runtime_error(std::string(what) + ": too many chunks");
  i32_gpu(chunks, chunks.numel(), what);
  if (flags.numel() < 1 || flags.numel() > (1 << 24)) throw std::runtime_error(std::string(what) + ": flags [T]");
  i32_gpu(flags, flags.numel(), what);
  if (extent < 0 || extent > n) throw std::runtime_error(std::string(what) + ": the chunk table exceeds the buffers");
  return {(int)chunks.size(0), (int)flags.numel()};
}
void seg_sumsq(const at::Tensor& a, const at::Tensor& b, const at::Tensor& chunks, const at::Tensor& flags,
               int64_t extent, at::Tensor partial) {
  const int64_t n = a.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "seg_sumsq");
  f32_numel(a, n, "seg_sumsq a");
  f32_numel(b, n, "seg_sumsq b");
  f32_numel(partial, 2 * (int64_t)t.nchunks, "seg_sumsq partial");
  check(dlmpi_seg_sumsq(ptr<float>(a), ptr<float>(b), ptr<int>(chunks), t.nchunks, n, t.T, ptr<float>(partial),
                        cur_stream()),
        "seg_sumsq");
}
void seg_finish(const at::Tensor& partial, const at::Tensor& chunk_first, const at::Tensor& flags, at::Tensor tab,
                at::Tensor step, const c10::optional<at::Tensor>& skip, int mode, double tc, double wd, double eps,
                double b1, double b2, int kind, double base_lr, double warmup, double total, double min_lr,
                double power) {
  const int64_t T = flags.numel();
  if (T < 1 || T > (1 << 24) || partial.numel() % 2) throw std::runtime_error("seg_finish: table sizes");
  const int64_t nchunks = partial.numel() / 2;
  f32_numel(partial, 2 * nchunks, "seg_finish partial");
  i32_gpu(chunk_first, T + 1, "seg_finish chunk_first");
  i32_gpu(flags, T, "seg_finish flags");
  f32_numel(tab, dlmpi_lw_tab() + T, "seg_finish tab");
  f32_numel(step, 1, "seg_finish step");
  if (skip && skip->defined()) f32_numel(*skip, 1, "seg_finish skip");
  if (mode < 0 || mode > 2 || kind < 0 || kind > 2) throw std::runtime_error("seg_finish: mode / kind");
  check(dlmpi_seg_finish(ptr<float>(partial), (int)nchunks, ptr<int>(chunk_first), ptr<int>(flags), (int)T,
                         ptr<float>(tab), ptr<float>(step), optr<float>(skip), mode, (float)tc, (float)wd, (float)eps,
                         b1, b2, kind, (float)base_lr, (float)warmup, (float)total, (float)min_lr,
                         (float)power, cur_stream()),
        "seg_finish");
}
void lars_update(at::Tensor p, const at::Tensor& g, at::Tensor m, const at::Tensor& chunks, const at::Tensor& flags,
                 int64_t extent, const at::Tensor& tab, double momentum, double wd, bool nesterov) {
  const int64_t n = p.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "lars_update");
  f32_numel(p, n, "lars_update p");
  f32_numel(g, n, "lars_update g");
  f32_numel(m, n, "lars_update m");
  f32_numel(tab, dlmpi_lw_tab() + t.T, "lars_update tab");
  check(dlmpi_lars_update(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<int>(chunks), t.nchunks, n, ptr<int>(flags),
                          t.T, ptr<float>(tab), (float)momentum, (float)wd, nesterov ? 1 : 0, cur_stream()),
        "lars_update");
}
void lamb_moments(const at::Tensor& p, const at::Tensor& g, at::Tensor m, at::Tensor v, const at::Tensor& chunks,
                  const at::Tensor& flags, int64_t extent, at::Tensor partial, const at::Tensor& tab,
                  const c10::optional<at::Tensor>& clip, double b1, double b2, double eps, double wd) {
  const int64_t n = p.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "lamb_moments");
  f32_numel(p, n, "lamb_moments p");
  f32_numel(g, n, "lamb_moments g");
  f32_numel(m, n, "lamb_moments m");
  f32_numel(v, n, "lamb_moments v");
  f32_numel(partial, 2 * (int64_t)t.nchunks, "lamb_moments partial");
  f32_numel(tab, dlmpi_lw_tab() + t.T, "lamb_moments tab");
  if (clip && clip->defined()) f32_numel(*clip, 2, "lamb_moments clip");
  if (!(eps > 0)) throw std::runtime_error("lamb_moments: eps > 0");
  check(dlmpi_lamb_moments(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<float>(v), ptr<int>(chunks), t.nchunks, n,
                           ptr<int>(flags), t.T, ptr<float>(partial), ptr<float>(tab), optr<float>(clip), b1, b2,
                           (float)eps, (float)wd, cur_stream()),
        "lamb_moments");
}
void lamb_update(at::Tensor p, const at::Tensor& m, const at::Tensor& v, const at::Tensor& chunks,
                 const at::Tensor& flags, int64_t extent, const at::Tensor& tab, double eps, double wd) {
  const int64_t n = p.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "lamb_update");
  f32_numel(p, n, "lamb_update p");
  f32_numel(m, n, "lamb_update m");
  f32_numel(v, n, "lamb_update v");
  f32_numel(tab, dlmpi_lw_tab() + t.T, "lamb_update tab");
  if (!(eps > 0)) throw std::runtime_error("lamb_update: eps > 0");
  check(dlmpi_lamb_update(ptr<float>(p), ptr<float>(m), ptr<float>(v), ptr<int>(chunks), t.nchunks, n, ptr<int>(flags),
                          t.T, ptr<float>(tab), (float)eps, (float)wd, cur_stream()),
        "lamb_update");
}

// --------------------------------- utilities -----------------------------------------------
void fill_(at::Tensor t, double v) {
  if (t.scalar_type() != at::kFloat || !t.is_contiguous()) throw std::runtime_error("fill_: contiguous fp32 tensor");
  check(dlmpi_fill_f32(ptr<float>(t), t.numel(), (float)v, cur_stream()), "fill");
}
// t: int64 [blocks][4] on the device (bench.py clock stamps)
void clock_stamp(at::Tensor t) {
  if (t.scalar_type() != at::kLong || !t.is_contiguous() || t.dim() != 2 || t.size(1) != 4)
    throw std::runtime_error("clock_stamp: contiguous int64 [blocks][4]");
  check(dlmpi_clock_stamp(reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()), (int)t.size(0), cur_stream()),
        "clock_stamp");
}
void add_i64_(at::Tensor t, int64_t v) {
  if (t.scalar_type() != at::kLong || !t.is_contiguous()) throw std::runtime_error("add_i64_: contiguous int64 tensor");
  check(dlmpi_add_i64(ptr<int64_t>(t), t.numel(), v, cur_stream()), "add_i64");
}
// dst.view(-1)[i] (+)= src.view(-1)[idx[i]]  (idx < 0: 0), every i < idx.numel()
void gather_(at::Tensor dst, const at::Tensor& src, const at::Tensor& idx, bool accumulate) {
  if (dst.scalar_type() != src.scalar_type() || !dst.is_contiguous() || !src.is_contiguous() ||
      idx.scalar_type() != at::kLong || !idx.is_contiguous() || idx.numel() > dst.numel())
    throw std::runtime_error("gather_: contiguous dst/src of one dtype, int64 idx no longer than dst");
  check(dlmpi_gather(dst.data_ptr(), src.data_ptr(), ptr<int64_t>(idx), idx.numel(), (int)dst.element_size(),
                     accumulate ? 1 : 0, cur_stream()),
        "gather");
}

// --------------------------------- device-resident input pipeline ---------------------------
void image_batch(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, int H, int W, int C,
                 int pad, bool augment, int64_t seed, int64_t epoch, std::vector<double> mean, std::vector<double> sd,
                 at::Tensor out, const c10::optional<at::Tensor>& out_labels) {
  require_gpu(data, "data");
  if (mean.size() != (size_t)C || sd.size() != (size_t)C) throw std::runtime_error("image_batch: mean/std per channel");
  if (data.scalar_type() != at::kByte || idx.scalar_type() != at::kLong || out.scalar_type() != at::kFloat)
    throw std::runtime_error("image_batch: uint8 data, int64 indices, fp32 output");
  float m3[3] = {0.f, 0.f, 0.f}, s3[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m3[c] = (float)mean[c]; s3[c] = (float)sd[c]; }
  const int B = (int)idx.numel();
  if (out.numel() != (int64_t)B * C * H * W) throw std::runtime_error("image_batch: output size");
  check(dlmpi_image_batch(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), B, H, W, C, pad, augment ? 1 : 0,
                          (uint32_t)seed, (uint32_t)epoch, m3, s3, ptr<float>(out), optr<int64_t>(out_labels),
                          cur_stream()),
        "image_batch");
}

// The mixed batch of the device-resident pipeline and the in-place mix of any fp32 NCHW batch (data.hip); kind
// 0 none / 1 mixup / 2 CutMix with the box rows [y0, y1) x columns [x0, x1) inside the image.
static void batch_labels_ok(const char* fn, const char* name, const at::Tensor& t, int B) {
  if (t.scalar_type() != at::kLong || !t.is_contiguous() || t.numel() != B || !t.is_cuda())
    throw std::runtime_error(std::string(fn) + ": " + name + " must be contiguous int64 [B] on the GPU");
}
static void mix_args_ok(const char* fn, int kind, double lam, int H, int W, int y0, int y1, int x0, int x1,
                        const at::Tensor& labels_a, const at::Tensor& labels_b, const at::Tensor& lam_out, int B) {
  if (kind < 0 || kind > 2) throw std::runtime_error(std::string(fn) + ": kind must be 0, 1 or 2");
  if (!(lam >= 0 && lam <= 1)) throw std::runtime_error(std::string(fn) + ": lam must lie in [0, 1]");
  if (y0 < 0 || y1 < y0 || y1 > H || x0 < 0 || x1 < x0 || x1 > W)
    throw std::runtime_error(std::string(fn) + ": the box must lie inside the image");
  batch_labels_ok(fn, "labels", labels_a, B);
  batch_labels_ok(fn, "labels_b", labels_b, B);
  f32_numel(lam_out, 1, (std::string(fn) + " lam").c_str());
}
void image_batch_mix(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, int H, int W, int C,
                     int pad, bool augment, int64_t seed, int64_t epoch, std::vector<double> mean,
                     std::vector<double> sd, int kind, double lam, int y0, int y1, int x0, int x1, at::Tensor out,
                     at::Tensor out_labels, at::Tensor labels_b, at::Tensor lam_out) {
  require_gpu(data, "data");
  if (mean.size() != (size_t)C || sd.size() != (size_t)C || C < 1 || C > 3)
    throw std::runtime_error("image_batch_mix: mean/std per channel, 1..3 channels");
  if (data.scalar_type() != at::kByte || idx.scalar_type() != at::kLong || out.scalar_type() != at::kFloat ||
      labels.scalar_type() != at::kLong)
    throw std::runtime_error("image_batch_mix: uint8 data, int64 labels and indices, fp32 output");
  float m3[3] = {0.f, 0.f, 0.f}, s3[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m3[c] = (float)mean[c]; s3[c] = (float)sd[c]; }
  const int B = (int)idx.numel();
  if (B < 1 || H < 1 || W < 1) throw std::runtime_error("image_batch_mix: empty batch");
  if (!idx.is_contiguous() || !idx.is_cuda() || !out.is_contiguous() || !out.is_cuda() ||
      out.numel() != (int64_t)B * C * H * W)
    throw std::runtime_error("image_batch_mix: contiguous GPU indices and a contiguous fp32 [B, C, H, W] GPU output");
  mix_args_ok("image_batch_mix", kind, lam, H, W, y0, y1, x0, x1, out_labels, labels_b, lam_out, B);
  check(dlmpi_image_batch_mix(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), B, H, W, C, pad,
                              augment ? 1 : 0, (uint32_t)seed, (uint32_t)epoch, m3, s3, kind, (float)lam, y0, y1, x0,
                              x1, ptr<float>(out), ptr<int64_t>(out_labels), ptr<int64_t>(labels_b),
                              ptr<float>(lam_out), cur_stream()),
        "image_batch_mix");
}
void mix_batch_(at::Tensor x, const at::Tensor& labels, int kind, double lam, int y0, int y1, int x0, int x1,
                at::Tensor labels_b, at::Tensor lam_out) {
  if (x.dim() != 4 || x.scalar_type() != at::kFloat || !x.is_contiguous() || !x.is_cuda() || x.numel() < 1)
    throw std::runtime_error("mix_batch_: x must be a contiguous fp32 [B, C, H, W] GPU tensor");
  const int B = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  mix_args_ok("mix_batch_", kind, lam, H, W, y0, y1, x0, x1, labels, labels_b, lam_out, B);
  check(dlmpi_mix_batch(ptr<float>(x), ptr<int64_t>(labels), B, C, H, W, kind, (float)lam, y0, y1, x0, x1,
                        ptr<int64_t>(labels_b), ptr<float>(lam_out), cur_stream()),
        "mix_batch_");
}

// Segmentation augmentation (seg_aug.hip): images fp32 [N, C, H, W] and masks [N, H, W] (float32 | int64) gathered
// by idx [B] and resampled through rows idx[b] of table (int32 [N, 6], Q16) into out [B, C, Ho, Wo] and out_mask
// [B, Ho, Wo].  idx values are trusted.
static void seg_arg_ok(const char* name, const at::Tensor& t, at::ScalarType type, const char* tname,
                       std::vector<int64_t> shape) {
  std::string want;
  for (size_t i = 0; i < shape.size(); ++i) want += (i ? ", " : "") + std::to_string(shape[i]);
  if (!t.is_cuda() || t.scalar_type() != type || !t.is_contiguous() || t.sizes().vec() != shape)
    throw std::runtime_error(std::string("seg_aug_batch: ") + name + " must be a contiguous " + tname + " [" + want +
                             "] GPU tensor");
}
void seg_aug_batch(const at::Tensor& images, const at::Tensor& masks, const at::Tensor& idx, const at::Tensor& table,
                   double image_fill, double mask_fill, at::Tensor out, at::Tensor out_mask) {
  if (!images.is_cuda() || images.scalar_type() != at::kFloat || !images.is_contiguous() || images.dim() != 4 ||
      images.numel() < 1)
    throw std::runtime_error("seg_aug_batch: images must be a contiguous fp32 [N, C, H, W] GPU tensor");
  const int64_t N = images.size(0), C = images.size(1), H = images.size(2), W = images.size(3);
  const bool i64 = masks.scalar_type() == at::kLong;
  if (!i64 && masks.scalar_type() != at::kFloat)
    throw std::runtime_error("seg_aug_batch: masks must be float32 or int64");
  const at::ScalarType mt = i64 ? at::kLong : at::kFloat;
  const char* mname = i64 ? "int64" : "fp32";
  seg_arg_ok("masks", masks, mt, mname, {N, H, W});
  if (!idx.is_cuda() || idx.scalar_type() != at::kLong || !idx.is_contiguous() || idx.dim() != 1 || idx.numel() < 1)
    throw std::runtime_error("seg_aug_batch: idx must be a contiguous int64 [B] GPU tensor, B >= 1");
  seg_arg_ok("table", table, at::kInt, "int32", {N, 6});
  if (out.dim() != 4 || out.numel() < 1)
    throw std::runtime_error("seg_aug_batch: out must be a contiguous fp32 [B, C, Ho, Wo] GPU tensor");
  const int64_t B = idx.numel(), Ho = out.size(2), Wo = out.size(3);
  seg_arg_ok("out", out, at::kFloat, "fp32", {B, C, Ho, Wo});
  seg_arg_ok("out_mask", out_mask, mt, mname, {B, Ho, Wo});
  if (H * W > INT32_MAX || out_mask.numel() > INT32_MAX || C > INT32_MAX)
    throw std::runtime_error("seg_aug_batch: an images plane and out_mask hold at most 2^31 - 1 pixels");
  if (!std::isfinite(image_fill) || !std::isfinite(mask_fill))
    throw std::runtime_error("seg_aug_batch: image_fill and mask_fill must be finite");
  check(dlmpi_seg_aug_batch(ptr<float>(images), masks.data_ptr(), i64 ? 1 : 0, ptr<int64_t>(idx), ptr<int>(table),
                            (int)B, (int)C, (int)H, (int)W, (int)Ho, (int)Wo, (float)image_fill, (float)mask_fill,
                            (int64_t)std::llround(mask_fill), ptr<float>(out), out_mask.data_ptr(), cur_stream()),
        "seg_aug_batch");
}

// RandomResizedCrop batch (rrc.hip): data uint8 [N, H, W, C] gathered by idx [B], cropped to rows idx[b] of table
// (int32 [N, 5]: top, left, h, w, flip), resized to out [B, C, Ho, Wo], flipped and normalised; labels gathered into
// out_labels.  idx values are trusted.  The kernel reads whatever box the table names, so the WHOLE table is checked
// here -- on the host, the one call of this file that synchronises -- the first time it is seen, once per epoch:
// the checked tables are remembered by storage, version counter and geometry, and held so that their memory
// cannot be handed to another tensor meanwhile.
namespace {
struct CheckedTable {
  at::Tensor table;
  const void* ptr;
  uint32_t version;
  int64_t H, W, Ho, Wo;
};
[[noreturn]] void rrc_fail(const std::string& why) { throw std::runtime_error("image_rrc_batch: " + why); }

void rrc_table_ok(const at::Tensor& table, int64_t H, int64_t W, int64_t Ho, int64_t Wo) {
  static std::vector<CheckedTable>* seen = new std::vector<CheckedTable>();   // (never destroyed: outlives HIP)
  const uint32_t version = table._version();
  for (const CheckedTable& c : *seen)
    if (c.ptr == table.data_ptr() && c.version == version && c.table.is_alias_of(table) &&
        c.table.sizes() == table.sizes() && c.H == H && c.W == W && c.Ho == Ho && c.Wo == Wo)
      return;
  const at::Tensor host = table.cpu();
  const int* t = host.data_ptr<int>();
  const int64_t cap = dlmpi_rrc_max_scale();
  for (int64_t i = 0; i < host.size(0); ++i, t += 5) {
    const int64_t top = t[0], left = t[1], h = t[2], w = t[3];
    const std::string row = "table row " + std::to_string(i) + " (" + std::to_string(top) + ", " +
                            std::to_string(left) + ", " + std::to_string(h) + ", " + std::to_string(w) + ", " +
                            std::to_string(t[4]) + ")";
    if (h < 1 || w < 1) rrc_fail(row + ": h and w must be at least 1");
    if (top < 0 || left < 0 || top + h > H || left + w > W)
      rrc_fail(row + ": the box does not lie inside the " + std::to_string(H) + " x " + std::to_string(W) + " image");
    if (t[4] != 0 && t[4] != 1) rrc_fail(row + ": flip must be 0 or 1");
    if (h > cap * Ho || w > cap * Wo)
      rrc_fail(row + ": down-scaled by more than " + std::to_string(cap) + "x to " + std::to_string(Ho) + " x " +
               std::to_string(Wo) + " (the weight table of the kernel holds 32 taps)");
  }
  if (seen->size() >= 4) seen->erase(seen->begin());   // a training and an evaluation table, with room to spare
  seen->push_back({table, table.data_ptr(), version, H, W, Ho, Wo});
}
}  // namespace

void image_rrc_batch(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, const at::Tensor& table,
                     std::vector<double> mean, std::vector<double> sd, at::Tensor out, at::Tensor out_labels) {
  if (!data.is_cuda() || !labels.is_cuda() || !idx.is_cuda() || !table.is_cuda() || !out.is_cuda() ||
      !out_labels.is_cuda())
    rrc_fail("every tensor must be on the GPU");
  if (data.scalar_type() != at::kByte || labels.scalar_type() != at::kLong || idx.scalar_type() != at::kLong ||
      table.scalar_type() != at::kInt || out.scalar_type() != at::kFloat || out_labels.scalar_type() != at::kLong)
    rrc_fail("uint8 data, int64 labels and indices, an int32 table, fp32 output and int64 output labels");
  if (!data.is_contiguous() || !labels.is_contiguous() || !idx.is_contiguous() || !table.is_contiguous() ||
      !out.is_contiguous() || !out_labels.is_contiguous())
    rrc_fail("every tensor must be contiguous");
  if (data.dim() != 4 || data.numel() < 1) rrc_fail("data must be [N, H, W, C]");
  const int64_t N = data.size(0), H = data.size(1), W = data.size(2), C = data.size(3);
  if (C != 1 && C != 3) rrc_fail("C must be 1 or 3, got " + std::to_string(C));
  if (mean.size() != (size_t)C || sd.size() != (size_t)C) rrc_fail("mean/std per channel");
  if (labels.dim() != 1 || labels.size(0) != N) rrc_fail("labels must be [N]");
  if (table.dim() != 2 || table.size(0) != N || table.size(1) != 5) rrc_fail("the table must be [N, 5]");
  const int64_t B = idx.numel();
  if (idx.dim() != 1 || B < 1 || B > 65535) rrc_fail("idx must be [B], 1 <= B <= 65535");
  if (out.dim() != 4 || out.size(0) != B || out.size(1) != C || out.size(2) < 1 || out.size(3) < 1)
    rrc_fail("out must be [B, C, Ho, Wo]");
  if (out_labels.dim() != 1 || out_labels.size(0) != B) rrc_fail("out_labels must be [B]");
  const int64_t Ho = out.size(2), Wo = out.size(3);
  if (H > INT32_MAX / 4 || W > INT32_MAX / 4 || Ho > (1 << 20) || Wo > (1 << 20))
    rrc_fail("image sides past the kernel's index range");
  rrc_table_ok(table, H, W, Ho, Wo);
  float m3[3] = {0.f, 0.f, 0.f}, s3[3] = {1.f, 1.f, 1.f};
  for (int c = 0; c < C; ++c) { m3[c] = (float)mean[c]; s3[c] = (float)sd[c]; }
  check(dlmpi_image_rrc_batch(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), ptr<int>(table), (int)B,
                              (int)H, (int)W, (int)C, (int)Ho, (int)Wo, m3, s3, ptr<float>(out),
                              ptr<int64_t>(out_labels), cur_stream()),
        "image_rrc_batch");
}

void register_ops(pybind11::module& m) {
  namespace py = pybind11;
  register_conv_fwd(m);
  register_conv_bwd(m);
  m.def("bn_finalize", &bn_finalize);
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
  m.def("reduce_blocks", &reduce_blocks);
  m.def("bn_stats", &bn_stats);
  m.def("bn_apply", &bn_apply);
  m.def("bn_bwd_reduce", &bn_bwd_reduce);
  m.def("bn_bwd_finalize", &bn_bwd_finalize);
  m.def("bn_bwd_finalize_fused", &bn_bwd_finalize_fused);
  m.def("bn_bwd_apply", &bn_bwd_apply);
  m.def("dual_dgrad_weights", &dual_dgrad_weights);
  m.def("channel_sum", &channel_sum);
  m.def("maxpool_fwd", &maxpool_fwd, py::arg("x"), py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"),
        py::arg("ldx"), py::arg("xoff"), py::arg("k"), py::arg("stride"), py::arg("pad"), py::arg("y"), py::arg("idx"),
        py::arg("OH"), py::arg("OW"), py::arg("scale"), py::arg("shift"), py::arg("ys") = py::none(),
        py::arg("ldys") = 0, py::arg("ysoff") = 0);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("maxpool_bwd_bn", &maxpool_bwd_bn);
  m.def("outer_dgrad_bn", &outer_dgrad_bn);
  m.def("head_dgrad_bn", &head_dgrad_bn);
  m.def("nhwc_pad_cast", &nhwc_pad_cast);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("nchw_to_nhwc", &nchw_to_nhwc);
  m.def("s2d_nchw", &s2d_nchw);
  m.def("image_batch", &image_batch);
  m.def("upsample2x_fwd", &upsample2x_fwd);
  m.def("upsample2x_bwd", &upsample2x_bwd);
  m.def("cast_weights", &cast_weights);
  m.def("softmax_ce_fwd", &softmax_ce_fwd);
  m.def("softmax_ce_bwd", &softmax_ce_bwd);
  m.def("cls_ce_fwd", &cls_ce_fwd);
  m.def("cls_ce_bwd", &cls_ce_bwd);
  m.def("cls_ce_check", &check_cls_ce_args, py::arg("fn") = "cls_ce_fwd", py::arg("N"), py::arg("K"), py::arg("ldl"),
        py::arg("logits_numel"), py::arg("logits_f32") = true, py::arg("labels_numel"), py::arg("labels_i64") = true,
        py::arg("labels_b_numel") = -1, py::arg("labels_b_i64") = true, py::arg("lam_numel") = -1,
        py::arg("lam_f32") = true, py::arg("weight_numel") = -1, py::arg("weight_f32") = true, py::arg("eps") = 0.0,
        py::arg("lse_numel"), py::arg("rows_numel"), py::arg("den_numel") = 1, py::arg("dlogits_numel") = -1,
        py::arg("go_numel") = -1);
  m.def("image_batch_mix", &image_batch_mix);
  m.def("mix_batch_", &mix_batch_);
  m.def("seg_aug_batch", &seg_aug_batch);
  m.def("image_rrc_batch", &image_rrc_batch);
  m.def("rrc_max_scale", []() { return dlmpi_rrc_max_scale(); });
  m.def("bce_fwd", &bce_fwd);
  m.def("bce_bwd", &bce_bwd);
  m.def("argmax_correct", &argmax_correct);
  m.def("dice", &dice);
  m.def("pixel_ce_fwd", &pixel_ce_fwd);
  m.def("set_pixel_tiles", [](int on) { dlmpi_set_pixel_tiles(on); });
  m.def("pixel_ce_bwd", &pixel_ce_bwd);
  m.def("seg_counts", &seg_counts);
  m.def("pixel_ce_dice_fwd", &pixel_ce_dice_fwd);
  m.def("pixel_ce_dice_bwd", &pixel_ce_dice_bwd);
  m.def("bce_dice_fwd", &bce_dice_fwd);
  m.def("bce_dice_bwd", &bce_dice_bwd);
  m.def("sgd_step", &sgd_step);
  m.def("adam_step", &adam_step);
  m.def("grad_norm", &grad_norm);
  m.def("seg_sumsq", &seg_sumsq);
  m.def("seg_finish", &seg_finish);
  m.def("lars_update", &lars_update);
  m.def("lamb_moments", &lamb_moments);
  m.def("lamb_update", &lamb_update);
  m.def("lw_chunk", []() { return dlmpi_lw_chunk(); });
  m.def("lw_tab", []() { return dlmpi_lw_tab(); });
  m.def("scale_", &scale_);
  m.def("fill_", &fill_);
  m.def("clock_stamp", &clock_stamp);
  m.def("add_i64_", &add_i64_);
  m.def("gather_", &gather_);
  m.attr("CAST_ENTRY_BYTES") = (int)sizeof(CastEntry);
}

}  // namespace dlmpi_ext
