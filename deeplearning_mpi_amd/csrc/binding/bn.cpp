// Torch binding of the BatchNorm family (kernels/bn.hip, bnfin.h): statistics, finalize, apply, the backward reduce /
// finalize / apply, the dual 1x1 data-gradient weights and the channel sum.  Argument checks: a few integer
// compares per call, before anything is launched.  The kernels index by M, C, ld and off alone, so whatever passes
// here stays inside every operand.
#include "common.h"

namespace dlmpi_ext {

// the chunked row reductions (rowreduce.h rowmap): 256 / (C / 8) row lanes per block
void rowmap_shape(int64_t M, int C, const char* what) {
  if (C < 8 || C % 8 || C > 2048) fail(what, "C must be a multiple of 8 in [8, 2048]");
  if (M < 1) fail(what, "M < 1");
}
namespace {
// the elementwise kernels: one thread per 8 channels
void ew_shape(int64_t M, int C, const char* what) {
  if (C < 8 || C % 8) fail(what, "C must be a positive multiple of 8");
  if (M < 1) fail(what, "M < 1");
}
// the column reduce + finalize over partial [T][ns][C]
void colsum_shape(const at::Tensor& partial, int T, int ns, int C, double count, const char* what) {
  if (T < 1 || C < 1) fail(what, "needs at least one partial row and one channel");
  if (!(count >= 1.0)) fail(what, "count < 1");
  floats_ok(partial, (int64_t)T * ns * C, what, "partial");
}

void bn_finalize(const at::Tensor& partial, int ntiles, int C, double count, const c10::optional<at::Tensor>& gamma,
                 const c10::optional<at::Tensor>& beta, const c10::optional<at::Tensor>& running_mean,
                 const c10::optional<at::Tensor>& running_var, double momentum, double eps, at::Tensor scale,
                 at::Tensor shift, const c10::optional<at::Tensor>& save_mean,
                 const c10::optional<at::Tensor>& save_invstd) {
  colsum_shape(partial, ntiles, 2, C, count, "bn_finalize");
  floats_ok(gamma, C, "bn_finalize", "gamma");
  floats_ok(beta, C, "bn_finalize", "beta");
  if (given(running_mean) != given(running_var)) fail("bn_finalize", "running_mean / running_var come together");
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
  if (nblk < 1) fail("bn_stats", "nblk < 1");
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
  if (given(mbits) && mbits->numel() != M * (C / 8)) fail("bn_apply", "mask bits must be [M][C/8]");
  if (given(rscale) != given(rshift) || (given(rscale) && !given(res)))
    fail("bn_apply", "rscale / rshift come together, with a residual");
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
  if (nblk < 1) fail("bn_bwd_reduce", "nblk < 1");
  if (given(x) && !(given(mean) && given(invstd))) fail("bn_bwd_reduce", "x needs mean and invstd");
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
void bwd_fin_vectors(int C, bool raw_z, const c10::optional<at::Tensor>& gamma,
                     const c10::optional<at::Tensor>& mean, const c10::optional<at::Tensor>& invstd,
                     const c10::optional<at::Tensor>& dgamma, const c10::optional<at::Tensor>& dbeta,
                     const c10::optional<at::Tensor>& coef, const char* what) {
  if ((given(coef) || raw_z) && !(given(mean) && given(invstd))) fail(what, "coef needs mean and invstd");
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
  if (partial.dim() != 3) fail("bn_bwd_finalize_fused", "partial must be [tiles][ns][C]");
  const int T = (int)partial.size(0), ns = (int)partial.size(1);
  if (partial.size(2) != C) fail("bn_bwd_finalize_fused", "channel mismatch");
  if (ns < 2 || ns > 3 || k2 < 1 || k2 >= ns) fail("bn_bwd_finalize_fused", "ns in {2, 3} and 1 <= k2 < ns");
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
    fail("dual_dgrad_weights", "shapes / dtypes");
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
}  // namespace

void register_bn(pybind11::module& m) {
  m.def("bn_finalize", &bn_finalize);
  m.def("reduce_blocks", &reduce_blocks);
  m.def("bn_stats", &bn_stats);
  m.def("bn_apply", &bn_apply);
  m.def("bn_bwd_reduce", &bn_bwd_reduce);
  m.def("bn_bwd_finalize", &bn_bwd_finalize);
  m.def("bn_bwd_finalize_fused", &bn_bwd_finalize_fused);
  m.def("bn_bwd_apply", &bn_bwd_apply);
  m.def("dual_dgrad_weights", &dual_dgrad_weights);
  m.def("channel_sum", &channel_sum);
}

}  // namespace dlmpi_ext
