// Torch binding of the losses and evaluation counts (kernels/loss.hip, cls_ce.hip, pixel_ce.hip, seg_dice.hip,
// ohem.hip, lovasz.hip, edt.hip, boundary.hip, surface.hip).
// softmax_ce_*, bce_*, argmax_correct and dice take their shapes from the caller (NativeBackend) unchecked.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace dlmpi_ext {
namespace {

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
void pix_check(const at::Tensor& t, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
               const at::Tensor& labels, const char* fn, const char* name) {
  if (!t.is_cuda()) fail(fn, std::string(name) + " must be a GPU tensor");
  if (t.scalar_type() != at::kFloat || N < 1 || K < 2 || K > 256 || HW < 1 || sn < 0 || sk < 0 || sp < 0)
    fail(fn, std::string(name) + " must be fp32 with N, HW >= 1, 2 <= K <= 256 and non-negative strides");
  const int64_t last = (N - 1) * sn + (K - 1) * sk + (HW - 1) * sp;
  const int64_t avail = (int64_t)(t.storage().nbytes() / sizeof(float)) - t.storage_offset();
  if (last >= avail) fail(fn, std::string(name) + ": strides reach outside the tensor's storage");
  dense(labels, at::kLong, (int64_t)N * HW, fn, "labels");
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
bool is_f32(const c10::optional<at::Tensor>& t) { return !given(t) || t->scalar_type() == at::kFloat; }
bool is_i64(const c10::optional<at::Tensor>& t) { return !given(t) || t->scalar_type() == at::kLong; }
// After the integer rules: the operands forward and backward share, each once for "contiguous, on the GPU, dtype"
// (the logits are rows of ldl, so only their place is checked).
void cls_ce_operands(const char* fn, const at::Tensor& logits, const at::Tensor& labels,
                     const c10::optional<at::Tensor>& labels_b, const c10::optional<at::Tensor>& lam,
                     const c10::optional<at::Tensor>& weight, int64_t N, int64_t K, const at::Tensor& lse,
                     const at::Tensor& rows, const at::Tensor& den) {
  if (!logits.is_cuda()) fail(fn, "logits must be a GPU tensor");
  dense(labels, at::kLong, N, fn, "labels");
  dense(labels_b, at::kLong, N, fn, "labels_b");
  dense(lam, at::kFloat, onumel(lam), fn, "lam");
  dense(weight, at::kFloat, K, fn, "weight");
  dense(lse, at::kFloat, N, fn, "lse");
  dense(rows, at::kFloat, 3 * N, fn, "rows");
  dense(den, at::kFloat, 1, fn, "den");
}
void cls_ce_fwd(const at::Tensor& logits, int64_t ldl, const at::Tensor& labels,
                const c10::optional<at::Tensor>& labels_b, const c10::optional<at::Tensor>& lam,
                const c10::optional<at::Tensor>& weight, int64_t N, int64_t K, int64_t ignore_index, double eps,
                at::Tensor lse, at::Tensor rows, at::Tensor loss, at::Tensor den) {
  require_ok(check_cls_ce_args("cls_ce_fwd", N, K, ldl, logits.numel(), is_f32(logits), labels.numel(), is_i64(labels),
                               onumel(labels_b), is_i64(labels_b), onumel(lam), is_f32(lam), onumel(weight),
                               is_f32(weight), eps, lse.numel(), rows.numel(), den.numel(), -1, -1));
  cls_ce_operands("cls_ce_fwd", logits, labels, labels_b, lam, weight, N, K, lse, rows, den);
  dense(loss, at::kFloat, 1, "cls_ce_fwd", "loss");
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
  cls_ce_operands("cls_ce_bwd", logits, labels, labels_b, lam, weight, N, K, lse, rows, den);
  dense(dlogits, at::kFloat, N * K, "cls_ce_bwd", "dlogits");
  dense(go, at::kFloat, 1, "cls_ce_bwd", "go");
  check(dlmpi_cls_ce_bwd(ptr<float>(logits), (int)ldl, ptr<int64_t>(labels), optr<int64_t>(labels_b), optr<float>(lam),
                         given(lam) && lam->numel() > 1 ? 1 : 0, optr<float>(weight), (int)N, (int)K, ignore_index,
                         (float)eps, ptr<float>(lse), ptr<float>(rows), ptr<float>(den), optr<float>(go),
                         ptr<float>(dlogits), cur_stream()),
        "cls_ce_bwd");
}

// The preambles of the four pixel-loss binders (fn: the binder's name, kept in the error texts).  tab: the fused
// loss's Dice table [N][K][2], null for the cross-entropy alone; loss: null when the backward's preamble calls.
void pix_fwd_check(const char* fn, const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                   int64_t HW, const at::Tensor& labels, const c10::optional<at::Tensor>& weight, const at::Tensor& lse,
                   const at::Tensor& den, const at::Tensor* tab, const at::Tensor* loss) {
  pix_check(logits, sn, sk, sp, N, K, HW, labels, fn, "logits");
  dense(weight, at::kFloat, K, fn, "weight");
  dense(lse, at::kFloat, (int64_t)N * HW, fn, "lse");
  dense(den, at::kFloat, 1, fn, "den");
  if (tab) dense(*tab, at::kFloat, (int64_t)N * K * 2, fn, "tab");
  if (loss) dense(*loss, at::kFloat, 1, fn, "loss");
}
void pix_bwd_check(const char* fn, const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                   int64_t HW, const at::Tensor& labels, const c10::optional<at::Tensor>& weight, const at::Tensor& lse,
                   const at::Tensor& den, const at::Tensor* tab, const at::Tensor& dlogits,
                   const c10::optional<at::Tensor>& go) {
  pix_fwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, tab, nullptr);
  pix_check(dlogits, sn, sk, sp, N, K, HW, labels, fn, "dlogits");
  dense(go, at::kFloat, 1, fn, "go");
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
  pix_check(logits, sn, sk, sp, N, K, HW, labels, "seg_counts", "logits");
  dense(counts, at::kLong, (int64_t)N * K * 3, "seg_counts", "counts");
  check(dlmpi_seg_counts(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                         ptr<int64_t>(counts), cur_stream()),
        "seg_counts");
}
// Soft Dice fused into the pixel CE / BCE passes (seg_dice.hip).  The weights are checked here, host-side:
// finite, >= 0, not both 0, smooth > 0; the partial buffers are allocated here as pixel_ce_fwd's.
void dice_weight_check(double a, double b, double smooth, const char* fn) {
  if (!std::isfinite(a) || !std::isfinite(b) || a < 0 || b < 0 || (a == 0 && b == 0))
    fail(fn, "the two loss weights must be finite, >= 0 and not both 0");
  if (!std::isfinite(smooth) || !(smooth > 0)) fail(fn, "smooth must be > 0");
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
  if (!std::isfinite(ce_weight) || ce_weight < 0) fail("pixel_ce_dice_bwd", "ce_weight must be finite and >= 0");
  check(dlmpi_pixel_ce_dice_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                optr<float>(weight), ptr<float>(lse), optr<float>(go), ptr<float>(den),
                                ptr<float>(tab), (float)ce_weight, ptr<float>(dlogits), cur_stream()),
        "pixel_ce_dice_bwd");
}
// logits, target: contiguous fp32 [N][HW]
void bce_dice_fwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW, double bce_weight,
                  double dice_weight, double smooth, at::Tensor loss, at::Tensor tab) {
  if (N < 1 || HW < 1) fail("bce_dice_fwd", "N, HW >= 1");
  dense(logits, at::kFloat, (int64_t)N * HW, "bce_dice_fwd", "logits");
  dense(target, at::kFloat, (int64_t)N * HW, "bce_dice_fwd", "target");
  dice_weight_check(bce_weight, dice_weight, smooth, "bce_dice_fwd");
  dense(loss, at::kFloat, 1, "bce_dice_fwd", "loss");
  dense(tab, at::kFloat, (int64_t)N * 2, "bce_dice_fwd", "tab");
  at::Tensor part = at::empty({N, (int64_t)dlmpi_seg_dice_blocks(HW, N), 4}, logits.options());
  check(dlmpi_bce_dice_fwd(ptr<float>(logits), ptr<float>(target), N, HW, (float)bce_weight, (float)dice_weight,
                           (float)smooth, ptr<float>(part), ptr<float>(loss), ptr<float>(tab), cur_stream()),
        "bce_dice_fwd");
}
void bce_dice_bwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW,
                  const c10::optional<at::Tensor>& go, const at::Tensor& tab, double bce_weight, at::Tensor dlogits) {
  if (N < 1 || HW < 1) fail("bce_dice_bwd", "N, HW >= 1");
  dense(logits, at::kFloat, (int64_t)N * HW, "bce_dice_bwd", "logits");
  dense(target, at::kFloat, (int64_t)N * HW, "bce_dice_bwd", "target");
  dense(dlogits, at::kFloat, (int64_t)N * HW, "bce_dice_bwd", "dlogits");
  dense(tab, at::kFloat, (int64_t)N * 2, "bce_dice_bwd", "tab");
  if (!std::isfinite(bce_weight) || bce_weight < 0) fail("bce_dice_bwd", "bce_weight must be finite and >= 0");
  dense(go, at::kFloat, 1, "bce_dice_bwd", "go");
  check(dlmpi_bce_dice_bwd(ptr<float>(logits), ptr<float>(target), N, HW, optr<float>(go), ptr<float>(tab),
                           (float)bce_weight, ptr<float>(dlogits), cur_stream()),
        "bce_dice_bwd");
}
// Online hard example mining (ohem.hip).  The selection's parameters are checked here, host-side; tau = -log(thresh)
// is formed in double and rounded once to fp32.  state: int32 [8] = {k, n_valid, n_selected, the bits of cut, ...};
// the histograms and the partial sums are allocated here as pixel_ce_fwd's partials are.
struct OhemParams {
  int has_tau;
  float tau;
  at::Tensor ws, partial;
};
OhemParams ohem_params(const char* fn, double keep_ratio, int64_t min_kept, const c10::optional<double>& tau,
                       int64_t M, const at::Tensor& like, const at::Tensor& state) {
  if (!(keep_ratio > 0 && keep_ratio <= 1)) fail(fn, "keep_ratio must lie in (0, 1]");
  if (min_kept < 1) fail(fn, "min_kept must be >= 1");
  if (tau.has_value() && !(*tau > 0 && std::isfinite(*tau) && (float)*tau > 0))
    fail(fn, "thresh must lie in (0, 1) (tau = -log(thresh) finite and > 0)");
  if (M < 1 || M > 2147483647LL) fail(fn, "the selection counts in uint32: 1 <= pixels < 2^31");
  dense(state, at::kInt, 8, fn, "state");
  return {tau.has_value() ? 1 : 0, tau.has_value() ? (float)*tau : 0.f,
          at::empty({(int64_t)dlmpi_ohem_ws_words()}, like.options().dtype(at::kInt)),
          at::empty({(int64_t)dlmpi_ohem_partial_floats(M)}, like.options().dtype(at::kFloat))};
}
c10::optional<double> ohem_tau(const char* fn, const c10::optional<double>& thresh) {
  if (!thresh.has_value()) return c10::nullopt;
  if (!(*thresh > 0 && *thresh < 1)) fail(fn, "thresh must lie in (0, 1)");
  return -std::log(*thresh);
}
void ohem_select(const at::Tensor& nll, double keep_ratio, int64_t min_kept, const c10::optional<double>& tau,
                 at::Tensor state, at::Tensor loss, at::Tensor den) {
  if (layout_fault(nll, at::kFloat) != Fault::none) fail("ohem_select", "nll must be a contiguous fp32 GPU tensor");
  OhemParams p = ohem_params("ohem_select", keep_ratio, min_kept, tau, nll.numel(), nll, state);
  dense(loss, at::kFloat, 1, "ohem_select", "loss");
  dense(den, at::kFloat, 1, "ohem_select", "den");
  check(dlmpi_ohem_select(ptr<float>(nll), nll.numel(), keep_ratio, min_kept, p.has_tau, p.tau, ptr<uint32_t>(p.ws),
                          ptr<float>(p.partial), ptr<uint32_t>(state), ptr<float>(loss), ptr<float>(den),
                          cur_stream()),
        "ohem_select");
}
void ohem_ce_fwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                 const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                 double keep_ratio, int64_t min_kept, const c10::optional<double>& thresh, at::Tensor lse,
                 at::Tensor nll, at::Tensor state, at::Tensor loss, at::Tensor den) {
  pix_fwd_check("ohem_ce_fwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, nullptr, &loss);
  dense(nll, at::kFloat, (int64_t)N * HW, "ohem_ce_fwd", "nll");
  OhemParams p = ohem_params("ohem_ce_fwd", keep_ratio, min_kept, ohem_tau("ohem_ce_fwd", thresh), (int64_t)N * HW,
                             logits, state);
  check(dlmpi_ohem_ce_fwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                          optr<float>(weight), keep_ratio, min_kept, p.has_tau, p.tau, ptr<float>(lse),
                          ptr<float>(nll), ptr<uint32_t>(p.ws), ptr<float>(p.partial), ptr<uint32_t>(state),
                          ptr<float>(loss), ptr<float>(den), cur_stream()),
        "ohem_ce_fwd");
}
void ohem_ce_bwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                 const at::Tensor& labels, int64_t ignore_index, const c10::optional<at::Tensor>& weight,
                 const at::Tensor& lse, const at::Tensor& nll, const at::Tensor& cut,
                 const c10::optional<at::Tensor>& go, const at::Tensor& den, at::Tensor dlogits) {
  pix_bwd_check("ohem_ce_bwd", logits, sn, sk, sp, N, K, HW, labels, weight, lse, den, nullptr, dlogits, go);
  dense(nll, at::kFloat, (int64_t)N * HW, "ohem_ce_bwd", "nll");
  dense(cut, at::kFloat, 1, "ohem_ce_bwd", "cut");
  check(dlmpi_ohem_ce_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                          optr<float>(weight), ptr<float>(lse), ptr<float>(nll), ptr<float>(cut), optr<float>(go),
                          ptr<float>(den), ptr<float>(dlogits), cur_stream()),
        "ohem_ce_bwd");
}
// logits, target: contiguous fp32 of M elements
void ohem_bce_fwd(const at::Tensor& logits, const at::Tensor& target, int64_t M, double keep_ratio, int64_t min_kept,
                  const c10::optional<double>& thresh, at::Tensor nll, at::Tensor state, at::Tensor loss,
                  at::Tensor den) {
  OhemParams p = ohem_params("ohem_bce_fwd", keep_ratio, min_kept, ohem_tau("ohem_bce_fwd", thresh), M, logits, state);
  dense(logits, at::kFloat, M, "ohem_bce_fwd", "logits");
  dense(target, at::kFloat, M, "ohem_bce_fwd", "target");
  dense(nll, at::kFloat, M, "ohem_bce_fwd", "nll");
  dense(loss, at::kFloat, 1, "ohem_bce_fwd", "loss");
  dense(den, at::kFloat, 1, "ohem_bce_fwd", "den");
  check(dlmpi_ohem_bce_fwd(ptr<float>(logits), ptr<float>(target), M, keep_ratio, min_kept, p.has_tau, p.tau,
                           ptr<float>(nll), ptr<uint32_t>(p.ws), ptr<float>(p.partial), ptr<uint32_t>(state),
                           ptr<float>(loss), ptr<float>(den), cur_stream()),
        "ohem_bce_fwd");
}
void ohem_bce_bwd(const at::Tensor& logits, const at::Tensor& target, int64_t M, const at::Tensor& nll,
                  const at::Tensor& cut, const c10::optional<at::Tensor>& go, const at::Tensor& den,
                  at::Tensor dlogits) {
  if (M < 1 || M > 2147483647LL) fail("ohem_bce_bwd", "1 <= pixels < 2^31");
  dense(logits, at::kFloat, M, "ohem_bce_bwd", "logits");
  dense(target, at::kFloat, M, "ohem_bce_bwd", "target");
  dense(nll, at::kFloat, M, "ohem_bce_bwd", "nll");
  dense(dlogits, at::kFloat, M, "ohem_bce_bwd", "dlogits");
  dense(cut, at::kFloat, 1, "ohem_bce_bwd", "cut");
  dense(den, at::kFloat, 1, "ohem_bce_bwd", "den");
  dense(go, at::kFloat, 1, "ohem_bce_bwd", "go");
  check(dlmpi_ohem_bce_bwd(ptr<float>(logits), ptr<float>(target), M, ptr<float>(nll), ptr<float>(cut),
                           optr<float>(go), ptr<float>(den), ptr<float>(dlogits), cur_stream()),
        "ohem_bce_bwd");
}
// Lovasz-Softmax / Lovasz hinge (lovasz.hip).  S segments of L pixels; the workspace (keys and payloads ping-pong,
// histograms, partials) comes from the caching allocator per call.  g fp32 [S * L], coef fp32 [S], stats int32 [2 + S].
void lovasz_weight_check(double a, double b, const char* fn) {
  if (!std::isfinite(a) || !std::isfinite(b) || a < 0 || b < 0)
    fail(fn, "the two loss weights must be finite and >= 0");
}
at::Tensor lovasz_ws(const char* fn, int64_t S, int64_t L, int64_t M, const at::Tensor& like) {
  if (L >= 2147483648LL) fail(fn, "a segment's pixels are indexed in 31 bits: L < 2^31");
  const int64_t words = dlmpi_lovasz_ws_words(S, L, M);
  if (words < 0) fail(fn, "1 <= segments <= 65535 and 1 <= pixels per segment < 2^31");
  return at::empty({words}, like.options().dtype(at::kInt));
}
void lovasz_out_check(const char* fn, int64_t S, int64_t L, const at::Tensor& g, const at::Tensor& coef,
                      const at::Tensor* stats) {
  dense(g, at::kFloat, S * L, fn, "g");
  dense(coef, at::kFloat, S, fn, "coef");
  if (stats) dense(*stats, at::kInt, 2 + S, fn, "stats");
}
void lovasz_rank(const at::Tensor& err, const at::Tensor& fg, const at::Tensor& valid, bool hinge, at::Tensor g,
                 at::Tensor perm, at::Tensor seg_loss) {
  if (err.dim() != 2 || err.numel() < 1) fail("lovasz_rank", "err must be [S, L] with S, L >= 1");
  const int64_t S = err.size(0), L = err.size(1);
  dense(err, at::kFloat, S * L, "lovasz_rank", "err");
  dense(fg, at::kByte, S * L, "lovasz_rank", "fg");
  dense(valid, at::kByte, S * L, "lovasz_rank", "valid");
  dense(g, at::kFloat, S * L, "lovasz_rank", "g");
  dense(perm, at::kInt, S * L, "lovasz_rank", "perm");
  dense(seg_loss, at::kFloat, S, "lovasz_rank", "seg_loss");
  at::Tensor ws = lovasz_ws("lovasz_rank", S, L, 1, err);
  check(dlmpi_lovasz_rank(ptr<float>(err), ptr<uint8_t>(fg), ptr<uint8_t>(valid), S, L, hinge ? 1 : 0,
                          ptr<uint32_t>(ws), ptr<float>(g), ptr<int32_t>(perm), ptr<float>(seg_loss), cur_stream()),
        "lovasz_rank");
}
void lovasz_softmax_fwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                        const at::Tensor& labels, int64_t ignore_index, bool per_image, bool classes_all,
                        double ce_weight, double lovasz_weight, at::Tensor lse, at::Tensor g, at::Tensor coef,
                        at::Tensor stats, at::Tensor loss, at::Tensor den) {
  const char* fn = "lovasz_softmax_fwd";
  pix_fwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, c10::nullopt, lse, den, nullptr, &loss);
  lovasz_weight_check(ce_weight, lovasz_weight, fn);
  const int64_t M = (int64_t)N * HW, S = per_image ? (int64_t)N * K : K, L = per_image ? HW : M;
  at::Tensor ws = lovasz_ws(fn, S, L, M, logits);
  lovasz_out_check(fn, S, L, g, coef, &stats);
  check(dlmpi_lovasz_softmax_fwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                 per_image ? 1 : 0, classes_all ? 1 : 0, (float)ce_weight, (float)lovasz_weight,
                                 ptr<float>(lse), ptr<uint32_t>(ws), ptr<float>(g), ptr<float>(coef),
                                 ptr<int32_t>(stats), ptr<float>(loss), ptr<float>(den), cur_stream()),
        fn);
}
void lovasz_softmax_bwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                        const at::Tensor& labels, int64_t ignore_index, bool per_image, const at::Tensor& lse,
                        const at::Tensor& g, const at::Tensor& coef, const at::Tensor& den,
                        const c10::optional<at::Tensor>& go, double ce_weight, double lovasz_weight,
                        at::Tensor dlogits) {
  const char* fn = "lovasz_softmax_bwd";
  pix_bwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, c10::nullopt, lse, den, nullptr, dlogits, go);
  lovasz_weight_check(ce_weight, lovasz_weight, fn);
  const int64_t M = (int64_t)N * HW, S = per_image ? (int64_t)N * K : K, L = per_image ? HW : M;
  lovasz_out_check(fn, S, L, g, coef, nullptr);
  check(dlmpi_lovasz_softmax_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                 per_image ? 1 : 0, ptr<float>(lse), ptr<float>(g), ptr<float>(coef), ptr<float>(den),
                                 optr<float>(go), (float)ce_weight, (float)lovasz_weight, ptr<float>(dlogits),
                                 cur_stream()),
        fn);
}
// logits, target: contiguous fp32 [N][HW]
void lovasz_hinge_fwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW, bool per_image,
                      double bce_weight, double lovasz_weight, at::Tensor g, at::Tensor coef, at::Tensor stats,
                      at::Tensor loss, at::Tensor den) {
  const char* fn = "lovasz_hinge_fwd";
  if (N < 1 || HW < 1) fail(fn, "N, HW >= 1");
  const int64_t M = (int64_t)N * HW, S = per_image ? N : 1, L = per_image ? HW : M;
  dense(logits, at::kFloat, M, fn, "logits");
  dense(target, at::kFloat, M, fn, "target");
  lovasz_weight_check(bce_weight, lovasz_weight, fn);
  at::Tensor ws = lovasz_ws(fn, S, L, M, logits);
  lovasz_out_check(fn, S, L, g, coef, &stats);
  dense(loss, at::kFloat, 1, fn, "loss");
  dense(den, at::kFloat, 1, fn, "den");
  check(dlmpi_lovasz_hinge_fwd(ptr<float>(logits), ptr<float>(target), N, HW, per_image ? 1 : 0, (float)bce_weight,
                               (float)lovasz_weight, ptr<uint32_t>(ws), ptr<float>(g), ptr<float>(coef),
                               ptr<int32_t>(stats), ptr<float>(loss), ptr<float>(den), cur_stream()),
        fn);
}
void lovasz_hinge_bwd(const at::Tensor& logits, const at::Tensor& target, int N, int64_t HW, bool per_image,
                      const at::Tensor& g, const at::Tensor& coef, const c10::optional<at::Tensor>& go,
                      double bce_weight, double lovasz_weight, at::Tensor dlogits) {
  const char* fn = "lovasz_hinge_bwd";
  if (N < 1 || HW < 1) fail(fn, "N, HW >= 1");
  const int64_t M = (int64_t)N * HW, S = per_image ? N : 1, L = per_image ? HW : M;
  dense(logits, at::kFloat, M, fn, "logits");
  dense(target, at::kFloat, M, fn, "target");
  dense(dlogits, at::kFloat, M, fn, "dlogits");
  lovasz_weight_check(bce_weight, lovasz_weight, fn);
  lovasz_out_check(fn, S, L, g, coef, nullptr);
  dense(go, at::kFloat, 1, fn, "go");
  check(dlmpi_lovasz_hinge_bwd(ptr<float>(logits), ptr<float>(target), N, HW, per_image ? 1 : 0, ptr<float>(g),
                               ptr<float>(coef), optr<float>(go), (float)bce_weight, (float)lovasz_weight,
                               ptr<float>(dlogits), cur_stream()),
        fn);
}
// Exact Euclidean distance transform / signed distance map (edt.hip).  src [N, H, W]: int64 labels of K classes, or
// with K = 1 an fp32 target (G = {t > 0.5}) or a bool / uint8 mask; phi fp32, d2_in / d2_out int32, each [N, K, H, W]
// or absent.  The uint16 row plane and the row flags come from the caching allocator per call.
void edt(const at::Tensor& src, int64_t K, int64_t ignore_index, const c10::optional<at::Tensor>& phi,
         const c10::optional<at::Tensor>& d2_in, const c10::optional<at::Tensor>& d2_out) {
  const char* fn = "edt";
  if (src.dim() != 3 || src.numel() < 1) fail(fn, "src must be [N, H, W] with N, H, W >= 1");
  const int64_t N = src.size(0), H = src.size(1), W = src.size(2);
  const at::ScalarType t = src.scalar_type();
  const int source = t == at::kLong ? 0 : t == at::kFloat ? 1 : (t == at::kBool || t == at::kByte) ? 2 : -1;
  if (source < 0 || !src.is_cuda() || !src.is_contiguous())
    fail(fn, "src must be a contiguous int64, fp32, bool or uint8 GPU tensor");
  if (source != 0 && K != 1) fail(fn, "a target or a mask is one class: K = 1");
  const int64_t bytes = dlmpi_edt_ws_bytes(N, K, H, W);
  if (bytes < 0) fail(fn, "served shapes: 1 <= H <= 4096, 1 <= W <= 16384, 1 <= K <= 256");
  if (!given(phi) && !given(d2_in) && !given(d2_out)) fail(fn, "nothing to write");
  dense(phi, at::kFloat, N * K * H * W, fn, "phi");
  dense(d2_in, at::kInt, N * K * H * W, fn, "d2_in");
  dense(d2_out, at::kInt, N * K * H * W, fn, "d2_out");
  at::Tensor ws = at::empty({(bytes + 1) / 2}, src.options().dtype(at::kShort));
  check(dlmpi_edt(src.data_ptr(), source, N, (int)K, (int)H, (int)W, ignore_index, ws.data_ptr(), optr<float>(phi),
                  optr<int32_t>(d2_in), optr<int32_t>(d2_out), cur_stream()),
        fn);
}
// Surface-distance metrics (surface.hip).  Softmax form: logits addressed by (sn, sk, sp) over N x K x H W with int64
// labels [N, H, W]; binary form (K = 1): dense fp32 logits and target of N H W elements, the strides unused.  metrics
// fp32 [N, K, 3], counts int64 [N, K, 2].  The workspace comes from the caching allocator per call.
void surface_distances(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int64_t N, int64_t K, int64_t H,
                       int64_t W, const at::Tensor& target, int64_t ignore_index, double percentile,
                       at::Tensor metrics, at::Tensor counts) {
  const char* fn = "surface_distances";
  const int64_t bytes = dlmpi_surface_ws_bytes(N, K, H, W);
  if (bytes < 0) fail(fn, "served shapes: N >= 1, 1 <= H <= 4096, 1 <= W <= 16384, 1 <= K <= 256");
  if (!(percentile > 0.0 && percentile <= 100.0)) fail(fn, "percentile must lie in (0, 100]");
  const bool binary = target.scalar_type() != at::kLong;
  if (binary) {
    if (K != 1) fail(fn, "a float target is one class: K = 1");
    dense(logits, at::kFloat, N * H * W, fn, "logits");
    dense(target, at::kFloat, N * H * W, fn, "target");
  } else {
    pix_check(logits, sn, sk, sp, (int)N, (int)K, H * W, target, fn, "logits");
  }
  dense(metrics, at::kFloat, N * K * 3, fn, "metrics");
  dense(counts, at::kLong, N * K * 2, fn, "counts");
  at::Tensor ws = at::empty({bytes}, logits.options().dtype(at::kByte));   // the allocator's blocks are 512-B aligned
  check(dlmpi_surface_distances(ptr<float>(logits), sn, sk, sp, target.data_ptr(), binary ? 1 : 0, N, (int)K, (int)H,
                                (int)W, ignore_index, percentile / 100.0, ws.data_ptr(), ptr<float>(metrics),
                                ptr<int64_t>(counts), cur_stream()),
        fn);
}
// Boundary loss (boundary.hip).  boundary_weight: a finite float >= 0, or with bw_dev one fp32 on the device that the
// kernels read; phi fp32 [N * K * HW] (softmax form) / [M] (sigmoid form).
void boundary_weight_check(double plain, double bw, const c10::optional<at::Tensor>& bw_dev, const char* fn) {
  if (!std::isfinite(plain) || !std::isfinite(bw) || plain < 0 || bw < 0)
    fail(fn, "the two loss weights must be finite and >= 0");
  dense(bw_dev, at::kFloat, 1, fn, "boundary_weight");
}
void boundary_softmax_fwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                          const at::Tensor& labels, int64_t ignore_index, const at::Tensor& phi,
                          bool include_background, double ce_weight, double boundary_weight,
                          const c10::optional<at::Tensor>& bw_dev, at::Tensor lse, at::Tensor loss, at::Tensor den) {
  const char* fn = "boundary_softmax_fwd";
  pix_fwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, c10::nullopt, lse, den, nullptr, &loss);
  boundary_weight_check(ce_weight, boundary_weight, bw_dev, fn);
  dense(phi, at::kFloat, (int64_t)N * K * HW, fn, "phi");
  const int64_t nblk = dlmpi_boundary_blocks((int64_t)N * HW);
  at::Tensor part = at::empty({nblk, 2}, logits.options());
  at::Tensor cnt = at::empty({nblk}, logits.options().dtype(at::kInt));
  check(dlmpi_boundary_softmax_fwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                   ptr<float>(phi), include_background ? 1 : 0, (float)ce_weight,
                                   (float)boundary_weight, optr<float>(bw_dev), ptr<float>(lse), ptr<float>(part),
                                   ptr<uint32_t>(cnt), ptr<float>(loss), ptr<float>(den), cur_stream()),
        fn);
}
void boundary_softmax_bwd(const at::Tensor& logits, int64_t sn, int64_t sk, int64_t sp, int N, int K, int64_t HW,
                          const at::Tensor& labels, int64_t ignore_index, const at::Tensor& phi,
                          bool include_background, const at::Tensor& lse, const at::Tensor& den,
                          const c10::optional<at::Tensor>& go, double ce_weight, double boundary_weight,
                          const c10::optional<at::Tensor>& bw_dev, at::Tensor dlogits) {
  const char* fn = "boundary_softmax_bwd";
  pix_bwd_check(fn, logits, sn, sk, sp, N, K, HW, labels, c10::nullopt, lse, den, nullptr, dlogits, go);
  boundary_weight_check(ce_weight, boundary_weight, bw_dev, fn);
  dense(phi, at::kFloat, (int64_t)N * K * HW, fn, "phi");
  check(dlmpi_boundary_softmax_bwd(ptr<float>(logits), sn, sk, sp, N, K, HW, ptr<int64_t>(labels), ignore_index,
                                   ptr<float>(phi), include_background ? 1 : 0, ptr<float>(lse), ptr<float>(den),
                                   optr<float>(go), (float)ce_weight, (float)boundary_weight, optr<float>(bw_dev),
                                   ptr<float>(dlogits), cur_stream()),
        fn);
}
// logits, target, phi: contiguous fp32 of M elements
void boundary_sigmoid_fwd(const at::Tensor& logits, const at::Tensor& target, const at::Tensor& phi, int64_t M,
                          double bce_weight, double boundary_weight, const c10::optional<at::Tensor>& bw_dev,
                          at::Tensor loss, at::Tensor den) {
  const char* fn = "boundary_sigmoid_fwd";
  if (M < 1) fail(fn, "M >= 1");
  dense(logits, at::kFloat, M, fn, "logits");
  dense(target, at::kFloat, M, fn, "target");
  dense(phi, at::kFloat, M, fn, "phi");
  boundary_weight_check(bce_weight, boundary_weight, bw_dev, fn);
  dense(loss, at::kFloat, 1, fn, "loss");
  dense(den, at::kFloat, 1, fn, "den");
  at::Tensor part = at::empty({(int64_t)dlmpi_boundary_blocks(M), 2}, logits.options());
  check(dlmpi_boundary_sigmoid_fwd(ptr<float>(logits), ptr<float>(target), ptr<float>(phi), M, (float)bce_weight,
                                   (float)boundary_weight, optr<float>(bw_dev), ptr<float>(part), ptr<float>(loss),
                                   ptr<float>(den), cur_stream()),
        fn);
}
void boundary_sigmoid_bwd(const at::Tensor& logits, const at::Tensor& target, const at::Tensor& phi, int64_t M,
                          const c10::optional<at::Tensor>& go, double bce_weight, double boundary_weight,
                          const c10::optional<at::Tensor>& bw_dev, at::Tensor dlogits) {
  const char* fn = "boundary_sigmoid_bwd";
  if (M < 1) fail(fn, "M >= 1");
  dense(logits, at::kFloat, M, fn, "logits");
  dense(target, at::kFloat, M, fn, "target");
  dense(phi, at::kFloat, M, fn, "phi");
  dense(dlogits, at::kFloat, M, fn, "dlogits");
  boundary_weight_check(bce_weight, boundary_weight, bw_dev, fn);
  dense(go, at::kFloat, 1, fn, "go");
  check(dlmpi_boundary_sigmoid_bwd(ptr<float>(logits), ptr<float>(target), ptr<float>(phi), M, optr<float>(go),
                                   (float)bce_weight, (float)boundary_weight, optr<float>(bw_dev),
                                   ptr<float>(dlogits), cur_stream()),
        fn);
}
}  // namespace

void register_loss(pybind11::module& m) {
  namespace py = pybind11;
  m.def("softmax_ce_fwd", &softmax_ce_fwd);
  m.def("softmax_ce_bwd", &softmax_ce_bwd);
  m.def("bce_fwd", &bce_fwd);
  m.def("bce_bwd", &bce_bwd);
  m.def("argmax_correct", &argmax_correct);
  m.def("dice", &dice);
  m.def("cls_ce_fwd", &cls_ce_fwd);
  m.def("cls_ce_bwd", &cls_ce_bwd);
  m.def("cls_ce_check", &check_cls_ce_args, py::arg("fn") = "cls_ce_fwd", py::arg("N"), py::arg("K"), py::arg("ldl"),
        py::arg("logits_numel"), py::arg("logits_f32") = true, py::arg("labels_numel"), py::arg("labels_i64") = true,
        py::arg("labels_b_numel") = -1, py::arg("labels_b_i64") = true, py::arg("lam_numel") = -1,
        py::arg("lam_f32") = true, py::arg("weight_numel") = -1, py::arg("weight_f32") = true, py::arg("eps") = 0.0,
        py::arg("lse_numel"), py::arg("rows_numel"), py::arg("den_numel") = 1, py::arg("dlogits_numel") = -1,
        py::arg("go_numel") = -1);
  m.def("pixel_ce_fwd", &pixel_ce_fwd);
  m.def("set_pixel_tiles", [](int on) { dlmpi_set_pixel_tiles(on); });
  m.def("pixel_ce_bwd", &pixel_ce_bwd);
  m.def("seg_counts", &seg_counts);
  m.def("pixel_ce_dice_fwd", &pixel_ce_dice_fwd);
  m.def("pixel_ce_dice_bwd", &pixel_ce_dice_bwd);
  m.def("bce_dice_fwd", &bce_dice_fwd);
  m.def("bce_dice_bwd", &bce_dice_bwd);
  m.def("ohem_select", &ohem_select);
  m.def("ohem_ce_fwd", &ohem_ce_fwd);
  m.def("ohem_ce_bwd", &ohem_ce_bwd);
  m.def("ohem_bce_fwd", &ohem_bce_fwd);
  m.def("ohem_bce_bwd", &ohem_bce_bwd);
  m.def("set_ohem_aggregate", [](int on) { dlmpi_set_ohem_aggregate(on); });
  m.def("lovasz_tile", []() { return dlmpi_lovasz_tile(); });
  m.def("lovasz_rank", &lovasz_rank);
  m.def("lovasz_softmax_fwd", &lovasz_softmax_fwd);
  m.def("lovasz_softmax_bwd", &lovasz_softmax_bwd);
  m.def("lovasz_hinge_fwd", &lovasz_hinge_fwd);
  m.def("lovasz_hinge_bwd", &lovasz_hinge_bwd);
  m.def("edt_strip", []() { return dlmpi_edt_strip(); });
  m.def("edt_strip_rows", []() { return dlmpi_edt_strip_rows(); });
  m.def("edt", &edt);
  m.def("surface_tile", []() { return dlmpi_surface_tile(); });
  m.def("surface_distances", &surface_distances);
  m.def("boundary_softmax_fwd", &boundary_softmax_fwd);
  m.def("boundary_softmax_bwd", &boundary_softmax_bwd);
  m.def("boundary_sigmoid_fwd", &boundary_sigmoid_fwd);
  m.def("boundary_sigmoid_bwd", &boundary_sigmoid_bwd);
}

}  // namespace dlmpi_ext
