// Torch binding of the losses and evaluation counts (kernels/loss.hip, cls_ce.hip, pixel_ce.hip, seg_dice.hip).
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
}

}  // namespace dlmpi_ext
