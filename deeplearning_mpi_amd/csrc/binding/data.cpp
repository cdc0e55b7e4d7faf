// Torch binding of the device-resident input pipeline (kernels/data.hip, seg_aug.hip, rrc.hip).  Nothing here
// synchronises, with one exception outside the step: image_rrc_batch reads a crop table back the first time it
// sees it.
#include <cmath>
#include <vector>

#include "common.h"

namespace dlmpi_ext {
namespace {

// The operands image_batch and image_batch_mix share (C: norm3): data uint8 [.][H][W][C] gathered by idx [B] into out
// fp32 [B, C, H, W].  -> B
int batch_operands(const char* fn, const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, int H,
                   int W, int C, const at::Tensor& out) {
  if (!data.is_cuda() || data.scalar_type() != at::kByte) fail(fn, "data must be a uint8 GPU tensor");
  if (labels.scalar_type() != at::kLong) fail(fn, "labels must be int64");
  const int B = (int)idx.numel();
  if (B < 1 || H < 1 || W < 1) fail(fn, "empty batch");
  dense(idx, at::kLong, B, fn, "idx");
  dense(out, at::kFloat, (int64_t)B * C * H * W, fn, "out");
  return B;
}

void image_batch(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, int H, int W, int C,
                 int pad, bool augment, int64_t seed, int64_t epoch, std::vector<double> mean, std::vector<double> sd,
                 at::Tensor out, const c10::optional<at::Tensor>& out_labels) {
  const Norm3 n = norm3(mean, sd, C, "image_batch");
  const int B = batch_operands("image_batch", data, labels, idx, H, W, C, out);
  check(dlmpi_image_batch(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), B, H, W, C, pad, augment ? 1 : 0,
                          (uint32_t)seed, (uint32_t)epoch, n.m3, n.s3, ptr<float>(out), optr<int64_t>(out_labels),
                          cur_stream()),
        "image_batch");
}

// The mixed batch of the device-resident pipeline and the in-place mix of any fp32 NCHW batch (data.hip); kind
// 0 none / 1 mixup / 2 CutMix with the box rows [y0, y1) x columns [x0, x1) inside the image.
void mix_args_ok(const char* fn, int kind, double lam, int H, int W, int y0, int y1, int x0, int x1,
                 const at::Tensor& labels_a, const at::Tensor& labels_b, const at::Tensor& lam_out, int B) {
  if (kind < 0 || kind > 2) fail(fn, "kind must be 0, 1 or 2");
  if (!(lam >= 0 && lam <= 1)) fail(fn, "lam must lie in [0, 1]");
  if (y0 < 0 || y1 < y0 || y1 > H || x0 < 0 || x1 < x0 || x1 > W) fail(fn, "the box must lie inside the image");
  dense(labels_a, at::kLong, B, fn, "labels");
  dense(labels_b, at::kLong, B, fn, "labels_b");
  dense(lam_out, at::kFloat, 1, fn, "lam_out");
}
void image_batch_mix(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, int H, int W, int C,
                     int pad, bool augment, int64_t seed, int64_t epoch, std::vector<double> mean,
                     std::vector<double> sd, int kind, double lam, int y0, int y1, int x0, int x1, at::Tensor out,
                     at::Tensor out_labels, at::Tensor labels_b, at::Tensor lam_out) {
  const Norm3 n = norm3(mean, sd, C, "image_batch_mix");
  const int B = batch_operands("image_batch_mix", data, labels, idx, H, W, C, out);
  mix_args_ok("image_batch_mix", kind, lam, H, W, y0, y1, x0, x1, out_labels, labels_b, lam_out, B);
  check(dlmpi_image_batch_mix(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), B, H, W, C, pad,
                              augment ? 1 : 0, (uint32_t)seed, (uint32_t)epoch, n.m3, n.s3, kind, (float)lam, y0, y1,
                              x0, x1, ptr<float>(out), ptr<int64_t>(out_labels), ptr<int64_t>(labels_b),
                              ptr<float>(lam_out), cur_stream()),
        "image_batch_mix");
}
void mix_batch_(at::Tensor x, const at::Tensor& labels, int kind, double lam, int y0, int y1, int x0, int x1,
                at::Tensor labels_b, at::Tensor lam_out) {
  if (x.dim() != 4 || layout_fault(x, at::kFloat) != Fault::none || x.numel() < 1)
    fail("mix_batch_", "x must be a contiguous fp32 [B, C, H, W] GPU tensor");
  const int B = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2), W = (int)x.size(3);
  mix_args_ok("mix_batch_", kind, lam, H, W, y0, y1, x0, x1, labels, labels_b, lam_out, B);
  check(dlmpi_mix_batch(ptr<float>(x), ptr<int64_t>(labels), B, C, H, W, kind, (float)lam, y0, y1, x0, x1,
                        ptr<int64_t>(labels_b), ptr<float>(lam_out), cur_stream()),
        "mix_batch_");
}

// Segmentation augmentation (seg_aug.hip): images fp32 [N, C, H, W] and masks [N, H, W] (float32 | int64) gathered
// by idx [B] and resampled through rows idx[b] of table (int32 [N, 6], Q16) into out [B, C, Ho, Wo] and out_mask
// [B, Ho, Wo].  idx values are trusted.
void seg_aug_batch(const at::Tensor& images, const at::Tensor& masks, const at::Tensor& idx, const at::Tensor& table,
                   double image_fill, double mask_fill, at::Tensor out, at::Tensor out_mask) {
  const char* fn = "seg_aug_batch";
  if (layout_fault(images, at::kFloat) != Fault::none || images.dim() != 4 || images.numel() < 1)
    fail(fn, "images must be a contiguous fp32 [N, C, H, W] GPU tensor");
  const int64_t N = images.size(0), C = images.size(1), H = images.size(2), W = images.size(3);
  const bool i64 = masks.scalar_type() == at::kLong;
  if (!i64 && masks.scalar_type() != at::kFloat) fail(fn, "masks must be float32 or int64");
  const at::ScalarType mt = i64 ? at::kLong : at::kFloat;
  shaped(masks, mt, {N, H, W}, fn, "masks");
  if (layout_fault(idx, at::kLong) != Fault::none || idx.dim() != 1 || idx.numel() < 1)
    fail(fn, "idx must be a contiguous int64 [B] GPU tensor, B >= 1");
  shaped(table, at::kInt, {N, 6}, fn, "table");
  if (out.dim() != 4 || out.numel() < 1) fail(fn, "out must be a contiguous fp32 [B, C, Ho, Wo] GPU tensor");
  const int64_t B = idx.numel(), Ho = out.size(2), Wo = out.size(3);
  shaped(out, at::kFloat, {B, C, Ho, Wo}, fn, "out");
  shaped(out_mask, mt, {B, Ho, Wo}, fn, "out_mask");
  if (H * W > INT32_MAX || out_mask.numel() > INT32_MAX || C > INT32_MAX)
    fail(fn, "an images plane and out_mask hold at most 2^31 - 1 pixels");
  if (!std::isfinite(image_fill) || !std::isfinite(mask_fill)) fail(fn, "image_fill and mask_fill must be finite");
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
struct CheckedTable {
  at::Tensor table;
  const void* ptr;
  uint32_t version;
  int64_t H, W, Ho, Wo;
};
[[noreturn]] void rrc_fail(const std::string& why) { fail("image_rrc_batch", why); }

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

void image_rrc_batch(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& idx, const at::Tensor& table,
                     std::vector<double> mean, std::vector<double> sd, at::Tensor out, at::Tensor out_labels) {
  // all six tensors per fault, in this order: the texts speak of all of them, and tests pin them
  const std::pair<const at::Tensor*, at::ScalarType> operands[] = {{&data, at::kByte},  {&labels, at::kLong},
                                                                   {&idx, at::kLong},   {&table, at::kInt},
                                                                   {&out, at::kFloat},  {&out_labels, at::kLong}};
  static const char* const why[] = {
      "", "every tensor must be on the GPU",
      "uint8 data, int64 labels and indices, an int32 table, fp32 output and int64 output labels",
      "every tensor must be contiguous"};
  for (Fault f : {Fault::host, Fault::dtype, Fault::strided})
    for (const auto& o : operands)
      if (layout_fault(*o.first, o.second) == f) rrc_fail(why[(int)f]);
  if (data.dim() != 4 || data.numel() < 1) rrc_fail("data must be [N, H, W, C]");
  const int64_t N = data.size(0), H = data.size(1), W = data.size(2), C = data.size(3);
  if (C != 1 && C != 3) rrc_fail("C must be 1 or 3, got " + std::to_string(C));
  const Norm3 n = norm3(mean, sd, C, "image_rrc_batch");
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
  check(dlmpi_image_rrc_batch(ptr<uint8_t>(data), ptr<int64_t>(labels), ptr<int64_t>(idx), ptr<int>(table), (int)B,
                              (int)H, (int)W, (int)C, (int)Ho, (int)Wo, n.m3, n.s3, ptr<float>(out),
                              ptr<int64_t>(out_labels), cur_stream()),
        "image_rrc_batch");
}

}  // namespace

void register_data(pybind11::module& m) {
  m.def("image_batch", &image_batch);
  m.def("image_batch_mix", &image_batch_mix);
  m.def("mix_batch_", &mix_batch_);
  m.def("seg_aug_batch", &seg_aug_batch);
  m.def("image_rrc_batch", &image_rrc_batch);
  m.def("rrc_max_scale", []() { return dlmpi_rrc_max_scale(); });
}

}  // namespace dlmpi_ext
