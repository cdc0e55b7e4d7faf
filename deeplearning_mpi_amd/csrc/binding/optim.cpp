// Torch binding of the optimisers on flat fp32 buffers (kernels/optim.hip) and the layer-wise family over the
// segment / chunk tables of ParamArena.segments() (optim_layerwise.hip), and the weight EMA (ema.hip).  sgd_step,
// adam_step, grad_norm and scale_ take their buffers from the caller (NativeBackend) unchecked.
#include <algorithm>

#include "common.h"

namespace dlmpi_ext {
namespace {

void sgd_step(at::Tensor p, const at::Tensor& g, at::Tensor m, double lr, double momentum, double dampening,
              double wd, bool nesterov, bool first, const c10::optional<at::Tensor>& skip_flag) {
  check(dlmpi_sgd(ptr<float>(p), ptr<float>(g), ptr<float>(m), p.numel(), (float)lr, (float)momentum,
                  (float)dampening, (float)wd, nesterov ? 1 : 0, first ? 1 : 0, optr<float>(skip_flag), cur_stream()),
        "sgd");
}
void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, double lr, double b1, double b2,
               double eps, double wd, bool adamw, double bc1, double bc2, const c10::optional<at::Tensor>& clip,
               const c10::optional<at::Tensor>& tstep, bool clip_writeback) {
  check(dlmpi_adam(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<float>(v), p.numel(), (float)lr, b1, b2,
                   (float)eps, (float)wd, adamw ? 1 : 0, (float)bc1, (float)bc2, optr<float>(clip),
                   optr<float>(tstep), clip_writeback ? 1 : 0, cur_stream()),   // tstep advanced in place unless skipped
        "adam");
}
// total L2 norm of a flat fp32 buffer -> norm_out[0]; coef_out = {min(1, max_norm/(norm+1e-6)), nonfinite}
void grad_norm(const at::Tensor& g, double max_norm, at::Tensor norm_out, at::Tensor coef_out) {
  const int nblk = 1024;
  at::Tensor partial = at::empty({nblk}, g.options().dtype(at::kFloat));
  check(dlmpi_sumsq(ptr<float>(g), g.numel(), ptr<float>(partial), nblk, cur_stream()), "sumsq");
  if (coef_out.numel() < 2) fail("grad_norm", "coef_out needs 2 (or 4) floats");
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
// extent = the largest start + length of the chunk table (known to the host that built it)
LwTables lw_tables(const at::Tensor& chunks, const at::Tensor& flags, int64_t extent, int64_t n, const char* fn) {
  if (chunks.dim() != 2 || chunks.size(1) != 4) fail(fn, "chunks must be [n][4]");
  if (chunks.size(0) > (1 << 30)) fail(fn, "too many chunks");
  dense(chunks, at::kInt, chunks.numel(), fn, "chunks");
  if (flags.numel() < 1 || flags.numel() > (1 << 24)) fail(fn, "flags [T]");
  dense(flags, at::kInt, flags.numel(), fn, "flags");
  if (extent < 0 || extent > n) fail(fn, "extent: the chunk table exceeds the buffers");
  return {(int)chunks.size(0), (int)flags.numel()};
}
void seg_sumsq(const at::Tensor& a, const at::Tensor& b, const at::Tensor& chunks, const at::Tensor& flags,
               int64_t extent, at::Tensor partial) {
  const int64_t n = a.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "seg_sumsq");
  dense(a, at::kFloat, n, "seg_sumsq", "a");
  dense(b, at::kFloat, n, "seg_sumsq", "b");
  dense(partial, at::kFloat, 2 * (int64_t)t.nchunks, "seg_sumsq", "partial");
  check(dlmpi_seg_sumsq(ptr<float>(a), ptr<float>(b), ptr<int>(chunks), t.nchunks, n, t.T, ptr<float>(partial),
                        cur_stream()),
        "seg_sumsq");
}
void seg_finish(const at::Tensor& partial, const at::Tensor& chunk_first, const at::Tensor& flags, at::Tensor tab,
                at::Tensor step, const c10::optional<at::Tensor>& skip, int mode, double tc, double wd, double eps,
                double b1, double b2, int kind, double base_lr, double warmup, double total, double min_lr,
                double power) {
  const int64_t T = flags.numel();
  if (T < 1 || T > (1 << 24)) fail("seg_finish", "flags [T]");
  if (partial.numel() % 2) fail("seg_finish", "partial must be [2][nchunks]");
  const int64_t nchunks = partial.numel() / 2;
  dense(partial, at::kFloat, 2 * nchunks, "seg_finish", "partial");
  dense(chunk_first, at::kInt, T + 1, "seg_finish", "chunk_first");
  dense(flags, at::kInt, T, "seg_finish", "flags");
  dense(tab, at::kFloat, dlmpi_lw_tab() + T, "seg_finish", "tab");
  dense(step, at::kFloat, 1, "seg_finish", "step");
  dense(skip, at::kFloat, 1, "seg_finish", "skip");
  if (mode < 0 || mode > 2 || kind < 0 || kind > 2) fail("seg_finish", "mode / kind");
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
  dense(p, at::kFloat, n, "lars_update", "p");
  dense(g, at::kFloat, n, "lars_update", "g");
  dense(m, at::kFloat, n, "lars_update", "m");
  dense(tab, at::kFloat, dlmpi_lw_tab() + t.T, "lars_update", "tab");
  check(dlmpi_lars_update(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<int>(chunks), t.nchunks, n, ptr<int>(flags),
                          t.T, ptr<float>(tab), (float)momentum, (float)wd, nesterov ? 1 : 0, cur_stream()),
        "lars_update");
}
void lamb_moments(const at::Tensor& p, const at::Tensor& g, at::Tensor m, at::Tensor v, const at::Tensor& chunks,
                  const at::Tensor& flags, int64_t extent, at::Tensor partial, const at::Tensor& tab,
                  const c10::optional<at::Tensor>& clip, double b1, double b2, double eps, double wd) {
  const int64_t n = p.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "lamb_moments");
  dense(p, at::kFloat, n, "lamb_moments", "p");
  dense(g, at::kFloat, n, "lamb_moments", "g");
  dense(m, at::kFloat, n, "lamb_moments", "m");
  dense(v, at::kFloat, n, "lamb_moments", "v");
  dense(partial, at::kFloat, 2 * (int64_t)t.nchunks, "lamb_moments", "partial");
  dense(tab, at::kFloat, dlmpi_lw_tab() + t.T, "lamb_moments", "tab");
  dense(clip, at::kFloat, 2, "lamb_moments", "clip");
  if (!(eps > 0)) fail("lamb_moments", "eps > 0");
  check(dlmpi_lamb_moments(ptr<float>(p), ptr<float>(g), ptr<float>(m), ptr<float>(v), ptr<int>(chunks), t.nchunks, n,
                           ptr<int>(flags), t.T, ptr<float>(partial), ptr<float>(tab), optr<float>(clip), b1, b2,
                           (float)eps, (float)wd, cur_stream()),
        "lamb_moments");
}
void lamb_update(at::Tensor p, const at::Tensor& m, const at::Tensor& v, const at::Tensor& chunks,
                 const at::Tensor& flags, int64_t extent, const at::Tensor& tab, double eps, double wd) {
  const int64_t n = p.numel();
  const LwTables t = lw_tables(chunks, flags, extent, n, "lamb_update");
  dense(p, at::kFloat, n, "lamb_update", "p");
  dense(m, at::kFloat, n, "lamb_update", "m");
  dense(v, at::kFloat, n, "lamb_update", "v");
  dense(tab, at::kFloat, dlmpi_lw_tab() + t.T, "lamb_update", "tab");
  if (!(eps > 0)) fail("lamb_update", "eps > 0");
  check(dlmpi_lamb_update(ptr<float>(p), ptr<float>(m), ptr<float>(v), ptr<int>(chunks), t.nchunks, n, ptr<int>(flags),
                          t.T, ptr<float>(tab), (float)eps, (float)wd, cur_stream()),
        "lamb_update");
}

// ---- weight EMA (ema.hip): e toward w over the flat masters, eb toward b over the flat BN statistics ----
bool overlaps(const at::Tensor& a, const at::Tensor& b) {
  const char *a0 = ptr<char>(a), *b0 = ptr<char>(b);
  return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
}
// the second range of both launches: both or neither, the same length, disjoint
int64_t second_range(const c10::optional<at::Tensor>& a, const c10::optional<at::Tensor>& b, const char* fn,
                     const char* an, const char* bn) {
  if (given(a) != given(b)) fail(fn, std::string(an) + " and " + bn + " come together");
  if (!given(a)) return 0;
  dense(*a, at::kFloat, a->numel(), fn, an);
  dense(*b, at::kFloat, a->numel(), fn, bn);
  if (a->numel() && overlaps(*a, *b)) fail(fn, std::string(an) + " overlaps " + bn);
  return a->numel();
}
void ema_update(at::Tensor e, const at::Tensor& w, const c10::optional<at::Tensor>& eb,
                const c10::optional<at::Tensor>& b, at::Tensor state, const c10::optional<at::Tensor>& skip_flag,
                const c10::optional<at::Tensor>& counter, int64_t every, bool warmup, double decay,
                bool advance) {
  const int64_t n = e.numel();
  dense(e, at::kFloat, n, "ema_update", "e");
  dense(w, at::kFloat, n, "ema_update", "w");
  if (n && overlaps(e, w)) fail("ema_update", "e overlaps w");
  const int64_t nb = second_range(eb, b, "ema_update", "eb", "b");
  shaped(state, at::kFloat, {8}, "ema_update", "state");
  if (state.device() != e.device()) fail("ema_update", "state must be on the device of e");
  dense(skip_flag, at::kFloat, 1, "ema_update", "skip_flag");
  dense(counter, at::kFloat, 1, "ema_update", "counter");
  if (every < 1 || every > (1 << 24)) fail("ema_update", "every must be in [1, 2^24]");
  if (!(decay >= 0.0 && decay < 1.0)) fail("ema_update", "decay must be in [0, 1)");
  check(dlmpi_ema_update(ptr<float>(e), ptr<float>(w), n, optr<float>(eb), optr<float>(b), nb, ptr<float>(state),
                         optr<float>(skip_flag), optr<float>(counter), (int)every, warmup ? 1 : 0, decay,
                         advance ? 1 : 0, cur_stream()),
        "ema_update");
}
void ema_swap(at::Tensor a, at::Tensor b, const c10::optional<at::Tensor>& a2, const c10::optional<at::Tensor>& b2) {
  const int64_t n = a.numel();
  dense(a, at::kFloat, n, "ema_swap", "a");
  dense(b, at::kFloat, n, "ema_swap", "b");
  if (n && overlaps(a, b)) fail("ema_swap", "a overlaps b");
  const int64_t n2 = second_range(a2, b2, "ema_swap", "a2", "b2");
  check(dlmpi_swap_f32(ptr<float>(a), ptr<float>(b), n, optr<float>(a2), optr<float>(b2), n2, cur_stream()),
        "ema_swap");
}
}  // namespace

void register_optim(pybind11::module& m) {
  m.def("sgd_step", &sgd_step);
  m.def("adam_step", &adam_step);
  m.def("grad_norm", &grad_norm);
  m.def("scale_", &scale_);
  m.def("seg_sumsq", &seg_sumsq);
  m.def("seg_finish", &seg_finish);
  m.def("lars_update", &lars_update);
  m.def("lamb_moments", &lamb_moments);
  m.def("lamb_update", &lamb_update);
  m.def("ema_update", &ema_update);
  m.def("ema_swap", &ema_swap);
  m.def("lw_chunk", []() { return dlmpi_lw_chunk(); });
  m.def("lw_tab", []() { return dlmpi_lw_tab(); });
}

}  // namespace dlmpi_ext
