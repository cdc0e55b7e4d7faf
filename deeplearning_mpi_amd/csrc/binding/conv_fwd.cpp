// Forward convolutions: the planned launch (conv_plan.h) with its BN-statistics / finalize variants,
// the fused BN-apply consumers, the 1x1 head, ConvTranspose2d(2, 2) and the tile autotuner.
// Every function launches on the current HIP stream and never synchronises, so a whole training
// step can be captured into a hipGraph.
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "common.h"

namespace dlmpi_ext {

using dlmpi::ConvArgs;
using dlmpi::ConvPhase;
using dlmpi::FinArgs;
using dlmpi::Stream1x1Args;
using dlmpi::make_fastdiv;

// Switch a fully set-up single-phase launch (bm 128 / 256) to halo tiles: its M-tiles (and stats rows)
// become N x tiles_h x tiles_w.
void apply_halo(ConvArgs& a, int N, int bm) {
  ConvPhase& p = a.ph[0];
  int th = 8, tw = 16, tiles_h = 1, tiles_w = 1;
  halo_geom(p.P, p.Q, bm, th, tw, tiles_h, tiles_w);
  a.halo = 1;
  a.th = th;
  a.tw = tw;
  a.tiles_h = tiles_h;
  a.tiles_w = tiles_w;
  a.fd_tw = make_fastdiv((uint32_t)tw);
  a.fd_tilesw = make_fastdiv((uint32_t)tiles_w);
  a.fd_thw = make_fastdiv((uint32_t)(tiles_h * tiles_w));
  p.mtiles = N * tiles_h * tiles_w;
  p.tile_base = 0;
}

// ---- conv tile autotuner ("benchmark mode", the reference's cudnn.benchmark = True,
// pytorch/resnet/main.py:29) ------------------------------------------------------------------------
// At batch 256 most ResNet-50 layers quantize badly on 256 CUs (784 tiles of a 14^2 layer on 768
// resident-block slots take two tile-times).  The first time a (conv, pass, epilogue) signature is
// launched outside a hipGraph capture, every valid (BM, BN, split-K) plan is timed on the real
// operands with the device otherwise idle and the fastest is cached for the process; later calls
// (and captures) use the cached plan.  Outputs are overwritten by every trial (the epilogues are
// idempotent; BN partials go to a scratch buffer), so the call's result is the chosen plan's.
// (conv_plan.cpp conv_autotune_on: the switch and why it defaults to off.)
static std::map<std::string, TuneCand> g_conv_plans;

static std::string conv_key(const ConvArgs& a, int pass) {
  std::string k = std::to_string(pass);
  auto add = [&](int64_t v) { k += ',' + std::to_string(v); };
  add(a.f32); add(a.Nimg); add(a.H); add(a.W); add(a.C); add(a.ldx); add(a.Kout); add(a.ldw); add(a.S);
  add(a.OH); add(a.OW); add(a.ldy); add(a.so); add(a.sa); add(a.nphase); add(a.kvalid); add(a.vec_store);
  add(a.out_f32); add(a.bias != nullptr); add(a.res != nullptr); add(a.scale != nullptr); add(a.relu);
  add(a.stats != nullptr); add(a.nstat); add(a.mask != nullptr); add(a.mscale != nullptr); add(a.mbits != nullptr);
  add(a.z != nullptr); add(a.z2 != nullptr); add(a.pro);
  for (int i = 0; i < a.nphase; ++i) {
    const ConvPhase& p = a.ph[i];
    add(p.P); add(p.Q); add(p.Tr); add(p.Ts); add(p.dh0); add(p.dw0); add(p.wr0); add(p.ws0);
  }
  return k;
}

// (re)tile a fully set-up launch for BM x BN: M-tiles and stats bases of every phase
static int apply_tiles(ConvArgs& a, int bm, int bn) {
  a.ntiles = ceil_div(a.Kout, bn);
  int t = 0;
  for (int i = 0; i < a.nphase; ++i) {
    ConvPhase& p = a.ph[i];
    p.mtiles = ceil_div((int64_t)a.Nimg * p.P * p.Q, bm);
    p.tile_base = t;
    t += p.mtiles;
  }
  return t;
}

// Plan for a fully set-up (default-tiled) launch: the cached one, or tune now.  Returns false if
// autotuning does not apply (the caller keeps its static plan).
bool autotune(ConvArgs& a, int pass, int& bm, int& bn) {
  if (!conv_autotune_on() || a.pro != 0 || a.halo) return false;
  // trials re-run the launch: an output that is also one of its inputs (in-place residual / mask /
  // z) would be transformed once per trial -- keep the static plan there
  const void* y = a.y;
  if (y == a.x || y == a.res || y == a.z || y == a.z2 || y == a.mask) return false;
  const std::string key = conv_key(a, pass);
  auto it = g_conv_plans.find(key);
  if (it == g_conv_plans.end()) {
    hipStream_t st = cur_stream();
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
    int maxk = 0;
    for (int i = 0; i < a.nphase; ++i) maxk = std::max(maxk, a.ph[i].ksteps);
    const std::vector<TuneCand> cands = tune_candidates(a.f32, a.C, a.Kout, maxk);
    // BN partials of the trials: scratch rows for the smallest tile
    at::Tensor scratch;
    float* real_stats = a.stats;
    if (a.stats) {
      ConvArgs t = a;
      const int rows = apply_tiles(t, 64, 64);
      scratch = at::empty({(int64_t)rows * a.nstat * a.Kout}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
    }
    check(hipDeviceSynchronize(), "autotune sync");
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    TuneCand best{bm, bn, 0};
    float best_ms = 1e30f;
    for (const TuneCand& c : cands) {
      ConvArgs t = a;
      apply_tiles(t, c.bm, c.bn);
      t.splitk_req = c.splitk_req;
      if (t.stats) t.stats = ptr<float>(scratch);
      if (dlmpi_conv_igemm(&t, c.bm, c.bn, st) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      hipEventRecord(e0, st);
      for (int r = 0; r < 3; ++r) (void)dlmpi_conv_igemm(&t, c.bm, c.bn, st);
      hipEventRecord(e1, st);
      if (hipEventSynchronize(e1) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      float ms = 0.f;
      hipEventElapsedTime(&ms, e0, e1);
      if (ms < best_ms) {
        best_ms = ms;
        best = c;
      }
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    a.stats = real_stats;
    if (getenv("DLMPI_CONV_AUTOTUNE") && atoi(getenv("DLMPI_CONV_AUTOTUNE")) == 2)
      fprintf(stderr, "[dlmpi autotune] pass %d %s -> %dx%d split %d (%.1f us; static %dx%d)\n", pass, key.c_str(),
              best.bm, best.bn, best.splitk_req, best_ms / 3 * 1000, bm, bn);
    it = g_conv_plans.emplace(key, best).first;
  }
  bm = it->second.bm;
  bn = it->second.bn;
  a.splitk_req = it->second.splitk_req;
  apply_tiles(a, bm, bn);
  return true;
}

void finish_phase(ConvPhase& p, int Nimg, int C, int bm, bool f32) {
  p.mtiles = ceil_div((int64_t)Nimg * p.P * p.Q, bm);
  p.ksteps = ceil_div((int64_t)p.Tr * p.Ts * C, f32 ? 32 : 64);
  if (p.Tr * p.Ts == 0) p.ksteps = 0;
  p.fdPQ = make_fastdiv((uint32_t)std::max(1, p.P * p.Q));
  p.fdQ = make_fastdiv((uint32_t)std::max(1, p.Q));
  p.fdTs = make_fastdiv((uint32_t)std::max(1, p.Ts));
}

void single_phase(ConvArgs& a, int P, int Q, int R, int S, int pad, int bm) {
  a.nphase = 1;
  ConvPhase& p = a.ph[0];
  p.P = P; p.Q = Q; p.Tr = R; p.Ts = S;
  p.dh0 = -pad; p.dhs = 1; p.dw0 = -pad; p.dws = 1;
  p.wr0 = 0; p.wrs = 1; p.ws0 = 0; p.wss = 1;
  p.oh0 = 0; p.ow0 = 0;
  finish_phase(p, a.Nimg, a.C, bm, a.f32);
}

// the gathered operand, weights and output grid of a forward conv
static ConvArgs fwd_args(const at::Tensor& x, const ConvShape& s, int ldx, int xoff, const at::Tensor& w) {
  ConvArgs a{};
  a.f32 = s.f32;
  a.x = ptr<uint16_t>(x);
  a.H = s.H; a.W = s.W; a.C = s.C; a.ldx = ldx; a.xoff = xoff;
  a.w = ptr<uint16_t>(w);
  a.ldw = s.R * s.S * s.C;
  a.S = s.S;
  a.OH = s.P(); a.OW = s.Q();
  a.so = 1; a.sa = s.stride;
  a.Nimg = s.N; a.Kout = s.K;
  return a;
}

void fill_epilogue(ConvArgs& a, at::Tensor& y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
                   const c10::optional<at::Tensor>& res, int ldres, int resoff,
                   const c10::optional<at::Tensor>& scale, const c10::optional<at::Tensor>& shift, bool relu,
                   const c10::optional<at::Tensor>& stats) {
  a.y = y.data_ptr();
  a.out_f32 = y.scalar_type() == at::kFloat ? 1 : 0;
  a.ldy = ldy;
  a.yoff = yoff;
  a.kvalid = a.Kout;
  a.bias = optr<float>(bias);
  a.res = optr<uint16_t>(res);
  a.ldres = ldres;
  a.resoff = resoff;
  a.scale = optr<float>(scale);
  a.shift = optr<float>(shift);
  a.relu = relu ? 1 : 0;
  a.stats = optr<float>(stats);
  a.nstat = 2;
}

// Extras of a pro-3 launch (conv2d_fwd_bn_apply sets them around the shared forward path).
struct Pro3Extra {
  const float* rscale;
  const float* rshift;
  uint16_t* y;
  int ldy, yoff;
  uint8_t* mbits;
};
static thread_local const Pro3Extra* g_pro3 = nullptr;

// Operand prologue of the gathered operand (ConvArgs::pro 3): (k0 scale, k1 shift, pz = residual) of
// the producer block's BN-apply + residual + ReLU, computed and stored by the consumer's prologue.
void set_prologue(ConvArgs& a, int pro, const c10::optional<at::Tensor>& k0, const c10::optional<at::Tensor>& k1,
                  const c10::optional<at::Tensor>& pz, int ldpz, int pzoff) {
  a.pro = pro;
  if (pro == 0) return;
  if (pro != 3) throw std::runtime_error("conv prologue: mode 3 (the producer's pending BN-apply) or none");
  if (a.C < 64 || a.C % 64) throw std::runtime_error("conv prologue: channel count must be a multiple of 64");
  a.pscale = optr<float>(k0);
  a.pshift = optr<float>(k1);
  a.pz = optr<uint16_t>(pz);
  a.ldpz = ldpz;
  a.pzoff = pzoff;
  const Pro3Extra* e = g_pro3;
  if (!e || !a.pscale || !a.pshift || !a.pz || !e->y || !e->mbits || k0->numel() < a.C || k1->numel() < a.C ||
      (ldpz | pzoff | e->ldy | e->yoff) % 8 || ((e->rscale != nullptr) != (e->rshift != nullptr)) || a.f32)
    throw std::runtime_error("conv prologue 3: scale / shift, an aligned residual, y and mask bits required");
  a.prscale = e->rscale;
  a.prshift = e->rshift;
  a.py = e->y;
  a.ldpy = e->ldy;
  a.pyoff = e->yoff;
  a.pmbits = e->mbits;
}

dlmpi::Conv3StreamArgs conv3_args(const at::Tensor& x, int N, int H, int W, int ldx, int xoff, const at::Tensor& w,
                                  int flip, void* y, int ldy, int yoff, int th, int tw, int G) {
  dlmpi::Conv3StreamArgs c{};
  c.x = ptr<uint16_t>(x);
  c.ldx = ldx; c.xoff = xoff;
  c.w = ptr<uint16_t>(w);
  c.ldw = 9 * 64; c.flip = flip;
  c.y = reinterpret_cast<uint16_t*>(y);
  c.ldy = ldy; c.yoff = yoff;
  c.N = N; c.H = H; c.W = W;
  c.th = th; c.tw = tw;
  c.tiles_h = ceil_div(H, th);
  c.tiles_w = ceil_div(W, tw);
  c.ntiles = N * c.tiles_h * c.tiles_w;
  c.G = G;
  return c;
}

// The streaming 1x1 kernel's arguments: x [M][C] -> y [.][Kout] over an H x W input grid (strided
// and up-sampling launches set s2 / up2 on top).
static Stream1x1Args fill_stream1x1(const at::Tensor& x, int ldx, int xoff, const at::Tensor& w, at::Tensor& y,
                                    int ldy, int yoff, int64_t M, int C, int Kout, const float* bias, int H, int W,
                                    int P, int Q, int sbm, int sbn, int G) {
  Stream1x1Args sa{};
  sa.x = ptr<uint16_t>(x);
  sa.ldx = ldx; sa.xoff = xoff;
  sa.w = ptr<uint16_t>(w);
  sa.y = ptr<uint16_t>(y);
  sa.ldy = ldy; sa.yoff = yoff;
  sa.y_bytes = (int)std::min<int64_t>(INT32_MAX, (int64_t)y.numel() * 2);   // (UP2: per-tile descriptors)
  sa.M = (int)M; sa.C = C; sa.Kout = Kout;
  sa.bias = bias;
  sa.G = G; sa.ntiles = Kout / sbn; sa.mtiles = ceil_div(M, sbm);
  sa.H = H; sa.W = W;
  sa.fdPQ = make_fastdiv((uint32_t)(P * Q));
  sa.fdQ = make_fastdiv((uint32_t)Q);
  return sa;
}

// the training-BN finalize arguments of a conv's statistics
static FinArgs make_fin(double count, const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                        const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                        double momentum, double eps, at::Tensor& bnscale, at::Tensor& bnshift,
                        const c10::optional<at::Tensor>& save_mean, const c10::optional<at::Tensor>& save_invstd) {
  FinArgs f{};
  f.mode = 0;
  f.count = count;
  f.gamma = optr<float>(gamma);
  f.beta = optr<float>(beta);
  f.running_mean = optr<float>(running_mean);
  f.running_var = optr<float>(running_var);
  f.momentum = (float)momentum;
  f.eps = (float)eps;
  f.scale = ptr<float>(bnscale);
  f.shift = ptr<float>(bnshift);
  f.save_mean = optr<float>(save_mean);
  f.save_invstd = optr<float>(save_invstd);
  return f;
}

// the BN finalize of a forward conv's statistics [rows][2][K]
static void run_fin_after(const at::Tensor& stats, int rows, int K, const FinArgs* fin) {
  at::Tensor ws = colsum_ws(stats, rows, K);
  check(dlmpi_bn_finalize(ptr<float>(stats), rows, K, fin->count, fin->gamma, fin->beta, fin->running_mean,
                          fin->running_var, fin->momentum, fin->eps, fin->scale, fin->shift, fin->save_mean,
                          fin->save_invstd, ptr<double>(ws), cur_stream()),
        "bn_finalize");
}

// the sizes of a forward call, for check_fwd_args (conv_plan.h)
static FwdCheck fwd_check(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K,
                          int R, int S, int stride, int pad, const at::Tensor& y, int ldy, int yoff,
                          const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& res, int ldres,
                          int resoff, const c10::optional<at::Tensor>& scale, const c10::optional<at::Tensor>& shift,
                          const c10::optional<at::Tensor>& stats, int kvalid) {
  FwdCheck c{N, H, W, C, K, R, S, stride, pad, kvalid, operand(x, ldx, xoff), operand(y, ldy, yoff),
             operand(res, ldres, resoff), (int64_t)w.numel()};
  c.bias_numel = onumel(bias);
  c.scale_numel = onumel(scale);
  c.shift_numel = onumel(shift);
  if (stats.has_value() && stats->defined()) {
    c.stats_rows = stats->dim() > 0 ? stats->size(0) : 0;
    c.stats_cols = c.stats_rows > 0 ? stats->numel() / c.stats_rows : 0;
    c.stats_f32 = stats->scalar_type() == at::kFloat;
  }
  return c;
}

// y[n, p, q, yoff + k] = epilogue( sum_{r,s,c} x[n, p*stride - pad + r, q*stride - pad + s, xoff + c] * w[k][r][s][c] )
// fin (with stats): also finalize the BatchNorm over these statistics, by the standalone finalize
// right after the launch.  Returns the rows of the stats partial buffer the launch wrote.
static int conv2d_fwd_impl(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K, int R,
               int S, int stride, int pad, at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
               const c10::optional<at::Tensor>& res, int ldres, int resoff, const c10::optional<at::Tensor>& scale,
               const c10::optional<at::Tensor>& shift, bool relu, const c10::optional<at::Tensor>& stats, int bm_req,
               int kvalid, int bn_req, int pro, const c10::optional<at::Tensor>& pk0,
               const c10::optional<at::Tensor>& pk1, const c10::optional<at::Tensor>& pz, int ldpz, int pzoff,
               const FinArgs* fin) {
  require_gpu(x, "x");
  require_ok(check_fwd_args(fwd_check(x, N, H, W, C, ldx, xoff, w, K, R, S, stride, pad, y, ldy, yoff, bias, res, ldres,
                                      resoff, scale, shift, stats, kvalid)));
  const ConvShape s{N, H, W, C, K, R, S, stride, pad, pro, act_f32(x, "conv2d_fwd"), bm_req, bn_req};
  const int P = s.P(), Q = s.Q();
  same_type(x, w, "conv2d_fwd w");
  same_type(x, res, "conv2d_fwd res");
  ConvArgs a = fwd_args(x, s, ldx, xoff, w);
  fill_epilogue(a, y, ldy, yoff, bias, res, ldres, resoff, scale, shift, relu, stats);
  if (kvalid > 0 && kvalid < K) a.kvalid = kvalid;
  a.vec_store = (a.kvalid == a.Kout && (ldy % 8) == 0 && (yoff % 8) == 0) ? 1 : 0;
  set_kstep(a, C);
  set_prologue(a, pro, pk0, pk1, pz, ldpz, pzoff);
  const FwdOperands o{res.has_value(), scale.has_value(), relu, stats.has_value(), fin != nullptr, a.kvalid,
                      ldx, xoff, ldy, yoff, a.ldw, std::max(a.ldpz, a.ldpy), y.scalar_type() == at::kBFloat16,
                      y.scalar_type() == at::kFloat, w.scalar_type() == at::kBFloat16};
  const FwdPlan pl = plan_fwd(s, o);
  int bm = pl.bm, bn = pl.bn, rows = pl.rows;
  g_ran.stream = g_ran.conv3 = g_ran.head = g_ran.c8 = g_ran.c16 = 0;
  const auto need_rows = [&](int n) {
    if (fin != nullptr && (!a.stats || stats->size(0) < n))
      throw std::runtime_error("conv2d_fwd_bn: stats [mtiles][2][K] required");
    if (a.stats && stats->size(0) < n) throw std::runtime_error("conv2d_fwd: stats buffer too small");
  };
  if (pl.path < FwdPath::pipe) need_rows(rows);   // (the tiled launch: after the autotuner, below)
  switch (pl.path) {
    case FwdPath::c8:    // the UNet input conv: 8-channel image -> 64, 3x3
    case FwdPath::c16: {   // the ResNet stem (space-to-depth image, 16 channels -> 64, 4x4 taps)
      const bool c8 = pl.path == FwdPath::c8;
      check((c8 ? dlmpi_conv3x3_c8 : dlmpi_conv4x4_c16)(a.x, ldx, xoff, N, H, W, a.w, a.bias, a.y, ldy, yoff, a.stats,
                                                        pl.G, cur_stream()),
            c8 ? "conv2d_fwd (8-channel 3x3)" : "conv2d_fwd (stem 4x4 x 16 channels)");
      (c8 ? g_ran.c8 : g_ran.c16) = 1;
      break;
    }
    case FwdPath::head:
      check(dlmpi_head1x1(a.x, ldx, xoff, (int64_t)N * H * W, C, a.w, a.ldw, a.bias, a.y, ldy, yoff, a.kvalid,
                          o.y_f32 ? 1 : 0, nullptr, nullptr, cur_stream()),
            "conv2d_fwd (1x1 head)");
      g_ran.head = 1;
      return 0;
    case FwdPath::stream3x3: {
      dlmpi::Conv3StreamArgs c = conv3_args(x, N, H, W, ldx, xoff, w, 0, a.y, ldy, yoff, pl.th, pl.tw, pl.G);
      c.bias = a.bias;
      c.stats = a.stats;
      check(dlmpi_conv3x3_stream(&c, a.stats ? 0 : 1, cur_stream()), "conv2d_fwd (stream 3x3)");
      g_ran.conv3 = 1;
      break;
    }
    case FwdPath::stream1x1: {
      Stream1x1Args sa = fill_stream1x1(x, ldx, xoff, w, y, ldy, yoff, s.M(), C, K, a.bias, H, W, P, Q, pl.sbm,
                                        pl.sbn, pl.G);
      sa.stats = a.stats;
      sa.s2 = stride == 2 ? 1 : 0;
      check(dlmpi_conv1x1_stream(&sa, pl.sbm, pl.sbn, cur_stream()), "conv2d_fwd (stream 1x1)");
      g_ran.stream = 1;
      break;
    }
    case FwdPath::apply1x1:
      a.ntiles = ceil_div(K, bn);
      single_phase(a, P, Q, R, S, pad, bm);
      check(dlmpi_conv1x1_apply(&a, bm, cur_stream()), "conv2d_fwd (fused apply 1x1)");
      break;
    case FwdPath::pipe:
    case FwdPath::halo:
    case FwdPath::igemm:
      a.ntiles = ceil_div(K, bn);
      single_phase(a, P, Q, R, S, pad, bm);
      if (pl.path == FwdPath::halo) apply_halo(a, N, bm);
      g_ran.halo = pl.path == FwdPath::halo ? 1 : 0;
      // autotuned tiling: BN-stats launches only through conv2d_fwd_bn (its buffer is sized for the
      // largest row count, fwd_rows_bound, and its finalize uses the actual one)
      if (!pl.pipe && (fin != nullptr || !a.stats) && s.free_tiles() && autotune(a, 0, bm, bn)) rows = a.ph[0].mtiles;
      if (fin != nullptr) need_rows(rows);
      if (g_sw.splitk > 0) a.splitk_req = g_sw.splitk;
      check(dlmpi_conv_igemm_ex(&a, bm, bn, pl.pipe, cur_stream()), "conv2d_fwd");
      break;
  }
  if (fin != nullptr) run_fin_after(*stats, rows, K, fin);
  return rows;   // rows of the stats partial buffer
}

int conv2d_fwd_pro(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K, int R,
               int S, int stride, int pad, at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
               const c10::optional<at::Tensor>& res, int ldres, int resoff, const c10::optional<at::Tensor>& scale,
               const c10::optional<at::Tensor>& shift, bool relu, const c10::optional<at::Tensor>& stats, int bm_req,
               int kvalid, int bn_req, int pro, const c10::optional<at::Tensor>& pk0,
               const c10::optional<at::Tensor>& pk1, const c10::optional<at::Tensor>& pz, int ldpz, int pzoff) {
  return conv2d_fwd_impl(x, N, H, W, C, ldx, xoff, w, K, R, S, stride, pad, y, ldy, yoff, bias, res, ldres, resoff,
                         scale, shift, relu, stats, bm_req, kvalid, bn_req, pro, pk0, pk1, pz, ldpz, pzoff, nullptr);
}

int conv2d_fwd(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K, int R,
               int S, int stride, int pad, at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
               const c10::optional<at::Tensor>& res, int ldres, int resoff, const c10::optional<at::Tensor>& scale,
               const c10::optional<at::Tensor>& shift, bool relu, const c10::optional<at::Tensor>& stats, int bm_req,
               int kvalid, int bn_req) {
  return conv2d_fwd_pro(x, N, H, W, C, ldx, xoff, w, K, R, S, stride, pad, y, ldy, yoff, bias, res, ldres, resoff,
                        scale, shift, relu, stats, bm_req, kvalid, bn_req, 0, c10::nullopt, c10::nullopt,
                        c10::nullopt, 0, 0);
}

// conv2d_fwd_pro + the training BatchNorm finalize of its statistics (scale / shift / saved mean and
// invstd / running statistics).
int conv2d_fwd_bn(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K, int R,
                  int S, int stride, int pad, at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& bias,
                  const at::Tensor& stats, int pro, const c10::optional<at::Tensor>& pk0,
                  const c10::optional<at::Tensor>& pk1, const c10::optional<at::Tensor>& pz, int ldpz, int pzoff,
                  double count, const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                  const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                  double momentum, double eps, at::Tensor bnscale, at::Tensor bnshift,
                  const c10::optional<at::Tensor>& save_mean, const c10::optional<at::Tensor>& save_invstd) {
  const FinArgs f = make_fin(count, gamma, beta, running_mean, running_var, momentum, eps, bnscale, bnshift, save_mean,
                             save_invstd);
  return conv2d_fwd_impl(x, N, H, W, C, ldx, xoff, w, K, R, S, stride, pad, y, ldy, yoff, bias, c10::nullopt, 0, 0,
                         c10::nullopt, c10::nullopt, false, stats, 0, 0, 0, pro, pk0, pk1, pz, ldpz, pzoff, &f);
}

// conv2d_fwd_bn whose input is the PRODUCER's pending BN-apply: x = that BN's input z (scale, shift),
// res = its residual (rscale / rshift: a BN-output residual applied on the fly); the conv's operand
// prologue (pro 3) computes relu(z * scale + shift + res), consumes it AND stores it to yapp with
// its ReLU mask bits -- the standalone BN-apply pass and the consumer's re-read of its output go.
int conv2d_fwd_bn_apply(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w, int K,
                        at::Tensor z, int ldz, int zoff, const c10::optional<at::Tensor>& bias, const at::Tensor& stats,
                        const at::Tensor& ascale, const at::Tensor& ashift, const at::Tensor& res, int ldres,
                        int resoff, const c10::optional<at::Tensor>& rscale, const c10::optional<at::Tensor>& rshift,
                        at::Tensor yapp, int ldyapp, int yappoff, at::Tensor mbits, double count,
                        const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                        const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                        double momentum, double eps, at::Tensor bnscale, at::Tensor bnshift,
                        const c10::optional<at::Tensor>& save_mean, const c10::optional<at::Tensor>& save_invstd) {
  same_type(x, res, "conv2d_fwd_bn_apply res");
  same_type(x, yapp, "conv2d_fwd_bn_apply y");
  if (mbits.scalar_type() != at::kByte || mbits.numel() < (int64_t)N * H * W * (C / 8))
    throw std::runtime_error("conv2d_fwd_bn_apply: mask bits [pixels][C/8] uint8 required");
  Pro3Extra e{optr<float>(rscale), optr<float>(rshift), ptr<uint16_t>(yapp), ldyapp, yappoff, ptr<uint8_t>(mbits)};
  struct Scope {   // cleared on every way out
    explicit Scope(const Pro3Extra* p) { g_pro3 = p; }
    ~Scope() { g_pro3 = nullptr; }
  } scope(&e);
  return conv2d_fwd_bn(x, N, H, W, C, ldx, xoff, w, K, 1, 1, 1, 0, z, ldz, zoff, bias, stats, 3, ascale, ashift, res,
                       ldres, resoff, count, gamma, beta, running_mean, running_var, momentum, eps, bnscale, bnshift,
                       save_mean, save_invstd);
}

// conv2d_fwd_bn of a 3x3 / s1 / p1 64 -> 64 conv whose input is the producer's pending BN-apply + ReLU
// (no residual): x = that BN's input z, (ascale, ashift) its coefficients; the streaming kernel applies
// them to its staged halo and stores the applied input to yapp (each pixel once).  Returns the
// statistics rows (G), or -1 if the fused launch does not apply (conv3_pro_ok; the caller applies first).
int conv3x3_fwd_bn_apply(const at::Tensor& x, int N, int H, int W, int ldx, int xoff, const at::Tensor& w,
                         at::Tensor z, int ldz, int zoff, const c10::optional<at::Tensor>& bias, const at::Tensor& stats,
                         const at::Tensor& ascale, const at::Tensor& ashift, at::Tensor yapp, int ldyapp, int yappoff,
                         double count, const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                         const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                         double momentum, double eps, at::Tensor bnscale, at::Tensor bnshift,
                         const c10::optional<at::Tensor>& save_mean, const c10::optional<at::Tensor>& save_invstd) {
  require_gpu(x, "conv3x3_fwd_bn_apply x");
  if (act_f32(x, "conv3x3_fwd_bn_apply") || z.scalar_type() != at::kBFloat16 || yapp.scalar_type() != at::kBFloat16 ||
      !conv3_pro_ok(N, H, W, 64, 64, ldx, xoff, ldz, zoff, ldyapp, yappoff) || ascale.numel() < 64 ||
      ashift.numel() < 64)
    return -1;
  require_ok(check_fwd_args(fwd_check(x, N, H, W, 64, ldx, xoff, w, 64, 3, 3, 1, 1, z, ldz, zoff, bias, yapp, ldyapp,
                                      yappoff, c10::nullopt, c10::nullopt, stats, 0)));   // yapp: N*H*W x 64, like a residual
  int th, tw, G;
  stream3x3_shape(N, H, W, 64, 64, 3, 3, 1, 1, 0, 0, th, tw, G);
  if (stats.size(0) < G) throw std::runtime_error("conv3x3_fwd_bn_apply: stats buffer too small");
  dlmpi::Conv3StreamArgs c = conv3_args(x, N, H, W, ldx, xoff, w, 0, z.data_ptr(), ldz, zoff, th, tw, G);
  c.bias = optr<float>(bias);
  c.stats = ptr<float>(stats);
  c.psc = ptr<float>(ascale);
  c.psh = ptr<float>(ashift);
  c.py = ptr<uint16_t>(yapp);
  c.ldpy = ldyapp;
  c.pyoff = yappoff;
  check(dlmpi_conv3x3_stream(&c, 0, cur_stream()), "conv3x3_fwd_bn_apply");
  g_ran.conv3 = 1;
  const FinArgs f = make_fin(count, gamma, beta, running_mean, running_var, momentum, eps, bnscale, bnshift, save_mean,
                             save_invstd);
  run_fin_after(stats, G, 64, &f);
  return G;
}

// The 1x1 head (<= 4 outputs) over a deferred BN-apply + ReLU input relu(z * scale + shift) (the UNet's
// last decoder BN output, never stored): head.hip with the apply computed on the fly.
void conv1x1_head_affine(const at::Tensor& z, int N, int H, int W, int C, int ldz, int zoff, const at::Tensor& w,
                         int ldw, int kv, const at::Tensor& scale, const at::Tensor& shift, at::Tensor y, int ldy,
                         int yoff, const c10::optional<at::Tensor>& bias) {
  require_gpu(z, "z");
  if (act_f32(z, "conv1x1_head_affine") || !dlmpi_head1x1_ok(C, kv) || ldz % 8 || zoff % 8 ||
      scale.numel() < C || shift.numel() < C || (y.scalar_type() != at::kFloat && y.scalar_type() != at::kBFloat16))
    throw std::runtime_error("conv1x1_head_affine: bf16 z, C in 16..512, <= 4 outputs, aligned rows");
  if (ldw < C || w.numel() < (int64_t)(kv - 1) * ldw + C)
    throw std::runtime_error("conv1x1_head_affine: weight rows [kv][ldw] reach outside w");
  check(dlmpi_head1x1(z.data_ptr(), ldz, zoff, (int64_t)N * H * W, C, w.data_ptr(), ldw, optr<float>(bias),
                      y.data_ptr(), ldy, yoff, kv, y.scalar_type() == at::kFloat ? 1 : 0, ptr<float>(scale),
                      ptr<float>(shift), cur_stream()),
        "conv1x1_head_affine");
  g_ran.head = 1;
}

// Forward conv whose output is the gradient of y = relu(BN(z)) (a BN+ReLU without residual): the
// epilogue applies the ReLU mask [z * mscale + mshift > 0] before the store and emits that BN's
// backward partials [tiles][2][K] = {sum v, sum v*z}, returned.  (UNet: the ConvTranspose2d
// data-gradient -- a 2x2/s2 conv -- into the DoubleConv output below it.)
at::Tensor conv2d_fwd_bnbwd(const at::Tensor& x, int N, int H, int W, int C, int ldx, int xoff, const at::Tensor& w,
                            int K, int R, int S, int stride, int pad, at::Tensor y, int ldy, int yoff,
                            const at::Tensor& z, int ldz, int zoff, const at::Tensor& mscale,
                            const at::Tensor& mshift) {
  require_gpu(x, "x");
  {
    FwdCheck c = fwd_check(x, N, H, W, C, ldx, xoff, w, K, R, S, stride, pad, y, ldy, yoff, c10::nullopt, z, ldz, zoff,
                           mscale, mshift, c10::nullopt, 0);   // z: an N*P*Q x K operand like a residual
    require_ok(check_fwd_args(c));
  }
  const ConvShape s{N, H, W, C, K, R, S, stride, pad, 0, act_f32(x, "conv2d_fwd_bnbwd"), 0, 0};
  same_type(x, w, "conv2d_fwd_bnbwd w");
  same_type(x, z, "conv2d_fwd_bnbwd z");
  same_type(x, y, "conv2d_fwd_bnbwd y");
  ConvArgs a = fwd_args(x, s, ldx, xoff, w);
  fill_epilogue(a, y, ldy, yoff, c10::nullopt, c10::nullopt, 0, 0, c10::nullopt, c10::nullopt, false, c10::nullopt);
  a.vec_store = ((ldy % 8) == 0 && (yoff % 8) == 0) ? 1 : 0;
  a.z = ptr<uint16_t>(z);
  a.ldz = ldz; a.zoff = zoff;
  a.mscale = ptr<float>(mscale);
  a.mshift = ptr<float>(mshift);
  a.nstat = 2;
  if ((ldz | zoff) % 8 != 0 || !a.vec_store || K % 8)
    throw std::runtime_error("conv2d_fwd_bnbwd: fused BN tensors must be 8-channel aligned");
  set_kstep(a, C);
  TileQuery q{s.M(), K, s.red(), C, R, S, stride, pad, s.P(), s.Q(), s.f32, 0};
  q.halo_ok = false;   // (no halo variant of this epilogue)
  const Tiles t = select_tiles(q);
  a.ntiles = ceil_div(K, t.bn);
  single_phase(a, s.P(), s.Q(), R, S, pad, t.bm);
  at::Tensor stats = at::empty({(int64_t)a.ph[0].mtiles, 2, (int64_t)K}, x.options().dtype(at::kFloat));
  a.stats = ptr<float>(stats);
  if (g_sw.splitk > 0) a.splitk_req = g_sw.splitk;
  check(dlmpi_conv_igemm_ex(&a, t.bm, t.bn, t.pipe, cur_stream()), "conv2d_fwd_bnbwd");
  return stats;
}

// Number of BN-stat partial rows conv2d_fwd will produce at most (so the caller can size `stats`).
int conv2d_fwd_mtiles_pro(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int bm_req, int pro,
                          int f32) {
  return fwd_rows_bound(ConvShape{N, H, W, C, K, R, S, stride, pad, pro, f32, bm_req, 0});
}
int conv2d_fwd_mtiles(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int bm_req) {
  return conv2d_fwd_mtiles_pro(N, H, W, C, K, R, S, stride, pad, bm_req, 0, 0);
}

// plan_fwd, read-only (tests): the kernel, tiles and statistics rows of a forward launch with these
// operand facts (bf16 / fp32 storage throughout, as f32 says)
pybind11::dict conv2d_fwd_plan(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int pro, int f32,
                               int bm_req, int bn_req, bool has_res, bool has_scale, bool relu, bool has_stats,
                               bool has_fin, int kvalid, int ldx, int xoff, int ldy, int yoff) {
  const ConvShape s{N, H, W, C, K, R, S, stride, pad, pro, f32, bm_req, bn_req};
  const FwdOperands o{has_res, has_scale, relu, has_stats, has_fin, kvalid > 0 && kvalid < K ? kvalid : K,
                      ldx, xoff, ldy, yoff, R * S * C, pro == 3 ? ldx : 0, !f32, f32 != 0, !f32};
  const FwdPlan p = plan_fwd(s, o);
  pybind11::dict d;
  d["path"] = fwd_path_name(p.path);
  d["bm"] = p.bm; d["bn"] = p.bn; d["pipe"] = p.pipe; d["rows"] = p.rows;
  d["G"] = p.G; d["th"] = p.th; d["tw"] = p.tw; d["sbm"] = p.sbm; d["sbn"] = p.sbn;
  return d;
}

// ConvTranspose2d(k=2, s=2): y[n, 2h+i, 2w+j, yoff + co] = bias[co] + sum_ci x[n,h,w,ci] * wf[co][i][j][ci]
void convT2x2_fwd(const at::Tensor& x, int N, int H, int W, int Cin, int ldx, int xoff, const at::Tensor& wf, int Cout,
                  at::Tensor y, int ldy, int yoff, const c10::optional<at::Tensor>& bias) {
  require_gpu(x, "x");
  ConvArgs a{};
  a.f32 = act_f32(x, "convT2x2_fwd");
  same_type(x, wf, "convT2x2_fwd w");
  same_type(x, y, "convT2x2_fwd y");
  a.x = ptr<uint16_t>(x);
  a.H = H; a.W = W; a.C = Cin; a.ldx = ldx; a.xoff = xoff;
  a.w = ptr<uint16_t>(wf);
  a.ldw = 4 * Cin;
  a.S = 2;
  a.OH = 2 * H; a.OW = 2 * W;
  a.so = 2; a.sa = 1;
  a.Nimg = N; a.Kout = Cout;
  fill_epilogue(a, y, ldy, yoff, bias, c10::nullopt, 0, 0, c10::nullopt, c10::nullopt, false, c10::nullopt);
  a.vec_store = ((ldy % 8) == 0 && (yoff % 8) == 0) ? 1 : 0;
  set_kstep(a, Cin);
  g_ran.convT_stream = 0;
  {  // the streaming 1x1 kernel over 4 Cout columns (input read once for the four sub-pixel positions)
    const int64_t M = (int64_t)N * H * W;
    int sbm, sbn, G;
    // (output offsets are relative to each tile's first output row: any buffer size; input 32-bit)
    if (g_sw.convT_stream && !a.f32 && a.vec_store && ldx % 8 == 0 && xoff % 8 == 0 && M * ldx < (1ll << 31) &&
        4 * (int64_t)W * ldy * 2 * 4 < (1ll << 31) && 4 * M < (1ll << 31) &&
        dlmpi_stream1x1_plan(M, Cin, 4 * Cout, 1, &sbm, &sbn, &G) && Cout % sbn == 0) {
      Stream1x1Args sa = fill_stream1x1(x, ldx, xoff, wf, y, ldy, yoff, M, Cin, 4 * Cout, a.bias, H, W, H, W, sbm, sbn,
                                        G);
      sa.up2 = 1; sa.Cup = Cout;
      check(dlmpi_conv1x1_stream(&sa, sbm, sbn, cur_stream()), "convT2x2_fwd (stream)");
      g_ran.convT_stream = 1;
      return;
    }
  }
  TileQuery q{(int64_t)N * H * W, Cout, Cin, Cin, 1, 1, 1, 0, H, W, a.f32, 0};
  q.halo_ok = q.pipe_ok = q.wide1x1 = false;   // 4-phase convT: unmeasured at 256 rows
  const Tiles t = select_tiles(q);
  a.ntiles = ceil_div(Cout, t.bn);
  a.nphase = 4;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      ConvPhase& p = a.ph[i * 2 + j];
      p.P = H; p.Q = W; p.Tr = 1; p.Ts = 1;
      p.dh0 = 0; p.dhs = 0; p.dw0 = 0; p.dws = 0;
      p.wr0 = i; p.wrs = 0; p.ws0 = j; p.wss = 0;
      p.oh0 = i; p.ow0 = j;
      finish_phase(p, N, Cin, t.bm, a.f32);
    }
  check(dlmpi_conv_igemm(&a, t.bm, t.bn, cur_stream()), "convT2x2_fwd");
}

void register_conv_fwd(pybind11::module& m) {
  m.def("conv2d_fwd", &conv2d_fwd);
  m.def("conv2d_fwd_pro", &conv2d_fwd_pro);
  m.def("conv2d_fwd_bn", &conv2d_fwd_bn);
  m.def("conv2d_fwd_bn_apply", &conv2d_fwd_bn_apply);
  m.def("conv2d_fwd_mtiles", &conv2d_fwd_mtiles);
  m.def("conv2d_fwd_mtiles_pro", &conv2d_fwd_mtiles_pro);
  m.def("conv2d_fwd_plan", &conv2d_fwd_plan);
  // check_fwd_args on plain integers (tests, no GPU): "" or the refusal conv2d_fwd* would throw.
  // Element counts of absent operands: -1.
  m.def(
      "conv2d_fwd_check",
      [](int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int kvalid, int64_t x_numel, int ldx,
         int xoff, int64_t w_numel, int64_t y_numel, int ldy, int yoff, int64_t bias_numel, int64_t res_numel, int ldres,
         int resoff, int64_t scale_numel, int64_t shift_numel, int64_t stats_rows, int64_t stats_cols, bool stats_f32) {
        FwdCheck c{N, H, W, C, K, R, S, stride, pad, kvalid, Operand{x_numel, ldx, xoff}, Operand{y_numel, ldy, yoff},
                   Operand{res_numel, ldres, resoff}, w_numel};
        c.bias_numel = bias_numel;
        c.scale_numel = scale_numel;
        c.shift_numel = shift_numel;
        c.stats_rows = stats_rows;
        c.stats_cols = stats_cols;
        c.stats_f32 = stats_f32;
        return check_fwd_args(c);
      },
      pybind11::arg("N"), pybind11::arg("H"), pybind11::arg("W"), pybind11::arg("C"), pybind11::arg("K"),
      pybind11::arg("R"), pybind11::arg("S"), pybind11::arg("stride"), pybind11::arg("pad"),
      pybind11::arg("kvalid") = 0, pybind11::arg("x_numel"), pybind11::arg("ldx"), pybind11::arg("xoff"),
      pybind11::arg("w_numel"), pybind11::arg("y_numel"), pybind11::arg("ldy"), pybind11::arg("yoff"),
      pybind11::arg("bias_numel") = -1, pybind11::arg("res_numel") = -1, pybind11::arg("ldres") = 0,
      pybind11::arg("resoff") = 0, pybind11::arg("scale_numel") = -1, pybind11::arg("shift_numel") = -1,
      pybind11::arg("stats_rows") = -1, pybind11::arg("stats_cols") = 0, pybind11::arg("stats_f32") = true);
  m.def("conv_tune_tiles", [](int f32, int C, int K) {
    std::vector<std::pair<int, int>> v;
    for (const TuneCand& c : tune_candidates(f32, C, K, 0)) v.emplace_back(c.bm, c.bn);
    return v;
  });
  m.def("conv2d_fwd_bnbwd", &conv2d_fwd_bnbwd);
  m.def("convT2x2_fwd", &convT2x2_fwd);
  m.def("conv1x1_head_affine", &conv1x1_head_affine);
  m.def("conv3_pro_ok", &conv3_pro_ok);
  m.def("conv3x3_fwd_bn_apply", &conv3x3_fwd_bn_apply);
  m.def("clear_conv_plans", []() { g_conv_plans.clear(); });
  m.def("set_conv_stream", [](int mode) { dlmpi_set_conv_stream(mode); });
  m.def("set_conv3_stream", [](int mode) { dlmpi_set_conv3_stream(mode); });
  m.def("set_halo_pipe", [](int on) { dlmpi_set_halo_pipe(on); });
  m.def("set_dgs_blocks", [](int n) { dlmpi_set_dgs_blocks(n); });
  m.def("dgs_blocks", []() { return dlmpi_dgs_blocks(); });
  def_int(m, "set_conv_autotune", nullptr, &g_sw.autotune);
  def_int(m, "set_conv_halo", nullptr, &g_sw.halo);
  def_int(m, "set_halo_first", nullptr, &g_sw.halo_first);
  def_int(m, "set_conv_splitk", nullptr, &g_sw.splitk);
  def_int(m, "set_conv_pipe", nullptr, &g_sw.pipe);
  def_int(m, "set_conv_apply", nullptr, &g_sw.apply);
  def_int(m, "set_head1x1", "head1x1_on", &g_sw.head);
  def_int(m, "set_conv_c8", nullptr, &g_sw.c8);
  def_int(m, "set_conv_c16", nullptr, &g_sw.c16);
  def_int(m, "set_conv3_pro", nullptr, &g_sw.c3pro);
  def_int(m, "set_convT_stream", nullptr, &g_sw.convT_stream);
  def_int(m, nullptr, "conv_stream_last", &g_ran.stream);
  def_int(m, nullptr, "conv3_stream_last", &g_ran.conv3);
  def_int(m, nullptr, "conv_halo_last", &g_ran.halo);
  def_int(m, nullptr, "conv_c8_last", &g_ran.c8);
  def_int(m, nullptr, "conv_c16_last", &g_ran.c16);
  def_int(m, nullptr, "head1x1_last", &g_ran.head);
  def_int(m, nullptr, "convT_stream_last", &g_ran.convT_stream);
}

}  // namespace dlmpi_ext
