// Backward convolutions: the data gradient (sub-pixel phases, streaming kernels, BN-backward
// epilogues), the split-K weight gradient and its deferred-reduction queue.
#include <c10/hip/HIPCachingAllocator.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "ops.h"

namespace dlmpi_ext {

using dlmpi::ConvArgs;
using dlmpi::ConvPhase;
using dlmpi::DgradStreamArgs;
using dlmpi::make_fastdiv;
using dlmpi::WgradArgs;

// dx[n, h, w, dxoff + c] = sum_{r,s,k} dy[n, (h+pad-r)/stride, (w+pad-s)/stride, k] * wT[c][r][s][k]  (+ res)
// as stride^2 dense sub-pixel phases.
//
// Optional BN-backward fusion (dx is the gradient of y = relu(BN(z)) [+ BN2(z2)]): the epilogue
// applies the ReLU mask [y > 0] before storing and emits per-tile partials
// [tiles][2|3][C] = {sum dx, sum dx*z [, sum dx*z2]}, returned (None without z).
c10::optional<at::Tensor> conv2d_dgrad_pro(const at::Tensor& dy, int N, int P, int Q, int K, int lddy, int dyoff,
                                       const at::Tensor& wT, int C, int R, int S, int stride, int pad, int H, int W,
                                       at::Tensor dx, int lddx, int dxoff, const c10::optional<at::Tensor>& res,
                                       int ldres, int resoff, const c10::optional<at::Tensor>& mask, int ldmask,
                                       int maskoff, const c10::optional<at::Tensor>& z, int ldz, int zoff,
                                       const c10::optional<at::Tensor>& z2, int ldz2, int z2off,
                                       const c10::optional<at::Tensor>& mscale,
                                       const c10::optional<at::Tensor>& mshift,
                                       const c10::optional<at::Tensor>& mbits, bool colsum, int pro,
                                       const c10::optional<at::Tensor>& pk0, const c10::optional<at::Tensor>& pk1,
                                       const c10::optional<at::Tensor>& pz, int ldpz, int pzoff,
                                       const c10::optional<at::Tensor>& bias) {
  require_gpu(dy, "dy");
  {
    DgradCheck c{N, P, Q, K, C, R, S, stride, pad, H, W, operand(dy, lddy, dyoff), operand(dx, lddx, dxoff),
                 operand(res, ldres, resoff), operand(mask, ldmask, maskoff), operand(z, ldz, zoff),
                 operand(z2, ldz2, z2off), (int64_t)wT.numel()};
    c.bias_numel = onumel(bias);
    c.mscale_numel = onumel(mscale);
    c.mshift_numel = onumel(mshift);
    c.mbits_numel = onumel(mbits);
    c.colsum = colsum;
    require_ok(check_dgrad_args(c));
  }
  if (bias.has_value() && bias->defined() && bias->scalar_type() != at::kFloat)
    throw std::runtime_error("conv2d_dgrad: bias must be fp32");
  ConvArgs a{};
  a.f32 = act_f32(dy, "conv2d_dgrad");
  same_type(dy, wT, "conv2d_dgrad wT");
  same_type(dy, dx, "conv2d_dgrad dx");
  same_type(dy, res, "conv2d_dgrad res");
  same_type(dy, mask, "conv2d_dgrad mask");
  same_type(dy, z, "conv2d_dgrad z");
  same_type(dy, z2, "conv2d_dgrad z2");
  a.x = ptr<uint16_t>(dy);
  a.H = P; a.W = Q; a.C = K; a.ldx = lddy; a.xoff = dyoff;
  a.w = ptr<uint16_t>(wT);
  a.ldw = R * S * K;
  a.S = S;
  a.OH = H; a.OW = W;
  a.so = stride; a.sa = 1;
  a.Nimg = N; a.Kout = C;
  fill_epilogue(a, dx, lddx, dxoff, bias, res, ldres, resoff, c10::nullopt, c10::nullopt, false, c10::nullopt);
  a.vec_store = ((lddx % 8) == 0 && (dxoff % 8) == 0) ? 1 : 0;
  a.mask = optr<uint16_t>(mask);
  a.ldmask = ldmask; a.maskoff = maskoff;
  a.z = optr<uint16_t>(z);
  a.ldz = ldz; a.zoff = zoff;
  a.z2 = optr<uint16_t>(z2);
  a.ldz2 = ldz2; a.z2off = z2off;
  a.mscale = optr<float>(mscale);
  a.mshift = optr<float>(mshift);
  a.mbits = optr<uint8_t>(mbits);
  a.nstat = a.z2 ? 3 : 2;
  if (a.z && !a.mask && !a.mscale && !a.mbits)
    throw std::runtime_error("conv2d_dgrad: fused BN statistics need the ReLU mask");
  if (a.mscale && (!a.z || !a.mshift)) throw std::runtime_error("conv2d_dgrad: mask from z needs z, scale, shift");
  if ((a.mask || a.mscale || a.mbits) && ((ldmask | maskoff | ldz | zoff | ldz2 | z2off) % 8 != 0 || !a.vec_store))
    throw std::runtime_error("conv2d_dgrad: fused BN tensors must be 8-channel aligned");
  g_ran.dgrad_stream = 0;
  g_ran.conv3 = 0;
  if (R == 1 && S == 1 && K == 8) g_ran.head_dgrad = 0;   // a padded-K head's data gradient through the GEMM
  {  // streaming 3x3 data gradient (conv3x3_stream.hip, 64 -> 64): a forward conv of dy with wT, taps flipped
    const int mode = a.mscale ? 2 : 0;
    int th, tw, G;
    if (stream3x3_shape(N, H, W, K, C, R, S, stride, pad, pro, a.f32, th, tw, G) && P == H && Q == W && !colsum &&
        !a.mask && !a.mbits && !a.z2 && !a.res && !a.bias && (a.z != nullptr) == (mode == 2) && a.vec_store &&
        a.kvalid == C && (lddy | dyoff) % 8 == 0 && (int64_t)H * W * lddx * 2 < (1ll << 31) &&
        dx.scalar_type() == at::kBFloat16) {
      dlmpi::Conv3StreamArgs c = conv3_args(dy, N, H, W, lddy, dyoff, wT, 1, a.y, lddx, dxoff, th, tw, G);
      c.z = static_cast<const uint16_t*>(a.z);
      c.ldz = ldz; c.zoff = zoff;
      c.mscale = a.mscale; c.mshift = a.mshift;
      c10::optional<at::Tensor> st;
      if (a.z) {
        st = at::empty({(int64_t)G, 2, (int64_t)C}, dy.options().dtype(at::kFloat));
        c.stats = ptr<float>(*st);
      }
      check(dlmpi_conv3x3_stream(&c, mode == 2 ? 2 : 1, cur_stream()), "conv2d_dgrad (stream 3x3)");
      g_ran.conv3 = 1;
      return st;
    }
  }
  {  // streaming 1x1 data gradient (conv1x1_dgrad_stream.hip): memory-bound GEMMs with a heavy epilogue
    const int64_t M = (int64_t)N * H * W;
    const int mode = a.mbits ? 1 : (a.mscale ? 2 : 0);
    int sbm, sbn, G;
    const auto fits = [](int64_t rows, int64_t ld) { return rows * ld < (1ll << 31); };
    if (R == 1 && S == 1 && stride == 1 && pad == 0 && !a.f32 && pro == 0 && !colsum && !a.mask &&
        (a.z != nullptr) == (mode != 0) && a.vec_store && a.kvalid == C && (lddy | dyoff) % 8 == 0 &&
        (!a.res || (ldres | resoff) % 8 == 0) && fits(M, lddy) && fits(M, lddx) && (!a.res || fits(M, ldres)) &&
        (!a.z || fits(M, ldz)) && (!a.z2 || fits(M, ldz2)) && dx.scalar_type() == at::kBFloat16 &&
        dlmpi_dgrad_stream_plan(M, K, C, mode, a.z2 ? 1 : 0, a.res ? 1 : 0, &sbm, &sbn, &G)) {
      DgradStreamArgs sa{};
      sa.x = ptr<uint16_t>(dy);
      sa.ldx = lddy; sa.xoff = dyoff;
      sa.w = ptr<uint16_t>(wT);
      sa.y = reinterpret_cast<uint16_t*>(a.y);
      sa.ldy = lddx; sa.yoff = dxoff;
      sa.y_bytes = (int)std::min<int64_t>(INT32_MAX, (int64_t)dx.numel() * 2);
      sa.M = (int)M; sa.K = K; sa.Kout = C;
      sa.bias = a.bias;
      sa.res = static_cast<const uint16_t*>(a.res);
      sa.ldres = ldres; sa.resoff = resoff;
      sa.z = static_cast<const uint16_t*>(a.z);
      sa.ldz = ldz; sa.zoff = zoff;
      sa.z2 = static_cast<const uint16_t*>(a.z2);
      sa.ldz2 = ldz2; sa.z2off = z2off;
      sa.mbits = a.mbits;
      sa.mscale = a.mscale; sa.mshift = a.mshift;
      sa.G = G; sa.ntiles = C / sbn; sa.mtiles = (int)ceil_div(M, sbm);
      c10::optional<at::Tensor> st;
      if (a.z) {
        st = at::empty({(int64_t)G, (int64_t)a.nstat, (int64_t)C}, dy.options().dtype(at::kFloat));
        sa.stats = ptr<float>(*st);
      }
      check(dlmpi_conv1x1_dgrad_stream(&sa, sbm, sbn, mode, cur_stream()), "conv2d_dgrad (stream 1x1)");
      g_ran.dgrad_stream = 1;
      return st;
    }
  }
  set_kstep(a, K);
  set_prologue(a, pro, pk0, pk1, pz, ldpz, pzoff);
  // the GEMM of one sub-pixel phase; halo tiles where the gradient's grid is the output's
  TileQuery q{(int64_t)N * H * W / (stride * stride), C, (int64_t)R * S * K / (stride * stride), K, R, S, stride, pad,
              H, W, a.f32, pro};
  q.halo_ok = P == H && Q == W;
  q.pipe_ok = g_sw.pipe_dgrad != 0;
  const Tiles t = select_tiles(q);
  int bm = t.bm, bn = t.bn;
  const int pipe = t.pipe;
  const bool halo = t.halo;
  a.ntiles = ceil_div(C, bn);
  a.nphase = stride * stride;
  int tiles = 0;
  for (int ph = 0; ph < stride; ++ph) {
    for (int pw = 0; pw < stride; ++pw) {
      ConvPhase& p = a.ph[ph * stride + pw];
      const int r0 = (ph + pad) % stride, s0 = (pw + pad) % stride;
      p.P = (H - ph + stride - 1) / stride;
      p.Q = (W - pw + stride - 1) / stride;
      p.Tr = r0 < R ? (R - r0 + stride - 1) / stride : 0;
      p.Ts = s0 < S ? (S - s0 + stride - 1) / stride : 0;
      p.dh0 = (ph + pad - r0) / stride; p.dhs = -1;
      p.dw0 = (pw + pad - s0) / stride; p.dws = -1;
      p.wr0 = r0; p.wrs = stride; p.ws0 = s0; p.wss = stride;
      p.oh0 = ph; p.ow0 = pw;
      finish_phase(p, N, K, bm, a.f32);
      p.tile_base = tiles;
      tiles += p.mtiles;
    }
  }
  if (halo) {
    apply_halo(a, N, bm);
    tiles = a.ph[0].mtiles;
  }
  g_ran.halo = halo ? 1 : 0;
  {  // autotuned tiling (statistics: a placeholder until the tile count is known -- the trials
     // write to scratch)
    const bool want_stats = a.z || colsum;
    a.stats = want_stats ? reinterpret_cast<float*>(static_cast<uintptr_t>(256)) : nullptr;
    if (!pipe && autotune(a, 1, bm, bn)) {
      tiles = 0;
      for (int i = 0; i < a.nphase; ++i) tiles += a.ph[i].mtiles;
    }
    a.stats = nullptr;
  }
  c10::optional<at::Tensor> stats;
  if (a.z || colsum) {
    // colsum without BN fusion: per-tile {sum dx, sum dx^2} of the stored gradient (UNet: the
    // column sums of the up-sampling slice are the ConvTranspose2d bias gradient).  The epilogue takes
    // them before it would add a residual, so check_dgrad_args refuses colsum together with res.
    stats = at::empty({(int64_t)tiles, (int64_t)a.nstat, (int64_t)C}, dy.options().dtype(at::kFloat));
    a.stats = ptr<float>(*stats);
  }
  if (g_sw.splitk > 0) a.splitk_req = g_sw.splitk;
  check(dlmpi_conv_igemm_ex(&a, bm, bn, pipe, cur_stream()), "conv2d_dgrad");
  return stats;
}

c10::optional<at::Tensor> conv2d_dgrad(const at::Tensor& dy, int N, int P, int Q, int K, int lddy, int dyoff,
                                       const at::Tensor& wT, int C, int R, int S, int stride, int pad, int H, int W,
                                       at::Tensor dx, int lddx, int dxoff, const c10::optional<at::Tensor>& res,
                                       int ldres, int resoff, const c10::optional<at::Tensor>& mask, int ldmask,
                                       int maskoff, const c10::optional<at::Tensor>& z, int ldz, int zoff,
                                       const c10::optional<at::Tensor>& z2, int ldz2, int z2off,
                                       const c10::optional<at::Tensor>& mscale,
                                       const c10::optional<at::Tensor>& mshift,
                                       const c10::optional<at::Tensor>& mbits, bool colsum) {
  return conv2d_dgrad_pro(dy, N, P, Q, K, lddy, dyoff, wT, C, R, S, stride, pad, H, W, dx, lddx, dxoff, res, ldres,
                          resoff, mask, ldmask, maskoff, z, ldz, zoff, z2, ldz2, z2off, mscale, mshift, mbits, colsum,
                          0, c10::nullopt, c10::nullopt, c10::nullopt, 0, 0, c10::nullopt);
}

// grad[ko][t][c] += sum_pix dy[pix][dyoff + ko] * x[gather(pix, t)][xoff + c]   (c < Creal, ko < Ko_real)
// dy is over the P x Q output grid of a conv (R x S, stride, pad) applied to x (H x W).
// Operand prologues: pro_a 2 -> the dy operand is dz = pcoef[0] dy + pcoef[1] Z + pcoef[2] (a deferred
// BN-backward apply, Z = the BN input); pro_b 1 -> the x operand is relu(x * pscale + pshift).
// ---- deferred weight-gradient split reductions --------------------------------------------------
// With set_wgrad_defer(1) (the engine backward) a weight gradient's split reduction is queued instead
// of launched; wgrad_flush() -- the DDP reducer before each bucket launch, the engine at the end of its
// backward, and a full queue (kWgradBatch entries) -- launches the queue as two batched kernels
// (conv_wgrad.hip wgrad_reduce_batch_s1/s2: the same sums in the same order as dlmpi_wgrad_reduce's
// two launches per gradient) on the current stream.  Queued entries keep their slab tensors alive; an entry queued on
// another stream is ordered before the flush by an event, and its slab's reuse by recordStream.
struct PendingReduce {
  at::Tensor ws;
  hipStream_t s;
  dlmpi::WgradReduceEntry e;
};
static std::vector<PendingReduce> g_pending;
static bool g_wgrad_defer = false;
static int g_wgrad_batch = dlmpi::kWgradBatch;   // queue length that triggers a flush (A/B: set_wgrad_batch)
static bool g_defer_direct = true;               // also queue the one-launch (G == 0) reductions (A/B)
static bool g_wgrad_bypass = false;              // reduce the next weight gradients immediately, queue kept
static int64_t g_reduce_launches = 0;   // reduction launches (either form), for tests / bench

// Launches the queue.  The queue is moved out first: if a launch throws midway, the batches already
// launched are not launched (and added into the gradients) a second time by a later flush, and the
// rest are dropped with the step that failed.
void wgrad_flush() {
  if (g_pending.empty()) return;
  std::vector<PendingReduce> pending;
  pending.swap(g_pending);
  const hipStream_t cur = cur_stream();
  std::vector<hipStream_t> waited;
  for (auto& p : pending) {
    if (p.s == cur) continue;
    if (std::find(waited.begin(), waited.end(), p.s) == waited.end()) {
      hipEvent_t ev;
      check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "wgrad_flush event");
      check(hipEventRecord(ev, p.s), "wgrad_flush record");
      check(hipStreamWaitEvent(cur, ev, 0), "wgrad_flush wait");
      check(hipEventDestroy(ev), "wgrad_flush event");
      waited.push_back(p.s);
    }
    c10::hip::HIPCachingAllocator::recordStream(p.ws.storage().data_ptr(), c10::hip::getCurrentHIPStream());
  }
  dlmpi::WgradReduceBatch b{};
  bool two = false;
  for (size_t i = 0; i < pending.size(); ++i) {
    const dlmpi::WgradReduceEntry& e = pending[i].e;
    two |= e.splits > 1 && dlmpi_wgrad_reduce_groups(e.splits, e.total) > 0;
    b.e[b.n++] = e;
    if (b.n == g_wgrad_batch || i + 1 == pending.size()) {
      check(dlmpi_wgrad_reduce_batch(&b, cur), "wgrad_reduce_batch");
      g_reduce_launches += two ? 2 : 1;
      b.n = 0;
      two = false;
    }
  }
}

// Drops the queue without launching it and turns deferral off: the backward that queued it failed
// (e.g. a hipGraph capture torn down mid-backward: its slabs were never computed and its streams are
// abandoned).  The engine's error path and CapturedStep's stream reset call it.
void wgrad_discard() {
  g_pending.clear();
  g_wgrad_defer = false;
  g_wgrad_bypass = false;
}

// the split reduction of a weight gradient: ws = [splits + G][wsz] (G = dlmpi_wgrad_reduce_groups)
static void wgrad_reduce_or_defer(const at::Tensor& ws, int splits, int G, int64_t wsz, int Ko, int T, int Cpad,
                                  int Creal, int Ko_real, at::Tensor& grad) {
  float* out = ptr<float>(grad);
  for (const auto& p : g_pending)   // a gradient accumulated twice: its first sum goes out first
    if (p.e.out == out) {
      wgrad_flush();
      break;
    }
  if (!g_wgrad_defer || g_wgrad_bypass || (!g_defer_direct && !(splits > 1 && G > 0))) {
    check(dlmpi_wgrad_reduce(ptr<float>(ws), splits, Ko, T, Cpad, Creal, Ko_real, out, ptr<float>(ws) + (int64_t)splits * wsz,
                             (int)std::min<int64_t>(INT32_MAX, (int64_t)G * wsz), cur_stream()),
          "wgrad_reduce");
    g_reduce_launches += splits > 1 && G > 0 ? 2 : 1;
    return;
  }
  if (Ko_real == 0 || wsz == 0) return;
  PendingReduce p{ws, cur_stream(), {}};
  p.e.ws = ptr<float>(ws);
  p.e.ws2 = G > 0 ? ptr<float>(ws) + (int64_t)splits * wsz : nullptr;
  p.e.out = out;
  p.e.total = (int64_t)Ko * T * Cpad;
  p.e.splits = splits;
  p.e.Ko_real = Ko_real;
  p.e.T = T;
  p.e.Cpad = Cpad;
  p.e.Creal = Creal;
  g_pending.push_back(std::move(p));
  if ((int)g_pending.size() >= g_wgrad_batch) wgrad_flush();
}

void conv2d_wgrad_pro(const at::Tensor& dy, int lddy, int dyoff, int Ko, const at::Tensor& x, int N, int H, int W,
                      int C, int ldx, int xoff, int R, int S, int stride, int pad, int P, int Q, at::Tensor grad,
                      int Creal, int Ko_real, int pro_a, const c10::optional<at::Tensor>& pcoef,
                      const c10::optional<at::Tensor>& pz, int ldpz, int pzoff, int pro_b,
                      const c10::optional<at::Tensor>& pscale, const c10::optional<at::Tensor>& pshift) {
  require_gpu(dy, "dy");
  require_ok(check_wgrad_args(WgradCheck{N, H, W, C, Ko, R, S, stride, pad, P, Q, Creal, Ko_real, operand(dy, lddy, dyoff),
                                         operand(x, ldx, xoff), (int64_t)grad.numel()}));
  if (grad.scalar_type() != at::kFloat) throw std::runtime_error("conv2d_wgrad: the gradient must be fp32");
  if (C % 8 != 0 || Ko % 8 != 0) throw std::runtime_error("conv2d_wgrad: channels must be multiples of 8");
  WgradArgs a{};
  a.f32 = act_f32(dy, "conv2d_wgrad");
  same_type(dy, x, "conv2d_wgrad x");
  if (a.f32 && (pro_a || pro_b)) throw std::runtime_error("conv2d_wgrad: operand prologues are bf16 only");
  a.pro_a = pro_a;
  a.pro_b = pro_b;
  if (pro_a) {
    a.pcoef = optr<float>(pcoef);
    a.pz = optr<uint16_t>(pz);
    a.ldpz = ldpz;
    a.pzoff = pzoff;
    if (pro_a != 2 || !a.pcoef || !a.pz || pcoef->numel() < 3 * Ko || (ldpz | pzoff) % 8)
      throw std::runtime_error("conv2d_wgrad: prologue a needs coef [3][Ko] and an aligned Z");
  }
  if (pro_b) {
    a.pscale = optr<float>(pscale);
    a.pshift = optr<float>(pshift);
    if (pro_b != 1 || !a.pscale || !a.pshift || pscale->numel() < C || pshift->numel() < C)
      throw std::runtime_error("conv2d_wgrad: prologue b needs scale / shift of C channels");
  }
  // 3x3 / stride 1 / pad 1 without operand prologues (UNet DoubleConv, ResNet conv2): the
  // spatial-tile kernel (conv_wgrad3.hip) -- X staged once per 8 x 8 pixel block for all 9 taps.
  int kt = 0, ct = 0;
  // Only where the 8 x 8 blocks are at least 3/4 full: 14^2 / 7^2 are (77 %), the 4^2 / 2^2 / 1^2 images
  // of ResNet-18 on 32^2 CIFAR are not (25 % / 6 % / 2 %) and take the gather kernel.
  const bool w3_full = 4 * H * W >= 3 * ceil_div(H, 8) * 8 * ceil_div(W, 8) * 8;
  if (g_sw.wgrad3 != 0 && (w3_full || g_sw.wgrad3 == 1) && !a.f32 && pro_a == 0 && pro_b == 0 &&
      R == 3 && S == 3 && stride == 1 && pad == 1 && P == H && Q == W && dlmpi_wgrad3_plan(Ko, C, &kt, &ct)) {
    dlmpi::Wgrad3Args b{};
    b.dy = ptr<uint16_t>(dy);
    b.ldy = lddy; b.dyoff = dyoff; b.Ko = Ko;
    b.x = ptr<uint16_t>(x);
    b.ldx = ldx; b.xoff = xoff; b.C = C;
    b.H = H; b.W = W;
    b.tiles_h = ceil_div(H, 8);
    b.tiles_w = ceil_div(W, 8);
    b.ntiles_pix = N * b.tiles_h * b.tiles_w;
    b.mtiles = Ko / kt;
    b.ntiles = C / ct;
    // one 512-thread block per CU (252 VGPRs: 2 waves per SIMD take a SIMD's whole register file,
    // so nothing of the data-gradient chain on the main stream can share a CU with it).  Large
    // gradients (UNet, >= 64 G MAC) fill the chip once; the ResNet-size ones (~30 G MAC) leave ~100
    // CUs to the main stream (measured, profiles/r3_wgrad3: ResNet-50 12,233 img/s at 256 blocks vs
    // 12,348 at 160; UNet-512 470 vs 466).
    const double macs = (double)N * H * W * Ko * 9.0 * C;
    // (UNet-size gradients: 224 blocks leave 32 CUs to the data-gradient chain's small kernels, which
    // otherwise wait for the whole kernel -- UNet-512 +0.65 %, UNet-1024 +0.4 % over 256, 5 same-box
    // pairs, profiles/r4_unet)
    // (64 x 64 tiles are 4-wave blocks, two per CU: twice the blocks for the same CUs)
    const int target = (g_sw.wgrad3_blocks > 0 ? g_sw.wgrad3_blocks : (macs >= 64e9 ? 224 : 160)) * (kt == 64 && ct == 64 ? 2 : 1);
    const int kc = b.mtiles * b.ntiles;
    int splits = std::max(1, std::min(b.ntiles_pix, target / kc));
    b.tiles_per_split = ceil_div(b.ntiles_pix, splits);
    splits = ceil_div(b.ntiles_pix, b.tiles_per_split);
    b.splits = splits;
    const int64_t wsz = (int64_t)Ko * 9 * C;
    const int G = splits > 1 ? dlmpi_wgrad_reduce_groups(splits, wsz) : 0;
    at::Tensor ws = at::empty({(int64_t)(splits + G) * wsz}, dy.options().dtype(at::kFloat));
    b.ws = ptr<float>(ws);
    g_ran.wgrad3 = 1;
    check(dlmpi_wgrad3x3(&b, kt, ct, cur_stream()), "conv2d_wgrad (3x3 tiles)");
    wgrad_reduce_or_defer(ws, splits, G, wsz, Ko, 9, C, Creal, Ko_real, grad);
    return;
  }
  g_ran.wgrad3 = 0;
  a.dy = ptr<uint16_t>(dy);
  a.ldy = lddy; a.dyoff = dyoff; a.Ko = Ko;
  a.x = ptr<uint16_t>(x);
  a.H = H; a.W = W; a.C = C; a.ldx = ldx; a.xoff = xoff;
  a.Nimg = N; a.P = P; a.Q = Q; a.S = S;
  a.stride_h = stride; a.stride_w = stride; a.pad_h = pad; a.pad_w = pad;
  a.TC = R * S * C;
  a.npix = N * P * Q;
  a.direct = (R == 1 && S == 1 && stride == 1 && pad == 0 && P == H && Q == W) ? 1 : 0;
  if (!dlmpi_wgrad_pro_ok(a.direct, pro_a, pro_b))
    throw std::runtime_error("conv2d_wgrad: operand prologues: one of them, x's only for 1x1 gradients");
  const int bm = a.f32 || Ko <= 64 ? 64 : 128;   // fp32: conv_wgrad_f32_kernel's 64 x 64 tile
  a.mtiles = ceil_div(Ko, bm);
  // Ko <= 64 gather-form (3x3 / strided / stem) weight gradients: 64 x 256 tiles (1 x 4 waves of
  // 64 x 64) -- each dy row staged once per 256 columns, fewer LDS reads per MFMA.  The tile holds
  // ~200 VGPRs (2 blocks per CU), so its split count is floored to fit the grid in one round
  // (profiles/r2_wgrad_wide).  Gather-form only (1x1s measured no gain).
  const bool w256 = !a.f32 && Ko <= 64 && pro_b == 0 && a.TC >= 256 && !a.direct;
  const int bn = a.f32 ? 64 : (w256 ? 256 : 128);
  a.ntiles = ceil_div(a.TC, bn);
  const int tiles = a.mtiles * a.ntiles;
  // split the pixel reduction so the grid covers the chip ~2 blocks deep, but keep each split at
  // least 8 K-steps (512 pixels) so the fp32 slab traffic stays small next to the MFMA work.
  // target grid size (the weight gradients share the GPU with the data-gradient
  // chain on another stream, so they need not fill it alone)
  const int target_blocks = g_sw.wgrad_blocks > 0 ? g_sw.wgrad_blocks : 512;
  const int maxsplit = std::max(1, ceil_div(a.npix, 512));
  int splits = std::max(1, std::min(maxsplit, w256 ? target_blocks / tiles : ceil_div(target_blocks, tiles)));
  int pps = ceil_div(a.npix, splits);
  pps = ceil_div(pps, 64) * 64;
  splits = ceil_div(a.npix, pps);
  a.splits = splits;
  a.pix_per_split = pps;
  a.fdPQ = make_fastdiv((uint32_t)(P * Q));
  a.fdQ = make_fastdiv((uint32_t)Q);
  a.fdC = make_fastdiv((uint32_t)C);
  a.fdS = make_fastdiv((uint32_t)S);
  const int64_t wsz = (int64_t)Ko * a.TC;
  const int G = splits > 1 ? dlmpi_wgrad_reduce_groups(splits, wsz) : 0;
  at::Tensor ws = at::empty({(int64_t)(splits + G) * wsz}, dy.options().dtype(at::kFloat));
  a.ws = ptr<float>(ws);
  check(dlmpi_conv_wgrad(&a, bm, bn, cur_stream()), "conv2d_wgrad");
  wgrad_reduce_or_defer(ws, splits, G, wsz, Ko, R * S, C, Creal, Ko_real, grad);
}

void conv2d_wgrad(const at::Tensor& dy, int lddy, int dyoff, int Ko, const at::Tensor& x, int N, int H, int W, int C,
                  int ldx, int xoff, int R, int S, int stride, int pad, int P, int Q, at::Tensor grad, int Creal,
                  int Ko_real) {
  conv2d_wgrad_pro(dy, lddy, dyoff, Ko, x, N, H, W, C, ldx, xoff, R, S, stride, pad, P, Q, grad, Creal, Ko_real, 0,
                   c10::nullopt, c10::nullopt, 0, 0, 0, c10::nullopt, c10::nullopt);
}

void register_conv_bwd(pybind11::module& m) {
  m.def("conv2d_dgrad", &conv2d_dgrad);
  m.def("conv2d_dgrad_pro", &conv2d_dgrad_pro);
  m.def("conv2d_wgrad", &conv2d_wgrad);
  m.def("conv2d_wgrad_pro", &conv2d_wgrad_pro);
  // check_dgrad_args / check_wgrad_args on plain integers (tests, no GPU): "" or the refusal the entry
  // point would throw.  Element counts of absent operands: -1.
  namespace py = pybind11;
  m.def(
      "conv2d_dgrad_check",
      [](int N, int P, int Q, int K, int C, int R, int S, int stride, int pad, int H, int W, int64_t dy_numel, int lddy,
         int dyoff, int64_t wT_numel, int64_t dx_numel, int lddx, int dxoff, int64_t res_numel, int ldres, int resoff,
         int64_t mask_numel, int ldmask, int maskoff, int64_t z_numel, int ldz, int zoff, int64_t z2_numel, int ldz2,
         int z2off, int64_t mscale_numel, int64_t mshift_numel, int64_t mbits_numel, int64_t bias_numel, bool colsum) {
        DgradCheck c{N, P, Q, K, C, R, S, stride, pad, H, W, Operand{dy_numel, lddy, dyoff},
                     Operand{dx_numel, lddx, dxoff}, Operand{res_numel, ldres, resoff},
                     Operand{mask_numel, ldmask, maskoff}, Operand{z_numel, ldz, zoff}, Operand{z2_numel, ldz2, z2off},
                     wT_numel};
        c.bias_numel = bias_numel;
        c.mscale_numel = mscale_numel;
        c.mshift_numel = mshift_numel;
        c.mbits_numel = mbits_numel;
        c.colsum = colsum;
        return check_dgrad_args(c);
      },
      py::arg("N"), py::arg("P"), py::arg("Q"), py::arg("K"), py::arg("C"), py::arg("R"), py::arg("S"),
      py::arg("stride"), py::arg("pad"), py::arg("H"), py::arg("W"), py::arg("dy_numel"), py::arg("lddy"),
      py::arg("dyoff"), py::arg("wT_numel"), py::arg("dx_numel"), py::arg("lddx"), py::arg("dxoff"),
      py::arg("res_numel") = -1, py::arg("ldres") = 0, py::arg("resoff") = 0, py::arg("mask_numel") = -1,
      py::arg("ldmask") = 0, py::arg("maskoff") = 0, py::arg("z_numel") = -1, py::arg("ldz") = 0, py::arg("zoff") = 0,
      py::arg("z2_numel") = -1, py::arg("ldz2") = 0, py::arg("z2off") = 0, py::arg("mscale_numel") = -1,
      py::arg("mshift_numel") = -1, py::arg("mbits_numel") = -1, py::arg("bias_numel") = -1,
      py::arg("colsum") = false);
  m.def(
      "conv2d_wgrad_check",
      [](int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad, int P, int Q, int Creal, int Ko_real,
         int64_t dy_numel, int lddy, int dyoff, int64_t x_numel, int ldx, int xoff, int64_t grad_numel) {
        return check_wgrad_args(WgradCheck{N, H, W, C, Ko, R, S, stride, pad, P, Q, Creal, Ko_real,
                                           Operand{dy_numel, lddy, dyoff}, Operand{x_numel, ldx, xoff}, grad_numel});
      },
      py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("Ko"), py::arg("R"), py::arg("S"),
      py::arg("stride"), py::arg("pad"), py::arg("P"), py::arg("Q"), py::arg("Creal"), py::arg("Ko_real"),
      py::arg("dy_numel"), py::arg("lddy"), py::arg("dyoff"), py::arg("x_numel"), py::arg("ldx"), py::arg("xoff"),
      py::arg("grad_numel"));
  m.def("set_wgrad_defer", [](bool on) {
    if (!on) wgrad_flush();
    g_wgrad_defer = on;
  });
  m.def("wgrad_flush", &wgrad_flush);
  m.def("wgrad_discard", &wgrad_discard);
  m.def("set_wgrad_batch", [](int n) { g_wgrad_batch = n > 0 && n <= dlmpi::kWgradBatch ? n : dlmpi::kWgradBatch; });
  m.def("set_defer_direct", [](int on) { g_defer_direct = on != 0; });
  m.def("set_wgrad_bypass", [](bool on) { g_wgrad_bypass = on; });
  m.def("wgrad_pending", []() { return (int)g_pending.size(); });
  m.def("wgrad_reduce_launches", []() { return g_reduce_launches; });
  m.def("set_dgrad_stream", [](int mode) { dlmpi_set_dgrad_stream(mode); });
  m.def("set_wgrad_fast", [](int on) { dlmpi_set_wgrad_fast(on); });
  def_int(m, "set_conv_pipe_dgrad", nullptr, &g_sw.pipe_dgrad);
  def_int(m, "set_wgrad3", nullptr, &g_sw.wgrad3);
  def_int(m, nullptr, "wgrad3_last", &g_ran.wgrad3);
  def_int(m, "set_wgrad3_blocks", nullptr, &g_sw.wgrad3_blocks);
  def_int(m, "set_wgrad_blocks", nullptr, &g_sw.wgrad_blocks);
  def_int(m, nullptr, "dgrad_stream_last", &g_ran.dgrad_stream);
  def_int(m, nullptr, "head_dgrad_last", &g_ran.head_dgrad);
}

}  // namespace dlmpi_ext
