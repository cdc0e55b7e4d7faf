// Convolution launch planning (conv_plan.h): tile rules, the forward kernel ladder and the
// BN-statistics row bound.  No torch, no HIP runtime calls.
#include "conv_plan.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <stdexcept>

namespace dlmpi_ext {

using dlmpi::ConvArgs;

Switches g_sw;
LastRan g_ran;

// ---- conv tile autotuner switch (the tuner itself: conv_fwd.cpp autotune) ------------------------
// DLMPI_CONV_AUTOTUNE=1 turns it on; default 0 = the static tile rules only (run-to-run
// bit-reproducible plans): ResNet-50 measured +0.3 %, inside the noise (12,407 / 12,458 img/s on vs
// 12,385 / 12,397 off, profiles/r3_autotune), while timing-chosen plans make two processes of the
// same job sum in different orders.
bool conv_autotune_on() {
  static const int v = [] {
    const char* e = getenv("DLMPI_CONV_AUTOTUNE");
    return e ? atoi(e) : 0;   // 2: also log every plan to stderr
  }();
  return (g_sw.autotune >= 0 ? g_sw.autotune : v) != 0;
}

// K-iteration constants: the reduction step (64 bf16 / 32 fp32 elements = one 128-byte LDS row)
// walks channels (C a multiple of it) or, for small C, every 16-byte piece is its own tap
void set_kstep(ConvArgs& a, int C) {
  if (C % 8 != 0) throw std::runtime_error("conv: channel count must be a multiple of 8 (pad it)");
  if (a.f32) {   // conv_igemm.hip launch_f32: C < 32 or C % 32 != 0 -> small-channel staging
    a.cstep = C % 32 == 0 ? 32 : 0;
    a.tstep = 0;
    return;
  }
  if (C >= 64) {
    if (C % 64 != 0) throw std::runtime_error("conv: channels >= 64 must be a multiple of 64");
    a.cstep = 64;
    a.tstep = 0;
  } else {
    if (64 % C != 0) throw std::runtime_error("conv: channels < 64 must divide 64");
    a.cstep = 0;
    a.tstep = 64 / C;
  }
}

// Tile choice.  256x128 (per-wave 128x64: 25 % less LDS traffic per MFMA than 128x128) wins on
// long reductions into wide outputs (UNet 3x3 convs with >= 256 channels: up to 1.3x, measured by
// benchmarks/conv_bench.py) and loses on the short / memory-bound ResNet GEMMs; 64-row tiles for
// small grids.  `red` = GEMM reduction length (R*S*C).
constexpr int kBm256MinTiles = 256;

// Shortest 1x1 reduction (red == cin) that takes the 256-row tile
// (default 1024: the 14^2 1024->256 forward and 256<-1024 data gradient, 128x128 -> 256x128 tiles
// halve the B-operand re-reads, -14 % each; ResNet-50 +0.8 %, profiles/r3_bm256red); other
// reductions from 2304 as before
constexpr int kBm256MinRed1x1 = 1024;

// cin: channel count of the GEMM's gathered operand
static void pick_tiles(int64_t M, int Kout, int64_t red, int cin, int& bm, int& bn, bool pro = false,
                       bool wide1x1 = true) {
  bn = Kout <= 64 ? 64 : 128;
  // 64 (mod 128) channels above 128 (the UNet's 192-channel top concat gradient): 64-wide tiles
  // cover them exactly instead of a half-empty last 128-wide tile (a third more MFMA work)
  if (Kout > 128 && Kout % 128 == 64) bn = 64;
  bm = 128;
  const int64_t nt = (Kout + bn - 1) / bn;
  const int64_t tiles = ((M + 127) / 128) * nt;
  // 64-channel outputs: 256 x 64 tiles (4 x 1 waves of 64 x 64).  Measured (conv_bench): wins for
  // the small-channel stems (-13 % ResNet 7x7, -10 % UNet first conv) and the 4M-row UNet level-1
  // 3x3s (-4 %), loses 3-8 % on the 0.8M-row ResNet layer1 GEMMs -> only there.
  if (bn == 64 && (M + 255) / 256 >= 512 && (cin < 64 || (M >= (2 << 20) && red >= 576))) bm = 256;
  else if (Kout >= 256 && (red >= 2304 || (wide1x1 && red == cin && red >= kBm256MinRed1x1)) && ((M + 255) / 256) * nt >= kBm256MinTiles) bm = 256;
  else if (tiles < 512) bm = 64;
  // grids that do not fill the chip even with 64-row tiles (ResNet-18 on 32 x 32 CIFAR: 8-128 tiles):
  // 64-wide output tiles too -- twice the blocks before split-K (the autotuner's choice on every such
  // layer, forward and data gradient: +5 % CIFAR img/s, profiles/r4_cifar).  Not for fused BN-apply
  // consumers (pro): their one output column is what lets column 0 alone store the applied input;
  // two columns would each recompute the prologue (profiles/r3_fuse_apply_2col_rejected).
  if (!pro && bm == 64 && bn == 128 && ((M + 63) / 64) * nt < 256) bn = 64;
}

// ---- pipelined 8-wave tiles (conv_igemm.hip conv_pipe_kernel) -----------------------------------
// Long reductions over >= 64-channel operands into 256-multiple outputs: one 8-wave block per CU
// with an LDS ring instead of 2-3 single-stage 4-wave blocks.  Of the pipelined tiles (256 x 256,
// 224 x 256, 128 x 256) the one with the least modeled time: rounds of the 256-CU chip x tile area
// x a per-area cost (128 x 256: per-wave 64 x 64 tiles, 1.25x the LDS traffic per MFMA of the
// 128 x 64 per-wave tiles of the others; profiles/r4_lab).  At batch 256 the 14^2 ResNet layers are
// 50,176 rows: 196 tiles of 256 rows leave 60 CUs idle, 224 tiles of 224 rows 32.  Returns the kernel
// variant + 1 (0: keep the single-stage tile bm x bn).  g_sw.pipe (tests): -1 the rule, 0 never,
// 1 wherever the kernel applies.
// conv_igemm.hip VAR of the DMA issue: A pieces before the first K-half of MFMAs, B pieces before the
// second (2) for the 256 / 224-row tiles; additionally staggered over the two waves of a SIMD (4) for
// 128 x 256 (profiles/r4_lab: 3-8 % over issuing all at once, on every measured shape)
static int pipe_select(int f32, int pro, int cin, int64_t M, int Kout, int64_t red, int& bm, int& bn) {
  if (f32 || pro != 0 || cin % 64 != 0 || cin > 4032 || g_sw.pipe == 0) return 0;   // (conv_igemm.hip kPipeMaxC)
  if (g_sw.pipe == 1) {
    bm = Kout >= 256 ? 256 : (Kout > 64 ? 256 : 512);
    bn = Kout >= 256 ? 256 : (Kout > 64 ? 128 : 64);
    return 2 + 1;
  }
  if (Kout < 256 || Kout % 256 != 0 || red < 1024) return 0;
  struct Cand { int bm; double unit; };
  const Cand cands[] = {{256, 1.0}, {224, 1.0}, {128, 1.25}};
  double best = 1e300;
  int pbm = 256;
  for (const Cand& c : cands) {
    const int64_t tiles = ((M + c.bm - 1) / c.bm) * (Kout / 256);
    const double t = (double)((tiles + 255) / 256) * c.bm * c.unit;
    if (t < best - 1e-9) {
      best = t;
      pbm = c.bm;
    }
  }
  // one block per CU and no split-K: small grids (ResNet-18 on 32 x 32 CIFAR reaches 2 tiles) stay
  // on the single-stage kernel, which splits their K over otherwise idle CUs
  if (((M + pbm - 1) / pbm) * (Kout / 256) < 96) return 0;
  bm = pbm;
  bn = 256;
  return (bm == 128 ? 4 : 2) + 1;
}

// ---- the producer's BN-apply fused into a 1x1 consumer (conv_igemm.hip conv1x1_apply_kernel) ----
// pro-3 launches whose Kout is one 64 / 128 / 256-channel tile column run the register-staged kernel
// (128-row tiles: 64-row tiles measured slower, profiles/r5_apply) instead of the single-stage pro-3
// conv_igemm_kernel.  set_conv_apply(0): the latter.  Every other pro-3 launch -- and one whose
// operands the register-staged kernel cannot address (apply1x1_operands) -- runs the single-stage kernel
// on 128 x 64 tiles (kPro3Bm x kPro3Bn; the larger pro-3 tiles spilled and are not built), so both
// paths produce ceil(M / 128) BN-statistics rows and the caller's buffer fits either.
constexpr int kPro3Bm = 128, kPro3Bn = 64;

// ---- 2-D halo tiles for 3x3 / stride-1 / pad-1 convolutions (conv_igemm.hip HALO) ----------------
// set_conv_halo(0) (tests): these convolutions through the im2col gather path too.
// Tile th x tw (th * tw <= bm, (th + 2) * (tw + 2) <= 192 / 352 rows for bm 128 / 256) covering a
// P x Q grid with the fewest tiles (ties: the wider tile).
void halo_geom(int P, int Q, int bm, int& th, int& tw, int& tiles_h, int& tiles_w) {
  int best = INT32_MAX;
  const int rows = bm == 256 ? 352 : 192;   // conv_igemm.hip HALO_ROWS
  for (int w = bm == 256 ? 32 : 16; w >= 4; --w) {
    const int h = std::min(bm / w, rows / (w + 2) - 2);
    if (h < 1) continue;
    const int t = ceil_div(P, h) * ceil_div(Q, w);
    if (t < best) {
      best = t;
      th = h;
      tw = w;
    }
  }
  tiles_h = ceil_div(P, th);
  tiles_w = ceil_div(Q, tw);
}
// Halo tile shape (profiles/r4_halo): 256-pixel tiles (16 x 16, 18 x 18 halo) for 64-channel
// outputs (+9 % on 56^2 / 512^2 grids: half the B-fragment reads per MFMA) and for >= 256-channel
// outputs (+2-4 %); 128-pixel tiles for 128-channel outputs, where the 256 x 128 tile loses 4-7 %.
static void halo_tiles(int Kout, int& bm, int& bn) {
  bn = std::min(bn, 128);
  bm = (bn == 64 || Kout >= 256) ? 256 : 128;
}
// Measured per shape (profiles/r3_halo): halo tiles win 1-6 % on grids >= 28 x 28 against the
// 128-row gather tiles, tie with the 8-wave 256 x 256 tiles, and lose on 14^2 / 7^2 grids (a
// 7 x 7 image fills a 126-pixel tile to 39 %) -- so only there, and not instead of 256 x 256 tiles.
static bool halo_eligible(int f32, int pro, int C, int R, int S, int stride, int pad, int P, int Q) {
  if (g_sw.halo == 0 || f32 || pro != 0 || C % 64 != 0 || R != 3 || S != 3 || stride != 1 || pad != 1) return false;
  return g_sw.halo == 2 || (P >= 28 && Q >= 28);   // 2: any grid (tests)
}
// Halo tiles before the pipelined kernel for >= 256 output channels (profiles/r4_halo: the 256 x 128
// halo tile beat the best pipe tile on every UNet 3x3 of >= 32^2 grid, 2-5 %; 32^2 1024 -> 1024: 231.6
// vs 243.2 us); the pipe kernel keeps the 14^2 / 7^2 grids, where halo tiles are not eligible.
static bool halo_first(bool halo_ok, int Kout) { return halo_ok && Kout >= 256 && g_sw.halo_first; }

// fp32: single-stage 4-wave tiles only, at most 128 x 128 (launch_f32)
static void f32_tiles(int& bm, int& bn) {
  bm = std::min(bm, 128);
  bn = std::min(bn, 128);
}

Tiles select_tiles(const TileQuery& q) {
  Tiles t{};
  pick_tiles(q.M, q.Kout, q.red, q.cin, t.bm, t.bn, q.pro != 0, q.wide1x1);
  if (q.f32) f32_tiles(t.bm, t.bn);
  const bool halo_ok = q.halo_ok && halo_eligible(q.f32, q.pro, q.cin, q.R, q.S, q.stride, q.pad, q.P, q.Q);
  t.pipe = q.pipe_ok && !halo_first(halo_ok, q.Kout)
               ? pipe_select(q.f32, q.pro, q.cin, q.M, q.Kout, q.red, t.bm, t.bn) : 0;
  t.halo = !t.pipe && halo_ok;
  if (t.halo) halo_tiles(q.Kout, t.bm, t.bn);
  return t;
}

// ---- conv tile autotuner ("benchmark mode"): the plans it times ----------------------------------
std::vector<TuneCand> tune_candidates(int f32, int C, int Kout, int maxk) {
  std::vector<TuneCand> cands;
  const int tiles_m[] = {64, 128, 256};
  for (int tbm : tiles_m)
    for (int tbn : {64, 128, 256}) {
      if (tbn > 64 && Kout <= tbn / 2) continue;   // mostly padding
      if (tbm == 256 && tbn == 256 && C < 64) continue;
      if (tbm == 128 && tbn == 256 && C < 64) continue;
      if (tbm == 64 && tbn == 256) continue;
      if (f32 && (tbm > 128 || tbn > 128)) continue;   // launch_f32's tiles
      cands.push_back({tbm, tbn, 0});
      if (maxk >= 16) cands.push_back({tbm, tbn, 2});
      if (maxk >= 8) cands.push_back({tbm, tbn, 1});
    }
  return cands;
}

// ---- the forward ladder -------------------------------------------------------------------------
// Persistent kernels write one statistics row per block (G rows) instead of one per M-tile.  Each
// rung has a shape-only predicate -- the statistics buffer is sized from it before the launch -- and
// an operand predicate (alignment, 32-bit extents, storage types) checked at launch time; when the
// latter fails the forward takes the next rung into the same buffer.
static bool fits32(int64_t elems) { return elems < (1ll << 31); }

// 3x3 / s1 / p1 from an 8-channel (padded image) input into 64 channels: conv_small.hip
static bool c8_shape(const ConvShape& s, FwdPlan& p) {
  if (!g_sw.c8 || !s.free_tiles() || s.C != 8 || s.K != 64 || s.R != 3 || s.S != 3 || s.stride != 1 || s.pad != 1 ||
      s.W % 16 || s.pro || s.f32)
    return false;
  p.rows = p.G = dlmpi_conv3x3_c8_blocks((int64_t)s.N * s.H * s.W);
  return true;
}
static bool c8_operands(const ConvShape& s, const FwdOperands& o) {
  return o.plain(s.K) && o.x_aligned() && o.y_aligned() && fits32((int64_t)s.N * s.H * s.W) && o.y_bf16;
}
// the ResNet stem on its 2x2 space-to-depth image (4x4 / s1 / p0, 16 channels -> 64): conv_small.hip
static bool c16_shape(const ConvShape& s, FwdPlan& p) {
  if (!g_sw.c16 || !s.free_tiles() || s.C != 16 || s.K != 64 || s.R != 4 || s.S != 4 || s.stride != 1 ||
      s.pad != 0 || s.H < 4 || (s.W - 3) % 16 || s.W < 19 || s.pro || s.f32)
    return false;
  p.rows = p.G = dlmpi_conv4x4_c16_blocks((int64_t)s.N * (s.H - 3) * (s.W - 3));
  return true;
}
static bool c16_operands(const ConvShape& s, const FwdOperands& o) {
  return o.plain(s.K) && o.x_aligned() && o.y_aligned() && fits32((int64_t)s.N * s.H * s.W * o.ldx) &&
         fits32(s.M() * o.ldy) && o.y_bf16 && o.ldw == 256;
}
// <= 4 output channels, 1x1, no epilogue beyond the bias (the UNet head): a streaming dot product
static bool head_shape(const ConvShape& s, FwdPlan& p) {
  p.rows = 0;
  return g_sw.head && s.free_tiles() && s.pro == 0 && !s.f32 && s.R == 1 && s.S == 1 && s.stride == 1 && s.pad == 0;
}
static bool head_operands(const ConvShape& s, const FwdOperands& o) {
  return !o.has_stats && !o.has_res && !o.has_scale && !o.relu && !o.has_fin && dlmpi_head1x1_ok(s.C, o.kvalid) &&
         o.x_aligned() && (o.y_f32 || o.y_bf16);
}
// The streaming 3x3 kernel (conv3x3_stream.hip: 64 -> 64 channels, stride 1, pad 1; the full-resolution
// UNet layers, ResNet layer-1 conv2).  Its grid shares the RCCL-aware budget of the streaming data
// gradient (one block per CU).
bool stream3x3_shape(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int pro, int f32, int& th,
                     int& tw, int& G) {
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || pro != 0 || f32) return false;
  return dlmpi_conv3_stream_plan(N, H, W, C, K, dlmpi_dgs_blocks(), &th, &tw, &G) != 0;
}
static bool s3_shape(const ConvShape& s, FwdPlan& p) {
  if (!s.free_tiles() ||
      !stream3x3_shape(s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.stride, s.pad, s.pro, s.f32, p.th, p.tw, p.G))
    return false;
  p.rows = p.G;
  return true;
}
static bool s3_operands(const ConvShape& s, const FwdOperands& o) {
  return o.plain(s.K) && o.y_aligned() && o.x_aligned() && fits32((int64_t)s.H * s.W * o.ldy * 2) && o.y_bf16 &&
         o.w_bf16;
}
// The streaming 1x1 kernel (conv1x1_stream.hip: short reductions into wide, memory-bound outputs)
static bool s1_shape(const ConvShape& s, FwdPlan& p) {
  if (!s.free_tiles() || s.R != 1 || s.S != 1 || (s.stride != 1 && s.stride != 2) || s.pad != 0 || s.pro != 0 || s.f32)
    return false;
  if (!dlmpi_stream1x1_plan(s.M(), s.C, s.K, s.stride, &p.sbm, &p.sbn, &p.G)) return false;
  p.rows = p.G;
  return true;
}
static bool s1_operands(const ConvShape& s, const FwdOperands& o) {
  return o.plain(s.K) && o.y_aligned() && o.x_aligned() && fits32((int64_t)s.N * s.H * s.W * o.ldx) &&
         fits32(s.M() * o.ldy * 2) && o.y_bf16;
}
// The register-staged pro-3 kernel (above); its launch-time conditions beyond the shape: 16-byte
// output rows and 32-bit element offsets of every operand
static bool apply1x1_shape(const ConvShape& s, FwdPlan& p) {
  if (!(g_sw.apply != 0 && s.free_tiles() && s.pro == 3 && !s.f32 && s.R == 1 && s.S == 1 && s.stride == 1 &&
        s.pad == 0 && dlmpi_conv1x1_apply_ok(s.C, s.K)))
    return false;
  p.bm = kPro3Bm;
  p.bn = s.K;
  p.rows = ceil_div(s.M(), kPro3Bm);
  return true;
}
static bool apply1x1_operands(const ConvShape& s, const FwdOperands& o) {
  return o.kvalid == s.K && o.y_aligned() && fits32((int64_t)s.N * s.H * s.W * std::max(o.ldx, o.ldpro));
}

struct Candidate {
  FwdPath path;
  bool (*shape)(const ConvShape&, FwdPlan&);   // fills the plan's geometry and rows
  bool (*operands)(const ConvShape&, const FwdOperands&);
};
static const Candidate kLadder[] = {
    {FwdPath::c8, c8_shape, c8_operands},         {FwdPath::c16, c16_shape, c16_operands},
    {FwdPath::head, head_shape, head_operands},   {FwdPath::stream3x3, s3_shape, s3_operands},
    {FwdPath::stream1x1, s1_shape, s1_operands},  {FwdPath::apply1x1, apply1x1_shape, apply1x1_operands},
};

const char* fwd_path_name(FwdPath p) {
  static const char* const names[] = {"c8", "c16", "head", "stream3x3", "stream1x1", "apply1x1", "pipe", "halo", "igemm"};
  return names[(int)p];
}

// the tiled fallback (conv_igemm / pipe / halo): the rules, then the forced tile shape
static FwdPlan plan_tiled(const ConvShape& s) {
  TileQuery q{s.M(), s.K, s.red(), s.C, s.R, s.S, s.stride, s.pad, s.P(), s.Q(), s.f32, s.pro};
  q.halo_ok = q.pipe_ok = s.free_tiles();
  const Tiles t = select_tiles(q);
  FwdPlan p{};
  p.bm = s.bm_req > 0 ? s.bm_req : t.bm;
  p.bn = s.bn_req > 0 ? s.bn_req : t.bn;
  p.pipe = t.pipe;
  if (s.bn_req == 256) {   // 256-column tiles (128 x 256, 256 x 256) exist only as the pipelined 8-wave kernel
    if (s.f32 || s.pro != 0 || s.C % 64 != 0 || (p.bm != 128 && p.bm != 256))
      throw std::runtime_error("conv2d_fwd: 256-column tiles need bf16, no prologue, C % 64 == 0, 128 / 256 rows");
    p.pipe = (p.bm == 128 ? 4 : 2) + 1;
  }
  if (s.pro == 3) {
    p.bm = kPro3Bm;
    p.bn = kPro3Bn;
  }
  p.path = t.halo ? FwdPath::halo : (p.pipe ? FwdPath::pipe : FwdPath::igemm);
  p.rows = ceil_div(s.M(), p.bm);
  if (t.halo) {
    int tiles_h = 1, tiles_w = 1;
    p.th = 8, p.tw = 16;
    halo_geom(s.P(), s.Q(), p.bm, p.th, p.tw, tiles_h, tiles_w);
    p.rows = s.N * tiles_h * tiles_w;
  }
  return p;
}

FwdPlan plan_fwd(const ConvShape& s, const FwdOperands& o) {
  const FwdPlan tiled = plan_tiled(s);
  if (s.pro == 3 && (s.R != 1 || s.S != 1 || s.stride != 1 || s.pad != 0))
    throw std::runtime_error("conv prologue 3: a 1x1 / stride-1 conv");
  for (const Candidate& c : kLadder) {
    FwdPlan p = tiled;
    if (c.shape(s, p) && c.operands(s, o)) {
      p.path = c.path;
      return p;
    }
  }
  return tiled;
}

int fwd_rows_bound(const ConvShape& s) {
  const FwdPlan tiled = plan_tiled(s);
  int rows = tiled.rows;
  // autotuned launches (conv_fwd.cpp autotune: plain single-stage launches only) may pick any of the
  // tuner's M tiles
  if (s.free_tiles() && conv_autotune_on() && s.pro == 0 && tiled.path == FwdPath::igemm)
    for (const TuneCand& c : tune_candidates(s.f32, s.C, s.K, 0)) rows = std::max(rows, ceil_div(s.M(), c.bm));
  for (const Candidate& c : kLadder) {
    FwdPlan p{};
    if (c.shape(s, p)) rows = std::max(rows, p.rows);
  }
  return rows;
}

// ---- argument checks (conv_plan.h) ----------------------------------------------------------------
namespace {
struct Checker {
  std::string err;
  bool ok() const { return err.empty(); }
  void fail(const std::string& m) {
    if (err.empty()) err = m;
  }
  void positive(const char* name, int64_t v) {
    if (v <= 0) fail(std::string(name) + " must be positive (got " + std::to_string(v) + ")");
  }
  // the extent rule of conv_plan.h
  void operand(const char* name, const Operand& o, int64_t rows, int width) {
    if (!ok() || !o.given()) return;
    if (o.off < 0 || o.ld <= 0 || (int64_t)o.off + width > o.ld)
      return fail(std::string(name) + ": channel slice [" + std::to_string(o.off) + ", " +
                  std::to_string((int64_t)o.off + width) + ") does not fit its row stride " + std::to_string(o.ld));
    const int64_t need = (rows - 1) * o.ld + o.off + width;
    if (o.numel < need)
      fail(std::string(name) + ": buffer of " + std::to_string(o.numel) + " elements is shorter than the " +
           std::to_string(need) + " the launch reaches (" + std::to_string(rows) + " rows of stride " +
           std::to_string(o.ld) + ")");
  }
  void required(const char* name, const Operand& o) {
    if (!o.given()) fail(std::string(name) + " is required");
  }
  void vec(const char* name, int64_t numel, int64_t need) {
    if (ok() && numel >= 0 && numel < need)
      fail(std::string(name) + ": " + std::to_string(numel) + " elements, " + std::to_string(need) + " needed");
  }
};
// sizes and the output grid; returns P, Q of the geometry (0 when it is not even defined)
void check_geometry(Checker& k, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int& P, int& Q) {
  k.positive("N", N); k.positive("H", H); k.positive("W", W); k.positive("C", C); k.positive("K", K);
  k.positive("R", R); k.positive("S", S); k.positive("stride", stride);
  if (pad < 0) k.fail("pad must not be negative");
  P = Q = 0;
  if (!k.ok()) return;
  if (H + 2 * pad < R || W + 2 * pad < S) return k.fail("the output grid is empty: the padded image is smaller than the kernel");
  P = (H + 2 * pad - R) / stride + 1;
  Q = (W + 2 * pad - S) / stride + 1;
  if ((int64_t)N * H * W >= (1ll << 31) || (int64_t)N * P * Q >= (1ll << 31)) k.fail("more than 2^31 - 1 pixels");
}
}  // namespace

std::string check_fwd_args(const FwdCheck& c) {
  Checker k;
  int P, Q;
  check_geometry(k, c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, P, Q);
  if (!k.ok()) return "conv2d_fwd: " + k.err;
  const int64_t Min = (int64_t)c.N * c.H * c.W, M = (int64_t)c.N * P * Q;
  const int stored = c.kvalid > 0 && c.kvalid < c.K ? c.kvalid : c.K;
  k.required("x", c.x);
  k.required("y", c.y);
  k.operand("x", c.x, Min, c.C);
  k.operand("y", c.y, M, stored);
  k.operand("res", c.res, M, c.K);
  k.vec("w", c.w_numel < 0 ? 0 : c.w_numel, (int64_t)c.K * c.R * c.S * c.C);
  k.vec("bias", c.bias_numel, c.K);
  k.vec("scale", c.scale_numel, c.K);
  k.vec("shift", c.shift_numel, c.K);
  if ((c.scale_numel >= 0) != (c.shift_numel >= 0)) k.fail("scale and shift come together");
  if (c.stats_rows >= 0) {
    if (!c.stats_f32) k.fail("stats must be fp32");
    if (c.stats_rows == 0 || c.stats_cols != 2 * (int64_t)c.K)
      k.fail("stats must be [rows][2*K]: " + std::to_string(c.stats_cols) + " columns for K = " + std::to_string(c.K));
  }
  return k.ok() ? "" : "conv2d_fwd: " + k.err;
}

std::string check_dgrad_args(const DgradCheck& c) {
  Checker k;
  int P, Q;
  check_geometry(k, c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, P, Q);
  if (k.ok() && c.stride > 2) k.fail("stride <= 2 supported");
  if (k.ok() && (c.P != P || c.Q != Q))
    k.fail("dy grid " + std::to_string(c.P) + " x " + std::to_string(c.Q) + " is not the " + std::to_string(P) + " x " +
           std::to_string(Q) + " output of this conv on a " + std::to_string(c.H) + " x " + std::to_string(c.W) + " input");
  if (!k.ok()) return "conv2d_dgrad: " + k.err;
  const int64_t Min = (int64_t)c.N * c.H * c.W, M = (int64_t)c.N * P * Q;
  k.required("dy", c.dy);
  k.required("dx", c.dx);
  k.operand("dy", c.dy, M, c.K);
  k.operand("dx", c.dx, Min, c.C);
  k.operand("res", c.res, Min, c.C);
  k.operand("mask", c.mask, Min, c.C);
  k.operand("z", c.z, Min, c.C);
  k.operand("z2", c.z2, Min, c.C);
  k.vec("wT", c.wT_numel < 0 ? 0 : c.wT_numel, (int64_t)c.C * c.R * c.S * c.K);
  k.vec("bias", c.bias_numel, c.C);
  k.vec("mscale", c.mscale_numel, c.C);
  k.vec("mshift", c.mshift_numel, c.C);
  if (c.mbits_numel >= 0 && (c.C % 8 || c.mbits_numel != Min * (c.C / 8))) k.fail("mask bits must be [N*H*W][C/8]");
  // conv_epilogue takes the unmasked column sums before it adds the residual: they would not be the
  // sums of the stored dx
  if (c.colsum && c.res.given() && !c.mask.given() && c.mscale_numel < 0 && c.mbits_numel < 0)
    k.fail("colsum with a residual is not built (the column sums are taken before the residual is added)");
  return k.ok() ? "" : "conv2d_dgrad: " + k.err;
}

std::string check_wgrad_args(const WgradCheck& c) {
  Checker k;
  int P, Q;
  check_geometry(k, c.N, c.H, c.W, c.C, c.Ko, c.R, c.S, c.stride, c.pad, P, Q);
  if (k.ok() && (c.P != P || c.Q != Q))
    k.fail("dy grid " + std::to_string(c.P) + " x " + std::to_string(c.Q) + " is not the " + std::to_string(P) + " x " +
           std::to_string(Q) + " output of this conv on a " + std::to_string(c.H) + " x " + std::to_string(c.W) + " input");
  if (k.ok() && (c.Creal < 0 || c.Creal > c.C || c.Ko_real < 0 || c.Ko_real > c.Ko))
    k.fail("Creal / Ko_real must lie in [0, C] / [0, Ko]");
  if (!k.ok()) return "conv2d_wgrad: " + k.err;
  k.required("dy", c.dy);
  k.required("x", c.x);
  k.operand("dy", c.dy, (int64_t)c.N * P * Q, c.Ko);
  k.operand("x", c.x, (int64_t)c.N * c.H * c.W, c.C);
  k.vec("grad", c.grad_numel < 0 ? 0 : c.grad_numel, (int64_t)c.Ko_real * c.R * c.S * c.Creal);
  return k.ok() ? "" : "conv2d_wgrad: " + k.err;
}

// The streaming 64 -> 64 3x3 forward takes this launch with the producer's BN-apply + ReLU fused
// (conv3x3_stream_kernel PRO): shape and operand conditions (the model asks before it defers the apply).
// The kernel addresses 64-channel rows of x and of the applied output from their offsets.
bool conv3_pro_ok(int N, int H, int W, int C, int K, int ldx, int xoff, int ldz, int zoff, int ldyapp, int yappoff) {
  int th, tw, G;
  return g_sw.c3pro && C == 64 && K == 64 && stream3x3_shape(N, H, W, C, K, 3, 3, 1, 1, 0, 0, th, tw, G) &&
         ldx % 8 == 0 && xoff % 8 == 0 && ldz % 8 == 0 && zoff % 8 == 0 && ldyapp % 8 == 0 && yappoff % 8 == 0 &&
         yappoff + 64 <= ldyapp && xoff + 64 <= ldx && (int64_t)H * W * std::max(ldz, ldyapp) * 2 < (1ll << 31);
}

}  // namespace dlmpi_ext
