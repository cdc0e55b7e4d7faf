// Convolution launch planning: which kernel a forward conv runs, on which tiles, and how many
// BN-statistics rows it writes.  Pure host arithmetic over shapes and operand facts -- no torch, no
// HIP runtime calls, no device state -- so the statistics buffer is sized (fwd_rows_bound) by the very
// rules the launch follows (plan_fwd), and both can be exercised without a GPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../kernels/dlmpi_kernels.h"

namespace dlmpi_ext {

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// A/B and test overrides (dlmpi_ext set_*): -1 = the rule, unless noted.  The switches that live in
// the kernel library (dlmpi_set_conv_stream and the like) stay there.
struct Switches {
  int pipe = -1;         // set_conv_pipe (tests): 0 never, 1 wherever the kernel applies
  int pipe_dgrad = -1;   // set_conv_pipe_dgrad (A/B): 0 keeps data gradients off it
  int apply = -1;        // set_conv_apply: 0 = pro-3 launches on the single-stage kernel
  int halo = -1;         // set_conv_halo (tests): 0 off, 2 any grid
  int halo_first = 1;    // set_halo_first (A/B): 0 = the pipelined kernel first where it applies
  int splitk = 0;        // set_conv_splitk (tests): > 0 forces that many K slices
  int autotune = -1;     // set_conv_autotune: >= 0 overrides DLMPI_CONV_AUTOTUNE
  int head = 1;          // set_head1x1 (A/B)
  int c8 = 1;            // set_conv_c8 (A/B)
  int c16 = 1;           // set_conv_c16 (A/B)
  int c3pro = 1;         // set_conv3_pro (A/B): 0 = the standalone BN-apply before the conv
  int convT_stream = 1;  // set_convT_stream (A/B)
  int wgrad3 = -1;       // set_wgrad3 (tests); -1: on
  int wgrad3_blocks = 0; // set_wgrad3_blocks (A/B): > 0 overrides the grid target
  int wgrad_blocks = 0;  // set_wgrad_blocks (A/B): > 0 overrides the gather kernel's grid target
};
// 1 if the last launch of that kind ran the kernel (tests: *_last)
struct LastRan {
  int halo = 0;          // conv2d_fwd / conv2d_dgrad: halo tiles
  int stream = 0;        // conv2d_fwd: the streaming 1x1 kernel
  int dgrad_stream = 0;  // conv2d_dgrad: the streaming 1x1 kernel
  int conv3 = 0;         // conv2d_fwd / conv2d_dgrad: the streaming 3x3 kernel
  int head = 0;          // conv2d_fwd: the 1x1 head kernel (head.hip)
  int c8 = 0;            // conv2d_fwd: the 8-channel 3x3 kernel (conv_small.hip)
  int c16 = 0;           // conv2d_fwd: the 16-channel 4x4 stem kernel
  int convT_stream = 0;  // convT2x2_fwd: the streaming kernel
  int wgrad3 = 0;        // weight gradient: the 3x3 spatial-tile kernel
  int head_dgrad = 0;    // data gradient of a <= 8-output 1x1 head: the streaming K = 2..4 kernel (head.hip)
};
extern Switches g_sw;
extern LastRan g_ran;
bool conv_autotune_on();

struct ConvShape {
  int N, H, W, C, K, R, S, stride, pad;
  int pro, f32;
  int bm_req, bn_req;   // tests / experiments: force a tile shape (<= 0: the rules)
  int P() const { return (H + 2 * pad - R) / stride + 1; }
  int Q() const { return (W + 2 * pad - S) / stride + 1; }
  int64_t M() const { return (int64_t)N * P() * Q(); }
  int64_t red() const { return (int64_t)R * S * C; }
  bool free_tiles() const { return bm_req <= 0 && bn_req <= 0; }
};

enum class FwdPath { c8, c16, head, stream3x3, stream1x1, apply1x1, pipe, halo, igemm };
const char* fwd_path_name(FwdPath p);

// What a forward launch's operands look like, as far as the kernel choice depends on them.
struct FwdOperands {
  bool has_res, has_scale, relu, has_stats, has_fin;
  int kvalid;              // stored output channels (K: all)
  int ldx, xoff, ldy, yoff, ldw;
  int ldpro;               // pro 3: the widest of the prologue's residual and applied-output rows
  bool y_bf16, y_f32, w_bf16;
  bool plain(int K) const { return !has_res && !has_scale && !relu && kvalid == K; }   // bias / statistics only
  bool x_aligned() const { return ldx % 8 == 0 && xoff % 8 == 0; }
  bool y_aligned() const { return ldy % 8 == 0 && yoff % 8 == 0; }
};

struct FwdPlan {
  FwdPath path;
  int bm, bn, pipe;       // tiled paths (apply1x1: bm x K)
  int rows;               // BN-statistics rows the launch writes
  int G, th, tw, sbm, sbn;   // persistent kernels: blocks, 3x3 tile, streaming 1x1 tile
};

void set_kstep(dlmpi::ConvArgs& a, int C);

// The GEMM whose tiles are wanted.  The data gradient passes its per-phase sizes (/ stride^2), its
// own halo condition and its pipe switch; conv2d_fwd_bnbwd has no halo variant.
struct TileQuery {
  int64_t M;
  int Kout;
  int64_t red;
  int cin;
  int R, S, stride, pad, P, Q;   // conv geometry and output grid (halo eligibility)
  int f32, pro;
  bool halo_ok = true;
  bool pipe_ok = true;
  bool wide1x1 = true;
};
struct Tiles {
  int bm, bn, pipe;
  bool halo;
};
Tiles select_tiles(const TileQuery& q);
void halo_geom(int P, int Q, int bm, int& th, int& tw, int& tiles_h, int& tiles_w);

// the (BM, BN, split-K) plans the autotuner times; maxk = the longest phase's K-steps
struct TuneCand {
  int bm, bn, splitk_req;
};
std::vector<TuneCand> tune_candidates(int f32, int C, int Kout, int maxk);

FwdPlan plan_fwd(const ConvShape& s, const FwdOperands& o);
// Upper bound of plan_fwd(s, any operands).rows -- and of an autotuned launch's: the caller's buffer.
int fwd_rows_bound(const ConvShape& s);

// ---- argument checks of the conv entry points ----------------------------------------------------
// Pure integer arithmetic over sizes and element counts, run by conv2d_fwd* / conv2d_dgrad* /
// conv2d_wgrad* before anything is launched (and by the conv2d_*_check bindings without a GPU).
// Each returns "" for a valid call, else what is wrong.
//
// An operand is a channel slice [off, off + width) of the rows of an [rows][ld] buffer of `numel`
// elements.  THE EXTENT RULE: the last element the launch may touch lies inside the buffer,
//   (rows - 1) * ld + off + width <= numel,  with off >= 0 and off + width <= ld
// (not rows * ld: a slice of a wider allocation may end with its last row).  numel < 0: operand absent.
struct Operand {
  int64_t numel = -1;
  int ld = 0, off = 0;
  bool given() const { return numel >= 0; }
};
struct FwdCheck {
  int N, H, W, C, K, R, S, stride, pad;
  int kvalid;                    // <= 0 or >= K: all K channels are stored
  Operand x, y, res;             // x: N*H*W rows of C; y: N*P*Q rows of the stored channels; res: N*P*Q rows of K
  int64_t w_numel;               // >= K*R*S*C
  int64_t bias_numel = -1, scale_numel = -1, shift_numel = -1;   // per-channel vectors: >= K
  int64_t stats_rows = -1, stats_cols = 0;                      // statistics [rows][2*K] ...
  bool stats_f32 = true;                                         // ... in fp32
};
struct DgradCheck {
  int N, P, Q, K, C, R, S, stride, pad, H, W;
  Operand dy, dx, res, mask, z, z2;   // dy: N*P*Q rows of K; the others N*H*W rows of C
  int64_t wT_numel;                   // >= C*R*S*K
  int64_t bias_numel = -1, mscale_numel = -1, mshift_numel = -1;   // >= C
  int64_t mbits_numel = -1;           // == N*H*W * C/8
  bool colsum = false;                // column sums without a mask: not together with res (taken before it is added)
};
struct WgradCheck {
  int N, H, W, C, Ko, R, S, stride, pad, P, Q;
  int Creal, Ko_real;            // 0 <= Creal <= C, 0 <= Ko_real <= Ko: the packed gradient [Ko_real][R*S][Creal]
  Operand dy, x;                 // dy: N*P*Q rows of Ko; x: N*H*W rows of C
  int64_t grad_numel;            // >= Ko_real * R*S * Creal
};
std::string check_fwd_args(const FwdCheck& c);
std::string check_dgrad_args(const DgradCheck& c);
std::string check_wgrad_args(const WgradCheck& c);

bool stream3x3_shape(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int pro, int f32, int& th,
                     int& tw, int& G);
bool conv3_pro_ok(int N, int H, int W, int C, int K, int ldx, int xoff, int ldz, int zoff, int ldyapp, int yappoff);

}  // namespace dlmpi_ext
