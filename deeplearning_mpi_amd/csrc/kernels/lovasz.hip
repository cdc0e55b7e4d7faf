// Lovasz-Softmax and Lovasz hinge losses (Berman et al., CVPR 2018): the Lovasz extension of the Jaccard loss,
// alone or added to the plain pixel-wise CE / BCE, by a segmented stable radix sort on the device.
//
// Definition.  A segment is the set of pixels ranked together: one per class over the batch (S = K, L = N H W),
// or with per_image one per (sample, class) (S = N K, L = H W).  A pixel is valid when pix_kept(label); invalid
// pixels get no rank, no count and an exact zero gradient.  Softmax form: p = exp(x - lse) in the arithmetic of
// pixel_ce.hip, fg = [y = c], e = |fg - p_c|.  Hinge form (one class, every pixel valid): fg = [t > 0.5],
// e = 1 - x (2 fg - 1).  Within a segment the valid pixels are ranked by e descending, equal e by ascending pixel
// index (a stable sort); -0 counts as +0 and a NaN ranks above everything.  With G the segment's fg count, a pixel
// at 0-based rank i with F fg pixels strictly before it, R = G - F and U = G + i - F:
//     g = 1 / U (fg),   g = R / (U (U + 1)) (bg),   g = 1 where U = 0 (an absent class: rank 0)
// which is J_i - J_{i-1} of the paper without the cancellation, formed in fp64 from the integers and rounded once.
// Segment loss = sum e g (hinge: sum max(e, 0) g).  A segment is counted when G > 0 (classes = present) or always
// (classes = all, and the hinge form); the loss is the mean over the samples (one "sample" without per_image) of
// the mean over that sample's counted segments, 0 where nothing is counted.  The gradient goes through e with g
// held constant: a_c = +-g_c coef_c, dx_j = p_j (a_j - sum_c a_c p_c); hinge: dx = -(2 fg - 1) g coef [e > 0].
// loss = ce_weight * CE + lovasz_weight * Lovasz with CE the plain unweighted mean over the valid pixels.
//
// Keys.  key = the bits of e mapped so that ascending uint32 = descending e: bits ^ 0x7FFFFFFF for e >= 0 (-0
// folded into +0), the bits themselves for e < 0, 0 for a NaN, 0xFFFFFFFF (above every valid key) for an invalid
// pixel.  payload = the pixel's index within its segment, fg in bit 31.  Both are [S][L].
//
// Passes (tile = 2048 items = 8 rounds of one 256-lane block; 8-bit digits, 4 sort passes):
//   err        per pixel: softmax (pixel_softmax.h blocks, both layouts in place), K keys and payloads, lse, and
//              the block's CE sum and valid count in a fixed order (no atomics)
//   4 x { hist     grid (tile, segment): the tile's 256-bin digit histogram in LDS -> tab[segment][digit][tile]
//         rowscan  grid (segment x digit): exclusive scan along the tiles, the row's total -> tot
//         scatter  grid (tile, segment): base of digit d = scan of tot + tab; items in input order, one block
//                  width per round; a lane's rank among the equal-digit lanes below it in its wave from 8 ballots
//                  (one per digit bit); waves and rounds combined through per-wave digit counters in LDS }
//   fgcount    per-tile popcount of the fg bits of the sorted payloads; rowscan over the tiles (its total is G)
//   jaccard    per tile: F from the scanned tile counts + ballots, g in closed form, e from the key, g scattered
//              to g[S][L] at the pixel's own index (an invalid pixel gets 0), sum e g per tile
//   segsum     per segment: the tile partials in fp64, fixed order
//   finish     one block: counted segments, coef[S], the loss scalar, den = n_valid, stats
//   bwd        one pointwise pass: p recomputed from lse, the Lovasz and the CE / BCE gradient, logits' strides
// Kernel boundaries are the only grid-wide synchronisation; every buffer is fully written before it is read, so
// nothing needs zeroing; no float atomics, no host read: the chain is a fixed list of kernel nodes under capture.
#include "pixel_softmax.h"

namespace dlmpi {

constexpr int kLvTile = 2048;
constexpr int kLvRounds = kLvTile / 256;
constexpr unsigned kLvInvalid = 0xFFFFFFFFu;
constexpr unsigned kLvFg = 0x80000000u;
constexpr int64_t kLvSegMax = 65535;   // the segment is grid dimension y

__device__ __forceinline__ unsigned lv_key(float e) {
  if (e != e) return 0u;
  const unsigned b = __float_as_uint(e);
  if ((b << 1) == 0u) return 0x7FFFFFFFu;
  return (b >> 31) ? b : b ^ 0x7FFFFFFFu;
}
__device__ __forceinline__ float lv_err(unsigned key) {
  return __uint_as_float((key >> 31) ? key : key ^ 0x7FFFFFFFu);
}
__device__ __forceinline__ float lv_bce_elem(float x, float t) {   // loss.hip's bce_elem
  return fmaxf(x, 0.f) - x * t + log1pf(__expf(-fabsf(x)));
}
__device__ __forceinline__ unsigned long long lv_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// exclusive prefix of v over the block's 256 threads (+ the block's total); sh: 4 words, free again on return
__device__ __forceinline__ unsigned lv_block_excl(unsigned v, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = (unsigned)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  unsigned ex = inc - v;
  for (int w = 0; w < wv; ++w) ex += sh[w];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return ex;
}

// the workspace, in 32-bit words from a 256-byte aligned base
struct LvWs {
  double* segsum;           // [S]
  unsigned *key[2], *pay[2];   // [S][L] each
  unsigned *tab, *tot;      // [S][256][ntiles], [S][256]
  unsigned *tilefg, *G;     // [S][ntiles], [S]
  float* part;              // [S][ntiles]
  float* cesum;             // [nce]
  unsigned* cecnt;          // [nce]
  int64_t words;
};
static inline int64_t lv_tiles(int64_t L) { return (L + kLvTile - 1) / kLvTile; }
static inline int lv_err_blocks(int64_t M) {
  const int64_t b = (M + 255) / 256;
  return (int)(b > 2048 ? 2048 : b < 1 ? 1 : b);
}
static LvWs lv_ws(uint32_t* base, int64_t S, int64_t L, int64_t M) {
  const int64_t n = S * L, nt = lv_tiles(L), nce = lv_err_blocks(M);
  LvWs w;
  int64_t o = 0;
  auto take = [&](int64_t words) { uint32_t* p = base + o; o += (words + 3) & ~(int64_t)3; return p; };
  w.segsum = reinterpret_cast<double*>(take(2 * S));
  for (int i = 0; i < 2; ++i) { w.key[i] = take(n); w.pay[i] = take(n); }
  w.tab = take(S * 256 * nt);
  w.tot = take(S * 256);
  w.tilefg = take(S * nt);
  w.G = take(S);
  w.part = reinterpret_cast<float*>(take(S * nt));
  w.cesum = reinterpret_cast<float*>(take(nce));
  w.cecnt = take(nce);
  w.words = o;
  return w;
}

// ---- keys of a caller's errors (dlmpi_lovasz_rank) ----

__global__ __launch_bounds__(256) void lovasz_keys_kernel(const float* __restrict__ err,
                                                          const uint8_t* __restrict__ fg,
                                                          const uint8_t* __restrict__ valid, int64_t n, int64_t L,
                                                          unsigned* __restrict__ key, unsigned* __restrict__ pay) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const bool v = valid[i] != 0;
    key[i] = v ? lv_key(err[i]) : kLvInvalid;
    pay[i] = (unsigned)(i % L) | (v && fg[i] ? kLvFg : 0u);
  }
}

__global__ __launch_bounds__(256) void lovasz_export_kernel(const unsigned* __restrict__ pay, int64_t n,
                                                            const double* __restrict__ segsum, int64_t S,
                                                            int* __restrict__ perm, float* __restrict__ seg_loss) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    perm[i] = (int)(pay[i] & ~kLvFg);
    if (i < S) seg_loss[i] = (float)segsum[i];
  }
}

// ---- error passes ----

// K keys and payloads per pixel, lse[m], the block's {sum (lse - x_t), count} over its valid pixels
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void lovasz_softmax_err_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                                 int64_t HW, int64_t M,
                                                                 const int64_t* __restrict__ labels,
                                                                 int64_t ignore_index, int per_image, int64_t L,
                                                                 float* __restrict__ lse, unsigned* __restrict__ key,
                                                                 unsigned* __restrict__ pay,
                                                                 float* __restrict__ cesum,
                                                                 unsigned* __restrict__ cecnt) {
  __shared__ float shf[4];
  __shared__ unsigned shu[4];
  float ce[1] = {0.f};
  unsigned cnt[1] = {0u};
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const float* x = logits + n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    const int64_t idx = per_image ? p : m;
    const int64_t a0 = (per_image ? n * K : 0) * L + idx;
    float l, xt = 0.f;
    if constexpr (KC > 0) {
      float v[KC], w[KC];
      pix_load<KC, VEC>(x, st.sk, v);
#pragma unroll
      for (int k = 0; k < KC; ++k) w[k] = v[k];
      const PixSoftmax r = pix_softmax_reg<KC>(w, lab);
      l = r.mx + __logf(r.s);
      xt = r.xt;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const bool fg = keep && (int64_t)c == lab;
        const float e = fabsf((fg ? 1.f : 0.f) - __expf(v[c] - l));
        key[a0 + c * L] = keep ? lv_key(e) : kLvInvalid;
        pay[a0 + c * L] = (unsigned)idx | (fg ? kLvFg : 0u);
      }
    } else {
      l = pix_online_lse(x, st.sk, K);
      if (keep) xt = x[lab * st.sk];
      for (int c = 0; c < K; ++c) {
        const bool fg = keep && (int64_t)c == lab;
        const float e = fabsf((fg ? 1.f : 0.f) - __expf(x[c * st.sk] - l));
        key[a0 + c * L] = keep ? lv_key(e) : kLvInvalid;
        pay[a0 + c * L] = (unsigned)idx | (fg ? kLvFg : 0u);
      }
    }
    lse[m] = l;
    if (keep) {
      ce[0] += l - xt;
      cnt[0] += 1u;
    }
  }
  pix_block_sums<1, 1>(ce, cnt, shf, shu);
  if (threadIdx.x == 0) {
    cesum[blockIdx.x] = ce[0];
    cecnt[blockIdx.x] = cnt[0];
  }
}

__global__ __launch_bounds__(256) void lovasz_hinge_err_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ target, int64_t HW, int64_t M,
                                                               int per_image, int64_t L, unsigned* __restrict__ key,
                                                               unsigned* __restrict__ pay, float* __restrict__ cesum,
                                                               unsigned* __restrict__ cecnt) {
  __shared__ float shf[4];
  __shared__ unsigned shu[4];
  float ce[1] = {0.f};
  unsigned cnt[1] = {0u};
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const float x = logits[m], t = target[m];
    const bool fg = t > 0.5f;
    const float e = 1.f - x * (fg ? 1.f : -1.f);
    const int64_t idx = per_image ? m % HW : m;   // segment n holds [n HW, (n + 1) HW): key[m] either way
    key[m] = lv_key(e);
    pay[m] = (unsigned)idx | (fg ? kLvFg : 0u);
    ce[0] += lv_bce_elem(x, t);
    cnt[0] += 1u;
  }
  pix_block_sums<1, 1>(ce, cnt, shf, shu);
  if (threadIdx.x == 0) {
    cesum[blockIdx.x] = ce[0];
    cecnt[blockIdx.x] = cnt[0];
  }
}

// ---- the segmented stable LSD radix sort: grid (tile, segment) ----

__global__ __launch_bounds__(256) void lovasz_hist_kernel(const unsigned* __restrict__ key, int64_t L, int64_t ntiles,
                                                          int shift, unsigned* __restrict__ tab) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t seg = blockIdx.y, i0 = blockIdx.x * (int64_t)kLvTile;
  const unsigned* k = key + seg * L;
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const int64_t i = i0 + r * 256 + threadIdx.x;
    if (i < L) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);   // integer, in LDS: exact in any order
  }
  __syncthreads();
  tab[(seg * 256 + threadIdx.x) * ntiles + blockIdx.x] = h[threadIdx.x];
}

// row blockIdx.x of [rows][len]: exclusive scan in place, the row's sum -> tot[row]
__global__ __launch_bounds__(256) void lovasz_rowscan_kernel(unsigned* __restrict__ tab, int64_t len,
                                                             unsigned* __restrict__ tot) {
  __shared__ unsigned sh[4];
  unsigned* p = tab + blockIdx.x * len;
  unsigned carry = 0u;
  for (int64_t j0 = 0; j0 < len; j0 += 256) {
    const int64_t j = j0 + threadIdx.x;
    const unsigned v = j < len ? p[j] : 0u;
    unsigned total;
    const unsigned ex = lv_block_excl(v, sh, total);
    if (j < len) p[j] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void lovasz_scatter_kernel(const unsigned* __restrict__ kin,
                                                             const unsigned* __restrict__ pin,
                                                             unsigned* __restrict__ kout, unsigned* __restrict__ pout,
                                                             int64_t L, int64_t ntiles, int shift,
                                                             const unsigned* __restrict__ tab,
                                                             const unsigned* __restrict__ tot) {
  __shared__ unsigned run[256];       // where the next item of digit d goes
  __shared__ unsigned wcnt[4][256];   // this round's items of digit d in wave w
  __shared__ unsigned sh[4];
  const int64_t seg = blockIdx.y, i0 = blockIdx.x * (int64_t)kLvTile, base = seg * L;
  const int wv = threadIdx.x >> 6;
  unsigned total;
  const unsigned dbase = lv_block_excl(tot[seg * 256 + threadIdx.x], sh, total);
  run[threadIdx.x] = dbase + tab[(seg * 256 + threadIdx.x) * ntiles + blockIdx.x];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0u;
  __syncthreads();
  const unsigned long long below = lv_below();
  for (int r = 0; r < kLvRounds; ++r) {
    const int64_t i = i0 + r * 256 + threadIdx.x;
    const bool act = i < L;
    const unsigned k = act ? kin[base + i] : 0u, p = act ? pin[base + i] : 0u;
    const unsigned d = (k >> shift) & 255u;
    unsigned long long same = __ballot(act);   // the active lanes of this wave with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(act && bit);
      same &= bit ? bal : ~bal;
    }
    const unsigned rank = (unsigned)__popcll(same & below);
    if (act && rank == 0u) wcnt[wv][d] = (unsigned)__popcll(same);
    __syncthreads();
    if (act) {
      unsigned pos = run[d] + rank;
      for (int w = 0; w < wv; ++w) pos += wcnt[w][d];
      if ((int64_t)pos < L) {
        kout[base + pos] = k;
        pout[base + pos] = p;
      }
    }
    __syncthreads();
    run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0u;
    __syncthreads();
  }
}

// ---- Jaccard gradient over the sorted payloads ----

__global__ __launch_bounds__(256) void lovasz_fgcount_kernel(const unsigned* __restrict__ pay, int64_t L,
                                                             int64_t ntiles, unsigned* __restrict__ tilefg) {
  __shared__ unsigned shu[4];
  const int64_t seg = blockIdx.y, i0 = blockIdx.x * (int64_t)kLvTile;
  unsigned cnt[1] = {0u};
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const int64_t i = i0 + r * 256 + threadIdx.x;
    if (i < L) cnt[0] += pay[seg * L + i] >> 31;
  }
  pix_block_sums<0, 1>(nullptr, cnt, nullptr, shu);
  if (threadIdx.x == 0) tilefg[seg * ntiles + blockIdx.x] = cnt[0];
}

__global__ __launch_bounds__(256) void lovasz_jaccard_kernel(const unsigned* __restrict__ key,
                                                             const unsigned* __restrict__ pay, int64_t L,
                                                             int64_t ntiles, const unsigned* __restrict__ tilefg,
                                                             const unsigned* __restrict__ G, int hinge,
                                                             float* __restrict__ g, float* __restrict__ part) {
  __shared__ unsigned wfg[4];
  __shared__ float shf[4];
  const int64_t seg = blockIdx.y, i0 = blockIdx.x * (int64_t)kLvTile, base = seg * L;
  const int wv = threadIdx.x >> 6;
  const int64_t Gs = G[seg];
  int64_t run = tilefg[seg * ntiles + blockIdx.x];   // fg items before this tile
  const unsigned long long below = lv_below();
  float acc[1] = {0.f};
  for (int r = 0; r < kLvRounds; ++r) {
    const int64_t i = i0 + r * 256 + threadIdx.x;
    const bool act = i < L;
    const unsigned k = act ? key[base + i] : kLvInvalid, p = act ? pay[base + i] : 0u;
    const bool fg = (p >> 31) != 0u;
    const unsigned long long bal = __ballot(fg);
    if ((threadIdx.x & 63) == 0) wfg[wv] = (unsigned)__popcll(bal);
    __syncthreads();
    int64_t F = run + __popcll(bal & below);
    for (int w = 0; w < wv; ++w) F += wfg[w];
    run += wfg[0] + wfg[1] + wfg[2] + wfg[3];
    if (act) {
      float gv = 0.f;
      if (k != kLvInvalid) {   // valid items come first, so i is the rank
        const int64_t U = Gs + i - F;
        const double gd = fg ? 1.0 / (double)U
                             : U == 0 ? 1.0 : (double)(Gs - F) / ((double)U * (double)(U + 1));
        gv = (float)gd;
        float e = lv_err(k);
        if (hinge) e = e <= 0.f ? 0.f : e;   // max(e, 0) that keeps a NaN
        acc[0] += e * gv;
      }
      const int64_t idx = p & ~kLvFg;
      if (idx < L) g[base + idx] = gv;
    }
    __syncthreads();
  }
  pix_block_sums<1, 0>(acc, nullptr, shf, nullptr);
  if (threadIdx.x == 0) part[seg * ntiles + blockIdx.x] = acc[0];
}

__device__ __forceinline__ double lv_block_sum_d(double v, double* sh) {
  v = warp_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(256) void lovasz_segsum_kernel(const float* __restrict__ part, int64_t ntiles,
                                                            double* __restrict__ segsum) {
  __shared__ double sh[4];
  double a = 0.0;
  for (int64_t j = threadIdx.x; j < ntiles; j += 256) a += (double)part[blockIdx.x * ntiles + j];
  a = lv_block_sum_d(a, sh);
  if (threadIdx.x == 0) segsum[blockIdx.x] = a;
}

// One block.  Ns samples of K segments (Ns = 1 without per_image): coef[s] = 1 / (Ns * the sample's counted
// segments) on a counted segment, 0 elsewhere; loss = lovasz_weight * sum coef segsum + ce_weight * cesum / n_valid
// (the CE term is left out at ce_weight = 0); stats = {n_valid, counted segments, G[0..S)}.
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* __restrict__ segsum,
                                                            const unsigned* __restrict__ G, int Ns, int K, int all,
                                                            const float* __restrict__ cesum,
                                                            const unsigned* __restrict__ cecnt, int nce,
                                                            float ce_weight, float lovasz_weight,
                                                            float* __restrict__ coef, int* __restrict__ stats,
                                                            float* __restrict__ loss, float* __restrict__ den) {
  __shared__ double sh[4];
  __shared__ unsigned shu[8];
  double lov = 0.0, ce = 0.0;
  unsigned u[2] = {0u, 0u};   // counted segments, valid pixels
  for (int n = threadIdx.x; n < Ns; n += 256) {
    unsigned cnt = 0u;
    for (int c = 0; c < K; ++c) cnt += (all || G[(int64_t)n * K + c] > 0u) ? 1u : 0u;
    const double inv = cnt ? 1.0 / ((double)Ns * (double)cnt) : 0.0;
    double s = 0.0;
    for (int c = 0; c < K; ++c) {
      const int64_t sg = (int64_t)n * K + c;
      const bool counted = all || G[sg] > 0u;
      coef[sg] = counted ? (float)inv : 0.f;
      stats[2 + sg] = (int)G[sg];
      if (counted) s += segsum[sg];
    }
    lov += s * inv;
    u[0] += cnt;
  }
  for (int j = threadIdx.x; j < nce; j += 256) {
    ce += (double)cesum[j];
    u[1] += cecnt[j];
  }
  lov = lv_block_sum_d(lov, sh);
  ce = lv_block_sum_d(ce, sh);
  pix_block_sums<0, 2>(nullptr, u, nullptr, shu);
  if (threadIdx.x == 0) {
    double v = (double)lovasz_weight * lov;
    if (ce_weight != 0.f) v += (double)ce_weight * (ce / (double)u[1]);
    *loss = (float)v;
    *den = (float)u[1];
    stats[0] = (int)u[1];
    stats[1] = (int)u[0];
  }
}

// ---- backward ----

// dx_j = p_j (a_j - sum_c a_c p_c) + cs (p_j - [j = t]),  a_c = -+g_c coef_c lovasz_weight go,  cs = ce_weight go /
// n_valid; exact zeros at invalid pixels
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void lovasz_softmax_bwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                                 int64_t HW, int64_t M,
                                                                 const int64_t* __restrict__ labels,
                                                                 int64_t ignore_index, int per_image, int64_t L,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ g,
                                                                 const float* __restrict__ coef,
                                                                 const float* __restrict__ den,
                                                                 const float* __restrict__ go, float ce_weight,
                                                                 float lovasz_weight, float* __restrict__ dlogits) {
  const float gout = go ? *go : 1.f;
  const float lw = lovasz_weight * gout;
  const float cs = ce_weight != 0.f ? ce_weight * gout / *den : 0.f;
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const int64_t off = n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index);
    const int64_t s0 = per_image ? n * K : 0;
    const int64_t a0 = s0 * L + (per_image ? p : m);
    const float l = lse[m];
    if constexpr (KC > 0) {
      float v[KC], a[KC];
      if (keep) {
        pix_load<KC, VEC>(logits + off, st.sk, v);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          v[c] = __expf(v[c] - l);
          a[c] = ((int64_t)c == lab ? -lw : lw) * (g[a0 + c * L] * coef[s0 + c]);
          dot += a[c] * v[c];
        }
#pragma unroll
        for (int c = 0; c < KC; ++c) v[c] = v[c] * (a[c] - dot) + (v[c] - ((int64_t)c == lab ? 1.f : 0.f)) * cs;
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) v[c] = 0.f;
      }
      pix_store<KC, VEC>(dlogits + off, st.sk, v);
    } else {
      if (keep) {
        float dot = 0.f;
        for (int c = 0; c < K; ++c) {
          const float pc = __expf(logits[off + c * st.sk] - l);
          dot += ((int64_t)c == lab ? -lw : lw) * (g[a0 + c * L] * coef[s0 + c]) * pc;
        }
        for (int c = 0; c < K; ++c) {
          const float pc = __expf(logits[off + c * st.sk] - l);
          const float ac = ((int64_t)c == lab ? -lw : lw) * (g[a0 + c * L] * coef[s0 + c]);
          dlogits[off + c * st.sk] = pc * (ac - dot) + (pc - ((int64_t)c == lab ? 1.f : 0.f)) * cs;
        }
      } else {
        for (int c = 0; c < K; ++c) dlogits[off + c * st.sk] = 0.f;
      }
    }
  }
}

// dx = -(2 fg - 1) g coef lovasz_weight go [e > 0] + bce_weight go (sigmoid(x) - t) / M
__global__ __launch_bounds__(256) void lovasz_hinge_bwd_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ target, int64_t HW, int64_t M,
                                                               int per_image, const float* __restrict__ g,
                                                               const float* __restrict__ coef,
                                                               const float* __restrict__ go, float bce_weight,
                                                               float lovasz_weight, float* __restrict__ dlogits) {
  const float gout = go ? *go : 1.f;
  const float lw = lovasz_weight * gout;
  const float bs = bce_weight != 0.f ? bce_weight * gout / (float)M : 0.f;
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const float x = logits[m], t = target[m];
    const float sgn = t > 0.5f ? 1.f : -1.f;
    const float e = 1.f - x * sgn;
    float d = e > 0.f ? -sgn * lw * (g[m] * coef[per_image ? m / HW : 0]) : 0.f;
    if (bce_weight != 0.f) d += (1.f / (1.f + __expf(-x)) - t) * bs;
    dlogits[m] = d;
  }
}

// ---- host side ----

static inline unsigned lv_stream_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b > 16384 ? 16384 : b < 1 ? 1 : b);
}
static inline bool lv_shape_ok(int64_t S, int64_t L) { return S >= 1 && S <= kLvSegMax && L >= 1 && L < 2147483648LL; }

// keys / payloads in key[0] / pay[0] -> sorted there again (4 passes), g[S][L], segsum[S], G[S]
static void lv_chain(const LvWs& w, int64_t S, int64_t L, int hinge, float* g, hipStream_t s) {
  const int64_t nt = lv_tiles(L);
  const dim3 grid((unsigned)nt, (unsigned)S), blk(256);
  for (int pass = 0; pass < 4; ++pass) {
    const int a = pass & 1, b = a ^ 1, shift = 8 * pass;
    hipLaunchKernelGGL(lovasz_hist_kernel, grid, blk, 0, s, w.key[a], L, nt, shift, w.tab);
    hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3((unsigned)(S * 256)), blk, 0, s, w.tab, nt, w.tot);
    hipLaunchKernelGGL(lovasz_scatter_kernel, grid, blk, 0, s, w.key[a], w.pay[a], w.key[b], w.pay[b], L, nt, shift,
                       w.tab, w.tot);
  }
  hipLaunchKernelGGL(lovasz_fgcount_kernel, grid, blk, 0, s, w.pay[0], L, nt, w.tilefg);
  hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3((unsigned)S), blk, 0, s, w.tilefg, nt, w.G);
  hipLaunchKernelGGL(lovasz_jaccard_kernel, grid, blk, 0, s, w.key[0], w.pay[0], L, nt, w.tilefg, w.G, hinge, g,
                     w.part);
  hipLaunchKernelGGL(lovasz_segsum_kernel, dim3((unsigned)S), blk, 0, s, w.part, nt, w.segsum);
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_lovasz_tile() { return kLvTile; }
extern "C" int64_t dlmpi_lovasz_ws_words(int64_t S, int64_t L, int64_t M) {
  if (!lv_shape_ok(S, L) || M < 1) return -1;
  return lv_ws(nullptr, S, L, M).words;
}

extern "C" hipError_t dlmpi_lovasz_rank(const float* err, const uint8_t* fg, const uint8_t* valid, int64_t S, int64_t L,
                                        int hinge, uint32_t* ws, float* g, int32_t* perm, float* seg_loss,
                                        hipStream_t s) {
  if (!lv_shape_ok(S, L)) return hipErrorInvalidValue;
  const LvWs w = lv_ws(ws, S, L, 1);
  const int64_t n = S * L;
  hipLaunchKernelGGL(lovasz_keys_kernel, dim3(lv_stream_blocks(n)), dim3(256), 0, s, err, fg, valid, n, L, w.key[0],
                     w.pay[0]);
  lv_chain(w, S, L, hinge, g, s);
  hipLaunchKernelGGL(lovasz_export_kernel, dim3(lv_stream_blocks(n)), dim3(256), 0, s, w.pay[0], n, w.segsum, S, perm,
                     seg_loss);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_lovasz_softmax_fwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                               int64_t HW, const int64_t* labels, int64_t ignore_index, int per_image,
                                               int classes_all, float ce_weight, float lovasz_weight, float* lse,
                                               uint32_t* ws, float* g, float* coef, int32_t* stats, float* loss,
                                               float* den, hipStream_t s) {
  if (K < 2 || K > 256 || HW < 1 || N < 1) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW, S = per_image ? (int64_t)N * K : K, L = per_image ? HW : M;
  if (!lv_shape_ok(S, L)) return hipErrorInvalidValue;
  const LvWs w = lv_ws(ws, S, L, M);
  const int nce = lv_err_blocks(M);
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, nullptr, K, sn, sk, sp);
  PIX_DISPATCH(lovasz_softmax_err_kernel, dim3((unsigned)nce), vec, logits, st, K, HW, M, labels, ignore_index,
               per_image, L, lse, w.key[0], w.pay[0], w.cesum, w.cecnt);
  lv_chain(w, S, L, 0, g, s);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, s, w.segsum, w.G, per_image ? N : 1, K, classes_all,
                     w.cesum, w.cecnt, nce, ce_weight, lovasz_weight, coef, stats, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_lovasz_softmax_bwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                               int64_t HW, const int64_t* labels, int64_t ignore_index, int per_image,
                                               const float* lse, const float* g, const float* coef, const float* den,
                                               const float* go, float ce_weight, float lovasz_weight, float* dlogits,
                                               hipStream_t s) {
  if (K < 2 || K > 256 || HW < 1 || N < 1 || !den) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW, L = per_image ? HW : M;
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, dlogits, K, sn, sk, sp);
  PIX_DISPATCH(lovasz_softmax_bwd_kernel, dim3(lv_stream_blocks(M)), vec, logits, st, K, HW, M, labels, ignore_index,
               per_image, L, lse, g, coef, den, go, ce_weight, lovasz_weight, dlogits);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_lovasz_hinge_fwd(const float* logits, const float* target, int N, int64_t HW,
                                             int per_image, float bce_weight, float lovasz_weight, uint32_t* ws,
                                             float* g, float* coef, int32_t* stats, float* loss, float* den,
                                             hipStream_t s) {
  if (HW < 1 || N < 1) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW, S = per_image ? N : 1, L = per_image ? HW : M;
  if (!lv_shape_ok(S, L)) return hipErrorInvalidValue;
  const LvWs w = lv_ws(ws, S, L, M);
  const int nce = lv_err_blocks(M);
  hipLaunchKernelGGL(lovasz_hinge_err_kernel, dim3((unsigned)nce), dim3(256), 0, s, logits, target, HW, M, per_image,
                     L, w.key[0], w.pay[0], w.cesum, w.cecnt);
  lv_chain(w, S, L, 1, g, s);
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, s, w.segsum, w.G, per_image ? N : 1, 1, 1, w.cesum,
                     w.cecnt, nce, bce_weight, lovasz_weight, coef, stats, loss, den);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_lovasz_hinge_bwd(const float* logits, const float* target, int N, int64_t HW,
                                             int per_image, const float* g, const float* coef, const float* go,
                                             float bce_weight, float lovasz_weight, float* dlogits, hipStream_t s) {
  if (HW < 1 || N < 1) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  hipLaunchKernelGGL(lovasz_hinge_bwd_kernel, dim3(lv_stream_blocks(M)), dim3(256), 0, s, logits, target, HW, M,
                     per_image, g, coef, go, bce_weight, lovasz_weight, dlogits);
  return hipGetLastError();
}
