// Online hard example mining for the pixel-wise cross-entropy and BCE: the loss is the (weighted) mean over
// the hardest pixels of the batch, chosen by an exact, deterministic k-th-largest selection on the device.
//
// Definition.  Per pixel m: l_m = max(0, lse_m - x_m[t_m]) in the fp32 arithmetic of pixel_ce_fwd_kernel
// (pixel_softmax.h), valid(m) = pix_kept(label); the binary form has l_m = max(x, 0) - x t + log1p(exp(-|x|))
// and every pixel valid.  With n_valid the device's count of valid pixels,
//     k = min(n_valid, max(min_kept, ceil(keep_ratio * (double)n_valid)))       (one fp64 product, fp64 ceil)
// t_k = the k-th largest l over the valid pixels, cut = t_k, or min(tau, t_k) with a threshold (tau =
// -log(thresh), rounded once to fp32 by the host), S = {m valid : l_m >= cut}: every tie at the cut is in S,
// so |S| >= k and S depends on no traversal order.  loss = sum_S w[t] l / sum_S w[t]; the gradient is the plain
// loss's expression with den = sum_S w[t] on S and an exact zero elsewhere.  A NaN l gets the largest key (it is
// selected; the loss is then NaN), n_valid = 0 gives 0 / 0 = NaN and a zero gradient.
//
// Selection: a three-level radix select on the fp32 bit patterns.  l >= 0, so its bits order as unsigned
// integers; bit 31 is the "not valid" mark (ignored pixels are stored as -1).  Level 1 histograms bits 30..20
// (2048 bins), level 2 bits 19..9 (2048 bins) of the keys in level 1's bin, level 3 bits 8..0 (512 bins) of the
// keys in level 2's bin.  Histograms are uint32 in LDS per block, flushed with integer atomics (zero bins
// skipped): exact in any order.  Exact zeros (common once a model is confident) and invalid pixels never touch a
// histogram: each lane counts them in a register, one block sum and one atomic per block add them to two
// counters, and a search puts the zeros into bin 0 while the prefix so far is all zero.
//
// Passes (M pixels, K classes; bytes per pixel of the K = 2 softmax form):
//   zero         the three histograms and two counters (one allocation).  A kernel, not hipMemsetAsync: the
//                chain is recorded into captured graphs, where it then consists of kernel nodes only.
//   fwd          the plain forward's per-pixel work in its three forms (registers / online / LDS tile), writes
//                lse and nll (l, or -1 for an ignored pixel) and the level-1 histogram     8 + 8 read, 4 + 4 written
//   hist<2>      every block repeats the level-1 search (a descending scan of 2048 counts in LDS; k is formed
//                here from n_valid), then streams nll with 16-byte loads and histograms bits 19..9    4 read
//   hist<3>      the level-2 search, then bits 8..0                                                   4 read
//   sum          the level-3 search gives t_k bit-exactly; {sum w l, sum w, count} of S per block      4 read
//                (+ 8 for the label, only with a class weight)
//   finish       one block, fp64, fixed order: loss, den, n_selected
// Fusing each search into the next pass saves the one-block launches between passes; block 0 writes what it
// found into `state` for the passes after it, so nothing is read by the host.
// hist<1> is the level-1 histogram of a caller's nll buffer (dlmpi_ohem_select).
//
// Wave-level aggregation of the LDS atomics (lanes that hit the first active lane's bin issue one atomic) is a
// run-time switch, dlmpi_set_ohem_aggregate, for benchmarks/ohem_bench.py; profiles/ohem/README.md says which
// form is the default and why.
#include <cstring>

#include "pixel_softmax.h"

namespace dlmpi {

// words of the zeroed workspace
constexpr int kOhemH1 = 0, kOhemH2 = 2048, kOhemH3 = 4096, kOhemNValid = 4608, kOhemNZero = 4609;
constexpr int kOhemWsWords = 4616;
// words of the state vector: k, n_valid, n_selected, the bits of cut, then the chain's own {bin, rank left}
enum { kStK = 0, kStNValid = 1, kStNSel = 2, kStCut = 3, kStBin1 = 4, kStRem1 = 5, kStBin2 = 6, kStRem2 = 7 };
constexpr unsigned kOhemInvalid = 0x80000000u;
constexpr int kOhemStreamBlocksMax = 512;

struct OhemSel {
  double keep_ratio;
  unsigned min_kept;
  unsigned tau_bits;   // the bits of tau (> 0, finite)
  int has_tau;
};

// max(0, d) that keeps a NaN (fmaxf would drop it) and turns -0 into +0: bit 31 stays free
__device__ __forceinline__ float ohem_clamp(float d) { return d <= 0.f ? 0.f : d; }
// the sort key of a valid loss: its bits, a NaN above everything
__device__ __forceinline__ unsigned ohem_key(float l) { return l != l ? 0x7FC00000u : __float_as_uint(l); }
__device__ __forceinline__ bool ohem_selected(unsigned key, unsigned cut) { return (int)key >= (int)cut; }

__device__ __forceinline__ float ohem_bce_elem(float x, float t) {   // loss.hip's bce_elem
  return fmaxf(x, 0.f) - x * t + log1pf(__expf(-fabsf(x)));
}

__device__ __forceinline__ unsigned ohem_k(unsigned nv, const OhemSel& sel) {
  const double c = ceil(sel.keep_ratio * (double)nv);
  unsigned k = c >= (double)nv ? nv : (unsigned)c;
  k = k > sel.min_kept ? k : sel.min_kept;
  return k < nv ? k : nv;
}

// h[bin] += 1 for the lanes with act; called by whole waves.  agg: the lanes that share the first active lane's
// bin issue one atomic between them.
__device__ __forceinline__ void ohem_hist_add(unsigned* h, unsigned bin, bool act, int agg) {
  if (!agg) {
    if (act) atomicAdd(&h[bin], 1u);
    return;
  }
  const unsigned long long am = __ballot(act);
  if (!am) return;
  const int leader = __ffsll((long long)am) - 1;
  const unsigned lb = (unsigned)__shfl((int)bin, leader, 64);
  const bool same = act && bin == lb;
  const unsigned n = (unsigned)__popcll(__ballot(same));
  if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[lb], n);
  else if (act && !same) atomicAdd(&h[bin], 1u);
}

// level 1 of one key: zeros and invalid pixels into the lane's counters, the rest into the histogram
__device__ __forceinline__ void ohem_count(unsigned key, unsigned* h, unsigned* nvz, int agg) {
  const bool valid = !(key >> 31);
  nvz[0] += valid;
  nvz[1] += valid && key == 0u;
  ohem_hist_add(h, key >> 20, valid && key != 0u, agg);
}

__device__ __forceinline__ void ohem_zero_lds(unsigned* h, int nb) {
  for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0u;
  __syncthreads();
}
__device__ __forceinline__ void ohem_flush(const unsigned* h, int nb, unsigned* __restrict__ g) {
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256)
    if (h[i]) atomicAdd(&g[i], h[i]);
}
__device__ __forceinline__ void ohem_flush_counts(unsigned* nvz, unsigned* shu, unsigned* __restrict__ ws) {
  pix_block_sums<0, 2>(nullptr, nvz, nullptr, shu);
  if (threadIdx.x == 0) {
    if (nvz[0]) atomicAdd(&ws[kOhemNValid], nvz[0]);
    if (nvz[1]) atomicAdd(&ws[kOhemNZero], nvz[1]);
  }
}

// The bin that holds rank r (1 = the largest) of the 256 * PER counts g[] (+ extra0 in bin 0), and the rank left
// inside it.  Thread t owns the PER bins below NB - t * PER, top down; a block-wide exclusive scan of the owners'
// sums gives the count above each, and the one owner whose range holds r walks its bins.  r = 0 or r above the
// total: {0, 0}.  h: NB words, sh: 8 words of LDS, both free again on return.
template <int PER>
__device__ __forceinline__ void ohem_search(const unsigned* __restrict__ g, unsigned extra0, unsigned r, unsigned* h,
                                            unsigned* sh, unsigned& bin, unsigned& rem) {
  constexpr int NB = 256 * PER;
  for (int i = threadIdx.x; i < NB; i += 256) h[i] = g[i] + (i == 0 ? extra0 : 0u);
  if (threadIdx.x == 0) { sh[4] = 0u; sh[5] = 0u; }
  __syncthreads();
  const int top = NB - 1 - (int)threadIdx.x * PER;
  unsigned loc = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) loc += h[top - j];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = (unsigned)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  unsigned above = inc - loc;
  for (int w = 0; w < wv; ++w) above += sh[w];
  if (above < r && r <= above + loc) {
    unsigned a = above;
    for (int j = 0; j < PER; ++j) {
      const unsigned c = h[top - j];
      if (r <= a + c) {
        sh[4] = (unsigned)(top - j);
        sh[5] = r - a;
        break;
      }
      a += c;
    }
  }
  __syncthreads();
  bin = sh[4];
  rem = sh[5];
  __syncthreads();
}

// nll is streamed in 16-byte groups counted from the aligned address at or below it: group g holds pixels
// 4 g - ph .. 4 g + 3 - ph (ph = the buffer's offset within its 16 bytes), so one partial group at either end
// is read by single loads and everything between by one load.  Pixels outside [0, M) read as invalid.
struct OhemStream {
  const float* nll;
  const float* base;
  int ph;
  int64_t M, ngroups;
  __device__ __forceinline__ OhemStream(const float* p, int64_t m)
      : nll(p), base(p - pix_tile_phase(p)), ph(pix_tile_phase(p)), M(m), ngroups((m + pix_tile_phase(p) + 3) >> 2) {}
  __device__ __forceinline__ int64_t first(int64_t g) const { return 4 * g - ph; }
  __device__ __forceinline__ void load(int64_t g, unsigned* key) const {
    const int64_t m0 = first(g);
    if (g < ngroups && m0 >= 0 && m0 + 3 < M) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(base + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) key[e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = m0 + e;
        key[e] = (g < ngroups && m >= 0 && m < M) ? __float_as_uint(nll[m]) : kOhemInvalid;
      }
    }
  }
};

__global__ __launch_bounds__(256) void ohem_zero_kernel(unsigned* __restrict__ ws) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kOhemWsWords) ws[i] = 0u;
}

// LEVEL 1: the level-1 histogram and the two counters of a caller's nll.  LEVEL 2, 3: the previous level's
// search, then the histogram of the next bits of the keys under the prefix found so far.
template <int LEVEL>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ nll, int64_t M,
                                                        unsigned* __restrict__ ws, unsigned* __restrict__ state,
                                                        OhemSel sel, int agg) {
  __shared__ unsigned h[2048];
  __shared__ unsigned shu[8];
  constexpr int NB = LEVEL == 3 ? 512 : 2048;
  unsigned prefix = 0;
  if constexpr (LEVEL == 2) {
    const unsigned nv = ws[kOhemNValid], k = ohem_k(nv, sel);
    unsigned bin, rem;
    ohem_search<8>(ws + kOhemH1, ws[kOhemNZero], k, h, shu, bin, rem);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      state[kStK] = k;
      state[kStNValid] = nv;
      state[kStBin1] = bin;
      state[kStRem1] = rem;
    }
    prefix = bin;
  } else if constexpr (LEVEL == 3) {
    const unsigned bin1 = state[kStBin1];
    unsigned bin, rem;
    ohem_search<8>(ws + kOhemH2, bin1 == 0u ? ws[kOhemNZero] : 0u, state[kStRem1], h, shu, bin, rem);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      state[kStBin2] = bin;
      state[kStRem2] = rem;
    }
    prefix = bin1 << 11 | bin;
  }
  ohem_zero_lds(h, NB);
  unsigned nvz[2] = {0u, 0u};
  const OhemStream in(nll, M);
  for (int64_t g0 = blockIdx.x * (int64_t)256; g0 < in.ngroups; g0 += (int64_t)gridDim.x * 256) {
    unsigned key[4];
    in.load(g0 + threadIdx.x, key);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool live = !(key[e] >> 31) && key[e] != 0u;
      if constexpr (LEVEL == 1) ohem_count(key[e], h, nvz, agg);
      else if constexpr (LEVEL == 2) ohem_hist_add(h, (key[e] >> 9) & 2047u, live && (key[e] >> 20) == prefix, agg);
      else ohem_hist_add(h, key[e] & 511u, live && (key[e] >> 9) == prefix, agg);
    }
  }
  ohem_flush(h, NB, ws + (LEVEL == 1 ? kOhemH1 : LEVEL == 2 ? kOhemH2 : kOhemH3));
  if constexpr (LEVEL == 1) ohem_flush_counts(nvz, shu, ws);
}

// The level-3 search completes t_k; partial[blk] = {sum w l, sum w} and pcount[blk] = |S| over the block's pixels.
__global__ __launch_bounds__(256) void ohem_sum_kernel(const float* __restrict__ nll, int64_t M,
                                                       const int64_t* __restrict__ labels,
                                                       const float* __restrict__ weight,
                                                       const unsigned* __restrict__ ws, unsigned* __restrict__ state,
                                                       OhemSel sel, float* __restrict__ partial,
                                                       unsigned* __restrict__ pcount) {
  __shared__ unsigned h[512];
  __shared__ unsigned shu[8];
  __shared__ float shf[8];
  const unsigned bin1 = state[kStBin1], bin2 = state[kStBin2];
  unsigned bin3, rem;
  ohem_search<2>(ws + kOhemH3, (bin1 | bin2) == 0u ? ws[kOhemNZero] : 0u, state[kStRem2], h, shu, bin3, rem);
  unsigned cut = bin1 << 20 | bin2 << 9 | bin3;
  if (sel.has_tau && sel.tau_bits < cut) cut = sel.tau_bits;
  if (blockIdx.x == 0 && threadIdx.x == 0) state[kStCut] = cut;
  float f[2] = {0.f, 0.f};
  unsigned cnt[1] = {0u};
  const OhemStream in(nll, M);
  for (int64_t g0 = blockIdx.x * (int64_t)256; g0 < in.ngroups; g0 += (int64_t)gridDim.x * 256) {
    unsigned key[4];
    in.load(g0 + threadIdx.x, key);
    const int64_t m0 = in.first(g0 + threadIdx.x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!ohem_selected(key[e], cut)) continue;
      const float w = weight ? weight[labels[m0 + e]] : 1.f;
      f[0] += w * __uint_as_float(key[e]);
      f[1] += w;
      cnt[0] += 1u;
    }
  }
  pix_block_sums<2, 1>(f, cnt, shf, shu);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = f[0];
    partial[2 * blockIdx.x + 1] = f[1];
    pcount[blockIdx.x] = cnt[0];
  }
}

// loss = sum partial[.][0] / sum partial[.][1] in fp64, den = the denominator, n_selected = sum pcount
__global__ __launch_bounds__(256) void ohem_finish_kernel(const float* __restrict__ partial,
                                                          const unsigned* __restrict__ pcount, int nblk,
                                                          float* __restrict__ loss, float* __restrict__ den,
                                                          unsigned* __restrict__ state) {
  __shared__ double sh[2][4];
  __shared__ unsigned shu[4];
  double a = 0.0, b = 0.0;
  unsigned c = 0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    a += (double)partial[2 * i];
    b += (double)partial[2 * i + 1];
    c += pcount[i];
  }
  a = warp_sum_d(a);
  b = warp_sum_d(b);
  c = warp_sum_u(c);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][wv] = a; sh[1][wv] = b; shu[wv] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    b = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    *loss = (float)(a / b);
    *den = (float)b;
    state[kStNSel] = shu[0] + shu[1] + shu[2] + shu[3];
  }
}

// ---- softmax form: pixel_ce.hip's forward and backward kernels with the mining operands ----

// lse[m], nll[m] = l or -1, the level-1 histogram; K in registers (KC > 0) or online (KC = 0)
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void ohem_ce_fwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                          int64_t HW, int64_t M, const int64_t* __restrict__ labels,
                                                          int64_t ignore_index, float* __restrict__ lse,
                                                          float* __restrict__ nll, unsigned* __restrict__ ws,
                                                          int agg) {
  __shared__ unsigned h[2048];
  __shared__ unsigned shu[8];
  ohem_zero_lds(h, 2048);
  unsigned nvz[2] = {0u, 0u};
  for (int64_t mb = blockIdx.x * (int64_t)256; mb < M; mb += (int64_t)gridDim.x * 256) {   // whole waves stay in the loop
    const int64_t m = mb + threadIdx.x;
    unsigned key = kOhemInvalid;
    if (m < M) {
      const int64_t n = m / HW, p = m - n * HW;
      const float* x = logits + n * st.sn + p * st.sp;
      const int64_t lab = labels[m];
      const bool keep = pix_kept(lab, K, ignore_index);
      float l, xt = 0.f;
      if constexpr (KC > 0) {
        float v[KC];
        pix_load<KC, VEC>(x, st.sk, v);
        const PixSoftmax r = pix_softmax_reg<KC>(v, lab);
        l = r.mx + __logf(r.s);
        xt = r.xt;
      } else {
        l = pix_online_lse(x, st.sk, K);
        if (keep) xt = x[lab * st.sk];
      }
      lse[m] = l;
      if (keep) key = ohem_key(ohem_clamp(l - xt));
      nll[m] = keep ? __uint_as_float(key) : -1.f;
    }
    ohem_count(key, h, nvz, agg);
  }
  ohem_flush(h, 2048, ws + kOhemH1);
  ohem_flush_counts(nvz, shu, ws);
}

// class-last logits with K > 4 through LDS tiles of P pixels (pixel_ce_fwd_tile_kernel)
__global__ __launch_bounds__(256) void ohem_ce_fwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                               int64_t M, const int64_t* __restrict__ labels,
                                                               int64_t ignore_index, float* __restrict__ lse,
                                                               float* __restrict__ nll, unsigned* __restrict__ ws,
                                                               int agg) {
  extern __shared__ __align__(16) float tile[];
  __shared__ unsigned h[2048];
  __shared__ unsigned shu[8];
  ohem_zero_lds(h, 2048);
  unsigned nvz[2] = {0u, 0u};
  const int64_t ntiles = (M + P - 1) / P;
  const int k0 = threadIdx.x % K;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m0 = t * P;
    const int np = (int)(M - m0 < P ? M - m0 : P);
    pix_tile_copy<true>(tile, const_cast<float*>(logits + m0 * K), np * K, 0);
    __syncthreads();
    unsigned key = kOhemInvalid;
    if ((int)threadIdx.x < np) {
      const float* row = tile + threadIdx.x * K;
      const float l = pix_row_lse(row, K, k0);
      const int64_t m = m0 + threadIdx.x;
      const int64_t lab = labels[m];
      const bool keep = pix_kept(lab, K, ignore_index);
      lse[m] = l;
      if (keep) key = ohem_key(ohem_clamp(l - row[lab]));
      nll[m] = keep ? __uint_as_float(key) : -1.f;
    }
    ohem_count(key, h, nvz, agg);
    __syncthreads();
  }
  ohem_flush(h, 2048, ws + kOhemH1);
  ohem_flush_counts(nvz, shu, ws);
}

// dlogits[m][k] = (exp(x[m][k] - lse[m]) - [k == t]) * w[t] * go / den on S, exact zeros elsewhere
template <int KC, bool VEC>
__global__ __launch_bounds__(256) void ohem_ce_bwd_kernel(const float* __restrict__ logits, PixStrides st, int K,
                                                          int64_t HW, int64_t M, const int64_t* __restrict__ labels,
                                                          int64_t ignore_index, const float* __restrict__ weight,
                                                          const float* __restrict__ lse,
                                                          const float* __restrict__ nll,
                                                          const float* __restrict__ cutp,
                                                          const float* __restrict__ go, const float* __restrict__ den,
                                                          float* __restrict__ dlogits) {
  const float g0 = (go ? *go : 1.f) / *den;
  const unsigned cut = __float_as_uint(*cutp);
  for (int64_t m = blockIdx.x * (int64_t)256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t n = m / HW, p = m - n * HW;
    const int64_t off = n * st.sn + p * st.sp;
    const int64_t lab = labels[m];
    const bool keep = pix_kept(lab, K, ignore_index) && ohem_selected(__float_as_uint(nll[m]), cut);
    float g = 0.f;
    if (keep) g = g0 * (weight ? weight[lab] : 1.f);
    const float l = lse[m];
    if constexpr (KC > 0) {
      float v[KC];
      if (keep) {
        pix_load<KC, VEC>(logits + off, st.sk, v);
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = (__expf(v[k] - l) - ((int64_t)k == lab ? 1.f : 0.f)) * g;
      } else {
#pragma unroll
        for (int k = 0; k < KC; ++k) v[k] = 0.f;
      }
      pix_store<KC, VEC>(dlogits + off, st.sk, v);
    } else {
      if (keep) {
        for (int k = 0; k < K; ++k)
          dlogits[off + k * st.sk] = (__expf(logits[off + k * st.sk] - l) - ((int64_t)k == lab ? 1.f : 0.f)) * g;
      } else {
        for (int k = 0; k < K; ++k) dlogits[off + k * st.sk] = 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ohem_ce_bwd_tile_kernel(const float* __restrict__ logits, int K, int P,
                                                               int64_t M, const int64_t* __restrict__ labels,
                                                               int64_t ignore_index,
                                                               const float* __restrict__ weight,
                                                               const float* __restrict__ lse,
                                                               const float* __restrict__ nll,
                                                               const float* __restrict__ cutp,
                                                               const float* __restrict__ go,
                                                               const float* __restrict__ den,
                                                               float* __restrict__ dlogits) {
  extern __shared__ __align__(16) float tile[];
  const float g0 = (go ? *go : 1.f) / *den;
  const unsigned cut = __float_as_uint(*cutp);
  const int64_t ntiles = (M + P - 1) / P;
  const int k0 = threadIdx.x % K;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m0 = t * P;
    const int np = (int)(M - m0 < P ? M - m0 : P);
    const int nf = np * K;
    pix_tile_copy<true>(tile, const_cast<float*>(logits + m0 * K), nf, 0);
    __syncthreads();
    if ((int)threadIdx.x < np) {
      float* row = tile + threadIdx.x * K;
      const int64_t m = m0 + threadIdx.x;
      const int64_t lab = labels[m];
      int kk = k0;
      if (pix_kept(lab, K, ignore_index) && ohem_selected(__float_as_uint(nll[m]), cut)) {
        const float g = g0 * (weight ? weight[lab] : 1.f);
        const float l = lse[m];
        for (int k = 0; k < K; ++k) {
          row[kk] = (__expf(row[kk] - l) - ((int64_t)kk == lab ? 1.f : 0.f)) * g;
          kk = pix_row_next(kk, K);
        }
      } else {
        pix_row_zero(row, K, k0);
      }
    }
    __syncthreads();
    pix_tile_copy<false>(tile, dlogits + m0 * K, nf, 0);
    __syncthreads();
  }
}

// ---- binary form: one logit and one target per pixel, four pixels per lane; 16-byte access where vec ----

__global__ __launch_bounds__(256) void ohem_bce_fwd_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ target, int64_t M, int vec,
                                                           float* __restrict__ nll, unsigned* __restrict__ ws,
                                                           int agg) {
  __shared__ unsigned h[2048];
  __shared__ unsigned shu[8];
  ohem_zero_lds(h, 2048);
  unsigned nvz[2] = {0u, 0u};
  const int64_t ng = (M + 3) >> 2;
  for (int64_t g0 = blockIdx.x * (int64_t)256; g0 < ng; g0 += (int64_t)gridDim.x * 256) {
    const int64_t m0 = 4 * (g0 + threadIdx.x);
    unsigned key[4];
    if (vec && m0 + 3 < M) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(logits + m0), t = *reinterpret_cast<const f32x4*>(target + m0);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        key[e] = ohem_key(ohem_clamp(ohem_bce_elem(x[e], t[e])));
        o[e] = __uint_as_float(key[e]);
      }
      *reinterpret_cast<f32x4*>(nll + m0) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        key[e] = kOhemInvalid;
        if (m0 + e < M) {
          key[e] = ohem_key(ohem_clamp(ohem_bce_elem(logits[m0 + e], target[m0 + e])));
          nll[m0 + e] = __uint_as_float(key[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ohem_count(key[e], h, nvz, agg);
  }
  ohem_flush(h, 2048, ws + kOhemH1);
  ohem_flush_counts(nvz, shu, ws);
}

// dlogits = (sigmoid(x) - t) * go / |S| on S, exact zeros elsewhere (den = |S|)
__global__ __launch_bounds__(256) void ohem_bce_bwd_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ target, int64_t M, int vec,
                                                           const float* __restrict__ nll,
                                                           const float* __restrict__ cutp,
                                                           const float* __restrict__ go, const float* __restrict__ den,
                                                           float* __restrict__ dlogits) {
  const float g = (go ? *go : 1.f) / *den;
  const unsigned cut = __float_as_uint(*cutp);
  const int64_t ng = (M + 3) >> 2;
  for (int64_t gi = blockIdx.x * (int64_t)256 + threadIdx.x; gi < ng; gi += (int64_t)gridDim.x * 256) {
    const int64_t m0 = 4 * gi;
    if (vec && m0 + 3 < M) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(logits + m0), t = *reinterpret_cast<const f32x4*>(target + m0);
      const u32x4 key = *reinterpret_cast<const u32x4*>(nll + m0);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = ohem_selected(key[e], cut) ? (1.f / (1.f + __expf(-x[e])) - t[e]) * g : 0.f;
      *reinterpret_cast<f32x4*>(dlogits + m0) = o;
    } else {
      for (int e = 0; e < 4 && m0 + e < M; ++e) {
        const int64_t m = m0 + e;
        dlogits[m] = ohem_selected(__float_as_uint(nll[m]), cut)
                         ? (1.f / (1.f + __expf(-logits[m])) - target[m]) * g : 0.f;
      }
    }
  }
}

static inline unsigned ohem_ce_blocks(int64_t M) {   // pixel_ce.hip's forward grid
  int64_t b = (M + 255) / 256;
  return (unsigned)(b > 2048 ? 2048 : b < 1 ? 1 : b);
}
static inline unsigned ohem_group_blocks(int64_t M, int64_t cap) {   // a lane per four pixels (+ a partial group)
  int64_t b = ((M + 6) / 4 + 255) / 256;
  return (unsigned)(b > cap ? cap : b < 1 ? 1 : b);
}
static inline bool ohem_al16(const void* p) { return !((uintptr_t)p & 15); }

int g_ohem_agg = 0;

static bool ohem_sel(double keep_ratio, int64_t min_kept, int has_tau, float tau, int64_t M, OhemSel* sel) {
  if (!(keep_ratio > 0.0 && keep_ratio <= 1.0) || min_kept < 1 || M < 1 || M > 2147483647LL) return false;
  if (has_tau && !(tau > 0.f && tau < INFINITY)) return false;
  uint32_t tb = 0;
  memcpy(&tb, &tau, 4);
  *sel = OhemSel{keep_ratio, (unsigned)(min_kept > 2147483647LL ? 2147483647LL : min_kept), tb, has_tau ? 1 : 0};
  return true;
}

static void ohem_zero(unsigned* ws, hipStream_t s) {
  hipLaunchKernelGGL(ohem_zero_kernel, dim3((kOhemWsWords + 255) / 256), dim3(256), 0, s, ws);
}

// levels 2 and 3, the sum and the finish over a filled nll and level-1 histogram
static void ohem_select_tail(const float* nll, int64_t M, const int64_t* labels, const float* weight,
                             const OhemSel& sel, unsigned* ws, float* partial, unsigned* state, float* loss,
                             float* den, hipStream_t s) {
  const unsigned nblk = ohem_group_blocks(M, kOhemStreamBlocksMax);
  hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(nblk), dim3(256), 0, s, nll, M, ws, state, sel, g_ohem_agg);
  hipLaunchKernelGGL(ohem_hist_kernel<3>, dim3(nblk), dim3(256), 0, s, nll, M, ws, state, sel, g_ohem_agg);
  unsigned* pcount = reinterpret_cast<unsigned*>(partial + 2 * nblk);
  hipLaunchKernelGGL(ohem_sum_kernel, dim3(nblk), dim3(256), 0, s, nll, M, labels, weight, ws, state, sel, partial,
                     pcount);
  hipLaunchKernelGGL(ohem_finish_kernel, dim3(1), dim3(256), 0, s, partial, pcount, (int)nblk, loss, den, state);
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" void dlmpi_set_ohem_aggregate(int on) { g_ohem_agg = on ? 1 : 0; }
extern "C" int dlmpi_ohem_ws_words() { return kOhemWsWords; }
extern "C" int dlmpi_ohem_partial_floats(int64_t M) { return 3 * (int)ohem_group_blocks(M, kOhemStreamBlocksMax); }

extern "C" hipError_t dlmpi_ohem_select(const float* nll, int64_t M, double keep_ratio, int64_t min_kept, int has_tau,
                                        float tau, uint32_t* ws, float* partial, uint32_t* state, float* loss,
                                        float* den, hipStream_t s) {
  OhemSel sel;
  if (!ohem_sel(keep_ratio, min_kept, has_tau, tau, M, &sel)) return hipErrorInvalidValue;
  ohem_zero(ws, s);
  hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(ohem_group_blocks(M, kOhemStreamBlocksMax)), dim3(256), 0, s, nll, M,
                     ws, state, sel, g_ohem_agg);
  ohem_select_tail(nll, M, nullptr, nullptr, sel, ws, partial, state, loss, den, s);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_ohem_ce_fwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                        int64_t HW, const int64_t* labels, int64_t ignore_index, const float* weight,
                                        double keep_ratio, int64_t min_kept, int has_tau, float tau, float* lse,
                                        float* nll, uint32_t* ws, float* partial, uint32_t* state, float* loss,
                                        float* den, hipStream_t s) {
  OhemSel sel;
  if (K < 2 || K > 256 || HW < 1 || N < 1) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  if (!ohem_sel(keep_ratio, min_kept, has_tau, tau, M, &sel)) return hipErrorInvalidValue;
  ohem_zero(ws, s);
  const unsigned nblk = ohem_ce_blocks(M);
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, nullptr, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, nullptr, K, HW, sn, sk, sp);
  if (P > 0)
    hipLaunchKernelGGL(ohem_ce_fwd_tile_kernel, dim3(nblk), dim3(256), (size_t)P * K * sizeof(float), s, logits, K, P,
                       M, labels, ignore_index, lse, nll, ws, g_ohem_agg);
  else
    PIX_DISPATCH(ohem_ce_fwd_kernel, dim3(nblk), vec, logits, st, K, HW, M, labels, ignore_index, lse, nll, ws,
                 g_ohem_agg);
  ohem_select_tail(nll, M, labels, weight, sel, ws, partial, state, loss, den, s);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_ohem_ce_bwd(const float* logits, int64_t sn, int64_t sk, int64_t sp, int N, int K,
                                        int64_t HW, const int64_t* labels, int64_t ignore_index, const float* weight,
                                        const float* lse, const float* nll, const float* cut, const float* go,
                                        const float* den, float* dlogits, hipStream_t s) {
  if (K < 2 || K > 256 || HW < 1 || N < 1 || !den || !cut) return hipErrorInvalidValue;
  const int64_t M = (int64_t)N * HW;
  const PixStrides st{sn, sk, sp};
  const bool vec = pix_vec_ok(logits, dlogits, K, sn, sk, sp);
  const int P = pix_tile_pixels(logits, dlogits, K, HW, sn, sk, sp);
  if (P > 0) {
    int64_t b = (M + P - 1) / P;
    hipLaunchKernelGGL(ohem_ce_bwd_tile_kernel, dim3((unsigned)(b > 16384 ? 16384 : b)), dim3(256),
                       (size_t)P * K * sizeof(float), s, logits, K, P, M, labels, ignore_index, weight, lse, nll, cut,
                       go, den, dlogits);
  } else {
    int64_t b = (M + 255) / 256;
    PIX_DISPATCH(ohem_ce_bwd_kernel, dim3((unsigned)(b > 16384 ? 16384 : b)), vec, logits, st, K, HW, M, labels,
                 ignore_index, weight, lse, nll, cut, go, den, dlogits);
  }
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_ohem_bce_fwd(const float* logits, const float* target, int64_t M, double keep_ratio,
                                         int64_t min_kept, int has_tau, float tau, float* nll, uint32_t* ws,
                                         float* partial, uint32_t* state, float* loss, float* den, hipStream_t s) {
  OhemSel sel;
  if (!ohem_sel(keep_ratio, min_kept, has_tau, tau, M, &sel)) return hipErrorInvalidValue;
  ohem_zero(ws, s);
  const int vec = ohem_al16(logits) && ohem_al16(target) && ohem_al16(nll);
  hipLaunchKernelGGL(ohem_bce_fwd_kernel, dim3(ohem_group_blocks(M, 2048)), dim3(256), 0, s, logits, target, M, vec,
                     nll, ws, g_ohem_agg);
  ohem_select_tail(nll, M, nullptr, nullptr, sel, ws, partial, state, loss, den, s);
  return hipGetLastError();
}

extern "C" hipError_t dlmpi_ohem_bce_bwd(const float* logits, const float* target, int64_t M, const float* nll,
                                         const float* cut, const float* go, const float* den, float* dlogits,
                                         hipStream_t s) {
  if (M < 1 || M > 2147483647LL || !den || !cut) return hipErrorInvalidValue;
  const int vec = ohem_al16(logits) && ohem_al16(target) && ohem_al16(nll) && ohem_al16(dlogits);
  hipLaunchKernelGGL(ohem_bce_bwd_kernel, dim3(ohem_group_blocks(M, 16384)), dim3(256), 0, s, logits, target, M, vec,
                     nll, cut, go, den, dlogits);
  return hipGetLastError();
}
