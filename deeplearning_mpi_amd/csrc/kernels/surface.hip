// Surface-distance metrics of a segmentation: Hausdorff distance, its percentile (HD95) and the average symmetric
// surface distance (ASSD), per sample and class, exact in integers up to one fp64 root per value.
//
// Definition.  pred(q) = argmax_k logits (ties to the lowest index), gt(q) = label at the valid pixels (label not
// ignore_index and inside [0, K)), "no class" elsewhere; binary form: pred = [x > 0], gt = [t > 0.5], one class.
// For a map M and class c the edge set is {q : M(q) = c and a 4-neighbour of q has M != c}, a neighbour outside the
// image counting as outside (scipy's binary_erosion with the cross and border_value 0).  With P, G the edge sets of
// pred and gt for (n, c): D(A->B) = {sqrt(min_{s in B} |q - s|^2) : q in A}, the minimum an exact int32, the root fp64.
// metrics[n][c] = {max of both D, max over both directions of the `linear` percentile of D, the pooled mean}, all fp64
// and rounded once; counts[n][c] = {|P|, |G|}; NaN where both sets are empty, +inf where exactly one is.
//
// Four kernels of this file around one call of dlmpi_edt (edt.hip, unchanged):
//  1 surface_edge_kernel, one block per (sample, 32 x 32 tile).  The tile's two class maps with a one-pixel halo go
//    to LDS as uint16 (0xFFFF: no class, also outside the image); every thread then tests the four neighbours of its
//    four pixels in both maps from LDS.  Out: the int64 edge-label maps [2][N][H][W] (the class where the pixel is an
//    edge pixel of that map, else -1) and the tile's edge counts per (map, class), uint32 [2][N][K][T], every entry
//    written (an integer LDS histogram, so exact in any order).
//  - dlmpi_edt on the edge-label maps as 2 N samples of K classes, d2_in only: int32 [2 N][K][H][W].
//  2 surface_scan_kernel, one block per (map, sample): the exclusive scan of its K T counts in place, class-major,
//    which is at once the start of every (class, tile) run inside the sample's list; the class starts go to
//    segoff [2][N][K + 1].  A pixel is an edge of at most one class per map, so a sample's list has <= H W items.
//  3 surface_scatter_kernel, the grid of 1: a wave owns 8 rows of the tile and ranks its pixels of one (map, class)
//    by ballot in row-major order, the waves' counts chain through LDS; item = d2_in[other map][n][c][q] goes to
//    list[map][n][start + rank].  Stable: a list is in tile order, row-major inside a tile, on every run.
//  4 surface_select_kernel, one block per (n, c), over both directions' lists: integer maximum, fp64 sum of roots
//    in a fixed tree, and an exact radix select (8 bits a level, uint32 histograms in LDS) that carries both target
//    ranks lo and hi = lo + 1 through the same passes; the levels above the largest possible key (H-1)^2 + (W-1)^2
//    are skipped.  It applies the empty-set rules and writes the row.
// No host read, no float atomics, nothing needs zeroing: the same bits on every run, capturable.
//
// Limits (dlmpi_surface_ok): those of dlmpi_edt_ok for 2 N samples, K <= 256, N T < 2^31.  Workspace
// (dlmpi_surface_ws_bytes): 12 bytes per pixel and class (int32 d2_in of both maps, 8, and the transform's uint16
// plane, 4) + 24 per pixel (two int64 edge maps, two int32 lists) + the tile counts, 8 K bytes per tile.
#include "common.h"
#include "pixel_softmax.h"

namespace dlmpi {

constexpr int kSurfTile = 32;                 // tile edge of the edge and scatter passes
constexpr int kSurfHalo = kSurfTile + 2;
constexpr unsigned kSurfNone = 0xFFFFu;
constexpr int kSurfScanItems = 8;             // consecutive counts per thread of the scan

struct SurfTile {
  int64_t n;
  int t, y0, x0;
};
__device__ __forceinline__ SurfTile surf_tile(int tiles_x, int T) {
  SurfTile s;
  s.n = blockIdx.x / T;
  s.t = (int)(blockIdx.x - s.n * T);
  const int ty = s.t / tiles_x;
  s.y0 = ty * kSurfTile;
  s.x0 = (s.t - ty * tiles_x) * kSurfTile;
  return s;
}

// grid: N * T.  target: int64 labels (softmax form) or the fp32 target (BIN, logits contiguous [N][H][W], K = 1)
template <bool BIN>
__global__ __launch_bounds__(256) void surface_edge_kernel(const float* __restrict__ logits, PixStrides st,
                                                           const void* __restrict__ target, int64_t N, int K, int H,
                                                           int W, int tiles_x, int T, int64_t ignore_index,
                                                           int64_t* __restrict__ emap, uint32_t* __restrict__ tilecnt) {
  __shared__ uint16_t cls[2][kSurfHalo * kSurfHalo];
  __shared__ uint32_t hist[2][256];
  const SurfTile tl = surf_tile(tiles_x, T);
  const int64_t HW = (int64_t)H * W;
  hist[0][threadIdx.x] = 0u;
  hist[1][threadIdx.x] = 0u;
  for (int i = threadIdx.x; i < kSurfHalo * kSurfHalo; i += 256) {
    const int hy = i / kSurfHalo, hx = i - hy * kSurfHalo;
    const int y = tl.y0 + hy - 1, x = tl.x0 + hx - 1;
    unsigned p = kSurfNone, g = kSurfNone;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t q = (int64_t)y * W + x;
      if constexpr (BIN) {
        p = logits[tl.n * HW + q] > 0.f ? 0u : kSurfNone;
        g = static_cast<const float*>(target)[tl.n * HW + q] > 0.5f ? 0u : kSurfNone;
      } else {
        const int64_t lab = static_cast<const int64_t*>(target)[tl.n * HW + q];
        if (pix_kept(lab, K, ignore_index)) {
          const float* xq = logits + tl.n * st.sn + q * st.sp;
          float bv = xq[0];
          int bi = 0;
          for (int k = 1; k < K; ++k) {
            const float v = xq[k * st.sk];
            if (v > bv) { bv = v; bi = k; }
          }
          p = (unsigned)bi;
          g = (unsigned)lab;
        }
      }
    }
    cls[0][i] = (uint16_t)p;
    cls[1][i] = (uint16_t)g;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = r * 256 + threadIdx.x, ly = j >> 5, lx = j & 31;
    const int y = tl.y0 + ly, x = tl.x0 + lx;
    if (y < H && x < W) {
      const int ci = (ly + 1) * kSurfHalo + lx + 1;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const uint16_t* cm = cls[m];
        const unsigned c = cm[ci];
        const bool edge = c != kSurfNone && (cm[ci - kSurfHalo] != c || cm[ci + kSurfHalo] != c || cm[ci - 1] != c ||
                                             cm[ci + 1] != c);
        emap[((m * N + tl.n) * H + y) * W + x] = edge ? (int64_t)c : (int64_t)-1;
        if (edge) atomicAdd(&hist[m][c], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K; i += 256) {
    const int m = i / K, c = i - m * K;
    tilecnt[((m * N + tl.n) * K + c) * T + tl.t] = hist[m][c];
  }
}

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// grid: 2 * N.  cnt [2 N][K][T] -> its exclusive scan per (map, sample), in place; segoff [2 N][K + 1]
__global__ __launch_bounds__(256) void surface_scan_kernel(uint32_t* __restrict__ cnt, int K, int T,
                                                           uint32_t* __restrict__ segoff) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t L = (int64_t)K * T;
  uint32_t* base = cnt + blockIdx.x * L;
  uint32_t* so = segoff + (int64_t)blockIdx.x * (K + 1);
  uint32_t carry = 0u;
  for (int64_t i0 = 0; i0 < L; i0 += 256 * kSurfScanItems) {
    const int64_t i = i0 + (int64_t)threadIdx.x * kSurfScanItems;
    uint32_t v[kSurfScanItems], s = 0u;
#pragma unroll
    for (int e = 0; e < kSurfScanItems; ++e) {
      v[e] = i + e < L ? base[i + e] : 0u;
      s += v[e];
    }
    const uint32_t inc = wave_scan_incl(s, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    uint32_t ex = carry + inc - s, tot = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) ex += wsum[w];
      tot += wsum[w];
    }
#pragma unroll
    for (int e = 0; e < kSurfScanItems; ++e) {
      if (i + e < L) {
        base[i + e] = ex;
        const int64_t c = (i + e) / T;
        if (c * T == i + e) so[c] = ex;
        ex += v[e];
      }
    }
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) so[K] = carry;
}

// grid: N * T.  offs: the scanned counts; d2 int32 [2 N][K][H][W]; list int32 [2 N][H W]
__global__ __launch_bounds__(256) void surface_scatter_kernel(const int64_t* __restrict__ emap,
                                                              const uint32_t* __restrict__ offs,
                                                              const int32_t* __restrict__ d2, int64_t N, int K, int H,
                                                              int W, int tiles_x, int T, int32_t* __restrict__ list) {
  __shared__ uint32_t cnt[4][2][256];   // [wave][map][class]: the wave's pixels ranked so far
  const SurfTile tl = surf_tile(tiles_x, T);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t HW = (int64_t)H * W;
  for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) (&cnt[0][0][0])[i] = 0u;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  int cl[4][2];
  uint32_t rk[4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = wv * 256 + r * 64 + lane, y = tl.y0 + (j >> 5), x = tl.x0 + (j & 31);
    const bool in = y < H && x < W;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int c = in ? (int)emap[((m * N + tl.n) * H + y) * W + x] : -1;
      volatile uint32_t* wc = cnt[wv][m];   // read and written by this wave alone, in program order
      uint32_t rank = 0u;
      unsigned long long todo = __ballot(c >= 0);
      while (todo) {   // one round per class among the wave's 64 pixels; todo is the same in every lane
        const int leader = __ffsll((long long)todo) - 1;
        const int c0 = __shfl(c, leader, 64);
        const unsigned long long same = __ballot(c == c0);
        const uint32_t seen = wc[c0];
        if (c == c0) rank = seen + (uint32_t)__popcll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) wc[c0] = seen + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        todo &= ~same;
      }
      cl[r][m] = c;
      rk[r][m] = rank;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = wv * 256 + r * 64 + lane, y = tl.y0 + (j >> 5), x = tl.x0 + (j & 31);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int c = cl[r][m];
      if (c < 0) continue;
      uint32_t dst = offs[((m * N + tl.n) * K + c) * T + tl.t] + rk[r][m];
      for (int w = 0; w < wv; ++w) dst += cnt[w][m][c];
      list[(m * N + tl.n) * HW + dst] = d2[((((1 - m) * N + tl.n) * K + c) * H + y) * W + x];
    }
  }
}

// grid: N * K.  q = percentile / 100 in (0, 1]; shift0: the bit of the top radix level (a multiple of 8)
__global__ __launch_bounds__(256) void surface_select_kernel(const int32_t* __restrict__ list,
                                                             const uint32_t* __restrict__ segoff, int64_t N, int K,
                                                             int64_t HW, double q, int shift0,
                                                             float* __restrict__ metrics, int64_t* __restrict__ counts) {
  __shared__ uint32_t hist[2][256];
  __shared__ double rsum[256];
  __shared__ uint32_t rmax[256];
  __shared__ uint32_t sel[2][2];   // per target rank: {digit, rank inside the digit's bucket}
  const int64_t n = blockIdx.x / K;
  const int c = (int)(blockIdx.x - n * K);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t m[2];
  const uint32_t* L[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const uint32_t* so = segoff + (d * N + n) * (K + 1) + c;
    m[d] = so[1] - so[0];
    L[d] = reinterpret_cast<const uint32_t*>(list) + (d * N + n) * HW + so[0];
  }
  float* out = metrics + (int64_t)blockIdx.x * 3;
  if (tid == 0) {
    counts[(int64_t)blockIdx.x * 2] = m[0];
    counts[(int64_t)blockIdx.x * 2 + 1] = m[1];
  }
  if (m[0] == 0u || m[1] == 0u) {   // the same in every thread
    if (tid < 3) out[tid] = (m[0] | m[1]) ? __builtin_inff() : __builtin_nanf("");
    return;
  }
  double total = 0.0, qmax = 0.0;
  uint32_t gmax = 0u;
  for (int d = 0; d < 2; ++d) {
    const uint32_t* Ld = L[d];
    const uint32_t md = m[d];
    double s = 0.0;
    uint32_t mx = 0u;
    for (uint32_t i = tid; i < md; i += 256) {
      const uint32_t k = Ld[i];
      s += sqrt((double)k);
      mx = max(mx, k);
    }
    rsum[tid] = s;
    rmax[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {   // a fixed tree: the same sum on every run
      if (tid < o) {
        rsum[tid] += rsum[tid + o];
        rmax[tid] = max(rmax[tid], rmax[tid + o]);
      }
      __syncthreads();
    }
    total += rsum[0];
    gmax = max(gmax, rmax[0]);
    const double pos = (double)(md - 1u) * q;
    const uint32_t lo = min((uint32_t)floor(pos), md - 1u), hi = min(lo + 1u, md - 1u);
    const double t = pos - (double)lo;
    uint32_t pre[2] = {0u, 0u}, rk[2] = {lo, hi}, mask = 0u;
    for (int shift = shift0; shift >= 0; shift -= 8) {
      hist[0][tid] = 0u;
      hist[1][tid] = 0u;
      __syncthreads();
      for (uint32_t i = tid; i < md; i += 256) {
        const uint32_t k = Ld[i], dg = (k >> shift) & 255u;
        if ((k & mask) == pre[0]) atomicAdd(&hist[0][dg], 1u);
        if ((k & mask) == pre[1]) atomicAdd(&hist[1][dg], 1u);
      }
      __syncthreads();
      if (wv < 2) {   // wave j finds the bucket of target rank j: 4 bins a lane, a scan over the lanes
        const uint32_t* h = &hist[wv][lane * 4];
        const uint32_t a0 = h[0], a1 = h[1], a2 = h[2], a3 = h[3], s4 = a0 + a1 + a2 + a3;
        const uint32_t inc = wave_scan_incl(s4, lane), exc = inc - s4;
        uint32_t r = rk[wv];
        if (exc <= r && r < inc) {   // exactly one lane: r is below the bucket total of the level above
          r -= exc;
          uint32_t dg = 0u;
          if (r >= a0) { r -= a0; dg = 1u;
            if (r >= a1) { r -= a1; dg = 2u;
              if (r >= a2) { r -= a2; dg = 3u; } } }
          sel[wv][0] = (uint32_t)lane * 4u + dg;
          sel[wv][1] = r;
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        pre[j] |= sel[j][0] << shift;
        rk[j] = sel[j][1];
      }
      mask |= 255u << shift;
    }
    const double a = sqrt((double)pre[0]), b = sqrt((double)pre[1]);
    qmax = fmax(qmax, a + (b - a) * t);
    __syncthreads();   // rsum / rmax / sel are reused by the other direction
  }
  if (tid == 0) {
    out[0] = (float)sqrt((double)gmax);
    out[1] = (float)qmax;
    out[2] = (float)(total / (double)(m[0] + m[1]));
  }
}

static inline int64_t surf_tiles(int64_t H, int64_t W) {
  return ((H + kSurfTile - 1) / kSurfTile) * ((W + kSurfTile - 1) / kSurfTile);
}
static inline int64_t surf_up16(int64_t b) { return (b + 15) & ~(int64_t)15; }

struct SurfWs {
  int64_t emap, d2, edt, cnt, segoff, list, total;   // byte offsets of the sections
};
static inline SurfWs surf_ws(int64_t N, int64_t K, int64_t H, int64_t W) {
  const int64_t HW = H * W;
  SurfWs w;
  w.emap = 0;
  w.d2 = w.emap + surf_up16(2 * N * HW * 8);
  w.edt = w.d2 + surf_up16(2 * N * K * HW * 4);
  w.cnt = w.edt + surf_up16(dlmpi_edt_ws_bytes(2 * N, K, H, W));
  w.segoff = w.cnt + surf_up16(2 * N * K * surf_tiles(H, W) * 4);
  w.list = w.segoff + surf_up16(2 * N * (K + 1) * 4);
  w.total = w.list + surf_up16(2 * N * HW * 4);
  return w;
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_surface_tile() { return kSurfTile; }
extern "C" int dlmpi_surface_ok(int64_t N, int64_t K, int64_t H, int64_t W) {
  if (N < 1 || !dlmpi_edt_ok(2 * N, K, H, W)) return 0;
  return N * surf_tiles(H, W) < 2147483648LL && N * K < 2147483648LL;
}
extern "C" int64_t dlmpi_surface_ws_bytes(int64_t N, int64_t K, int64_t H, int64_t W) {
  return dlmpi_surface_ok(N, K, H, W) ? surf_ws(N, K, H, W).total : -1;
}

// binary 0: logits fp32 addressed n sn + k sk + p sp over N x K x H W, target int64 labels [N][H][W];
// binary 1: K = 1, logits and the fp32 target contiguous [N][H][W].  q = percentile / 100 in (0, 1].
// ws: dlmpi_surface_ws_bytes bytes, 16-byte aligned, nothing in it needs zeroing.  metrics fp32 [N][K][3],
// counts int64 [N][K][2].
extern "C" hipError_t dlmpi_surface_distances(const float* logits, int64_t sn, int64_t sk, int64_t sp,
                                              const void* target, int binary, int64_t N, int K, int H, int W,
                                              int64_t ignore_index, double q, void* ws, float* metrics,
                                              int64_t* counts, hipStream_t s) {
  if (!dlmpi_surface_ok(N, K, H, W) || (binary && K != 1) || !(q > 0.0 && q <= 1.0)) return hipErrorInvalidValue;
  const SurfWs o = surf_ws(N, K, H, W);
  char* b = static_cast<char*>(ws);
  int64_t* emap = reinterpret_cast<int64_t*>(b + o.emap);
  int32_t* d2 = reinterpret_cast<int32_t*>(b + o.d2);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(b + o.cnt);
  uint32_t* segoff = reinterpret_cast<uint32_t*>(b + o.segoff);
  int32_t* list = reinterpret_cast<int32_t*>(b + o.list);
  const int tiles_x = (W + kSurfTile - 1) / kSurfTile, T = (int)surf_tiles(H, W);
  const dim3 tiles((unsigned)(N * T)), blk(256);
  const PixStrides st{sn, sk, sp};
  if (binary)
    hipLaunchKernelGGL(surface_edge_kernel<true>, tiles, blk, 0, s, logits, st, target, N, K, H, W, tiles_x, T,
                       ignore_index, emap, cnt);
  else
    hipLaunchKernelGGL(surface_edge_kernel<false>, tiles, blk, 0, s, logits, st, target, N, K, H, W, tiles_x, T,
                       ignore_index, emap, cnt);
  const hipError_t e = dlmpi_edt(emap, 0, 2 * N, K, H, W, -1, b + o.edt, nullptr, d2, nullptr, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(surface_scan_kernel, dim3((unsigned)(2 * N)), blk, 0, s, cnt, K, T, segoff);
  hipLaunchKernelGGL(surface_scatter_kernel, tiles, blk, 0, s, emap, cnt, d2, N, K, H, W, tiles_x, T, list);
  const int64_t maxkey = (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1);
  int shift0 = 0;
  while ((maxkey >> (shift0 + 8)) != 0) shift0 += 8;
  hipLaunchKernelGGL(surface_select_kernel, dim3((unsigned)(N * K)), blk, 0, s, list, segoff, N, K, (int64_t)H * W, q,
                     shift0, metrics, counts);
  return hipGetLastError();
}
