// Exact Euclidean distance transform of a label map and the signed distance map of the boundary loss
// (Kervadec et al., MIDL 2019), separable and exact in integers.
//
// Definition.  A plane is one (sample, class): G = {q : label(q) = c}; ignored and out-of-range pixels are in no G.
// d2_in(q) = min over s in G of |q - s|^2, d2_out(q) = min over s not in G, both exact int32, INT32_MAX where the set
// is empty.  phi(q) = +sqrt(d2_in(q)) for q not in G, 1 - sqrt(d2_out(q)) for q in G (inner border pixels 0, the
// interior negative), 0 where the needed set is empty; the root is taken in fp64 from the integer and rounded once.
// A pixel only ever needs the distance to the nearest pixel of the OPPOSITE membership (its own set gives 0), so one
// transform per plane serves both signs.
//
// Row pass (edt_row_kernel), one block per image row, the row's labels read once and narrowed to uint16 in LDS.
// The block's 4 waves take the classes four at a time; a wave walks its class's row in segments of 64 pixels.  Within
// a segment the nearest lane of the opposite membership on either side comes from the membership ballot (clz / ctz
// of the masked word); across segments it comes from the carried index of the last pixel of each membership (a
// running scalar on the way right) and of the next one (a suffix pass over the ballots, kept per segment in LDS).
// Per pixel and class it writes uint16 e = m << 15 | r: m the membership bit, r the distance along the row to the
// nearest pixel of the opposite membership (0x7FFF: none in this row).  Cost: O(W) per row and class.
//
// Column pass (edt_col_kernel<SW>), one block per (plane, strip of SW columns), the strip's e over all H rows staged
// in LDS as [H][SW] uint16 (lanes run along x: a wave reads 64 / SW whole rows of the strip, 128 contiguous bytes).
// The row pass also leaves one byte per row and class saying which memberships the row holds; every wave ORs the
// plane's H bytes (a ballot, no LDS), and a pixel whose target set is empty in the whole plane is done at once, so an
// absent or image-filling class costs O(1) per pixel.  Otherwise the thread that owns pixel (y, x) starts from
// best = r(y)^2 and scans the rows y -+ k outward, best = min(best, f(y -+ k)^2 + k^2) with f = 0 where that row's
// pixel has the opposite membership, else its r; it stops when k^2 >= best (no farther row can win), and the wave
// leaves the loop when all its lanes have stopped.  Exact; O(distance to the boundary) LDS reads per pixel on real
// masks, O(H) at worst (one seed in a corner: H W (H + 1) / 2 reads per plane).  It writes phi fp32 [planes][H][W]
// and / or the two int32 transforms.
//
// Limits (dlmpi_edt_ok): 1 <= H <= 4096, 1 <= W <= 16384.  The strip is 64 columns while 64 H uint16 fit 64 KB of LDS
// (H <= 512), then halves with every doubling of H down to 8; the row pass holds 2 W bytes of labels and W / 2 bytes
// of carries.  r < 2^15 and both squares stay below 2^31.  Workspace (dlmpi_edt_ws_bytes): the uint16 plane e,
// 2 bytes per pixel and class, and the row flags, 1 byte per row and class (phi, 4 bytes per pixel and class, is the
// caller's).  No host read, no atomics, every buffer is fully written before it is read: a fixed pair of kernel
// nodes under capture, the same bits on every run.
#include "common.h"

namespace dlmpi {

constexpr int kEdtStrip = 64;          // widest column strip
constexpr int kEdtStripRows = 512;     // rows a strip of 64 columns holds
constexpr int kEdtMaxH = 4096, kEdtMaxW = 16384;
constexpr unsigned kEdtNone = 0x7FFFu;
constexpr int kEdtInf = 2147483647;

enum EdtSource { kEdtLabels = 0, kEdtTarget = 1, kEdtMask = 2 };

// the row's pixel x as a class index (0xFFFF: in no class)
template <int SRC>
__device__ __forceinline__ unsigned edt_narrow(const void* __restrict__ src, int64_t i, int K, int64_t ignore_index) {
  if constexpr (SRC == kEdtLabels) {
    const int64_t lab = static_cast<const int64_t*>(src)[i];
    return (lab != ignore_index && lab >= 0 && lab < K) ? (unsigned)lab : 0xFFFFu;
  } else if constexpr (SRC == kEdtTarget) {
    return static_cast<const float*>(src)[i] > 0.5f ? 0u : 0xFFFFu;
  } else {
    return static_cast<const uint8_t*>(src)[i] ? 0u : 0xFFFFu;
  }
}

// grid: N * H rows.  LDS: uint16 lab[W rounded up to 64] | int nxt[4 waves][2][nseg]
template <int SRC>
__global__ __launch_bounds__(256) void edt_row_kernel(const void* __restrict__ src, int K, int H, int W,
                                                      int64_t ignore_index, uint16_t* __restrict__ e,
                                                      uint8_t* __restrict__ rowflag) {
  extern __shared__ __align__(16) unsigned char edt_lds[];
  const int nseg = (W + 63) >> 6;
  uint16_t* lab = reinterpret_cast<uint16_t*>(edt_lds);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* nxt = reinterpret_cast<int*>(edt_lds + (size_t)nseg * 128) + wv * 2 * nseg;   // [membership][segment]
  const int64_t row = blockIdx.x, n = row / H, y = row - n * H;
  for (int x = threadIdx.x; x < nseg * 64; x += 256)
    lab[x] = x < W ? (uint16_t)edt_narrow<SRC>(src, row * W + x, K, ignore_index) : (uint16_t)0xFFFFu;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull, above = ~below & ~(1ull << lane);
  for (int c0 = 0; c0 < K; c0 += 4) {   // the same trip count in every wave: the barriers below are the block's
    const int c = c0 + wv;
    const bool on = c < K;
    if (on) {   // suffix pass: nxt[k][s] = the first pixel of membership k right of segment s (-1: none)
      int nin = -1, nout = -1;
      for (int s = nseg - 1; s >= 0; --s) {
        const int x = s * 64 + lane;
        const bool act = x < W;
        const unsigned long long in = __ballot(act && lab[x] == c), out = __ballot(act) & ~in;
        if (lane == 0) {
          nxt[s] = nout;
          nxt[nseg + s] = nin;
        }
        if (in) nin = s * 64 + __ffsll((long long)in) - 1;
        if (out) nout = s * 64 + __ffsll((long long)out) - 1;
      }
      if (lane == 0) rowflag[(n * K + c) * H + y] = (uint8_t)((nout >= 0 ? 1 : 0) | (nin >= 0 ? 2 : 0));
    }
    __syncthreads();
    if (on) {
      uint16_t* dst = e + ((n * K + c) * H + y) * (int64_t)W;
      int lin = -1, lout = -1;   // the last pixel of either membership left of this segment
      for (int s = 0; s < nseg; ++s) {
        const int x = s * 64 + lane;
        const bool act = x < W;
        const bool m = act && lab[x] == c;
        const unsigned long long in = __ballot(m), out = __ballot(act) & ~in;
        const unsigned long long opp = m ? out : in;
        const unsigned long long lo = opp & below, hi = opp & above;
        const int left = lo ? s * 64 + 63 - __clzll((long long)lo) : (m ? lout : lin);
        const int right = hi ? s * 64 + __ffsll((long long)hi) - 1 : nxt[(m ? 0 : nseg) + s];
        unsigned r = kEdtNone;
        if (left >= 0) r = (unsigned)(x - left);
        if (right >= 0) r = min(r, (unsigned)(right - x));
        if (act) dst[x] = (uint16_t)(r | (m ? 0x8000u : 0u));
        if (in) lin = s * 64 + 63 - __clzll((long long)in);
        if (out) lout = s * 64 + 63 - __clzll((long long)out);
      }
    }
    __syncthreads();
  }
}

// grid: planes * nstrips.  LDS: uint16 tile[H][SW]
template <int SW>
__global__ __launch_bounds__(256) void edt_col_kernel(const uint16_t* __restrict__ e,
                                                      const uint8_t* __restrict__ rowflag, int H, int W, int nstrips,
                                                      float* __restrict__ phi, int* __restrict__ d2_in,
                                                      int* __restrict__ d2_out) {
  extern __shared__ __align__(16) unsigned char edt_lds[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(edt_lds);
  constexpr int RP = 256 / SW;      // rows per round of the block
  const int64_t plane = blockIdx.x / nstrips;
  const int x0 = (int)(blockIdx.x - plane * nstrips) * SW;
  const int xl = threadIdx.x % SW, yl = threadIdx.x / SW, x = x0 + xl;
  const bool col = x < W;
  const int64_t base = plane * H * (int64_t)W + x;
  unsigned fl = 0u;
  for (int y = threadIdx.x & 63; y < H; y += 64) fl |= rowflag[plane * H + y];
  const bool has[2] = {__any(fl & 1u) != 0, __any(fl & 2u) != 0};   // the plane holds a pixel of membership k
  for (int y = yl; y < H; y += RP) tile[y * SW + xl] = col ? e[base + y * (int64_t)W] : (uint16_t)kEdtNone;
  __syncthreads();
  for (int y0 = 0; y0 < H; y0 += RP) {   // the same trip count in every lane of a wave (for __all)
    const int y = y0 + yl;
    const bool act = col && y < H;
    const unsigned own = act ? tile[y * SW + xl] : kEdtNone;
    const unsigned m = own >> 15, r0 = own & kEdtNone;
    const bool can = act && has[m ^ 1u];
    int best = can && r0 != kEdtNone ? (int)(r0 * r0) : kEdtInf;
    for (int k = 1;; ++k) {
      const bool up = y - k >= 0, down = y + k < H;
      const bool done = !can || k * k >= best || (!up && !down);
      if (__all(done)) break;
      if (!done) {
        if (up) {
          const unsigned v = tile[(y - k) * SW + xl];
          const unsigned f = (v >> 15) != m ? 0u : (v & kEdtNone);
          if (f != kEdtNone) best = min(best, (int)(f * f) + k * k);
        }
        if (down) {
          const unsigned v = tile[(y + k) * SW + xl];
          const unsigned f = (v >> 15) != m ? 0u : (v & kEdtNone);
          if (f != kEdtNone) best = min(best, (int)(f * f) + k * k);
        }
      }
    }
    if (act) {
      const int64_t o = base + y * (int64_t)W;
      if (phi) {
        const double root = sqrt((double)best);
        phi[o] = best == kEdtInf ? 0.f : (float)(m ? 1.0 - root : root);
      }
      if (d2_in) d2_in[o] = m ? 0 : best;
      if (d2_out) d2_out[o] = m ? best : 0;
    }
  }
}

static inline int edt_strip_for(int H) {
  int sw = kEdtStrip;
  while (sw > 8 && (int64_t)H * sw > (int64_t)kEdtStripRows * kEdtStrip) sw >>= 1;
  return sw;
}

template <int SW>
static void edt_col_launch(const uint16_t* e, const uint8_t* rowflag, int64_t planes, int H, int W, float* phi, int* d2_in, int* d2_out,
                           hipStream_t s) {
  const int nstrips = (W + SW - 1) / SW;
  hipLaunchKernelGGL(edt_col_kernel<SW>, dim3((unsigned)(planes * nstrips)), dim3(256), (size_t)H * SW * 2, s, e, rowflag,
                     H, W,
                     nstrips, phi, d2_in, d2_out);
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" int dlmpi_edt_strip() { return kEdtStrip; }
extern "C" int dlmpi_edt_strip_rows() { return kEdtStripRows; }
extern "C" int dlmpi_edt_ok(int64_t N, int64_t K, int64_t H, int64_t W) {
  if (N < 1 || K < 1 || K > 256 || H < 1 || H > kEdtMaxH || W < 1 || W > kEdtMaxW) return 0;
  const int64_t strips = (W + 7) / 8;   // the narrowest strip gives the largest grid
  return N * H < 2147483648LL && N * K * strips < 2147483648LL;
}

extern "C" int64_t dlmpi_edt_ws_bytes(int64_t N, int64_t K, int64_t H, int64_t W) {
  return dlmpi_edt_ok(N, K, H, W) ? N * K * H * (2 * W + 1) : -1;
}

// source: 0 int64 labels [N][H][W] (K classes), 1 fp32 target (K = 1, G = {t > 0.5}), 2 uint8 mask (K = 1, G = {!= 0}).
// ws: dlmpi_edt_ws_bytes bytes, 2-byte aligned, nothing in it needs zeroing; phi / d2_in / d2_out [N][K][H][W], each may be null.
extern "C" hipError_t dlmpi_edt(const void* src, int source, int64_t N, int K, int H, int W, int64_t ignore_index,
                                void* ws, float* phi, int32_t* d2_in, int32_t* d2_out, hipStream_t s) {
  if (!dlmpi_edt_ok(N, K, H, W) || (source != kEdtLabels && K != 1)) return hipErrorInvalidValue;
  const int nseg = (W + 63) >> 6;
  const size_t lds = (size_t)nseg * 128 + (size_t)4 * 2 * nseg * sizeof(int);
  const dim3 grid((unsigned)(N * H)), blk(256);
  const int64_t planes = N * K;
  uint16_t* e = static_cast<uint16_t*>(ws);
  uint8_t* rowflag = reinterpret_cast<uint8_t*>(e + planes * H * W);
  if (source == kEdtLabels) hipLaunchKernelGGL(edt_row_kernel<kEdtLabels>, grid, blk, lds, s, src, K, H, W, ignore_index, e, rowflag);
  else if (source == kEdtTarget) hipLaunchKernelGGL(edt_row_kernel<kEdtTarget>, grid, blk, lds, s, src, K, H, W, ignore_index, e, rowflag);
  else if (source == kEdtMask) hipLaunchKernelGGL(edt_row_kernel<kEdtMask>, grid, blk, lds, s, src, K, H, W, ignore_index, e, rowflag);
  else return hipErrorInvalidValue;
  switch (edt_strip_for(H)) {
    case 64: edt_col_launch<64>(e, rowflag, planes, H, W, phi, d2_in, d2_out, s); break;
    case 32: edt_col_launch<32>(e, rowflag, planes, H, W, phi, d2_in, d2_out, s); break;
    case 16: edt_col_launch<16>(e, rowflag, planes, H, W, phi, d2_in, d2_out, s); break;
    default: edt_col_launch<8>(e, rowflag, planes, H, W, phi, d2_in, d2_out, s); break;
  }
  return hipGetLastError();
}
