// Elastic deformation in the segmentation batch kernel (data/seg_aug.py: seg_elastic_field, draw_seg_elastic): the
// affine source coordinate of seg_aug.hip plus a smooth displacement of the OUTPUT pixel,
//   X = a x + b y + c + dX(x, y),   Y = d x + e y + f + dY(x, y)          (Q16, int64)
// after which taps, nearest, bilinear and the fills are seg_sample.h, as in the affine kernel.
//
// The field is a uniform cubic B-spline over the sample's control lattice D, int32 [2][L][L] in Q16 source pixels,
// L = G + 3.  The host gives one table per output axis, ex [Wo][5] and ey [Ho][5], rows (cell, w0, w1, w2, w3) with
// four non-negative Q20 weights that sum to 2^20.  The field is evaluated columns first, then rows, rounded after
// each pass, exactly as the torch reference does:
//   E_c[r][x] = (sum_a wx[x][a] D_c[r][ix[x] + a] + 2^19) >> 20          r in [0, L)
//   d_c(x, y) = (sum_b wy[y][b] E_c[iy[y] + b][x] + 2^19) >> 20
// Every product is int32 x int32 accumulated in 64 bits (v_mad_i64_i32).
//
// The column pass does not depend on the output row, so a block computes it ONCE for its tile:
//   split    256 threads own sample b = blockIdx.z and a tile of 32 rows x 32 V columns (V = 4: 16-byte stores,
//            V = 1: any shape and alignment, the rule of the affine kernel); thread (ty, tx) = (tid / 32, tid % 32)
//            owns columns 4 tx .. 4 tx + 3 of rows ty, ty + 8, ty + 16, ty + 24.  No division anywhere.
//   stage 1  wave 0 reads the tile's 32 rows of ey, clamps the cells and reduces their range [lo, hi] (the window
//            of lattice rows lo .. hi + 3 the tile touches); every thread takes the ex row of ONE tile column into
//            registers (the column pass is the only reader of ex, and a thread keeps its column throughout it);
//            then the window's lattice rows, whole and for both components, go to LDS.
//   stage 2  E for the window's rows and the tile's columns, int32 in LDS as [c][r][x]: consecutive x across lanes.
//   stage 3  per pixel four multiply-adds per component from LDS (ds_read_b128 on the 4-column path), then the
//            sampling and the stores of the affine kernel.
// Cell indices are clamped into [0, G - 1] wherever they are read, so the window has at most L rows whatever the
// tables hold, and LDS is sized for L rows: no table content can index outside the lattice or the block's LDS.
#include "seg_sample.h"

namespace dlmpi {

static constexpr int kElasticRows = 32;     // rows of a tile
static constexpr int kElasticMaxG = 32;     // cells per axis
static constexpr int kElasticMaxLds = 64 * 1024;

// ints of LDS of a block: E [2 L][TW], the lattice window [2][L][L], the tile's ey rows [32][5] and {lo, hi}
static constexpr int kElasticTail = kElasticRows * 5 + 2;
static inline size_t elastic_lds_bytes(int G, int TW) {
  const size_t L = (size_t)G + 3;
  return (2 * L * TW + 2 * L * L + kElasticTail) * sizeof(int);
}

__device__ __forceinline__ int elastic_cell(int i, int G) { return min(max(i, 0), G - 1); }

template <typename MT, int V>
__global__ __launch_bounds__(256) void seg_elastic_batch_kernel(
    const float* __restrict__ images, const MT* __restrict__ masks, const int64_t* __restrict__ idx,
    const int* __restrict__ table, const int* __restrict__ lattice, int G, const int* __restrict__ ex,
    const int* __restrict__ ey, int C, int H, int W, int Ho, int Wo, float image_fill, MT mask_fill,
    float* __restrict__ out, MT* __restrict__ out_mask) {
  constexpr int TW = 32 * V, GROUPS = 256 / TW;
  extern __shared__ __attribute__((aligned(16))) int lds[];
  const int L = G + 3;
  int* sE = lds;                    // [2 nr][TW]
  int* sD = sE + 2 * L * TW;        // [2 nr][L]
  int* sY = sD + 2 * L * L;         // [32][5], then lo, hi
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * kElasticRows;
  const int64_t s = idx[b];

  // ---- stage 1: the axis tables (rows and columns past the output repeat the last one: computed, never stored)
  if (tid < 64) {                   // wave 0, lanes 32..63 repeating lanes 0..31 so that every lane takes part
    const int r = tid & 31;
    const int* e = ey + (int64_t)min(y0 + r, Ho - 1) * 5;
    const int iy = elastic_cell(e[0], G);
    int lo = iy, hi = iy;
#pragma unroll
    for (int m = 16; m; m >>= 1) {
      lo = min(lo, __shfl_xor(lo, m));
      hi = max(hi, __shfl_xor(hi, m));
    }
    if (tid < 32) {
      sY[r * 5] = iy;
#pragma unroll
      for (int k = 1; k < 5; ++k) sY[r * 5 + k] = e[k];
    }
    if (tid == 0) {
      sY[kElasticRows * 5] = lo;
      sY[kElasticRows * 5 + 1] = hi;
    }
  }
  const int xc = tid & (TW - 1);    // the tile column of this thread in the column pass
  int ixc, wx[4];
  {
    const int* e = ex + (int64_t)min(x0 + xc, Wo - 1) * 5;
    ixc = elastic_cell(e[0], G);
#pragma unroll
    for (int k = 0; k < 4; ++k) wx[k] = e[1 + k];
  }
  __syncthreads();
  const int lo = sY[kElasticRows * 5];
  const int nr = sY[kElasticRows * 5 + 1] - lo + 4;      // <= G - 1 + 4 = L
  {
    // rows lo .. lo + nr - 1 of a component are contiguous in the lattice: nr L ints each
    const int* D = lattice + s * (2 * L * L) + lo * L;
    const int n = nr * L;
    for (int i = tid; i < n; i += 256) {
      sD[i] = D[i];
      sD[n + i] = D[L * L + i];
    }
  }
  __syncthreads();

  // ---- stage 2: the column pass, row j = c nr + r of E from row j of the window; ixc + 3 <= L - 1
  for (int j = tid / TW; j < 2 * nr; j += GROUPS) {
    const int* d = sD + j * L + ixc;
    int64_t acc = 1 << 19;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (int64_t)wx[k] * d[k];
    sE[j * TW + xc] = (int)(acc >> 20);
  }
  __syncthreads();

  // ---- stage 3: the row pass and the sampling
  const int tx = tid & 31, ty = tid >> 5;
  const int x = x0 + tx * V;
  if (x >= Wo) return;              // (V = 4: Wo % 4 == 0, so the four columns stand or fall together)
  const int* m = table + s * 6;
  const int64_t a = m[0], d = m[3];
  const int64_t HW = (int64_t)H * W, HWo = (int64_t)Ho * Wo;
  const MT* mplane = masks + s * HW;
  for (int yl = ty; yl < kElasticRows && y0 + yl < Ho; yl += 8) {
    const int y = y0 + yl;
    const int* wy = sY + yl * 5;
    const int* E = sE + (wy[0] - lo) * TW + tx * V;      // rows wy[0] - lo .. + 3 < nr
    int64_t ax[V], ay[V];
#pragma unroll
    for (int j = 0; j < V; ++j) ax[j] = ay[j] = 1 << 19;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t w = wy[1 + k];
      if constexpr (V == 4) {
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 e0 = *reinterpret_cast<const i32x4*>(E + k * TW);
        const i32x4 e1 = *reinterpret_cast<const i32x4*>(E + (nr + k) * TW);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ax[j] += w * e0[j];
          ay[j] += w * e1[j];
        }
      } else {
        ax[0] += w * E[k * TW];
        ay[0] += w * E[(nr + k) * TW];
      }
    }
    int64_t X = a * x + (int64_t)m[1] * y + m[2];
    int64_t Y = d * x + (int64_t)m[4] * y + m[5];
    SegTaps t[V];
    MT mv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t Xe = X + (ax[j] >> 20), Ye = Y + (ay[j] >> 20);
      t[j] = seg_taps(Xe, Ye, H, W);
      mv[j] = seg_nearest(mplane, Xe, Ye, H, W, mask_fill);
      X += a;
      Y += d;
    }
    const int64_t po = (int64_t)y * Wo + x;
    MT* om = out_mask + b * HWo + po;
    if constexpr (V == 4) {
      if constexpr (sizeof(MT) == 4) {
        *reinterpret_cast<f32x4*>(om) = f32x4{(float)mv[0], (float)mv[1], (float)mv[2], (float)mv[3]};
      } else {
        typedef long long i64x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<i64x2*>(om) = i64x2{(long long)mv[0], (long long)mv[1]};
        *reinterpret_cast<i64x2*>(om + 2) = i64x2{(long long)mv[2], (long long)mv[3]};
      }
    } else {
      om[0] = mv[0];
    }
    const float* plane = images + s * C * HW;
    float* o = out + (int64_t)b * C * HWo + po;
    for (int c = 0; c < C; ++c, plane += HW, o += HWo) {
      float v[V];
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = seg_bilinear(plane, t[j], W, image_fill);
      if constexpr (V == 4)
        *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      else
        o[0] = v[0];
    }
  }
}

template <typename MT>
static hipError_t launch_seg_elastic(const float* images, const MT* masks, const int64_t* idx, const int* table,
                                     const int* lattice, int G, const int* ex, const int* ey, int B, int C, int H,
                                     int W, int Ho, int Wo, float image_fill, MT mask_fill, float* out, MT* out_mask,
                                     hipStream_t s) {
  const bool vec = Wo % 4 == 0 && (((uintptr_t)out | (uintptr_t)out_mask) & 15u) == 0;
  const int TW = vec ? 128 : 32;
  const size_t lds = elastic_lds_bytes(G, TW);
  const int64_t gx = ((int64_t)Wo + TW - 1) / TW, gy = ((int64_t)Ho + kElasticRows - 1) / kElasticRows;
  if (lds > (size_t)kElasticMaxLds || gy > 65535 || B > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  if (vec)
    hipLaunchKernelGGL((seg_elastic_batch_kernel<MT, 4>), grid, dim3(256), lds, s, images, masks, idx, table, lattice,
                       G, ex, ey, C, H, W, Ho, Wo, image_fill, mask_fill, out, out_mask);
  else
    hipLaunchKernelGGL((seg_elastic_batch_kernel<MT, 1>), grid, dim3(256), lds, s, images, masks, idx, table, lattice,
                       G, ex, ey, C, H, W, Ho, Wo, image_fill, mask_fill, out, out_mask);
  return hipGetLastError();
}

}  // namespace dlmpi

using namespace dlmpi;

extern "C" hipError_t dlmpi_seg_elastic_batch(const float* images, const void* masks, int mask_i64,
                                              const int64_t* idx, const int* table, const int* lattice, int G,
                                              const int* ex, const int* ey, int B, int C, int H, int W, int Ho, int Wo,
                                              float image_fill, float mask_fill_f, int64_t mask_fill_i, float* out,
                                              void* out_mask, hipStream_t s) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || (int64_t)H * W > INT32_MAX ||
      (int64_t)B * Ho * Wo > INT32_MAX || G < 1 || G > kElasticMaxG || !images || !masks || !idx || !table ||
      !lattice || !ex || !ey || !out || !out_mask)
    return hipErrorInvalidValue;
  if (mask_i64)
    return launch_seg_elastic<int64_t>(images, (const int64_t*)masks, idx, table, lattice, G, ex, ey, B, C, H, W, Ho,
                                       Wo, image_fill, mask_fill_i, out, (int64_t*)out_mask, s);
  return launch_seg_elastic<float>(images, (const float*)masks, idx, table, lattice, G, ex, ey, B, C, H, W, Ho, Wo,
                                   image_fill, mask_fill_f, out, (float*)out_mask, s);
}
