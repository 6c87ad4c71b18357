// Input covariance (sae_input_cov): the centred scatter S = sum_k a_k a_k^T of a resident sample, float64, one pass.  No SAE, no context.
// The sample, its counted frames and the 256-frame units are those of input_stats.h; the decomposition is input_cov_plan.h.
//
// The rule.  a_ki = double(x_ki) - c_i (the conversion exact, the subtraction rounded once; c = NULL: zeros) for a counted frame k,
// a_ki = 0 for a frame that is not counted (never 0 - c_i).  S_ij = sum_k a_ki a_kj in float64, not divided by N; the whole matrix
// is written, the lower triangle the bit-for-bit mirror of the upper.
//
// The arithmetic is the fp64 matrix instruction v_mfma_f64_16x16x4_f64: D[16][16] += A[16][4] B[4][16] with every product fused into
// its add.  Both operands of an output tile come from the same slab of frames and none is transposed: lane l holds
// A = a[frame k0 + (l >> 4)][column i0 + (l & 15)] and B = the same with j0; its four results are D[row (l >> 4) + 4 reg][col l & 15]
// (the f64 layout: NOT the f32 one).
//
//   icv_tile_kernel<T>  one workgroup per (tile t, segment s): the 64 x 64 tile (ti, tj), ti <= tj, over the segment's units in
//                       ascending order.  A slab of ICV_SLAB frames x 64 columns of each of the two column blocks goes to LDS as
//                       float64, centred and converted ONCE there (a diagonal tile: one block); frames beyond the unit's counted
//                       ones and columns beyond d are zero operands, and a slab ends after ceil(frames / 4) steps of four frames:
//                       the padding of the last step is exact.  The next slab's loads are issued before the current slab's
//                       arithmetic.  Wave w owns the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2
//                       instruction tiles, 16 doubles per lane; the quarter below the diagonal of a diagonal tile is not computed.
//                       The result goes to part[s][t][64][64] (that quarter unwritten).
//   icv_fold_kernel     element (i, j) of tile t, i <= j: the segments' partials added in ascending s, written to S[i][j] and S[j][i].
// So every result is a function of (x, lengths, c) alone: not of the grid, the CU count, the stream or the workspace's contents.  No atomics.
#pragma once
#include "common.h"
#include "input_cov_plan.h"
#include "input_stats.h"

static_assert(ICV_UNIT == IN_UNIT, "input_cov_plan.h and input_stats.h disagree on the unit");
constexpr int ICV_SLAB = 32;              // frames per slab in LDS
constexpr int ICV_LD = ICV_TILE + 16;     // doubles per slab row: four consecutive rows of 16 columns fall into distinct LDS banks
static_assert(ICV_UNIT % ICV_SLAB == 0 && ICV_SLAB % 4 == 0 && ICV_TILE == 64, "the tile kernel's thread maps");

typedef double icv_f64x4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(256) void icv_tile_kernel(const T* __restrict__ x, int Trows, int d, IcvPlan plan,
                                                       const int32_t* __restrict__ lengths, const double* __restrict__ center,
                                                       double* __restrict__ part) {
  __shared__ double sA[ICV_SLAB * ICV_LD], sB[ICV_SLAB * ICV_LD];
  const int tile = blockIdx.x;
  const int64_t seg = blockIdx.y;
  int ti, tj;
  icv_tile_of(tile, plan.ntd, &ti, &tj);
  const bool diag = ti == tj;
  const int i0 = ti * ICV_TILE, j0 = tj * ICV_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int iw = (wave >> 1) * 32, jw = (wave & 1) * 32;
  const bool computes = !(diag && iw > jw);
  // the loads: column `col` of both blocks, frames fr, fr + 4, .. of the slab
  const int col = threadIdx.x & 63, fr = threadIdx.x >> 6;
  const bool okA = i0 + col < d, okB = !diag && j0 + col < d;
  const double cA = (okA && center) ? center[i0 + col] : 0.0;
  const double cB = (okB && center) ? center[j0 + col] : 0.0;
  const double* const sBp = diag ? sA : sB;

  icv_f64x4 acc[2][2];
  for (int m = 0; m < 2; ++m)
    for (int n = 0; n < 2; ++n) acc[m][n] = icv_f64x4{0.0, 0.0, 0.0, 0.0};

  int64_t u0, u1;
  icv_segment_units(plan, seg, &u0, &u1);
  // the slabs of the segment in ascending order: unit u, frames [s0, s0 + nr) of its nrows counted ones; u == u1: past the last
  int64_t u = u0;
  int s0 = 0, nr = 0;
  const T* base = x;
  auto seek = [&]() {
    for (; u < u1; ++u, s0 = 0) {
      const int64_t f = u / plan.units_per_file;
      const int r0 = (int)(u % plan.units_per_file) * ICV_UNIT;
      const int cnt = in_count_of(lengths, f, Trows);
      const int nrows = cnt - r0 < ICV_UNIT ? (cnt - r0 < 0 ? 0 : cnt - r0) : ICV_UNIT;
      if (s0 < nrows) {
        nr = nrows - s0 < ICV_SLAB ? nrows - s0 : ICV_SLAB;
        base = x + ((int64_t)f * Trows + r0 + s0) * d;
        return;
      }
    }
  };
  float va[ICV_SLAB / 4], vb[ICV_SLAB / 4];
  auto fetch = [&]() {
#pragma unroll
    for (int n = 0; n < ICV_SLAB / 4; ++n) {
      const int r = fr + 4 * n;
      const T* const row = base + (int64_t)r * d;
      va[n] = (r < nr && okA) ? load_as_float(row + i0 + col) : 0.f;
      vb[n] = (r < nr && okB) ? load_as_float(row + j0 + col) : 0.f;
    }
  };
  seek();
  if (u < u1) fetch();
  while (u < u1) {
    const int cur = nr;
    __syncthreads();   // the slab before this one has been read
#pragma unroll
    for (int n = 0; n < ICV_SLAB / 4; ++n) {
      const int r = fr + 4 * n;
      sA[r * ICV_LD + col] = (r < cur && okA) ? (double)va[n] - cA : 0.0;
      if (!diag) sB[r * ICV_LD + col] = (r < cur && okB) ? (double)vb[n] - cB : 0.0;
    }
    __syncthreads();
    // the next slab's loads are in flight under this one's arithmetic
    s0 += ICV_SLAB;
    seek();
    if (u < u1) fetch();
    if (computes) {
      const int steps = (cur + 3) >> 2;
      for (int ks = 0; ks < steps; ++ks) {
        const int k = ks * 4 + (lane >> 4);
        const double a0 = sA[k * ICV_LD + iw + (lane & 15)], a1 = sA[k * ICV_LD + iw + 16 + (lane & 15)];
        const double b0 = sBp[k * ICV_LD + jw + (lane & 15)], b1 = sBp[k * ICV_LD + jw + 16 + (lane & 15)];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  if (computes) {
    double* const P = part + (seg * plan.tiles + tile) * (int64_t)(ICV_TILE * ICV_TILE);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = iw + m * 16 + (lane >> 4) + 4 * reg, c = jw + n * 16 + (lane & 15);
          P[row * ICV_TILE + c] = acc[m][n][reg];
        }
  }
}

// grid (tiles, ICV_TILE^2 / 256): one element of the tile per thread
__global__ __launch_bounds__(256) void icv_fold_kernel(const double* __restrict__ part, IcvPlan plan, int d, double* __restrict__ out) {
  const int tile = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
  int ti, tj;
  icv_tile_of(tile, plan.ntd, &ti, &tj);
  const int li = e / ICV_TILE, lj = e % ICV_TILE;
  const int i = ti * ICV_TILE + li, j = tj * ICV_TILE + lj;
  if (i > j || i >= d || j >= d) return;
  const double* p = part + (int64_t)tile * (ICV_TILE * ICV_TILE) + e;
  const int64_t stride = (int64_t)plan.tiles * (ICV_TILE * ICV_TILE);
  double s = 0.0;
  for (int64_t g = 0; g < plan.segments; ++g) s += p[g * stride];
  out[(int64_t)i * d + j] = s;
  if (i != j) out[(int64_t)j * d + i] = s;
}
