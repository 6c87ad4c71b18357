// Feature co-activation (include/freud_sae.h, sae_coact_files / sae_coact_neighbor_keys): C[i][j] = the number of counted frames on
// which latents i and j are both active (> 0), for every pair, and per latent the keys from which file_top.h selects its
// neighbours.  "Active" is the rule of stats.h: the magnitude bits of the bf16 latent are not zero (a -0.0 is not active).
//
// A count table is a symmetric rank-K update of a 0/1 matrix: C += Zt Zt^T with Zt[latent][frame] in int8.  Three kernels:
//   * the mask pack writes Zt [n_p][Kp] -- latent-major, frames contiguous, Kp = the batch's rows rounded up to CO_BK -- from the
//     stored bf16 latent (L1, a transpose through LDS) or from the TopK selection (memset + scatter).  Trimmed frames, padding rows
//     and padding columns are zero, so they count nowhere.  Zt is context scratch allocated by the first call:
//     n_p x round_up(max_rows_p, CO_BK) bytes, 2.7 GB at n = 40 960 with 65 536 rows.
//   * the update runs on v_mfma_i32_32x32x32_i8 (twice the bf16 rate, exact i32 sums).  Both operands are row blocks of the same
//     Zt with K contiguous, so a lane's 16 operand bytes are one 16-byte read; A and B take the same k order, and a sum over k
//     does not care which.  Only the 128 x 128 tiles on or above the diagonal are computed; an off-diagonal tile is also written
//     transposed, so the table is the full symmetric matrix after every call.
//   * the key kernel turns a block of rows of C into 64-bit keys ord(score) << 32 | count for file_top_kernel.
//
// Decomposition.  A workgroup (4 waves, 2 x 2, 64 x 64 per wave = 2 x 2 MFMA tiles) owns one 128 x 128 tile and one K range.  With
// many tiles (n = 40 960: 51 360) every workgroup walks the whole K and adds to C with plain loads and stores: it alone owns the
// tile and its mirror.  With few (n = 3072: 300 tiles for 256 CUs that hold two workgroups each -- 192-196 registers per lane,
// accumulators included) K is split into the fewest ranges that give at least CO_MIN_WGS workgroups (n = 3072: 4 ranges, 1200
// workgroups), and the partial tiles are added with integer atomicAdd: integer sums do not depend on order, the table stays
// bitwise reproducible.
//
// The caller guarantees that no count exceeds 2^31 - 1: at most 2^31 - 1 counted frames over all calls on one table (the Python
// layer refuses a pass whose files x T exceeds it).
//
// The first part is free of any HIP type and compiles for the host as search_keys.h does (tests/test_coactivation_cpu.py).
#pragma once
#include "search_keys.h"

enum { CO_JACCARD = 0, CO_COND = 1, CO_COUNT = 2 };      // include/freud_sae.h: SAE_COACT_*

// the score of the pair (i, j): ONE fp64 division, then one conversion to fp32
SK_HD float co_score(int measure, int32_t cij, int32_t cii, int32_t cjj) {
  const double den = measure == CO_JACCARD ? (double)((int64_t)cii + (int64_t)cjj - (int64_t)cij) : measure == CO_COND ? (double)cii : 1.0;
  return (float)((double)cij / den);
}
// score descending, then the larger count; file_top.h breaks equal keys by the lower index.  0: not reported (the latent itself,
// a pair that never co-fires); a reported pair has a score > 0, so its key passes FT_POSITIVE.
SK_HD uint64_t co_key(int measure, int64_t i, int64_t j, int32_t cij, int32_t cii, int32_t cjj) {
  if (i == j || cij <= 0) return 0;
  return ((uint64_t)sk_ord(co_score(measure, cij, cii, cjj)) << 32) | (uint64_t)(uint32_t)cij;
}
SK_HD int32_t co_key_count(uint64_t k) { return (int32_t)(uint32_t)k; }
SK_HD float co_key_score(uint64_t k) { return sk_unord((uint32_t)(k >> 32)); }

#if defined(__HIPCC__)
#include "common.h"
#include "search.h"      // search_len

constexpr int CO_BM = 128;         // tile edge (latents)
constexpr int CO_BK = 128;         // frames per LDS stage, and the granule of Kp
constexpr int CO_MIN_WGS = 1024;   // the K split gives at least this many workgroups: 256 CUs x 2 resident x 2 rounds

typedef int co_i32x4 __attribute__((ext_vector_type(4)));
typedef int co_i32x16 __attribute__((ext_vector_type(16)));

// ---- mask pack, L1: lat [M_p][ld] bf16 bit patterns -> Zt [n_p][Kp].  Grid (Kp / 64, n_p / 64), 256 threads: 64 rows x 64 columns
// are read along the columns, transposed in LDS and written along the frames (16 bytes per thread).
__global__ __launch_bounds__(256) void coact_pack_l1_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t M, int T,
                                                            const int* __restrict__ lengths, int8_t* __restrict__ zt, int64_t Kp) {
  __shared__ int8_t tile[64][64 + 16];        // [column][row]; rows of 80 bytes keep the 16-byte reads aligned
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
  {
    const int cp = (tid & 31) * 2;            // a pair of columns
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = (tid >> 5) + 8 * i;
      const int64_t r = r0 + rr;
      bool ok = r < M;
      if (ok && lengths) {
        const int64_t f = r / T;
        ok = r - f * T < search_len(lengths, (int)f, T);
      }
      uint32_t w = 0;
      if (ok) w = *reinterpret_cast<const uint32_t*>(lat + r * ld + c0 + cp);     // (c0 + cp + 1 < n_p <= ld, r < M <= M_p)
      tile[cp][rr] = ((w & 0x7FFFu) != 0u && c0 + cp < n) ? 1 : 0;
      tile[cp + 1][rr] = ((w & 0x7FFF0000u) != 0u && c0 + cp + 1 < n) ? 1 : 0;
    }
  }
  __syncthreads();
  const int c = tid >> 2, q = (tid & 3) * 16;
  *reinterpret_cast<co_i32x4*>(zt + (int64_t)(c0 + c) * Kp + r0 + q) = *reinterpret_cast<const co_i32x4*>(&tile[c][q]);
}

// ---- mask pack, TopK: after a memset of Zt, one thread per selected (row, slot).  The indices of a row are distinct.
__global__ __launch_bounds__(256) void coact_pack_topk_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals, int k,
                                                              int64_t M, int T, const int* __restrict__ lengths, int n,
                                                              int8_t* __restrict__ zt, int64_t Kp) {
  const int64_t total = M * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / k;
    if (lengths) {
      const int64_t f = r / T;
      if (r - f * T >= search_len(lengths, (int)f, T)) continue;
    }
    const int j = idx[e];
    if ((vals[e] & 0x7FFFu) != 0u && j >= 0 && j < n) zt[(int64_t)j * Kp + r] = 1;
  }
}

// ---- the update.  Grid (n_p / 128, n_p / 128, ksplit); workgroups below the diagonal leave at once.  LDS: A and B stages of
// 128 rows x 128 bytes, the eight 16-byte chunks of a row XOR-swizzled by (row & 7) so that the 16-byte fragment reads of 8
// consecutive rows cover all banks.  The next stage's global loads are issued before the MFMAs of the current one.
// ATOMIC: K is split over blockIdx.z and partial tiles are added with atomicAdd; otherwise plain read-modify-write.
__device__ __forceinline__ int co_lds_off(int row, int chunk) { return row * CO_BK + ((chunk ^ (row & 7)) << 4); }

template <bool ATOMIC>
__device__ __forceinline__ void co_add(int32_t* p, int v) {
  if (ATOMIC) { if (v) atomicAdd(p, v); }
  else *p += v;
}

template <bool ATOMIC>
__global__ __launch_bounds__(256) void coact_update_kernel(const int8_t* __restrict__ zt, int64_t Kp, int n, int ksteps_per_split,
                                                              int32_t* __restrict__ C) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * CO_BM * CO_BK];
  int8_t* la = lds;
  int8_t* lb = lds + CO_BM * CO_BK;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;       // the wave's 64 x 64 corner inside the tile
  const int nsteps_all = (int)(Kp / CO_BK);
  const int s0 = blockIdx.z * ksteps_per_split;
  const int s1 = min(s0 + ksteps_per_split, nsteps_all);
  if (s0 >= s1) return;

  // staging: thread t moves chunk t & 7 of rows (t >> 3) + 32 i of both operands
  const int sc = tid & 7, sr = tid >> 3;
  const int8_t* ga = zt + ((int64_t)bi * CO_BM + sr) * Kp + sc * 16;
  const int8_t* gb = zt + ((int64_t)bj * CO_BM + sr) * Kp + sc * 16;
  co_i32x4 ra[4], rb[4];
  auto gload = [&](int s) {
    const int64_t k0 = (int64_t)s * CO_BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const co_i32x4*>(ga + (int64_t)(32 * i) * Kp + k0);
      rb[i] = *reinterpret_cast<const co_i32x4*>(gb + (int64_t)(32 * i) * Kp + k0);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<co_i32x4*>(la + co_lds_off(sr + 32 * i, sc)) = ra[i];
      *reinterpret_cast<co_i32x4*>(lb + co_lds_off(sr + 32 * i, sc)) = rb[i];
    }
  };

  co_i32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;

  const int fr = lane & 31, fh = lane >> 5;
  gload(s0);
  for (int s = s0; s < s1; ++s) {
    __syncthreads();                 // the previous stage's fragment reads are done
    lstore();
    __syncthreads();
    if (s + 1 < s1) gload(s + 1);
#pragma unroll
    for (int kk = 0; kk < CO_BK / 32; ++kk) {
      co_i32x4 fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        fa[a] = *reinterpret_cast<const co_i32x4*>(la + co_lds_off(wr + 32 * a + fr, 2 * kk + fh));
        fb[a] = *reinterpret_cast<const co_i32x4*>(lb + co_lds_off(wc + 32 * a + fr, 2 * kk + fh));
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }

  // C/D layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const bool diag = bi == bj;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = bj * CO_BM + wc + 32 * b + fr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = bi * CO_BM + wr + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (row < n && col < n) {
          const int v = acc[a][b][e];
          co_add<ATOMIC>(C + (int64_t)row * n + col, v);
          if (!diag) co_add<ATOMIC>(C + (int64_t)col * n + row, v);
        }
      }
    }
}

// ---- neighbour keys of the rows [row0, row0 + n_rows) of C: keys[n_rows][n]
__global__ __launch_bounds__(256) void coact_keys_kernel(const int32_t* __restrict__ C, int n, int64_t row0, int64_t n_rows, int measure,
                                                         uint64_t* __restrict__ keys) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int32_t cjj = C[(int64_t)j * n + j];
  for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const int64_t i = row0 + r;
    const int32_t cij = C[i * n + j];
    uint64_t key = 0;
    if (cij > 0 && i != j) key = co_key(measure, i, j, cij, C[i * n + i], cjj);
    keys[r * n + j] = key;
  }
}
#endif
