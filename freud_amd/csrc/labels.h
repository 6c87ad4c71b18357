// Feature labels (include/freud_sae.h, sae_label_files / sae_label_keys): A[l][j] = the number of counted frames that carry label l
// and on which latent j is active, for every (label, latent), and the keys from which file_top.h selects a label's best latents
// and a latent's best labels.  Frames and "active" are the rules of coact.h; a frame carries up to S distinct class ids in
// [0, C) in S slots (-1: an empty slot).  Row C of A is the "any" row: every counted frame carries it, so A[C][j] is the fire
// count of latent j and label_count[C] the number of counted frames.
//
// The table is the co-activation product with a second operand: A += Lt Zt^T.  Zt [n_p][Kp] is coact.h's mask pack, unchanged and
// in the same scratch.  Three kernels are added:
//   * the label pack writes Lt [C_p][Kp], C_p = C + 1 rounded up to CO_BM, label-major and frames contiguous as Zt is: a memset
//     plus one thread per (frame, slot).  Trimmed frames, padding rows, empty slots and ids outside [0, C) write nothing.  A second
//     small kernel adds the row sums of Lt to label_count.
//   * the update is coact.h's tile (the same LDS staging, swizzle and MFMA loop) over the (C_p / 128) x (n_p / 128) rectangle,
//     every tile computed and none mirrored.  The K split follows coact.h's rule with the rectangle's tile count: the
//     fewest K ranges that give at least CO_MIN_WGS workgroups, partial tiles added with integer atomicAdd (n = 3072, C <= 127: 24
//     tiles, 40 ranges at 45 000 rows); with CO_MIN_WGS tiles or more (n = 16 384, C = 1023: 8 x 128) one workgroup walks all of
//     K and adds with plain loads and stores.
//   * the key kernel turns a block of rows of A (by_latent = 0: labels) or of its transpose (by_latent = 1: latents) into the
//     64-bit keys ord(score) << 32 | count -- co_key's form, so file_top_kernel selects from them with FT_POSITIVE unchanged.
//
// The caller guarantees that no count exceeds 2^31 - 1 (at most 2^31 - 1 counted frames into one table).
//
// The first part is free of any HIP type and compiles for the host as coact.h's does (tests/test_feature_labels_cpu.py).
#pragma once
#include "coact.h"

enum { LB_F1 = 0, LB_PRECISION = 1, LB_RECALL = 2, LB_COUNT = 3 };      // include/freud_sae.h: SAE_LABEL_*
constexpr int LB_MAX_CLASSES = 4096;
constexpr int LB_MAX_SLOTS = 16;

// the score of (label l, latent j) with a = A[l][j], fire = A[C][j], lc = label_count[l]: ONE fp64 division, then one conversion to
// fp32 (2a and fire + lc are exact in fp64)
SK_HD float lb_score(int measure, int32_t a, int64_t fire, int64_t lc) {
  const double num = measure == LB_F1 ? (double)(2 * (int64_t)a) : (double)a;
  const double den = measure == LB_F1 ? (double)(fire + lc) : measure == LB_PRECISION ? (double)fire : measure == LB_RECALL ? (double)lc : 1.0;
  return (float)(num / den);
}
// score descending, then the larger count; file_top.h breaks equal keys by the lower index.  0: not reported (the label and the
// latent never meet); a reported pair has a score > 0, so its key passes FT_POSITIVE.  co_key_count / co_key_score read it back.
SK_HD uint64_t lb_key(int measure, int32_t a, int64_t fire, int64_t lc) {
  if (a <= 0) return 0;
  return ((uint64_t)sk_ord(lb_score(measure, a, fire, lc)) << 32) | (uint64_t)(uint32_t)a;
}

#if defined(__HIPCC__)

// ---- label pack: after a memset of Lt, one thread per (frame, slot).  labels [M][S]; row C is set by slot 0 of every counted frame.
__global__ __launch_bounds__(256) void label_pack_kernel(const int* __restrict__ labels, int S, int C, int64_t M, int T,
                                                         const int* __restrict__ lengths, int8_t* __restrict__ lt, int64_t Kp) {
  const int64_t total = M * S;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / S;
    if (lengths) {
      const int64_t f = r / T;
      if (r - f * T >= search_len(lengths, (int)f, T)) continue;
    }
    if (e - r * S == 0) lt[(int64_t)C * Kp + r] = 1;
    const int id = labels[e];
    if (id >= 0 && id < C) lt[(int64_t)id * Kp + r] = 1;
  }
}

// ---- label_count[l] += the number of frames of this batch that carry l: the sum of row l of Lt (bytes of 0 / 1).  Grid C + 1.
__global__ __launch_bounds__(256) void label_count_kernel(const int8_t* __restrict__ lt, int64_t Kp, unsigned long long* __restrict__ label_count) {
  __shared__ int part[4];
  const co_i32x4* row = reinterpret_cast<const co_i32x4*>(lt + (int64_t)blockIdx.x * Kp);      // (Kp is a multiple of CO_BK = 128)
  int sum = 0;
  for (int64_t q = threadIdx.x; q < Kp / 16; q += 256) {
    const co_i32x4 v = row[q];
    sum += __popc((unsigned)v[0]) + __popc((unsigned)v[1]) + __popc((unsigned)v[2]) + __popc((unsigned)v[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = part[0] + part[1] + part[2] + part[3];
    if (total) atomicAdd(label_count + blockIdx.x, (unsigned long long)total);
  }
}

// ---- the update A [rows][n] += Lt Zt^T, rows = C + 1.  Grid (n_p / 128, C_p / 128, ksplit).  coact_update_kernel's tile -- its LDS
// staging and swizzle (co_lds_off), its MFMA loop, its co_add -- with two operands, every tile computed and none mirrored.  (A
// kernel of its own: folding the two into one template changed the code the compiler makes for the symmetric form.)
template <bool ATOMIC>
__global__ __launch_bounds__(256) void label_update_kernel(const int8_t* __restrict__ lt, const int8_t* __restrict__ zt, int64_t Kp, int rows,
                                                           int n, int ksteps_per_split, int32_t* __restrict__ A) {
  const int bi = blockIdx.y, bj = blockIdx.x;
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
  const int8_t* ga = lt + ((int64_t)bi * CO_BM + sr) * Kp + sc * 16;
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
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = bj * CO_BM + wc + 32 * b + fr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = bi * CO_BM + wr + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (row < rows && col < n) co_add<ATOMIC>(A + (int64_t)row * n + col, acc[a][b][e]);
      }
    }
}

// ---- keys of the rows [row0, row0 + n_rows) of A (by_latent = 0: keys [n_rows][n], a row is a label) or of its transpose
// (by_latent = 1: keys [n_rows][C], a row is a latent).  Threads run along the key row; the transposed read of A goes through L2.
__global__ __launch_bounds__(256) void label_keys_kernel(const int32_t* __restrict__ A, const int64_t* __restrict__ label_count, int C, int n,
                                                         int measure, int by_latent, int64_t row0, int64_t n_rows,
                                                         uint64_t* __restrict__ keys) {
  const int ncols = by_latent ? C : n;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const int64_t l = by_latent ? col : row0 + r, j = by_latent ? row0 + r : col;
    const int32_t a = A[l * n + j];
    uint64_t key = 0;
    if (a > 0) key = lb_key(measure, a, A[(int64_t)C * n + j], label_count[l]);
    keys[r * ncols + col] = key;
  }
}
#endif
