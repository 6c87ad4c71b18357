// Cross-activation (include/freud_sae.h, sae_cross_mask_files / sae_cross_update / sae_cross_keys): how often latent i of dictionary
// A and latent j of dictionary B are active a fixed number of frames apart, for every pair, and the keys from which file_top.h
// selects each latent's partners on the other side.
//
// The rule.  A (n_a latents) and B (n_b latents) see the same files; file f has len_f counted frames (min(lengths[f], T), or T
// without lengths: cx_len, the rule of search_len).  "Active" is the rule of stats.h / coact.h: the value encode() returns has
// non-zero magnitude bits (a -0.0 and a selected zero of a TopK row are not active; a multi_topk context uses its k selection).
// For a lag l >= 0
//     X_l[i][j]   = #{ (f, t) : t + l < len_f, A_i active at (f, t), B_j active at (f, t + l) }
//     fire_a_l[i] = #{ (f, t) : t + l < len_f, A_i active at (f, t) }
//     fire_b_l[j] = #{ (f, t) : t + l < len_f, B_j active at (f, t + l) }
//     n_pairs_l   = sum_f max(len_f - l, 0)
// A pair of frames never crosses a file, and an uncounted frame is on neither side of a pair.  A negative lag is the same table with
// A and B swapped.  With A = B and l = 0, X is coact.h's C.  Counts are int32 (the caller keeps a pass below 2^31 frames);
// 0 <= l < CX_MAX_LAG, at most CX_MAX_LAGS distinct lags in one pass.
//
// One product gives all four: every mask carries one extra "margin" row (the idea of labels.h's "any" row) behind its n latent rows,
//     source mask, position (f, t):            row i = A_i active at (f, t) and t < len_f;       margin = t < len_f
//     target mask at lag l, position (f, t):   row j = B_j active at (f, t + l), t + l < len_f;  margin = t + l < len_f
// so that source x target^T is the table [(n_a + 1)][(n_b + 1)] with X_l inside, fire_a_l in the last column, fire_b_l in the last row
// and n_pairs_l in the corner: the margins come out of the same sums as the interior.  The source mask is the target mask at lag 0.
//
// Kernels.  The mask pack is coact.h's with the read shifted by the lag and the margin row added: [n_r][Kp] int8, n_r = n + 1
// rounded up to CO_BM, Kp = the batch's rows rounded up to CO_BK, latent-major with frames contiguous, every padding byte zero, in
// caller-owned memory (two contexts take part in one table; the passes' scratch belongs to one).  The update is labels.h's
// label_update_kernel as it stands -- a rectangle of 128 x 128 tiles, every tile computed, coact.h's K split -- one launch per lag.
// The key kernel reads the margins from the table itself, in either orientation.
//
// The first part is free of any HIP type and compiles for the host as coact.h's does (tests/test_cross_activation_cpu.py).
#pragma once
#include "labels.h"

enum { CX_JACCARD = 0, CX_COND = 1, CX_LIFT = 2, CX_COUNT = 3 };      // include/freud_sae.h: SAE_CROSS_*
enum { CX_SOURCE = 1, CX_TARGET = 2 };                                // ... SAE_CROSS_SOURCE / SAE_CROSS_TARGET
constexpr int CX_MAX_LAG = 32768;
constexpr int CX_MAX_LAGS = 8;
constexpr int64_t CX_MAX_N = 1 << 21;      // latents of one side: the (n + 1) / 64 row blocks of the pack fit one grid dimension

// the counted frames of file f
SK_HD int cx_len(const int* lengths, int64_t f, int T) {
  const int L = lengths ? lengths[f] : T;
  return L < 1 ? 1 : (L > T ? T : L);
}
// the window: frame t of a file of len counted frames is the first frame of a pair at lag l
SK_HD bool cx_window(int t, int lag, int len) { return t + lag < len; }

// the score of (A_i, B_j) with x = X_l[i][j], fa = fire_a_l[i], fb = fire_b_l[j], np = n_pairs_l; by_b: the row is a latent of B.
// One fixed fp64 expression, converted once to fp32.
SK_HD float cx_score(int measure, int by_b, int32_t x, int32_t fa, int32_t fb, int32_t np) {
  const double X = (double)x, FA = (double)fa, FB = (double)fb;
  if (measure == CX_JACCARD) return (float)(X / (double)((int64_t)fa + (int64_t)fb - (int64_t)x));
  if (measure == CX_COND) return (float)(X / (by_b ? FB : FA));
  if (measure == CX_LIFT) return (float)((X / FA) / (FB / (double)np));
  return (float)x;
}
// co_key's form: score descending, then the larger count; file_top.h breaks equal keys by the lower index.  0: not reported (a pair
// that never meets; the latent itself where both sides are one dictionary at lag 0: exclude_diagonal).  A reported pair has a
// score > 0, so its key passes FT_POSITIVE; co_key_count / co_key_score read it back.
SK_HD uint64_t cx_key(int measure, int by_b, int exclude_diagonal, int64_t i, int64_t j, int32_t x, int32_t fa, int32_t fb, int32_t np) {
  if (x <= 0 || (exclude_diagonal && i == j)) return 0;
  return ((uint64_t)sk_ord(cx_score(measure, by_b, x, fa, fb, np)) << 32) | (uint64_t)(uint32_t)x;
}

// The whole rule, serially, over dense 0/1 arrays za [F][T][n_a] and zb [F][T][n_b]: table [(n_a + 1)][(n_b + 1)] += one lag.
inline void cx_reference(const uint8_t* za, int n_a, const uint8_t* zb, int n_b, int64_t F, int T, const int* lengths, int lag,
                         int32_t* table) {
  const int64_t W = n_b + 1;
  for (int64_t f = 0; f < F; ++f) {
    const int len = cx_len(lengths, f, T);
    for (int t = 0; t < len; ++t) {
      const bool open = cx_window(t, lag, len);
      const uint8_t* a = za + (f * T + t) * n_a;
      const uint8_t* b = zb + (f * T + t + lag) * n_b;     // (read where the window is open only)
      for (int i = 0; i <= n_a; ++i) {
        if (i < n_a && !a[i]) continue;                    // (row n_a and column n_b are the margins)
        for (int j = 0; j <= n_b; ++j) {
          const bool on = j < n_b ? (open && b[j]) : open;
          if (on) table[i * W + j] += 1;
        }
      }
    }
  }
}

#if defined(__HIPCC__)

// whether position r = f T + t of a batch of M rows opens a pair at this lag; then row r + lag is in the same file and counted
__device__ __forceinline__ bool cx_pos_ok(int64_t r, int64_t M, int T, const int* __restrict__ lengths, int lag) {
  if (r >= M) return false;
  const int64_t f = r / T;
  return cx_window((int)(r - f * T), lag, cx_len(lengths, f, T));
}

// ---- mask pack, L1: lat [M_p][ld] bf16 bit patterns -> zt [n_r][Kp] at one lag.  coact_pack_l1_kernel's form -- grid (Kp / 64,
// n_r / 64), 256 threads, a transpose through LDS -- reading row r + lag for position r, with row n the margin.  n_r may exceed ld
// (n a multiple of 128): columns at or beyond ld are not read.
__global__ __launch_bounds__(256) void cross_pack_l1_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t M, int T,
                                                            const int* __restrict__ lengths, int lag, int8_t* __restrict__ zt, int64_t Kp) {
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
      const bool ok = cx_pos_ok(r, M, T, lengths, lag);
      uint32_t w = 0;
      if (ok && c0 + cp < ld) w = *reinterpret_cast<const uint32_t*>(lat + (r + lag) * ld + c0 + cp);     // (ld is even: c0 + cp + 1 < ld)
      const int ca = c0 + cp, cb = ca + 1;
      tile[cp][rr] = (ca < n ? (w & 0x7FFFu) != 0u : (ca == n && ok)) ? 1 : 0;
      tile[cp + 1][rr] = (cb < n ? (w & 0x7FFF0000u) != 0u : (cb == n && ok)) ? 1 : 0;
    }
  }
  __syncthreads();
  const int c = tid >> 2, q = (tid & 3) * 16;
  *reinterpret_cast<co_i32x4*>(zt + (int64_t)(c0 + c) * Kp + r0 + q) = *reinterpret_cast<const co_i32x4*>(&tile[c][q]);
}

// ---- mask pack, TopK: after a memset of zt, one thread per selected (row, slot) -- coact_pack_topk_kernel's form.  The selection of
// the counted frame (f, t') lands at position (f, t' - lag) where t' >= lag; slot 0 of the frame sets the margin there.
__global__ __launch_bounds__(256) void cross_pack_topk_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals, int k,
                                                              int64_t M, int T, const int* __restrict__ lengths, int n, int lag,
                                                              int8_t* __restrict__ zt, int64_t Kp) {
  const int64_t total = M * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / k;
    const int64_t f = r / T;
    const int t = (int)(r - f * T);
    if (t < lag || t >= cx_len(lengths, f, T)) continue;        // (cx_window(t - lag, lag, len))
    const int64_t pos = r - lag;
    if (e - r * k == 0) zt[(int64_t)n * Kp + pos] = 1;
    const int j = idx[e];
    if ((vals[e] & 0x7FFFu) != 0u && j >= 0 && j < n) zt[(int64_t)j * Kp + pos] = 1;
  }
}

// ---- keys of the rows [row0, row0 + n_rows) of a table X [(n_a + 1)][(n_b + 1)] (by_b = 0: keys [n_rows][n_b], a row is a latent
// of A) or of its transpose (by_b = 1: keys [n_rows][n_a], a row is a latent of B) -- label_keys_kernel's pattern.  The margins are
// the table's own last column, last row and corner.
__global__ __launch_bounds__(256) void cross_keys_kernel(const int32_t* __restrict__ X, int n_a, int n_b, int measure, int by_b,
                                                         int exclude_diagonal, int64_t row0, int64_t n_rows, uint64_t* __restrict__ keys) {
  const int ncols = by_b ? n_a : n_b;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  const int64_t W = (int64_t)n_b + 1;
  const int32_t np = X[(int64_t)n_a * W + n_b];
  for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
    const int64_t i = by_b ? col : row0 + r, j = by_b ? row0 + r : col;
    const int32_t x = X[i * W + j];
    uint64_t key = 0;
    if (x > 0) key = cx_key(measure, by_b, exclude_diagonal, i, j, x, X[i * W + n_b], X[(int64_t)n_a * W + j], np);
    keys[r * ncols + col] = key;
  }
}
#endif
