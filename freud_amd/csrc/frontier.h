// Sparsity frontier (include/freud_sae.h, sae_frontier_files): the squared reconstruction error of every counted frame at EVERY
// latent budget s = 0 .. K, in one walk of the row's K sorted slots.  Both decoders are linear in the latent, so the residual after
// the first s slots is a prefix sum of v w terms:
//   r_0 = float(x) - b,   r_{s+1} = fmaf(-v_s, w_{i_s}, r_s),   e_s = sum_i r_s[i]^2,
// with (v_s, i_s) exactly the slots of sae_collect_files (collect.h) and w_j the bf16 decoder operand row (L1: row j of the
// transposed copy Wt of the normalised W; TopK: row j of W_dec).  The frame's BUDGET at a threshold tau is the smallest s with
// e_s <= tau * e_0 (one fp32 product, one fp32 compare), K + 1 if there is none.
//
// The first part is free of any HIP type and compiles for the host (tests/test_sparsity_frontier_cpu.py replays fr_row_serial
// against a float64 rule); the kernels compute the same numbers in the same order:
//   * a LANE owns the C = d_p / 64 contiguous columns from lane * C; its share of e_s is the fmaf chain over those columns in
//     column order, starting from 0 (fr_lane_sq);
//   * e_s is the 64 lane shares added as two halves of 32 in lane order, then half 0 + half 1 (fr_wave_sum).
// Nothing in that order depends on K, the batch, the grid or the row's neighbours.
//
// The kernels.  frontier_walk_kernel: one wave per row, four per workgroup, FR_UNIT = 32 consecutive rows per workgroup (wave w
// takes rows 4 i + w of the unit in order).  The residual lives in registers for the whole walk.  The row's slots are loaded once
// into registers (lane l keeps slots l, 64 + l, ..) and read with v_readlane, so the walk issues no memory operation but the
// gathers, and those are unconditional: the loop runs over the slots up to the last non-zero value -- the padding behind them
// gathers nothing and repeats the norm -- in groups of FR_DEPTH = 4, every step consuming the oldest gathered row and issuing the
// gather 4 slots ahead into the registers it frees.  In the code object every wait of the loop leaves the three younger rows
// outstanding (s_waitcnt vmcnt(3) / (6) / (9) with 1 / 2 / 3 loads per row at d_p = 384 / 768 / 1280; the generic form loads all
// 12 dwords per row one by one and consumes them under vmcnt(36) .. (47)): four rows in flight after every issue.  What keeps it so: a gathered row is ONE vector
// value (its registers stay one tuple: as an array the 96-bit rows of d_p = 384 were copied apart behind a vmcnt(0) per group), and
// an empty asm that consumes the step's norm keeps the next gather behind the arithmetic that still reads its destination
// (lifted over it, the gather lands in fresh registers that are copied back behind a wait for every outstanding row).  Four is what
// the latency of one cache hit needs beside the step's own work (24 fmaf + the LDS write at d_p = 768) with 16 waves per CU; the
// operand tables of the measured shapes stay in the Infinity Cache, so depth buys latency here, not HBM bandwidth.
// The K + 1 norms take no cross-lane reduction per slot: the lane shares
// of FR_CHUNK = 32 norms go into the wave's LDS tile [32][65] (ds_write_b32 of 32 consecutive dwords per half-wave: one bank each),
// then lane (j, h) adds the 32 shares of half h of norm j in order (ds_read_b32 at dword j * 65 + 32 h + i: bank (j + i) % 32 per
// 32-lane group, distinct for the 32 values of j -- the odd row pitch is what makes the transposed read conflict-free) and one
// cross-lane exchange joins the halves: one exchange per 32 norms.  A chunk of 64 would double the tile (66 KiB per workgroup, 2
// workgroups per CU) to save one exchange per row; 37 KiB allow 4 workgroups per CU.  Per-unit sums of e_s (rows in order per wave,
// the four waves in order) are written with plain stores; the budgets and the cut count go out per row.  frontier_dim_kernel:
// sum_x / sum_x_sq partials per (128-row block, column), as recon_resid_kernel.  frontier_fold_kernel adds a batch's partials in a
// fixed order into the fp64 block and adds the budget histograms and the counts with integer atomics.  No float atomics anywhere:
// two runs give the same bytes.
//
// Measured (tools/bench_frontier.py, MI355X, 16 files of 1500 frames = 24 000 rows of N(0, 1), medians of 3 rounds of 5 calls, the
// passes interleaved in one process; K = 64 and every slot active):
//   TopK d = 768, n = 24 576, k = K = 64   the walk alone 0.32 ms = 7.4 TB/s of gathered operand rows (rows x 64 x d_p x 2 bytes; the
//                                          37.7 MB table stays in the Infinity Cache, so this is no HBM rate), against 0.85 ms for the
//                                          reconstruction report's decode + attribution kernels on the same batch (0.38 x); the
//                                          collect kernels into scratch 0.23 ms, dimension sums + fold 0.30 ms; the whole call
//                                          2.89 ms beside 2.28 ms for sae_collect_files and 3.05 ms for sae_recon_files
//   L1   d = 384, n = 12 288, K = 64       the walk 0.19 ms (6.2 TB/s), the collect kernels 0.87 ms, dimension sums + fold 0.29 ms;
//                                          the call 1.57 ms beside 1.11 ms (sae_collect_files) and 1.14 ms (sae_recon_files)
// (With one gather in flight -- the slots read from memory inside the loop, every wait a vmcnt(0) -- the walks took 0.34 and 0.32 ms.)
// The dimension sums + fold take as long as the walk; spreading the histogram and count rows over workgroups of 1024 rows did not
// change that, and where the 0.3 ms go is not measured.  Not tuned.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FR_HD __host__ __device__ __forceinline__
#define FR_H __host__ inline
#else
#define FR_HD inline
#define FR_H inline
#endif

#define FR_MAX_K 256             // include/freud_sae.h: SAE_FRONTIER_MAX_K
#define FR_MAX_TAU 8             // include/freud_sae.h: SAE_FRONTIER_MAX_TAU
#define FR_MAX_D 1536            // the padded model dimension the walk holds in registers (24 columns per lane)
#define FR_CHUNK 32              // norms per transposed reduction
#define FR_UNIT 32               // rows per partial of the sse sums

// one fp32 product, rounded once (no contraction into a neighbour)
FR_HD float fr_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  volatile float p = a * b;
  return p;
#endif
}
FR_HD float fr_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  volatile float p = a + b;
  return p;
#endif
}

// a lane's share of a norm: its C columns in order
FR_HD float fr_lane_sq(const float* r, int C) {
  float q = 0.f;
  for (int i = 0; i < C; ++i) q = fmaf(r[i], r[i], q);
  return q;
}

// the 64 lane shares: each half of 32 in lane order, then half 0 + half 1
FR_HD float fr_wave_sum(const float* q) {
  float h0 = q[0], h1 = q[32];
  for (int i = 1; i < 32; ++i) {
    h0 = fr_add(h0, q[i]);
    h1 = fr_add(h1, q[32 + i]);
  }
  return fr_add(h0, h1);
}

// the budget predicate: the smallest s in 0 .. K with e[s] <= tau * e[0], K + 1 if there is none (e_0 == 0: budget 0)
FR_HD int fr_budget(const float* e, int K, float tau) {
  const float lim = fr_mul(tau, e[0]);
  for (int s = 0; s <= K; ++s)
    if (e[s] <= lim) return s;
  return K + 1;
}

// Serial reference of one row.  vals[K]: the slot values; w [K][d_p]: the operand row of every slot (bf16 values as fp32; the row of
// a padding slot is not read); x[d_p], b[d_p] (or null: 0): the delivered row and the bias, zero in the padding columns; d_p a
// multiple of 128, d_p <= FR_MAX_D.  -> e[K + 1] and budgets[n_tau].  Host only.
FR_H void fr_row_serial(int K, const float* vals, const float* w, const float* x, const float* b, int d_p, const float* taus, int n_tau,
                        float* e, int* budgets) {
  const int C = d_p / 64;
  float r[FR_MAX_D], q[64];
  for (int i = 0; i < d_p; ++i) r[i] = fr_add(x[i], b ? -b[i] : -0.f);
  for (int l = 0; l < 64; ++l) q[l] = fr_lane_sq(r + l * C, C);
  e[0] = fr_wave_sum(q);
  for (int s = 0; s < K; ++s) {
    if (vals[s] != 0.f) {
      const float nv = -vals[s];
      for (int i = 0; i < d_p; ++i) r[i] = fmaf(nv, w[(int64_t)s * d_p + i], r[i]);
      for (int l = 0; l < 64; ++l) q[l] = fr_lane_sq(r + l * C, C);
      e[s + 1] = fr_wave_sum(q);
    } else {
      e[s + 1] = e[s];
    }
  }
  for (int t = 0; t < n_tau; ++t) budgets[t] = fr_budget(e, K, taus[t]);
}

#if defined(__HIPCC__)
#include "common.h"
#include "recon.h"       // recon_row_counts

constexpr int FR_FOLD_ROWS = 1024;       // rows per histogram / count workgroup of the fold
constexpr int FR_DEPTH = 4;              // gathered operand rows in flight per wave
constexpr int FR_PITCH = 65;             // dwords per tile row: 64 lane shares + 1 (odd: the transposed read is conflict-free)
constexpr int FR_E_LD = FR_MAX_K + 4;    // the row's norms in LDS
constexpr int FR_PART_LD = FR_MAX_K + 1; // floats per unit of the sse partials
constexpr uint32_t FR_COUNTED = 0x80000000u;   // rowinfo: the row counts; the low bits: its active latents beyond slot K

struct FrTau {
  float t[FR_MAX_TAU];
  int n;
};

// The per-row tail of a pass that keeps its rows' norms in memory (pursuit.h, refit.h; the walk takes them from LDS): rowinfo, and
// on a counted row the budgets of its e[K + 1] by the serial rule.  -> counted
__device__ __forceinline__ bool fr_row_finish(bool counted, int64_t row, const float* __restrict__ e, int K, const FrTau& tau,
                                              uint32_t* __restrict__ rowinfo, unsigned short* __restrict__ bud) {
  rowinfo[row] = counted ? FR_COUNTED : 0u;
  if (counted)
    for (int t = 0; t < tau.n; ++t) bud[row * FR_MAX_TAU + t] = (unsigned short)fr_budget(e, K, tau.t[t]);
  return counted;
}

// ---- the walk.  Grid: one workgroup per FR_UNIT rows.  vals / idx [M][K]: the slots collect.h wrote; row_nnz[M]: the row's active
// latents; W [n_p][d_p]: the bf16 operand rows; b: fp32 [d] or null.  NPAIR > 0: d_p == 128 NPAIR at compile time.
//   part    [units][FR_PART_LD]: sum of e_m over the unit's counted rows
//   rowinfo [M]: FR_COUNTED | max(nnz - K, 0) on a counted row, 0 elsewhere
//   bud     [M][FR_MAX_TAU]: the budgets of a counted row
template <typename T, int NPAIR>
__global__ __launch_bounds__(256) void frontier_walk_kernel(const T* __restrict__ x, const float* __restrict__ b, const float* __restrict__ vals,
                                                            const int* __restrict__ idx, const uint32_t* __restrict__ row_nnz, int K,
                                                            const bf16_t* __restrict__ W, int64_t M, int Trows, float inv_T,
                                                            const int* __restrict__ lengths, int d, int d_p, int n_p, FrTau tau,
                                                            float* __restrict__ part, uint32_t* __restrict__ rowinfo,
                                                            unsigned short* __restrict__ bud) {
  constexpr int MAXP = NPAIR > 0 ? NPAIR : FR_MAX_D / 128;      // column pairs per lane
  constexpr int NACC = (FR_MAX_K + 1 + 63) / 64;
  using RowT = unsigned __attribute__((ext_vector_type(MAXP)));   // a lane's columns of one operand row, bf16 pairs
  __shared__ float tile[4][FR_CHUNK][FR_PITCH];
  __shared__ float e_row[4][FR_E_LD];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int npair = NPAIR > 0 ? NPAIR : d_p >> 7;
  const int c0 = lane * 2 * npair;
  const int j = lane & 31, h = lane >> 5;
  float acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = 0.f;

  for (int i = 0; i < FR_UNIT / 4; ++i) {
    const int64_t row = (int64_t)blockIdx.x * FR_UNIT + 4 * i + w;                 // (wave-uniform)
    if (!recon_row_counts(row, M, Trows, inv_T, lengths)) {
      if (row < M && lane == 0) rowinfo[row] = 0u;
      continue;
    }
    float r[2 * MAXP];
#pragma unroll
    for (int c = 0; c < 2 * MAXP; ++c) {
      const int col = c0 + c;
      r[c] = (c < 2 * npair && col < d) ? __fsub_rn(load_as_float(x + row * d + col), b ? b[col] : 0.f) : 0.f;
    }
    const float* rv = vals + row * K;
    const int* ri = idx + row * K;

    auto lane_sq = [&]() {
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < 2 * MAXP; ++c)
        if (c < 2 * npair) q = fmaf(r[c], r[c], q);
      return q;
    };
    // the norms m0 .. m_last of one chunk (m0 a multiple of FR_CHUNK): the transposed reduction of the wave's tile
    auto flush = [&](int m_last) {
      const int m0 = m_last & ~(FR_CHUNK - 1);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      const float* tr = &tile[w][j][32 * h];
      float s = tr[0];
#pragma unroll
      for (int t = 1; t < 32; ++t) s = __fadd_rn(s, tr[t]);
      const float o = __shfl_xor(s, 32, 64);
      if (h == 0 && m0 + j <= m_last) e_row[w][m0 + j] = __fadd_rn(s, o);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    };
    // the row's slots in registers, so that the walk itself issues no memory operation but the gathers: lane l keeps slots
    // 64 bk + l, bk < 4 (one coalesced load each); a slot past K is a padding slot.  An index outside the table cannot come out
    // of the collect kernels: it is clamped so that the gather stays inside W and its value is dropped -- defensive only.
    float sv[FR_MAX_K / 64];
    int si[FR_MAX_K / 64];
    int na = 0;                                          // slots up to the last non-zero value: the ones that gather
#pragma unroll
    for (int bk = 0; bk < FR_MAX_K / 64; ++bk) {         // (all the loads first, then the tests that wait for them)
      const int s = 64 * bk + lane;
      sv[bk] = s < K ? rv[s] : 0.f;
      si[bk] = s < K ? ri[s] : 0;
    }
#pragma unroll
    for (int bk = 0; bk < FR_MAX_K / 64; ++bk) {
      const bool ok = (unsigned)si[bk] < (unsigned)n_p;
      sv[bk] = ok ? sv[bk] : 0.f;
      si[bk] = ok ? si[bk] : 0;
      const unsigned long long mask = __ballot(sv[bk] != 0.f);
      if (mask) na = 64 * bk + 64 - __clzll((long long)mask);
    }
    auto slot = [&](const auto (&reg)[FR_MAX_K / 64], int s) {         // slot s < FR_MAX_K of the wave, s wave-uniform: no memory
      const int l = s & 63, bk = s >> 6;
      int a = __builtin_amdgcn_readlane(__builtin_bit_cast(int, reg[0]), l);
#pragma unroll
      for (int t = 1; t < FR_MAX_K / 64; ++t) {
        const int o = __builtin_amdgcn_readlane(__builtin_bit_cast(int, reg[t]), l);
        a = bk == t ? o : a;
      }
      return a;
    };
    // the gather of slot s, unconditional: past the last gathering slot it re-reads that slot's row with the value 0, which leaves
    // the residual as it is.  -> the value
    auto fetch = [&](int s, RowT& dst) -> float {
      const int sc = s < na ? s : na - 1;
      const int ii = slot(si, sc);
      const unsigned* wr = reinterpret_cast<const unsigned*>(W + (int64_t)ii * d_p + c0);
      // (the generic form loads all MAXP dwords, those past the lane's columns from its last one: no branch around a load)
#pragma unroll
      for (int q = 0; q < MAXP; ++q) dst[q] = wr[q < npair ? q : npair - 1];
      return s < na ? __builtin_bit_cast(float, slot(sv, s)) : 0.f;
    };
    // norm m (the residual after m slots) into the tile; a full chunk, or the last norm, is reduced
    auto put = [&](int m, float q) {
      tile[w][m & (FR_CHUNK - 1)][lane] = q;
      if ((m & (FR_CHUNK - 1)) == FR_CHUNK - 1 || m == K) flush(m);
    };

    float q = lane_sq();
    put(0, q);
    int done = 0;
    if (na > 0) {                                        // (wave-uniform)
      RowT wb[FR_DEPTH];                                 // (one vector value per gathered row: its registers stay one tuple)
      float vv[FR_DEPTH];
#pragma unroll
      for (int u = 0; u < FR_DEPTH; ++u) vv[u] = fetch(u, wb[u]);
      // groups of FR_DEPTH slots, every step the same: consume the oldest gather, issue the one FR_DEPTH slots ahead into the
      // registers it frees -- FR_DEPTH gathers are outstanding at every wait.  The last group may run past na (values 0)
      for (int s0 = 0; s0 < na; s0 += FR_DEPTH) {
#pragma unroll
        for (int u = 0; u < FR_DEPTH; ++u) {
          const float nv = -vv[u];
#pragma unroll
          for (int p = 0; p < MAXP; ++p)
            if (p < npair) {
              r[2 * p] = fmaf(nv, __uint_as_float(wb[u][p] << 16), r[2 * p]);
              r[2 * p + 1] = fmaf(nv, __uint_as_float(wb[u][p] & 0xFFFF0000u), r[2 * p + 1]);
            }
          q = lane_sq();
          // (the next gather must stay behind the arithmetic that still reads its destination -- q depends on all of it: lifted
          // over it, the gather loads into fresh registers that are copied back at the end of the group behind a wait for EVERY
          // outstanding gather)
          asm volatile("" : "+v"(q) : : "memory");
          __builtin_amdgcn_sched_barrier(0);
          vv[u] = fetch(s0 + u + FR_DEPTH, wb[u]);
          if (s0 + u + 1 <= K) put(s0 + u + 1, q);
        }
        done = s0 + FR_DEPTH < K ? s0 + FR_DEPTH : K;
      }
    }
    for (int m = done + 1; m <= K; ++m) put(m, q);       // the padding slots behind: nothing is gathered, the norm repeats

    // the row is done: its norms into the unit's sums, its budgets, its cut
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      const int m = lane + 64 * a;
      if (m <= K) acc[a] = __fadd_rn(acc[a], e_row[w][m]);
    }
    const float e0 = e_row[w][0];
#pragma unroll
    for (int t = 0; t < FR_MAX_TAU; ++t)
      if (t < tau.n) {
        const float lim = __fmul_rn(tau.t[t], e0);
        int bsel = K + 1;
        for (int base = 0; base <= K; base += 64) {
          const int m = base + lane;
          const unsigned long long mask = __ballot(m <= K && e_row[w][m] <= lim);
          if (mask) {
            bsel = base + __ffsll((long long)mask) - 1;
            break;
          }
        }
        if (lane == 0) bud[row * FR_MAX_TAU + t] = (unsigned short)bsel;
      }
    if (lane == 0) {
      const uint32_t nnz = row_nnz[row];
      rowinfo[row] = FR_COUNTED | (nnz > (uint32_t)K ? nnz - (uint32_t)K : 0u);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                         // (e_row is rewritten by the next row)
  }

  // the four waves' sums in wave order (the tile is free: every wave is past its last flush)
  __syncthreads();
  float* fold = &tile[0][0][0];
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int m = lane + 64 * a;
    if (m <= K) fold[w * FR_E_LD + m] = acc[a];
  }
  __syncthreads();
  for (int m = threadIdx.x; m <= K; m += 256)
    part[(int64_t)blockIdx.x * FR_PART_LD + m] =
        __fadd_rn(__fadd_rn(__fadd_rn(fold[m], fold[FR_E_LD + m]), fold[2 * FR_E_LD + m]), fold[3 * FR_E_LD + m]);
}

// ---- sum_x / sum_x_sq: grid (128-row blocks, d_p / 64 column chunks), 4 waves as recon_resid_kernel -- wave w takes rows
// r0 + 4 i + w, lane l column 64 chunk + l; dimpart [row blocks][2][d_p]: per wave over its 32 rows in order, then the four waves in
// order
template <typename T>
__global__ __launch_bounds__(256) void frontier_dim_kernel(const T* __restrict__ x, int64_t M, int Trows, float inv_T,
                                                           const int* __restrict__ lengths, int d, int d_p, float* __restrict__ dimpart) {
  __shared__ float red[4][2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.y * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.x * STATS_RB;
  float sx = 0.f, sxx = 0.f;
  for (int i = 0; i < STATS_RB / 4; ++i) {
    const int64_t row = r0 + 4 * i + w;                                           // (wave-uniform)
    if (recon_row_counts(row, M, Trows, inv_T, lengths) && col < d) {
      const float xv = load_as_float(x + row * d + col);
      sx += xv;
      sxx = fmaf(xv, xv, sxx);
    }
  }
  red[w][0][lane] = sx;
  red[w][1][lane] = sxx;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      dimpart[((int64_t)blockIdx.x * 2 + q) * d_p + col] = ((red[0][q][lane] + red[1][q][lane]) + red[2][q][lane]) + red[3][q][lane];
  }
}

// ---- the fold of one batch into the caller's block.  Four kinds of workgroups:
//   [0, nb_s)               one thread per budget s <= K: the unit partials in unit order into sse
//   [nb_s, nb_s + nb_dim)   one thread per model dimension: the 128-row partials in order into sum_x / sum_x_sq
//   the next n_tau x chunks per threshold and chunk of FR_FOLD_ROWS rows: the histogram of the counted rows' budgets in LDS, its
//                           non-empty bins added to budget[t] (integer atomics: order-free)
//   the last chunks         n_frames, rows_cut, active_cut of a chunk (integer atomics)
struct FrOut {                  // the caller's block (include/freud_sae.h, SAE_FRONTIER_*, and the same fields of SAE_PURSUIT_* / SAE_REFIT_*)
  unsigned long long *n_frames, *rows_cut, *active_cut;        // rows_cut / active_cut: null in a block without them
  double *sse, *sx, *sxx;
  unsigned long long* budget;
};

__global__ __launch_bounds__(256) void frontier_fold_kernel(const float* __restrict__ part, int n_units, int K,
                                                            const float* __restrict__ dimpart, int nrb_dim, int d, int d_p,
                                                            const uint32_t* __restrict__ rowinfo, const unsigned short* __restrict__ bud,
                                                            int64_t M, int n_tau, FrOut o, int nb_s, int nb_dim, int n_chunks) {
  __shared__ unsigned hist[FR_MAX_K + 2];
  __shared__ unsigned long long tot[3];
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < nb_s) {
    const int m = blk * 256 + tid;
    if (m > K) return;
    double s = 0.0;
    for (int u = 0; u < n_units; ++u) s += (double)part[(int64_t)u * FR_PART_LD + m];
    o.sse[m] += s;
  } else if (blk < nb_s + nb_dim) {
    const int i = (blk - nb_s) * 256 + tid;
    if (i >= d) return;
    double s0 = 0.0, s1 = 0.0;
    for (int rb = 0; rb < nrb_dim; ++rb) {
      s0 += (double)dimpart[((int64_t)rb * 2 + 0) * d_p + i];
      s1 += (double)dimpart[((int64_t)rb * 2 + 1) * d_p + i];
    }
    o.sx[i] += s0;
    o.sxx[i] += s1;
  } else {
    // chunk ch of FR_FOLD_ROWS rows: threshold t's histogram (t < n_tau), or the three counts (t == n_tau); integer adds only
    const int q = blk - nb_s - nb_dim, t = q / n_chunks, ch = q % n_chunks;
    const int64_t row0 = (int64_t)ch * FR_FOLD_ROWS, row1 = row0 + FR_FOLD_ROWS < M ? row0 + FR_FOLD_ROWS : M;
    if (t < n_tau) {
      for (int bq = tid; bq < K + 2; bq += 256) hist[bq] = 0u;
      __syncthreads();
      for (int64_t row = row0 + tid; row < row1; row += 256)
        if (rowinfo[row] & FR_COUNTED) {
          const unsigned bsel = bud[row * FR_MAX_TAU + t];
          atomicAdd(&hist[bsel <= (unsigned)K + 1u ? bsel : (unsigned)K + 1u], 1u);
        }
      __syncthreads();
      for (int bq = tid; bq < K + 2; bq += 256)
        if (hist[bq]) atomicAdd(&o.budget[(int64_t)t * (K + 2) + bq], (unsigned long long)hist[bq]);
    } else {
      if (tid < 3) tot[tid] = 0ull;
      __syncthreads();
      unsigned long long nf = 0, rc = 0, ac = 0;
      for (int64_t row = row0 + tid; row < row1; row += 256) {
        const uint32_t ri = rowinfo[row];
        if (ri & FR_COUNTED) {
          const uint32_t cut = ri & ~FR_COUNTED;
          nf += 1;
          rc += cut ? 1 : 0;
          ac += cut;
        }
      }
      atomicAdd(&tot[0], nf);
      atomicAdd(&tot[1], rc);
      atomicAdd(&tot[2], ac);
      __syncthreads();
      if (tid == 0) {
        atomicAdd(o.n_frames, tot[0]);
        if (o.rows_cut) atomicAdd(o.rows_cut, tot[1]);
        if (o.active_cut) atomicAdd(o.active_cut, tot[2]);
      }
    }
  }
}
#endif
