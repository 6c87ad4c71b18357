// Feature collection (include/freud_sae.h, sae_collect_files): every row's K slots in the reference's indexed form -- the first K
// entries of a stable descending sort of the latent row encode() returns (value descending, equal values by the lower column).
//
// One 64-bit ENTRY per column carries the whole order: (pattern << 32) | (0xFFFFFFFF - column), with pattern = the bf16 bits of an
// ACTIVE latent (magnitude bits non-zero, sign clear: then the 15 magnitude bits order like the value) and 0 for every other
// column -- an inactive column, -0.0 included, is the value +0.0.  Larger entry = earlier slot, no two entries of a row are equal,
// and the zero-valued columns that pad a row with fewer than K active latents follow the active ones in increasing column order
// without a rule of their own.  The column takes the full low word (n_dict goes past 65 535).  An entry of 0 is no column's.
//
// The first part is free of any HIP type and compiles for the host as file_top.h and search_keys.h do
// (tests/test_collect_features_cpu.py replays cl_collect_serial against numpy's stable argsort); the kernels' answers are defined by
// it and they use the same entry word and predicate.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CL_HD __host__ __device__ __forceinline__
#define CL_H __host__ inline
#else
#define CL_HD inline
#define CL_H inline
#endif

enum { CL_IDX32 = 1 };           // include/freud_sae.h: SAE_COLLECT_IDX32
#define CL_MAX_K 1024            // include/freud_sae.h: SAE_COLLECT_MAX_K
enum { CL_ROWS = 0, CL_STORED = 1, CL_DROPPED = 2, CL_ROWS_DROPPED = 3, CL_MAX_ACTIVE = 4, CL_MAX_DROPPED = 5, CL_NSTATS = 8 };

// a latent is ACTIVE iff its magnitude bits are non-zero and its sign is clear (stats.h counts the same way)
CL_HD bool cl_active(uint32_t bits) { return (uint32_t)((bits & 0xFFFFu) - 1u) < 0x7FFFu; }
CL_HD uint64_t cl_entry(uint32_t bits, uint32_t col) { return ((uint64_t)(cl_active(bits) ? (bits & 0xFFFFu) : 0u) << 32) | (uint64_t)(0xFFFFFFFFu - col); }
CL_HD uint32_t cl_entry_bits(uint64_t e) { return (uint32_t)(e >> 32); }
CL_HD uint32_t cl_entry_col(uint64_t e) { return 0xFFFFFFFFu - (uint32_t)e; }
// entry a takes an earlier slot than entry b
CL_HD bool cl_before(uint64_t a, uint64_t b) { return a > b; }
// the stored fp32 value: the bf16 pattern widened (exact); an inactive column stores +0.0
CL_HD float cl_value(uint32_t pattern) { const uint32_t u = pattern << 16; float v; __builtin_memcpy(&v, &u, 4); return v; }

// Serial reference of one row: row_bits[n] (bf16 patterns) -> vals[K], idx[K] in slot order, and the row added to stats[8].
// 1 <= K <= n.  It keeps the best K + 1 entries: the entry behind slot K - 1 is the largest one that was cut.  Host only.
CL_H void cl_collect_serial(const uint16_t* row_bits, int64_t n, int K, float* vals, int64_t* idx, int64_t stats[8]) {
  const int cap = (int64_t)K + 1 < n ? K + 1 : (int)n;
  uint64_t* best = new uint64_t[cap];
  int m = 0;
  int64_t nnz = 0;
  for (int64_t j = 0; j < n; ++j) {
    const uint64_t e = cl_entry(row_bits[j], (uint32_t)j);
    nnz += cl_active(row_bits[j]) ? 1 : 0;
    if (m == cap && !cl_before(e, best[m - 1])) continue;
    int i = m < cap ? m : cap - 1;
    while (i > 0 && cl_before(e, best[i - 1])) { best[i] = best[i - 1]; --i; }
    best[i] = e;
    if (m < cap) ++m;
  }
  for (int i = 0; i < K; ++i) {
    vals[i] = cl_value(cl_entry_bits(best[i]));
    idx[i] = (int64_t)cl_entry_col(best[i]);
  }
  const int64_t stored = nnz < K ? nnz : K;
  const int64_t cut = cap > K ? (int64_t)cl_entry_bits(best[K]) : 0;      // 0: the entry behind the last slot is inactive, or none is
  stats[CL_ROWS] += 1;
  stats[CL_STORED] += stored;
  stats[CL_DROPPED] += nnz - stored;
  stats[CL_ROWS_DROPPED] += nnz > stored ? 1 : 0;
  if (nnz > stats[CL_MAX_ACTIVE]) stats[CL_MAX_ACTIVE] = nnz;
  if (cut > stats[CL_MAX_DROPPED]) stats[CL_MAX_DROPPED] = cut;
  delete[] best;
}

#if defined(__HIPCC__)
#include "common.h"
// ---- kernels.  Workgroups of CL_THREADS stride over the rows; entries live in LDS and a bitonic sort puts them in slot order, so
// the compaction order (LDS counters) never shows: the selected set is exact and its order total -- two runs give the same bytes.
// Row statistics stay in thread 0's registers until the workgroup is done: six integer atomics per workgroup, not per row.
// row_nnz (or null): the number of active latents of every row, for the sparsity frontier (frontier.h).
#define CL_THREADS 256
#define CL_COLS_PER_IT (8 * CL_THREADS)   // one 16-byte load per thread

// descending bitonic sort of e[0, P), P a power of two, by the nt threads t = 0 .. nt - 1 that share it; every thread of the
// workgroup calls it with the same P (workgroup barriers), after a barrier that made e visible
__device__ __forceinline__ void cl_sort_desc(uint64_t* e, int P, int t, int nt) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (P >> 1); p += nt) {
        const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
        const uint64_t a = e[lo], b = e[hi];
        const bool desc = (lo & k) == 0;
        if (desc ? cl_before(b, a) : cl_before(a, b)) { e[lo] = b; e[hi] = a; }
      }
      __syncthreads();
    }
}

template <typename IdxT>
__device__ __forceinline__ void cl_write_slots(const uint64_t* e, int K, int t, int nt, float* __restrict__ vals, IdxT* __restrict__ idx) {
  for (int j = t; j < K; j += nt) {
    const uint64_t w = e[j];
    vals[j] = cl_value(cl_entry_bits(w));
    idx[j] = (IdxT)cl_entry_col(w);
  }
}

__device__ __forceinline__ void cl_flush_stats(unsigned long long* st, unsigned long long rows, unsigned long long stored,
                                               unsigned long long dropped, unsigned long long rows_dropped, unsigned long long max_active,
                                               unsigned long long max_dropped) {
  if (rows == 0) return;
  atomicAdd(st + CL_ROWS, rows);
  atomicAdd(st + CL_STORED, stored);
  if (dropped) {
    atomicAdd(st + CL_DROPPED, dropped);
    atomicAdd(st + CL_ROWS_DROPPED, rows_dropped);
    atomicMax(st + CL_MAX_DROPPED, max_dropped);
  }
  atomicMax(st + CL_MAX_ACTIVE, max_active);
}

// slots of a wave's flagged lanes behind an LDS counter: one atomic per wave, the lanes in lane order behind it (every lane of the
// wave must call)
__device__ __forceinline__ uint32_t cl_wave_slot(bool flag, uint32_t* counter, int lane) {
  const unsigned long long m = __ballot(flag);
  if (m == 0) return 0;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, 0, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// position of the r-th (0-based) set bit of the nw-word mask; the caller knows it exists.  Every lane reads the same words (LDS
// broadcast); inside the word a binary search on the popcount of the low half
__device__ __forceinline__ uint32_t cl_nth_set_bit(const uint64_t* mask, int nw, uint32_t r) {
  for (int w = 0; w < nw; ++w) {
    uint64_t m = mask[w];
    const uint32_t c = (uint32_t)__popcll(m);
    if (r < c) {
      uint32_t pos = 0;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const uint32_t lc = (uint32_t)__popcll(m & ((1ull << s) - 1ull));
        if (r >= lc) { r -= lc; m >>= s; pos += s; }
      }
      return (uint32_t)w * 64u + pos;
    }
    r -= c;
  }
  return 0;
}

// the 256-bin histogram read from the top by wave 0: the bin in which the count from bin 255 down reaches `need`, and the count above
// that bin (lane l owns the bins 255 - 4 l ... 252 - 4 l).  need >= 1 and need <= the histogram's total.
__device__ __forceinline__ void cl_find_bin(const uint32_t* hist, uint32_t need, int tid, uint32_t* s_bin, uint32_t* s_above) {
  if (tid < 64) {
    uint32_t c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; s += c[j]; }
    uint32_t incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
      if (tid >= o) incl += t;
    }
    uint32_t run = incl - s;
    if (run < need && need <= incl) {
      bool done = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!done && run + c[j] >= need) { *s_bin = 255 - 4 * tid - j; *s_above = run; done = true; }
        if (!done) run += c[j];
      }
    }
  }
}

// ---- L1: the stored latent lat [M_p][ld] (bf16 bits, post-ReLU, ld a multiple of 8 and the rows 16-byte aligned), n <= ld columns
// count.  One workgroup per row at a time.  A row is read with one 16-byte load per thread and iteration, columns in thread order.
//
// First read: the active entries are compacted into ent[0, K) (those that fit) and counted, and the inactivity of the columns
// [0, K) is kept as a bit mask (a thread owns 8 adjacent columns: one byte of it).  A row with at most K active latents -- the
// common one -- is then done with reading: only its nnz entries are sorted (a power of two >= nnz of them, not K), and slot j >= nnz
// is the (j - nnz)-th inactive column, read off the mask by a popcount walk.  Those columns all lie below column K (at most nnz of
// the first K columns are active), so the mask never needs more than K bits.  No threshold search.
//
// A row with more than K active latents takes three more reads (from L2): two histogram passes find the K-th largest pattern t
// exactly (high 8 bits, then low 7 bits of the 15; a thread adds runs of equal digits with one LDS atomic), then a pass in column
// order takes every pattern above t and, of the ties at t, the first K - count(> t) by a prefix count over the workgroup (one barrier
// per iteration, skipped once the ties are complete); the largest pattern not taken is the row's largest dropped value.
template <typename IdxT>
__global__ __launch_bounds__(CL_THREADS) void collect_l1_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t M, int K,
                                                                float* __restrict__ vals, IdxT* __restrict__ idx,
                                                                unsigned long long* __restrict__ stats, uint32_t* __restrict__ row_nnz) {
  __shared__ uint64_t ent[CL_MAX_K];
  __shared__ uint64_t inact_mask[CL_MAX_K / 64];     // bit c: column c < K is inactive
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_cnt, s_bin, s_above, s_wt[2][4], s_wmax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int PK = 1;
  while (PK < K) PK <<= 1;
  unsigned long long st_rows = 0, st_stored = 0, st_dropped = 0, st_rows_dropped = 0, st_max_active = 0, st_max_dropped = 0;

  for (int64_t r = blockIdx.x; r < M; r += gridDim.x) {
    const unsigned short* row = lat + r * ld;
    if (tid == 0) s_cnt = 0;
    __syncthreads();

    // ---- the first read
    for (int base = 0; base < n; base += CL_COLS_PER_IT) {
      const int c0 = base + tid * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (c0 < n) v = *reinterpret_cast<const u32x4*>(row + c0);
      uint32_t inact = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = c0 + e;
        const uint32_t b = (v[e >> 1] >> ((e & 1) << 4)) & 0xFFFFu;
        const bool act = col < n && cl_active(b);
        const uint32_t slot = cl_wave_slot(act, &s_cnt, lane);
        if (act && slot < (uint32_t)K) ent[slot] = cl_entry(b, (uint32_t)col);
        inact |= (!act && col < K) ? 1u << e : 0u;                             // (K <= n: a column below K exists)
      }
      // the columns [0, CL_MAX_K) are those of the first iteration's threads 0 .. CL_MAX_K / 8 - 1; every byte is rewritten per row
      if (base == 0 && tid < CL_MAX_K / 8) reinterpret_cast<unsigned char*>(inact_mask)[tid] = (unsigned char)inact;
    }
    __syncthreads();
    const uint32_t nnz = s_cnt;
    uint32_t row_max_dropped = 0;

    if (nnz <= (uint32_t)K) {
      int PA = 1;
      while (PA < (int)nnz) PA <<= 1;
      for (int j = (int)nnz + tid; j < PA; j += CL_THREADS) ent[j] = 0;
      __syncthreads();
      cl_sort_desc(ent, PA, tid, CL_THREADS);
      float* rv = vals + r * K;
      IdxT* ri = idx + r * K;
      for (int j = tid; j < K; j += CL_THREADS) {
        if (j < (int)nnz) {
          const uint64_t w = ent[j];
          rv[j] = cl_value(cl_entry_bits(w));
          ri[j] = (IdxT)cl_entry_col(w);
        } else {
          rv[j] = 0.0f;
          ri[j] = (IdxT)cl_nth_set_bit(inact_mask, (K + 63) >> 6, (uint32_t)j - nnz);
        }
      }
    } else {
      // ---- the K-th largest pattern: high digit, then low digit
      uint32_t need = (uint32_t)K, hi_bin = 0, above = 0;
      for (int pass = 0; pass < 2; ++pass) {
        hist[tid] = 0;
        __syncthreads();
        uint32_t run_bin = 0, run_cnt = 0;
        for (int base = 0; base < n; base += CL_COLS_PER_IT) {
          const int c0 = base + tid * 8;
          if (c0 < n) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(row + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const uint32_t b = (v[e >> 1] >> ((e & 1) << 4)) & 0xFFFFu;
              if (c0 + e < n && cl_active(b) && (pass == 0 || (b >> 7) == hi_bin)) {
                const uint32_t d = pass == 0 ? b >> 7 : b & 0x7Fu;
                if (d != run_bin && run_cnt) { atomicAdd(&hist[run_bin], run_cnt); run_cnt = 0; }
                run_bin = d;
                ++run_cnt;
              }
            }
          }
        }
        if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
        __syncthreads();
        cl_find_bin(hist, need, tid, &s_bin, &s_above);
        __syncthreads();
        if (pass == 0) hi_bin = s_bin;
        above += s_above;
        need -= s_above;
        __syncthreads();                      // (s_bin / s_above are rewritten by the next pass)
      }
      const uint32_t thr = (hi_bin << 7) | s_bin;      // the K-th largest pattern; `above` patterns are larger, `need` ties are taken
      for (int j = K + tid; j < PK; j += CL_THREADS) ent[j] = 0;
      if (tid == 0) s_cnt = 0;
      __syncthreads();

      // ---- the take, in column order
      uint32_t tie_base = 0, dmax = 0;
      int it = 0;
      for (int base = 0; base < n; base += CL_COLS_PER_IT, ++it) {
        const int c0 = base + tid * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (c0 < n) v = *reinterpret_cast<const u32x4*>(row + c0);
        uint32_t bits[8], ties = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t b = (v[e >> 1] >> ((e & 1) << 4)) & 0xFFFFu;
          bits[e] = (c0 + e < n && cl_active(b)) ? b : 0u;
          ties += bits[e] == thr ? 1u : 0u;
        }
        uint32_t my_tie = need;                // rank of this thread's first tie among the row's ties; >= need: none is taken
        if (tie_base < need) {                 // (uniform: tie_base is the same in every thread)
          uint32_t incl = ties;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += t;
          }
          if (lane == 63) s_wt[it & 1][wave] = incl;
          __syncthreads();
          uint32_t before = 0, total = 0;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const uint32_t c = s_wt[it & 1][w];
            before += w < wave ? c : 0u;
            total += c;
          }
          my_tie = tie_base + before + incl - ties;
          tie_base += total;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t b = bits[e];
          const bool gt = b > thr;
          const uint32_t slot = cl_wave_slot(gt, &s_cnt, lane);
          if (gt && slot < above) ent[slot] = cl_entry(b, (uint32_t)(c0 + e));      // (exactly `above` patterns are larger; above < K)
          if (b == thr) {
            if (my_tie < need) ent[above + my_tie] = cl_entry(b, (uint32_t)(c0 + e));
            else dmax = thr;
            ++my_tie;
          } else if (b != 0 && !gt) {
            dmax = b > dmax ? b : dmax;
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)dmax, o, 64);
        dmax = t > dmax ? t : dmax;
      }
      if (lane == 0) s_wmax[wave] = dmax;
      __syncthreads();
      row_max_dropped = s_wmax[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) row_max_dropped = s_wmax[w] > row_max_dropped ? s_wmax[w] : row_max_dropped;
      cl_sort_desc(ent, PK, tid, CL_THREADS);
      cl_write_slots<IdxT>(ent, K, tid, CL_THREADS, vals + r * K, idx + r * K);
    }

    if (tid == 0) {
      const uint32_t stored = nnz < (uint32_t)K ? nnz : (uint32_t)K;
      if (row_nnz) row_nnz[r] = nnz;
      st_rows += 1;
      st_stored += stored;
      st_dropped += nnz - stored;
      st_rows_dropped += nnz > stored ? 1u : 0u;
      st_max_active = nnz > st_max_active ? nnz : st_max_active;
      st_max_dropped = row_max_dropped > st_max_dropped ? row_max_dropped : st_max_dropped;
    }
    __syncthreads();                          // (ent, s_cnt and s_wmax are rewritten by the next row)
  }
  if (tid == 0) cl_flush_stats(stats, st_rows, st_stored, st_dropped, st_rows_dropped, st_max_active, st_max_dropped);
}

// ---- TopK: the compact selection sel_idx / sel_vals [M][k] in the select kernels' arbitrary order.  One WAVE per row, four rows per
// workgroup at a time: a row's k entries (k <= 1024) are sorted in the wave's own LDS segment and the first K written.  The selected
// zeros of a row with fewer than k positives carry pattern 0: they come out behind the positives in column order, value +0.0.
// Every wave runs the same number of sort stages (PK is one number), so the workgroup barriers of cl_sort_desc are uniform.
template <typename IdxT>
__global__ __launch_bounds__(CL_THREADS) void collect_topk_kernel(const int* __restrict__ sel_idx, const unsigned short* __restrict__ sel_vals,
                                                                  int k, int64_t M, int K, float* __restrict__ vals, IdxT* __restrict__ idx,
                                                                  unsigned long long* __restrict__ stats, uint32_t* __restrict__ row_nnz) {
  __shared__ uint64_t ent_all[4 * CL_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t* ent = ent_all + wave * CL_MAX_K;
  int PK = 1;
  while (PK < k) PK <<= 1;
  unsigned long long st_rows = 0, st_stored = 0, st_dropped = 0, st_rows_dropped = 0, st_max_active = 0, st_max_dropped = 0;

  for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < M; r0 += (int64_t)gridDim.x * 4) {
    const int64_t r = r0 + wave;
    const bool live = r < M;
    uint32_t nnz = 0;
    for (int j = lane; j < PK; j += 64) {
      uint64_t e = 0;
      if (live && j < k) {
        const uint32_t b = sel_vals[r * k + j];
        e = cl_entry(b, (uint32_t)sel_idx[r * k + j]);
        nnz += cl_active(b) ? 1u : 0u;
      }
      ent[j] = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nnz += (uint32_t)__shfl_xor((int)nnz, o, 64);
    __syncthreads();
    cl_sort_desc(ent, PK, lane, 64);
    if (live) {
      cl_write_slots<IdxT>(ent, K, lane, 64, vals + r * K, idx + r * K);
      if (lane == 0) {
        const uint32_t stored = nnz < (uint32_t)K ? nnz : (uint32_t)K;
        if (row_nnz) row_nnz[r] = nnz;
        const uint32_t cut = nnz > stored ? cl_entry_bits(ent[K]) : 0u;        // (nnz > K: K < k, the entry exists)
        st_rows += 1;
        st_stored += stored;
        st_dropped += nnz - stored;
        st_rows_dropped += nnz > stored ? 1u : 0u;
        st_max_active = nnz > st_max_active ? nnz : st_max_active;
        st_max_dropped = cut > st_max_dropped ? cut : st_max_dropped;
      }
    }
    __syncthreads();                          // (ent is rewritten by the next row)
  }
  // the four waves' row statistics: one set of atomics per wave that saw a row
  if (lane == 0) cl_flush_stats(stats, st_rows, st_stored, st_dropped, st_rows_dropped, st_max_active, st_max_dropped);
}
#endif
