// The arithmetic of frame batches (frame_gather.h; include/freud_sae.h, sae_store_gather_frames; freud_amd/resident.py,
// ResidentFrameDataLoader), free of any HIP type so that the SAME functions compile for the host: tests/test_frame_batches_cpu.py
// builds them with g++ and tests/frame_batches_reference.py restates them in Python.  Everything is 64-bit: 200 000 files x 1500
// frames are 3e8 ordinals, and ordinal x frame_bytes leaves 32 bits long before that.
//
//   permutation  an epoch is a keyed bijection of [0, N), N = the counted frames of the store, EVALUATED per frame -- no index list
//                exists anywhere.  fp_permute is a Feistel network on b = bit_length(N - 1) bits (the left half takes the odd bit,
//                the halves trade widths every round, FP_ROUNDS is even so they end where they began) and walks the cycle until
//                the value is below N.  The domain D = 2^b is < 2N, the walk of position p visits only out-of-range values between
//                p and its image, and those stretches are disjoint for different p: summed over all p the network is evaluated at
//                most D times -- fewer than 2 per frame -- and every walk ends, because the cycle returns to p < N.
//                N <= 2 (b < 2: no two halves) is special-cased.  fp_unpermute walks the inverse network the same way.
//   position     rank r of W reads positions r, r + W, ...: fp_position(q, r, W) = q W + r is its q-th.
//   locate       counted ordinal g -> (file, t).  Untrimmed: g / T, g % T.  Trimmed: prefix[0 .. n_files] is the exclusive prefix
//                sum of the lengths (1 <= length <= T), file = the last one with prefix[file] <= g.  A result outside the store can
//                only come from a malformed prefix; it is clamped into the store and flagged.
//   blocks       a frame of frame_bytes is `upf` copy units of `width` bytes (16, 4 or 2; rs_copy_width of resident_index.h picks
//                it per launch).  One workgroup moves at most FP_SPAN_UNITS = FP_THREADS * FP_UNROLL units, so every thread has
//                its FP_UNROLL loads in flight before its first store and there is no loop: a frame longer than the span is cut
//                into pieces (one workgroup per piece of one row), shorter frames are dealt rows_per_block to a workgroup, at most
//                FP_MAX_ROWS (one lane evaluates one frame's permutation) -- unit e of the workgroup is unit e % n of its row e / n.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD inline
#endif

constexpr int FP_ROUNDS = 4;                                     // even: the halves end with the widths they began with
constexpr int FP_THREADS = 256;
constexpr int FP_UNROLL = 4;                                     // independent loads per thread before its first store
constexpr int64_t FP_SPAN_UNITS = (int64_t)FP_THREADS * FP_UNROLL;
constexpr int64_t FP_MAX_ROWS = FP_THREADS;
constexpr uint64_t FP_MAX_N = (1ull << 62) - 1;                  // N < 2^62

FP_HD uint64_t fp_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the key as the rounds use it: mixed once, so that neighbouring keys share nothing
FP_HD uint64_t fp_key_schedule(uint64_t key) { return fp_mix(key + 0x9E3779B97F4A7C15ull); }

// the round function of (half, round, key)
FP_HD uint64_t fp_round(uint64_t half, int round, uint64_t ks) { return fp_mix((half + (uint64_t)(round + 1) * 0x9E3779B97F4A7C15ull) ^ ks); }

// bit_length(N - 1): the width of the Feistel domain (0 for N = 1)
FP_HD int fp_bits(uint64_t N) { return N <= 1 ? 0 : 64 - __builtin_clzll(N - 1); }

FP_HD uint64_t fp_mask(int w) { return (1ull << w) - 1; }

// one pass of the network over [0, 2^b), b >= 2, and its inverse
FP_HD uint64_t fp_feistel(uint64_t ks, int b, uint64_t x) {
  int wr = b / 2, wl = b - wr;
  uint64_t L = x >> wr, R = x & fp_mask(wr);
  for (int r = 0; r < FP_ROUNDS; ++r) {
    const uint64_t nr = L ^ (fp_round(R, r, ks) & fp_mask(wl));
    L = R;
    R = nr;
    const int w = wl;
    wl = wr;
    wr = w;
  }
  return (L << wr) | R;
}

FP_HD uint64_t fp_feistel_inverse(uint64_t ks, int b, uint64_t y) {
  int wr = b / 2, wl = b - wr;                                   // after an even number of rounds: the widths of the start
  uint64_t L = y >> wr, R = y & fp_mask(wr);
  for (int r = FP_ROUNDS - 1; r >= 0; --r) {
    const int w = wl;
    wl = wr;
    wr = w;
    const uint64_t pl = R ^ (fp_round(L, r, ks) & fp_mask(wl));
    R = L;
    L = pl;
  }
  return (L << wr) | R;
}

// position p of the epoch `key` -> the counted ordinal it holds; *evals (optional) += evaluations of the network
FP_HD uint64_t fp_permute_counted(uint64_t key, uint64_t N, uint64_t p, uint64_t* evals) {
  const uint64_t ks = fp_key_schedule(key);
  if (N <= 2) return N == 2 ? (p ^ (ks & 1)) : 0;
  const int b = fp_bits(N);
  uint64_t x = p;
  do {
    x = fp_feistel(ks, b, x);
    if (evals) ++*evals;
  } while (x >= N);
  return x;
}

FP_HD uint64_t fp_permute(uint64_t key, uint64_t N, uint64_t p) { return fp_permute_counted(key, N, p, nullptr); }

// counted ordinal g -> its position in the epoch `key`
FP_HD uint64_t fp_unpermute(uint64_t key, uint64_t N, uint64_t g) {
  const uint64_t ks = fp_key_schedule(key);
  if (N <= 2) return N == 2 ? (g ^ (ks & 1)) : 0;
  const int b = fp_bits(N);
  uint64_t x = g;
  do {
    x = fp_feistel_inverse(ks, b, x);
  } while (x >= N);
  return x;
}

FP_HD uint64_t fp_position(uint64_t q, uint64_t rank, uint64_t world) { return q * world + rank; }

// counted ordinal g -> (file, t); returns whether the result had to be clamped into the store.  prefix: null (untrimmed) or the
// exclusive prefix sum of the trimmed lengths, n_files + 1 entries.
FP_HD bool fp_locate(const int64_t* prefix, int64_t n_files, int64_t T, int64_t g, int64_t* file, int64_t* t) {
  int64_t f, at;
  if (!prefix) {
    f = g / T;
    at = g % T;
  } else {
    int64_t lo = 0, hi = n_files;                                // prefix[lo] <= g < prefix[hi], as far as the prefix is sound
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (prefix[mid] <= g) lo = mid; else hi = mid;
    }
    f = lo;
    at = g - prefix[lo];
  }
  const bool bad = g < 0 || f < 0 || f >= n_files || at < 0 || at >= T;
  *file = f < 0 ? 0 : (f >= n_files ? n_files - 1 : f);
  *t = at < 0 ? 0 : (at >= T ? T - 1 : at);
  return bad;
}

// (file, t) -> the frame's row in the store's [n_files * T, d] view
FP_HD int64_t fp_store_row(int64_t file, int64_t T, int64_t t) { return file * T + t; }

// ---- the launch's decomposition
struct fp_plan {
  int64_t upf;             // copy units per frame
  int64_t pieces;          // workgroups per row (1 unless the frame is longer than the span)
  int64_t rows_per_block;  // rows per workgroup (1 when pieces > 1)
  int64_t blocks;          // the grid
};

FP_HD fp_plan fp_plan_of(int64_t frame_bytes, int width, int64_t rows) {
  fp_plan p;
  p.upf = frame_bytes / width;
  p.pieces = (p.upf + FP_SPAN_UNITS - 1) / FP_SPAN_UNITS;
  const int64_t fit = FP_SPAN_UNITS / p.upf;
  p.rows_per_block = p.pieces > 1 ? 1 : (fit > FP_MAX_ROWS ? FP_MAX_ROWS : fit);
  p.blocks = (rows + p.rows_per_block - 1) / p.rows_per_block * p.pieces;
  return p;
}

// workgroup w -> rows [row0, row0 + nrows) and, of each of them, the units [unit0, unit0 + n); nrows * n <= FP_SPAN_UNITS
FP_HD void fp_block_span(const fp_plan& p, int64_t rows, int64_t w, int64_t* row0, int* nrows, int64_t* unit0, int* n) {
  const int64_t rb = w / p.pieces, piece = w % p.pieces;
  *row0 = rb * p.rows_per_block;
  const int64_t left = rows - *row0;
  *nrows = (int)(left < p.rows_per_block ? left : p.rows_per_block);
  *unit0 = piece * FP_SPAN_UNITS;
  const int64_t rest = p.upf - *unit0;
  *n = (int)(rest < FP_SPAN_UNITS ? rest : FP_SPAN_UNITS);
}

// unit e of a workgroup (e < nrows * n) -> (row r of the workgroup, unit c of the span)
FP_HD void fp_unit_of(uint32_t e, uint32_t n, uint32_t* r, uint32_t* c) {
  *r = e / n;
  *c = e - *r * n;
}
