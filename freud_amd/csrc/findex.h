// Feature index (include/freud_sae.h, sae_findex_*; freud_amd/feature_index.py): the latent-major postings of an indexed feature
// store -- for every latent the (position, value) of the slots that fire it, positions ascending.  It is the transpose of the
// store's [rows][K] (value, latent) slots: a stable counting sort by latent over every slot of the dataset.
//
// A slot is POSTED iff its value is not +-0.0 (fi_posted) and its index lies in [0, n_dict); its position word is
// pos0 + row = file * T + frame (fi_position), which must stay below 2^32.  An index outside the dictionary is counted and never
// posted, and never becomes an address: the range test is made on the 64-bit value before it is narrowed.
//
// Build, per device batch of rows (a batch = whole files, in file order) and per latent range [j0, j1):
//   1. fi_count:  ONE WAVE per block of FI_ROWS rows and per segment of FI_SEG latents counts the block's posted slots per latent in
//                 LDS (32-bit counters, FI_SEG * 4 = 64 KiB per wave at most; the dictionary in segments, so any n_dict fits).
//                 Sweep 1 adds the counters to the int64 totals (integer atomic adds: order-free); sweep 2 writes them to the
//                 workspace table counts[block][latent - j0].
//   2. fi_scan:   per latent, the exclusive prefix of that table over the row blocks, started at the latent's cursor (the next free
//                 slot of its list, relative to the range's first slot); the cursor then advances by the batch's count -- lists
//                 carry on across batches.
//   3. fi_fill:   one wave per (row block, segment) loads its counters from that table and walks its rows IN ORDER; an LDS
//                 add-with-return hands every posted slot its place, which is written as (position, value).
//   4. fi_verify: over the finished lists of a range, the number of slots whose position is not strictly greater than the one before
//                 it in the same list, or is >= n_files * T.
//
// Determinism.  The place of a slot is cursor[j] + (posted slots of latent j in earlier row blocks of the batch) + (its rank among
// the block's slots of latent j).  The first two terms are integer sums of counts, whatever order they were added in.  The rank
// comes from the LDS counter of ONE wave: that wave issues its LDS adds in program order, row after row (for K > 64 the 64-slot
// chunks of a row one after the other, and only then the next row), the LDS executes the operations of one wave in the order they
// were issued, and the lanes of ONE add hold slots of one row, whose indices are distinct -- they never meet on a counter.  So
// the rank is the number of earlier rows of the block that fire the latent: it follows from the data alone.  No wave ever waits
// for, or races with, another wave for a place; there is no float atomic and no global atomic that returns a value.  A row that
// does repeat an index makes two lanes of one add meet; whichever order they get, both slots carry the same position, the list is
// then not strictly ascending and fi_verify counts it: such a store fails the build, it cannot make it irreproducible unnoticed.
//
// Cost model.  A wave reads 64 slots of one row per load (K = 64: whole 256- / 512-byte rows), FI_SUB units in flight together.
// K < 64 leaves 64 - K lanes idle: packing several rows into one LDS add would put slots of different rows -- possibly of one
// latent -- into a single instruction, and their order inside it is not something the ISA promises.  The index lists are read
// once per segment (n_dict = 24 576: twice) in each of the count and the fill; a batch (tens of MB) stays in the Infinity Cache
// between the two.  64 KiB of 32-bit counters: 128 KiB (32 768 latents) would fit gfx950's 160 KiB and save the second read at
// n_dict = 24 576, but leaves ONE wave per CU to hide a scattered 8-byte store per slot; at 64 KiB two waves per CU share it.
//
// The first part is free of any HIP type and compiles for the host (tests/test_feature_index_cpu.py replays fi_build_serial
// against numpy's stable argsort); the kernels use the same predicate and position word.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FI_HD __host__ __device__ __forceinline__
#define FI_H __host__ inline
#else
#define FI_HD inline
#define FI_H inline
#endif

enum { FI_IDX32 = 1 };           // include/freud_sae.h: SAE_FINDEX_IDX32
#define FI_MAX_K 1024            // include/freud_sae.h: SAE_COLLECT_MAX_K
#define FI_MAX_N (1 << 30)       // n_dict at most (an index is narrowed to int only after the range test)
enum { FI_SLOTS = 0, FI_ZERO = 1, FI_OUT_OF_RANGE = 2, FI_POSTED = 3, FI_NSTATS = 8 };

// a slot is posted iff its value is not +-0.0 (every other bit pattern, NaN included, is kept as stored)
FI_HD bool fi_posted(uint32_t value_bits) { return (value_bits << 1) != 0u; }
FI_HD bool fi_in_range(int64_t index, int64_t n_dict) { return index >= 0 && index < n_dict; }
// the position word of a row: pos0 = file0 * T of the batch's first row
FI_HD uint32_t fi_position(uint64_t pos0, int64_t row) { return (uint32_t)(pos0 + (uint64_t)row); }

// Serial reference build.  value_bits [rows][K], indices [rows][K]; starts [n_dict + 1], positions / values [posted slots] (pass
// null for both to learn starts[n_dict] first); stats[FI_NSTATS] is added to.  Host only.
template <typename IdxT>
FI_H void fi_build_serial(const uint32_t* value_bits, const IdxT* indices, int64_t rows, int K, int64_t n_dict, uint64_t pos0,
                          int64_t* starts, uint32_t* positions, uint32_t* values, int64_t stats[FI_NSTATS]) {
  for (int64_t j = 0; j <= n_dict; ++j) starts[j] = 0;
  for (int64_t e = 0; e < rows * K; ++e) {
    stats[FI_SLOTS] += 1;
    if (!fi_posted(value_bits[e])) { stats[FI_ZERO] += 1; continue; }
    if (!fi_in_range((int64_t)indices[e], n_dict)) { stats[FI_OUT_OF_RANGE] += 1; continue; }
    stats[FI_POSTED] += 1;
    starts[(int64_t)indices[e] + 1] += 1;
  }
  for (int64_t j = 0; j < n_dict; ++j) starts[j + 1] += starts[j];
  if (!positions || !values) return;
  int64_t* cursor = new int64_t[n_dict > 0 ? n_dict : 1];
  for (int64_t j = 0; j < n_dict; ++j) cursor[j] = starts[j];
  for (int64_t r = 0; r < rows; ++r)
    for (int q = 0; q < K; ++q) {
      const int64_t e = r * K + q;
      if (!fi_posted(value_bits[e]) || !fi_in_range((int64_t)indices[e], n_dict)) continue;
      const int64_t at = cursor[(int64_t)indices[e]]++;
      positions[at] = fi_position(pos0, r);
      values[at] = value_bits[e];
    }
  delete[] cursor;
}

// slots whose position is not strictly greater than the one before it in the same list, or is >= limit
FI_H int64_t fi_verify_serial(const int64_t* starts, int64_t n_dict, const uint32_t* positions, uint64_t limit) {
  int64_t bad = 0;
  for (int64_t j = 0; j < n_dict; ++j)
    for (int64_t i = starts[j]; i < starts[j + 1]; ++i)
      bad += ((uint64_t)positions[i] >= limit || (i > starts[j] && positions[i] <= positions[i - 1])) ? 1 : 0;
  return bad;
}

#if defined(__HIPCC__)
constexpr int FI_SUB = 32;            // (row, 64-slot chunk) units a wave holds in registers at a time
constexpr int FI_ROWS = 128;          // rows per block (one wave)
constexpr int FI_SEG = 16384;         // latents per segment: 64 KiB of 32-bit LDS counters per wave

// The units of one round: unit u = (row rs + u / nch, chunk u % nch), in that order.  jv[u] = latent - seg0 of the lane's slot if it is
// posted and inside [seg0, seg1), else -1; vb[u] its value bits.  Loads go to CLAMPED addresses and a select marks what is not
// there, so that all of them are in flight together (a predicated load is waited for inside its own block).
// ONE: K <= 64, one chunk per row (the divisions by nch fold away).
template <typename IdxT, bool ONE>
__device__ __forceinline__ void fi_load_round(const uint32_t* __restrict__ vbits, const IdxT* __restrict__ idx, int64_t rows, int K, int nch,
                                              int64_t rs, int64_t rend, int lane, int64_t n_dict, int seg0, int seg1, int (&jv)[FI_SUB],
                                              uint32_t (&vb)[FI_SUB], unsigned& n_zero, unsigned& n_oor, bool tally) {
  const int R = FI_SUB / nch;
  IdxT raw[FI_SUB];
#pragma unroll
  for (int u = 0; u < FI_SUB; ++u) {
    const int ur = ONE ? u : u / nch, q = (u - ur * nch) * 64 + lane;
    const int64_t r = rs + ur;
    const int64_t rc = r < rows ? r : rows - 1;
    const int qc = q < K ? q : K - 1;
    raw[u] = idx[rc * K + qc];
    vb[u] = vbits[rc * K + qc];
  }
#pragma unroll
  for (int u = 0; u < FI_SUB; ++u) {
    const int ur = ONE ? u : u / nch, q = (u - ur * nch) * 64 + lane;
    const bool there = ur < R && rs + ur < rend && q < K;
    const bool posted = fi_posted(vb[u]);
    const int64_t j = (int64_t)raw[u];
    const bool inr = fi_in_range(j, n_dict);
    if (tally) {
      n_zero += (there && !posted) ? 1u : 0u;
      n_oor += (there && posted && !inr) ? 1u : 0u;
    }
    jv[u] = (there && posted && inr && j >= seg0 && j < seg1) ? (int)(j - seg0) : -1;
  }
}

__device__ __forceinline__ unsigned long long fi_wave_sum(unsigned v) {
  unsigned long long s = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// ---- 1. count.  grid (row blocks, segments of [j0, j1)), 64 threads, segn * 4 bytes of LDS.
//   totals != null: totals[j] += the block's count (sweep 1);  counts != null: counts[block][j - j0] = it (sweep 2, ld = j1 - j0);
//   stats != null: the wave of segment 0 adds the block's tallies: slots seen, zero, out of range, posted.
template <typename IdxT, bool ONE>
__global__ __launch_bounds__(64) void fi_count_kernel(const uint32_t* __restrict__ vbits, const IdxT* __restrict__ idx, int64_t rows, int K,
                                                      int64_t n_dict, int j0, int j1, unsigned long long* __restrict__ totals,
                                                      unsigned int* __restrict__ counts, unsigned long long* __restrict__ stats) {
  extern __shared__ unsigned int fi_ctr[];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * FI_ROWS;
  const int64_t rend = r0 + FI_ROWS < rows ? r0 + FI_ROWS : rows;
  const int seg0 = j0 + (int)blockIdx.y * FI_SEG, seg1 = min(seg0 + FI_SEG, j1), segn = seg1 - seg0;
  for (int i = lane; i < segn; i += 64) fi_ctr[i] = 0u;
  __syncthreads();
  const int nch = ONE ? 1 : (K + 63) >> 6;           // <= 16 (K <= FI_MAX_K)
  const int R = FI_SUB / nch;
  const bool tally = stats != nullptr && blockIdx.y == 0;
  unsigned n_zero = 0, n_oor = 0;
  for (int64_t rs = r0; rs < rend; rs += R) {
    int jv[FI_SUB];
    uint32_t vb[FI_SUB];
    fi_load_round<IdxT, ONE>(vbits, idx, rows, K, nch, rs, rend, lane, n_dict, seg0, seg1, jv, vb, n_zero, n_oor, tally);
#pragma unroll
    for (int u = 0; u < FI_SUB; ++u)
      if (jv[u] >= 0) atomicAdd(&fi_ctr[jv[u]], 1u);
  }
  __syncthreads();
  if (counts) {
    unsigned int* out = counts + (int64_t)blockIdx.x * (j1 - j0) + (seg0 - j0);
    for (int i = lane; i < segn; i += 64) out[i] = fi_ctr[i];
  }
  if (totals)
    for (int i = lane; i < segn; i += 64) {
      const unsigned int c = fi_ctr[i];
      if (c) atomicAdd(totals + seg0 + i, (unsigned long long)c);
    }
  if (tally) {
    const unsigned long long z = fi_wave_sum(n_zero), o = fi_wave_sum(n_oor);
    if (lane == 0) {
      const unsigned long long seen = (unsigned long long)(rend - r0) * (unsigned long long)K;
      atomicAdd(stats + FI_SLOTS, seen);
      if (z) atomicAdd(stats + FI_ZERO, z);
      if (o) atomicAdd(stats + FI_OUT_OF_RANGE, o);
      atomicAdd(stats + FI_POSTED, seen - z - o);
    }
  }
}

// ---- 2. scan.  One workgroup = 64 latents (lane) x 16 waves; wave w owns the row blocks [w nb / 16, (w + 1) nb / 16).  In place:
// counts[b][j] becomes the first slot of (block b, latent j) relative to the range's first slot, cursor[j] advances by the total.
__global__ __launch_bounds__(1024) void fi_scan_kernel(unsigned int* __restrict__ counts, int nblocks, int j0, int j1,
                                                       long long* __restrict__ cursor, long long out_base) {
  __shared__ unsigned int part[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nr = j1 - j0;
  const int jr = blockIdx.x * 64 + lane;
  const int b0 = (int)((int64_t)nblocks * w / 16), b1 = (int)((int64_t)nblocks * (w + 1) / 16);
  unsigned int run = 0;
  if (jr < nr)
    for (int b = b0; b < b1; ++b) run += counts[(int64_t)b * nr + jr];
  part[w][lane] = run;
  __syncthreads();
  unsigned int base = 0, tot = 0;
  for (int ww = 0; ww < 16; ++ww) {
    const unsigned int v = part[ww][lane];
    base += ww < w ? v : 0u;
    tot += v;
  }
  long long cur = 0;
  if (jr < nr) {
    cur = cursor[j0 + jr];                          // (read by all 16 waves of the latent; wave 0 writes it behind the barrier)
    run = (unsigned int)(cur - out_base) + base;
    for (int b = b0; b < b1; ++b) {
      const unsigned int c = counts[(int64_t)b * nr + jr];
      counts[(int64_t)b * nr + jr] = run;
      run += c;
    }
  }
  __syncthreads();
  if (w == 0 && jr < nr) cursor[j0 + jr] = cur + (long long)tot;
}

// ---- 3. fill.  grid / LDS as the count.  block_off = the scanned table.  A place at or beyond `capacity` (the caller's buffers are
// smaller than the lists: a cursor that does not belong to this store) is not written; err[1] counts such slots.
template <typename IdxT, bool ONE>
__global__ __launch_bounds__(64) void fi_fill_kernel(const uint32_t* __restrict__ vbits, const IdxT* __restrict__ idx, int64_t rows, int K,
                                                     int64_t n_dict, int j0, int j1, unsigned long long pos0,
                                                     const unsigned int* __restrict__ block_off, uint32_t* __restrict__ positions,
                                                     uint32_t* __restrict__ values, unsigned long long capacity,
                                                     unsigned long long* __restrict__ err) {
  extern __shared__ unsigned int fi_ctr[];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * FI_ROWS;
  const int64_t rend = r0 + FI_ROWS < rows ? r0 + FI_ROWS : rows;
  const int seg0 = j0 + (int)blockIdx.y * FI_SEG, seg1 = min(seg0 + FI_SEG, j1), segn = seg1 - seg0;
  {
    const unsigned int* in = block_off + (int64_t)blockIdx.x * (j1 - j0) + (seg0 - j0);
    for (int i = lane; i < segn; i += 64) fi_ctr[i] = in[i];
  }
  __syncthreads();
  const int nch = ONE ? 1 : (K + 63) >> 6;           // <= 16 (K <= FI_MAX_K)
  const int R = FI_SUB / nch;
  unsigned n_zero = 0, n_over = 0;
  for (int64_t rs = r0; rs < rend; rs += R) {
    int jv[FI_SUB];
    uint32_t vb[FI_SUB];
    fi_load_round<IdxT, ONE>(vbits, idx, rows, K, nch, rs, rend, lane, n_dict, seg0, seg1, jv, vb, n_zero, n_zero, false);
    unsigned int at[FI_SUB];
#pragma unroll
    for (int u = 0; u < FI_SUB; ++u) {            // program order = row order: the rank of a slot is the number of earlier rows
      at[u] = 0xFFFFFFFFu;                        // of the block that fire its latent (header: Determinism)
      if (jv[u] >= 0) at[u] = atomicAdd(&fi_ctr[jv[u]], 1u);
    }
#pragma unroll
    for (int u = 0; u < FI_SUB; ++u) {
      if (jv[u] < 0) continue;
      if ((unsigned long long)at[u] >= capacity) { ++n_over; continue; }
      positions[at[u]] = fi_position(pos0, rs + (ONE ? u : u / nch));
      values[at[u]] = vb[u];
    }
  }
  const unsigned long long over = fi_wave_sum(n_over);
  if (over && lane == 0) atomicAdd(err + 1, over);
}

// ---- 4. verify.  One wave per latent of [j0, j1); starts are the absolute list starts, positions the range's buffer.
constexpr int FI_VERIFY_WAVES = 4;
__global__ __launch_bounds__(64 * FI_VERIFY_WAVES) void fi_verify_kernel(const long long* __restrict__ starts, int j0, int j1, long long out_base,
                                                                         const uint32_t* __restrict__ positions, long long capacity, unsigned long long limit,
                                                                         unsigned long long* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)j0 + (int64_t)blockIdx.x * FI_VERIFY_WAVES + (threadIdx.x >> 6);
  if (j >= j1) return;                             // wave-uniform
  const long long s = starts[j] - out_base, e = starts[j + 1] - out_base;
  if (s < 0 || e < s || e > capacity) {            // starts that do not belong to this buffer: nothing is read
    if (lane == 0) atomicAdd(err + 0, 1ull);
    return;
  }
  unsigned bad = 0;
  for (long long i = s + lane; i < e; i += 64) {
    const uint32_t p = positions[i];
    bad += ((unsigned long long)p >= limit || (i > s && p <= positions[i - 1])) ? 1u : 0u;
  }
  const unsigned long long b = fi_wave_sum(bad);
  if (b && lane == 0) atomicAdd(err + 0, b);
}
#endif  // __HIPCC__
