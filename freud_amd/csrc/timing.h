// Feature timing (include/freud_sae.h, sae_timing_files): for how long every latent fires -- per latent the histogram of its run
// durations (run_hist [n][NB]), of the gaps between consecutive runs of a file (gap_hist [n][NB]) and six totals (totals [n][6]: active
// frames, summed durations, runs, files with a run, the longest run, censored runs).  Runs, the bridge and the bins are
// timing_bins.h's; a frame is active iff the bf16 magnitude bits of the value encode() returns exceed threshold_bits; frames count
// as in stats.h (search_len).  Every output is an int64 running total, every sum an integer add and LONGEST an integer max: two runs
// give bitwise identical arrays, whatever the batch and the launch geometry.  These are the kernels of the tree that carry state
// from frame t to frame t + 1.
//
// L1 (timing_l1_kernel) reads the stored latent [M_p][ld] with the geometry of hist_l1_kernel: one thread owns one column and walks
// a chunk of whole files in row order, a workgroup is blockDim.x adjacent columns.  The state of the open run (first and last
// active frame; first < 0: none in this file yet) and the six totals are registers.  The two histograms are counted in LDS, two
// 16-bit counters per dword: h[q][thread], q < nq = (NB + 1) / 2 for the runs and nq <= q < 2 nq for the gaps, bins 2q' (low half) and
// 2q' + 1 (high half), so the dword of lane l is on bank l % 32 whatever the bin and a 32-lane group never conflicts.  A thread owns
// its column: plain read-modify-writes, no barrier anywhere.  Every run and every gap holds at least one row of its own, so the
// counts of a column since its last flush sum to at most the rows since then: the counters are flushed -- one global integer add
// per non-empty bin, the totals with them -- at the end of the chunk and before a file would take those rows past TM_FLUSH_ROWS =
// 65535; a half-word cannot wrap.  The loads of TM_UNROLL rows are in flight together; only the state update is serial.
//
// TopK (timing_topk_kernel) reads the selection idx / vals [M][k]: ONE WAVE per (file, segment of TM_SEG = 8192 latents).  LDS holds
// per latent of the segment one dword first | last << 16 (first = 0xFFFF: no run in this file yet; positions are <= 65534) and a
// 16-bit count of the active frames of the open run: 48 KiB per wave, three waves per CU, any n_dict in segments.  The wave walks
// the file's counted frames in order, its lanes take a row's slots in chunks of 64, TM_SUB (row, chunk) units loaded ahead.  A slot
// inside the segment that passes the threshold extends its latent's run if t - last - 1 <= g, else it closes the open run -- one
// global integer add into run_hist, one into gap_hist, the adds of the totals, none of them returning a value -- and opens one at
// t.  After the last counted frame a strided sweep closes what is open.  The lanes of one LDS instruction hold slots of ONE row,
// whose indices are distinct, and the LDS executes a wave's operations in the order they were issued (a wavefront-scope fence
// between two rows keeps the compiler from changing that order; it costs no instruction): no conflicts, no waiting.  A row that
// does repeat an index makes two lanes meet on one table entry: the counts of that latent are then unspecified, nothing else is.
// An index outside [0, n) is ignored and never becomes an address.
#pragma once
#include "common.h"
#include "hist.h"        // hist_add, hist_frames_kernel
#include "search.h"      // search_len: the trimmed length of a file
#include "timing_bins.h"

constexpr int TM_FLUSH_ROWS = 65535;     // rows between two flushes of the 16-bit LDS counters, at most
constexpr int TM_UNROLL = 16;            // rows of a column in flight (L1)
constexpr int TM_SEG = 8192;             // latents per segment (TopK): 4 + 2 bytes of LDS each
constexpr int TM_SUB = 16;               // (row, 64-slot chunk) units a wave loads ahead (TopK); k <= 1024: a row is at most 16
constexpr int TM_MAX_K = 1024;
constexpr uint32_t TM_NONE = 0xFFFFu;
static_assert(TM_FLUSH_ROWS >= TB_MAX_ROWS, "a file must fit between two flushes");
static_assert(TM_SUB * 64 >= TM_MAX_K, "a round holds at least one whole row");

__device__ __forceinline__ void timing_max(int64_t* p, uint32_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// ---- L1.  Grid (column blocks of blockDim.x, chunks of files_per_chunk files); dynamic LDS 2 ((NB + 1) / 2) * blockDim.x dwords.
__global__ __launch_bounds__(256) void timing_l1_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t n_files, int T,
                                                        const int* __restrict__ lengths, int files_per_chunk, int sub_bits, int bridge,
                                                        uint32_t threshold, int64_t* __restrict__ run_hist, int64_t* __restrict__ gap_hist,
                                                        int64_t* __restrict__ totals) {
  extern __shared__ uint32_t timing_lds[];
  const int nt = blockDim.x, tid = threadIdx.x;
  const int col = blockIdx.x * nt + tid;
  if (col >= n) return;                    // (no barrier below: a thread owns its column and its LDS dwords)
  const int nb = timing_nbins(sub_bits, T), nq = (nb + 1) >> 1;
  uint32_t* h = timing_lds + tid;
  for (int q = 0; q < 2 * nq; ++q) h[q * nt] = 0;
  int64_t* rh = run_hist + (int64_t)col * nb;
  int64_t* gh = gap_hist + (int64_t)col * nb;
  int64_t* tot = totals + (int64_t)col * TB_NTOTALS;
  uint32_t since = 0, active = 0, span = 0, runs = 0, files = 0, longest = 0, censored = 0;

  auto flush = [&]() {
    for (int q = 0; q < 2 * nq; ++q) {
      const uint32_t w = h[q * nt];
      if (w) {
        int64_t* o = q < nq ? rh + 2 * q : gh + 2 * (q - nq);
        if (w & 0xFFFFu) hist_add(o, w & 0xFFFFu);
        if (w >> 16) hist_add(o + 1, w >> 16);
        h[q * nt] = 0;
      }
    }
    if (active) hist_add(tot + TB_ACTIVE, active);
    if (runs) {
      hist_add(tot + TB_SPAN, span);
      hist_add(tot + TB_RUNS, runs);
      timing_max(tot + TB_LONGEST, longest);
    }
    if (files) hist_add(tot + TB_FILES, files);
    if (censored) hist_add(tot + TB_CENSORED, censored);
    since = active = span = runs = files = longest = censored = 0;
  };
  auto bump = [&](int base, uint32_t L) {
    const int b = timing_index(L, sub_bits) - 1;
    h[(base + (b >> 1)) * nt] += 1u << ((b & 1) << 4);
  };

  const int64_t f0 = (int64_t)blockIdx.y * files_per_chunk;
  const int64_t f1 = f0 + files_per_chunk < n_files ? f0 + files_per_chunk : n_files;
  for (int64_t f = f0; f < f1; ++f) {
    const int len = search_len(lengths, (int)f, T);
    const unsigned short* p = lat + f * T * ld + col;
    if (since + (uint32_t)len > (uint32_t)TM_FLUSH_ROWS) flush();
    since += (uint32_t)len;
    int first = -1, last = -1;
    auto close = [&](bool at_end) {
      const uint32_t dur = (uint32_t)(last - first + 1);
      bump(0, dur);
      span += dur;
      ++runs;
      longest = dur > longest ? dur : longest;
      censored += (first == 0 || (at_end && last == len - 1)) ? 1u : 0u;
    };
    auto step = [&](uint32_t bits, int t) {
      if (!timing_active(bits, threshold)) return;
      ++active;
      if (first < 0) {
        first = t;
      } else if (t - last - 1 > bridge) {
        close(false);                      // (a run closed by a later frame does not end on the last one)
        bump(nq, (uint32_t)(t - last - 1));
        first = t;
      }
      last = t;
    };
    int r = 0;
    for (; r + TM_UNROLL <= len; r += TM_UNROLL) {
      uint32_t v[TM_UNROLL];
#pragma unroll
      for (int e = 0; e < TM_UNROLL; ++e) v[e] = p[(int64_t)(r + e) * ld];
#pragma unroll
      for (int e = 0; e < TM_UNROLL; ++e) step(v[e], r + e);
    }
    for (; r < len; ++r) step(p[(int64_t)r * ld], r);
    if (first >= 0) {
      close(true);
      ++files;
    }
  }
  flush();
}

// ---- TopK.  Grid (files, segments of TM_SEG latents), 64 threads; static LDS TM_SEG * 6 bytes.
// closing the run [first, last] of latent j with `cnt` active frames: the global adds of one lane
__device__ __forceinline__ void timing_topk_close(int64_t* __restrict__ run_hist, int64_t* __restrict__ totals, int j, int nb, int sub_bits,
                                                  uint32_t first, uint32_t last, uint32_t cnt, bool censored) {
  const uint32_t dur = last - first + 1;
  int64_t* tot = totals + (int64_t)j * TB_NTOTALS;
  hist_add(run_hist + (int64_t)j * nb + (timing_index(dur, sub_bits) - 1), 1u);
  hist_add(tot + TB_ACTIVE, cnt);
  hist_add(tot + TB_SPAN, dur);
  hist_add(tot + TB_RUNS, 1u);
  timing_max(tot + TB_LONGEST, dur);
  if (censored) hist_add(tot + TB_CENSORED, 1u);
}

template <bool ONE>   // ONE: k <= 64, one chunk per row (the divisions by nch fold away)
__global__ __launch_bounds__(64) void timing_topk_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals, int k, int T,
                                                         const int* __restrict__ lengths, int n, int sub_bits, int bridge, uint32_t threshold,
                                                         int64_t* __restrict__ run_hist, int64_t* __restrict__ gap_hist,
                                                         int64_t* __restrict__ totals) {
  __shared__ uint32_t fl[TM_SEG];          // first | last << 16
  __shared__ unsigned short cnt[TM_SEG];   // active frames of the open run
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int seg0 = (int)blockIdx.y * TM_SEG, seg1 = min(seg0 + TM_SEG, n), segn = seg1 - seg0;
  const int len = search_len(lengths, (int)f, T);
  const int nb = timing_nbins(sub_bits, T);
  for (int i = lane; i < segn; i += 64) fl[i] = TM_NONE;
  __syncthreads();
  const int nch = ONE ? 1 : (k + 63) >> 6;           // <= 16 (k <= TM_MAX_K)
  const int R = TM_SUB / nch;                        // whole rows per round, >= 1
  const int* ip = idx + f * T * k;
  const unsigned short* vp = vals + f * T * k;
  for (int rs = 0; rs < len; rs += R) {
    int raw[TM_SUB];
    uint32_t vb[TM_SUB];
    // loads go to CLAMPED addresses and a select marks what is not there, so that all of them are in flight together
#pragma unroll
    for (int u = 0; u < TM_SUB; ++u) {
      const int ur = ONE ? u : u / nch, q = (u - ur * nch) * 64 + lane;
      const int t = rs + ur;
      const int64_t at = (int64_t)(t < len ? t : len - 1) * k + (q < k ? q : k - 1);
      raw[u] = ip[at];
      vb[u] = vp[at];
    }
#pragma unroll
    for (int u = 0; u < TM_SUB; ++u) {               // program order = row order
      const int ur = ONE ? u : u / nch, q = (u - ur * nch) * 64 + lane;
      const int t = rs + ur;
      const bool there = ur < R && t < len && q < k;
      const int j = raw[u];
      if (there && timing_active(vb[u], threshold) && j >= seg0 && j < seg1) {
        const int i = j - seg0;
        const uint32_t w = fl[i];
        uint32_t first = w & 0xFFFFu, c = cnt[i];
        const uint32_t last = w >> 16;
        if (first == TM_NONE) {
          first = (uint32_t)t;
          c = 0;
        } else if (t - (int)last - 1 > bridge) {
          timing_topk_close(run_hist, totals, j, nb, sub_bits, first, last, c, first == 0);
          hist_add(gap_hist + (int64_t)j * nb + (timing_index((uint32_t)t - last - 1, sub_bits) - 1), 1u);
          first = (uint32_t)t;
          c = 0;
        }
        fl[i] = first | ((uint32_t)t << 16);
        cnt[i] = (unsigned short)(c + 1);
      }
      // the table updates of this unit are issued before the reads of the next one (another row may hold the same latent)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
  __syncthreads();
  for (int i = lane; i < segn; i += 64) {
    const uint32_t w = fl[i];
    if ((w & 0xFFFFu) == TM_NONE) continue;
    const uint32_t first = w & 0xFFFFu, last = w >> 16;
    timing_topk_close(run_hist, totals, seg0 + i, nb, sub_bits, first, last, cnt[i], first == 0 || (int)last == len - 1);
    hist_add(totals + (int64_t)(seg0 + i) * TB_NTOTALS + TB_FILES, 1u);
  }
}
