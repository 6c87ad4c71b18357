// File features (the reference's `top_activations_for_audio`, utils/activations.py:135-209, for every file of a batch at once): the
// top-N latents of each file, selected from the per-(file, latent) keys that the feature search leaves (search_keys.h:
// ord(value) << 32 | (0xFFFFFFFF - frame), the maximum of the file's trimmed series and its first frame).
//
// Order of a file's answer: key descending -- value descending, then the earlier first frame, which is what the reference's stable
// sort over frames in order gives -- and for equal keys the lower latent index (this project's rule: the reference leaves that case
// to torch.topk's order within a frame).  With FT_POSITIVE only latents whose value is > 0 are reported (SAE latents: the
// reference pads a short answer with zero-valued latents that torch.topk picks among ties; they carry no information).  A key of
// 0 is no real value's key and is never reported.
//
// The first part is free of any HIP type and compiles for the host as search_keys.h does (tests/test_file_features_cpu.py replays
// the reference's own answers through ft_select_serial); the kernel below uses the same predicates.
#pragma once
#include "search_keys.h"

enum { FT_POSITIVE = 1 };        // include/freud_sae.h: SAE_FILE_TOP_POSITIVE
#define FT_MAX_TOP 1024          // include/freud_sae.h: SAE_FILE_TOP_MAX
#define FT_MAX_COLS (1 << 24)    // a latent index takes three radix digits

SK_HD bool ft_eligible(uint64_t key, int flags) {
  if (key == 0) return false;
  // ord(v) > ord(0): v > 0; -0.0 shares +0.0's code (sk_ord), so it is not positive
  return !(flags & FT_POSITIVE) || (uint32_t)(key >> 32) > 0x80000000u;
}

// (key a, latent la) comes before (key b, latent lb) in a file's answer
SK_HD bool ft_before(uint64_t ka, int32_t la, uint64_t kb, int32_t lb) { return ka > kb || (ka == kb && la < lb); }

// Serial reference select of one file: keys[ncols] -> lat[n_top] (-1 = empty), out[n_top] (0 = empty), best first.
SK_HD void ft_select_serial(const uint64_t* keys, int64_t ncols, int n_top, int flags, int32_t* lat, uint64_t* out) {
  for (int i = 0; i < n_top; ++i) { lat[i] = -1; out[i] = 0; }
  int m = 0;
  for (int64_t j = 0; j < ncols; ++j) {
    const uint64_t k = keys[j];
    if (!ft_eligible(k, flags)) continue;
    if (m == n_top && !ft_before(k, (int32_t)j, out[m - 1], lat[m - 1])) continue;
    int i = m < n_top ? m : n_top - 1;
    while (i > 0 && ft_before(k, (int32_t)j, out[i - 1], lat[i - 1])) { out[i] = out[i - 1]; lat[i] = lat[i - 1]; --i; }
    out[i] = k;
    lat[i] = (int32_t)j;
    if (m < n_top) ++m;
  }
}

#if defined(__HIPCC__)
// One workgroup per file.  An entry is the 88-bit number (key, 0xFFFFFF - latent): larger is better, and no two entries of a file
// are equal.  An exact radix select walks it from the top byte: per digit a 256-bin LDS histogram of the entries that match the
// digits decided so far, then the bin in which the count from the top reaches what is still needed.  It stops as soon as that bin
// is needed whole (at the latest at the last digit, where a bin holds one entry): then exactly the entries >= the decided prefix
// are the answer.  They are compacted into LDS -- in the arrival order of an LDS counter, which the bitonic sort that follows makes
// irrelevant: the set is exact and its order total, so two runs give the same bytes.  Histogram counts are order-free.
#define FT_THREADS 1024
#define FT_DIGITS 11

__device__ __forceinline__ uint32_t ft_digit(uint64_t key, uint32_t inv, int p) {
  return p < 8 ? (uint32_t)(key >> (56 - 8 * p)) & 0xFFu : (inv >> (16 - 8 * (p - 8))) & 0xFFu;
}

__global__ __launch_bounds__(FT_THREADS) void file_top_kernel(const uint64_t* __restrict__ fk, int64_t ncols, int n_top, int flags,
                                                              int32_t* __restrict__ top_lat, uint64_t* __restrict__ top_keys) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sel_key[FT_MAX_TOP];
  __shared__ int32_t sel_lat[FT_MAX_TOP];
  __shared__ uint32_t s_bin, s_run, s_cnt, s_total, s_nsel;
  const int tid = threadIdx.x;
  const uint64_t* keys = fk + (int64_t)blockIdx.x * ncols;
  uint64_t thr_key = 0, kmask = 0;       // the decided digits of the threshold entry and their mask
  uint32_t thr_inv = 0, imask = 0;
  uint32_t need = (uint32_t)n_top;       // entries still to take among those that match the decided digits
  if (tid == 0) s_nsel = 0;

  for (int p = 0; p < FT_DIGITS; ++p) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    // a thread adds runs of equal digits at once: a file of equal keys costs it one LDS atomic, not one per key
    uint32_t run_bin = 0, run_cnt = 0;
    for (int64_t base = tid; base < ncols; base += 4 * FT_THREADS) {
      uint64_t k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = base + (int64_t)u * FT_THREADS;
        k[u] = j < ncols ? keys[j] : 0;                       // (0 is never eligible)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t inv = 0xFFFFFFu - (uint32_t)(base + (int64_t)u * FT_THREADS);
        if (ft_eligible(k[u], flags) && ((k[u] ^ thr_key) & kmask) == 0 && ((inv ^ thr_inv) & imask) == 0) {
          const uint32_t b = ft_digit(k[u], inv, p);
          if (b != run_bin && run_cnt) { atomicAdd(&hist[run_bin], run_cnt); run_cnt = 0; }
          run_bin = b;
          ++run_cnt;
        }
      }
    }
    if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
    __syncthreads();
    if (tid < 64) {
      // lane l owns the bins 255 - 4 l ... 252 - 4 l; an inclusive scan over the lanes counts from the top bin down
      uint32_t c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; s += c[j]; }
      uint32_t incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (tid >= o) incl += t;
      }
      if (tid == 63) s_total = incl;
      uint32_t run = incl - s;
      if (run < need && need <= incl) {
        bool done = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!done && run + c[j] >= need) { s_bin = 255 - 4 * tid - j; s_run = run; s_cnt = c[j]; done = true; }
          if (!done) run += c[j];
        }
      }
    }
    __syncthreads();
    if (p == 0 && s_total <= need) break;                     // fewer eligible entries than slots: all of them (no digit decided)
    const uint32_t bin = s_bin, cnt = s_cnt;
    need -= s_run;
    if (p < 8) {
      thr_key |= (uint64_t)bin << (56 - 8 * p);
      kmask |= (uint64_t)0xFF << (56 - 8 * p);
    } else {
      thr_inv |= bin << (16 - 8 * (p - 8));
      imask |= 0xFFu << (16 - 8 * (p - 8));
    }
    if (cnt == need) break;                                   // the threshold bin is taken whole
  }

  // compaction of the entries >= the decided prefix (at most n_top of them)
  for (int64_t base = tid; base < ncols; base += 4 * FT_THREADS) {
    uint64_t k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = base + (int64_t)u * FT_THREADS;
      k[u] = j < ncols ? keys[j] : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = base + (int64_t)u * FT_THREADS;
      const uint32_t inv = 0xFFFFFFu - (uint32_t)j;
      const uint64_t km = k[u] & kmask;
      if (ft_eligible(k[u], flags) && (km > thr_key || (km == thr_key && (inv & imask) >= thr_inv))) {
        const uint32_t slot = atomicAdd(&s_nsel, 1u);
        if (slot < FT_MAX_TOP) { sel_key[slot] = k[u]; sel_lat[slot] = (int32_t)j; }
      }
    }
  }
  __syncthreads();
  const int nsel = s_nsel < (uint32_t)n_top ? (int)s_nsel : n_top;
  int P = 1;
  while (P < nsel) P <<= 1;
  if (tid >= nsel && tid < P) { sel_key[tid] = 0; sel_lat[tid] = 0x7FFFFFFF; }     // padding sorts last
  __syncthreads();
  // bitonic sort of the P entries by ft_before
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int o = tid ^ j;
      if (tid < P && o > tid) {
        const uint64_t ka = sel_key[tid], kb = sel_key[o];
        const int32_t la = sel_lat[tid], lb = sel_lat[o];
        const bool up = (tid & k) == 0;
        if (up ? ft_before(kb, lb, ka, la) : ft_before(ka, la, kb, lb)) {
          sel_key[tid] = kb; sel_lat[tid] = lb;
          sel_key[o] = ka; sel_lat[o] = la;
        }
      }
      __syncthreads();
    }
  }
  if (tid < n_top) {
    const int64_t o = (int64_t)blockIdx.x * n_top + tid;
    top_keys[o] = tid < nsel ? sel_key[tid] : 0;
    top_lat[o] = tid < nsel ? sel_lat[tid] : -1;
  }
}
#endif
