// Duration bins and the serial reference of the feature timing (timing.h; include/freud_sae.h, sae_timing_files), free of any HIP
// type so that the SAME functions compile for the host: tests/test_feature_timing_cpu.py builds them with g++.
//
// A duration or a gap is a number of frames L >= 1.  With sub_bits = s (0..3) and P = 2^s the bins are exact on the small integers
// and logarithmic, P per octave, above them -- integer arithmetic only:
//   idx(L) = L                                   L < 2P
//          = sh P + (L >> sh), sh = floor(log2 L) - s     otherwise          bin = idx - 1
//   lower edge of idx = idx                      idx < 2P
//                     = (P + idx % P) << (idx / P - 1)    otherwise
// The two branches meet at L = 2P (sh = 1: idx = P + P), so the bins are contiguous.  NB = idx(T) bins hold every L <= T; T <= 65535
// gives NB <= 111 (s = 3).  s = 2: durations 1..7 have a bin each, then four bins per octave; T = 1500: 37 bins.
//
// Runs (the one definition, restated in include/freud_sae.h): within the counted frames of one file the active frames t1 < t2 < ...
// of a latent; neighbours a < b share a run iff b - a - 1 <= g (the bridge, 0..15); duration = last - first + 1; the gap between two
// consecutive runs of a file is b - a - 1 > g; a run is censored iff it starts on frame 0 or ends on the file's last counted frame.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TB_HD __host__ __device__ __forceinline__
#else
#define TB_HD inline
#endif

constexpr int TB_MAX_ROWS = 65535;       // rows_per_file at most: a position fits a 16-bit word beside a sentinel
constexpr int TB_MAX_BINS = 111;         // timing_index(65535, 3)
constexpr int TB_MAX_BRIDGE = 15;
constexpr uint32_t TB_MAX_THRESHOLD = 0x7F80u;   // +Inf: above it nothing finite is left to pass
enum { TB_ACTIVE = 0, TB_SPAN = 1, TB_RUNS = 2, TB_FILES = 3, TB_LONGEST = 4, TB_CENSORED = 5, TB_NTOTALS = 6 };

TB_HD bool timing_spec_ok(int sub_bits, int bridge, uint32_t threshold_bits, int64_t rows_per_file) {
  return sub_bits >= 0 && sub_bits <= 3 && bridge >= 0 && bridge <= TB_MAX_BRIDGE && threshold_bits <= TB_MAX_THRESHOLD && rows_per_file >= 1 &&
         rows_per_file <= TB_MAX_ROWS;
}

// idx of the header, L >= 1
TB_HD int timing_index(uint32_t L, int sub_bits) {
  if (L < (2u << sub_bits)) return (int)L;
  const int sh = (31 - __builtin_clz(L)) - sub_bits;
  return (sh << sub_bits) + (int)(L >> sh);
}

// the smallest L of idx (idx >= 1; idx = NB + 1: one past the last bin)
TB_HD uint32_t timing_lower_edge(int idx, int sub_bits) {
  const int P = 1 << sub_bits;
  if (idx < 2 * P) return (uint32_t)idx;
  return (uint32_t)(P + (idx & (P - 1))) << ((idx >> sub_bits) - 1);
}

TB_HD int timing_nbins(int sub_bits, int64_t rows_per_file) { return timing_index((uint32_t)rows_per_file, sub_bits); }

TB_HD bool timing_active(uint32_t bits, uint32_t threshold_bits) { return (bits & 0x7FFFu) > threshold_bits; }

// one closed run [first, last] of a file with `len` counted frames
TB_HD void timing_close_ref(int first, int last, int len, int sub_bits, int64_t* run_hist, int64_t* totals) {
  const int dur = last - first + 1;
  run_hist[timing_index((uint32_t)dur, sub_bits) - 1] += 1;
  totals[TB_SPAN] += dur;
  totals[TB_RUNS] += 1;
  totals[TB_LONGEST] = dur > totals[TB_LONGEST] ? dur : totals[TB_LONGEST];
  totals[TB_CENSORED] += (first == 0 || last == len - 1) ? 1 : 0;
}

// Serial reference of one (file, latent): mask[t * stride] != 0 marks an active frame, t < len.  Adds to run_hist / gap_hist [NB] and
// totals [TB_NTOTALS] of the latent (LONGEST: a maximum), as the kernels of timing.h do.
TB_HD void timing_file_ref(const uint8_t* mask, int64_t stride, int len, int sub_bits, int bridge, int64_t* run_hist, int64_t* gap_hist,
                           int64_t* totals) {
  int first = -1, last = -1;
  for (int t = 0; t < len; ++t) {
    if (!mask[(int64_t)t * stride]) continue;
    totals[TB_ACTIVE] += 1;
    if (first < 0) {
      first = t;
    } else if (t - last - 1 > bridge) {
      timing_close_ref(first, last, len, sub_bits, run_hist, totals);
      gap_hist[timing_index((uint32_t)(t - last - 1), sub_bits) - 1] += 1;
      first = t;
    }
    last = t;
  }
  if (first >= 0) {
    timing_close_ref(first, last, len, sub_bits, run_hist, totals);
    totals[TB_FILES] += 1;
  }
}

// the trimmed length of file f (search.h's search_len)
TB_HD int timing_len(const int* lengths, int64_t f, int T) {
  const int L = lengths ? lengths[f] : T;
  return L < 1 ? 1 : (L > T ? T : L);
}

// Serial reference of one batch: lat [n_files T][ld] bf16 bit patterns, columns < n.  Adds to run_hist / gap_hist [n][NB], totals
// [n][TB_NTOTALS] and *n_frames.  Host only (it allocates the mask column).
inline void timing_rows_ref(const uint16_t* lat, int64_t ld, int n, int64_t n_files, int T, const int* lengths, int sub_bits, int bridge,
                            uint32_t threshold_bits, int64_t* run_hist, int64_t* gap_hist, int64_t* totals, int64_t* n_frames) {
  const int nb = timing_nbins(sub_bits, T);
  uint8_t* mask = new uint8_t[T > 0 ? T : 1];
  for (int64_t f = 0; f < n_files; ++f) {
    const int len = timing_len(lengths, f, T);
    *n_frames += len;
    for (int j = 0; j < n; ++j) {
      for (int t = 0; t < len; ++t) mask[t] = timing_active(lat[(f * T + t) * ld + j], threshold_bits) ? 1 : 0;
      timing_file_ref(mask, 1, len, sub_bits, bridge, run_hist + (int64_t)j * nb, gap_hist + (int64_t)j * nb, totals + (int64_t)j * TB_NTOTALS);
    }
  }
  delete[] mask;
}
