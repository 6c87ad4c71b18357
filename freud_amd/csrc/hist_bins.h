// Bin arithmetic of the activation histograms (hist.h; include/freud_sae.h, sae_hist_files), free of any HIP type so that the SAME
// functions compile for the host: tests/test_activation_hist_cpu.py builds them with g++.
//
// A latent value is binned on its own bf16 bit pattern, magnitude bits mag = bits & 0x7FFF.  A spec is three integers: lo_exp = L
// (>= -126), octaves = O (>= 1, L + O <= 128) and sub_bits = s (0..3): P = 2^s bins per octave, O P <= 128 of them, NB = O P + 3 bins.
//   bin 0        mag == 0: inactive (a -0.0 and a selected zero of a TopK row: the rule of stats.h)
//   bin 1        underflow, 0 < a < 2^L (every subnormal: L >= -126)
//   bin 2 + i    i = (mag >> (7 - s)) - ((L + 127) << s), 0 <= i < O P: 2^(L + i / P) (1 + (i % P) / P) <= a < the next edge
//   bin NB - 1   overflow, a >= 2^(L + O) (the Inf and NaN patterns: L + O <= 128)
// mag >> (7 - s) is the biased exponent followed by the top s mantissa bits, so every edge is a bf16 value and no comparison rounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HB_HD __host__ __device__ __forceinline__
#else
#define HB_HD inline
#endif

constexpr int HB_MAX_REGULAR = 128;                  // O P at most
constexpr int HB_MAX_BINS = HB_MAX_REGULAR + 3;

struct HistSpec { int lo_exp, octaves, sub_bits; };

HB_HD bool hist_spec_ok(HistSpec sp) {
  if (sp.sub_bits < 0 || sp.sub_bits > 3 || sp.lo_exp < -126 || sp.lo_exp > 127 || sp.octaves < 1 || sp.octaves > 254) return false;
  return sp.lo_exp + sp.octaves <= 128 && (sp.octaves << sp.sub_bits) <= HB_MAX_REGULAR;
}
HB_HD int hist_regular(HistSpec sp) { return sp.octaves << sp.sub_bits; }
HB_HD int hist_nbins(HistSpec sp) { return hist_regular(sp) + 3; }

// i of the header for mag != 0: < 0 underflow, >= O P overflow
HB_HD int hist_index(uint32_t mag, HistSpec sp) { return (int)(mag >> (7 - sp.sub_bits)) - ((sp.lo_exp + 127) << sp.sub_bits); }

HB_HD int hist_bin(uint32_t mag, HistSpec sp) {
  mag &= 0x7FFFu;
  if (mag == 0) return 0;
  const int i = hist_index(mag, sp), reg = hist_regular(sp);
  return i < 0 ? 1 : (i >= reg ? reg + 2 : 2 + i);
}

// the lower edge of bin 2 + i, 0 <= i <= O P (i = O P: the overflow bin's; +Inf when L + O = 128): the bf16 pattern with index i
HB_HD float hist_edge(int i, HistSpec sp) {
  const uint32_t u = ((uint32_t)(((sp.lo_exp + 127) << sp.sub_bits) + i) << (7 - sp.sub_bits)) << 16;
  float v;
  __builtin_memcpy(&v, &u, 4);
  return v;
}

// the trimmed length of file f (search.h's search_len)
HB_HD int hist_len(const int* lengths, int64_t f, int T) {
  const int L = lengths ? lengths[f] : T;
  return L < 1 ? 1 : (L > T ? T : L);
}

// Serial reference of one batch: lat [n_files T][ld] bf16 bit patterns, columns < n.  Adds to frame_hist / file_max_hist [n][NB] and
// to *n_frames, as the kernels of hist.h do.
HB_HD void hist_rows_ref(const uint16_t* lat, int64_t ld, int n, int64_t n_files, int T, const int* lengths, HistSpec sp, int64_t* frame_hist,
                         int64_t* file_max_hist, int64_t* n_frames) {
  const int nb = hist_nbins(sp);
  for (int64_t f = 0; f < n_files; ++f) {
    const int len = hist_len(lengths, f, T);
    *n_frames += len;
    for (int j = 0; j < n; ++j) {
      uint32_t mx = 0;
      for (int r = 0; r < len; ++r) {
        const uint32_t mag = lat[(f * T + r) * ld + j] & 0x7FFFu;
        frame_hist[(int64_t)j * nb + hist_bin(mag, sp)] += 1;
        mx = mag > mx ? mag : mx;
      }
      file_max_hist[(int64_t)j * nb + hist_bin(mx, sp)] += 1;
    }
  }
}
