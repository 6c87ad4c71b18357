// Refit frontier (include/freud_sae.h, sae_refit_files): the part of the rule that is free of any HIP type and compiles for the host
// (tests/test_refit_cpu.py) -- the dependence predicate, the shrinkage-ratio bin and the progressive Cholesky of one frame written
// serially.  refit.h runs the same chains, in the same order, one wave per frame.
//
// The frame's support has K slots in slot order; G [K][K] is the Gram matrix of their operand rows, c [K] the projections of r_0 on
// them, e_0 = |r_0|^2.  Every chain below runs over the KEPT slots u in ascending order (a slot is kept iff it is active and not
// dependent):
//   piv_s   = G[s][s], then fmaf(-L[s][u], L[s][u], .) over kept u < s
//   DEPENDENT iff piv_s <= 2^-10 * G[s][s] (one fp32 product, one compare; G[s][s] == 0 is dependent);  otherwise d_s = sqrt(piv_s)
//   L[s][t] = (G[s][t], then fmaf(-L[s][u], L[t][u], .) over kept u < t) / d_t            for kept t < s
//   y_s     = (c[s], then fmaf(-L[s][u], y_u, .) over kept u < s) / d_s
//   e_{s+1} = fmaxf(fmaf(-y_s, y_s, e_s), 0);   an empty, inactive or dependent slot has e_{s+1} = e_s
//   a_s     = (y_s, then fmaf(-L[u][s], a_u, .) over kept u > s, DESCENDING) / d_s;   every other slot has a_s = +0.0
// Square root and division are correctly rounded.  rf_row_serial is the left-looking form; the kernel's right-looking form (column u
// is applied to every later row as soon as it is final) gives every element the same chain in the same order, hence the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frontier.h"            // FR_HD / FR_H, fr_mul, fr_add, fr_lane_sq, fr_wave_sum, fr_budget, FR_MAX_*

#define RF_MAX_K 128             // include/freud_sae.h: SAE_REFIT_MAX_K
#define RF_MAX_TAU FR_MAX_TAU    // include/freud_sae.h: SAE_REFIT_MAX_TAU
#define RF_RATIO_BINS 36         // include/freud_sae.h: SAE_REFIT_RATIO_BINS
#define RF_DEP_THRESHOLD 0x1p-10f

// (device: sqrtf, which the compiler expands to v_sqrt_f32 plus the neighbour test that makes it correctly rounded; __fsqrt_rn
// compiles to the bare 1-ulp v_sqrt_f32 here and differs from the host in the last bit)
FR_HD float rf_sqrt(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrtf(a);
#else
  volatile float s = sqrtf(a);
  return s;
#endif
}
FR_HD float rf_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  volatile float p = a / b;
  return p;
#endif
}

// the dependence predicate: piv is the slot's pivot after the kept slots before it, g its own G[s][s]
FR_HD bool rf_dependent(float piv, float g) { return piv <= fr_mul(RF_DEP_THRESHOLD, g); }

// one step of the curve
FR_HD float rf_err_step(float e, float y) { return fmaxf(fmaf(-y, y, e), 0.f); }

// The bin of a shrinkage ratio a_s / v_s, on its fp32 bit pattern (the style of hist_bins.h: every edge is a bit pattern, no
// comparison rounds):  0 negative | 1 zero (either sign) | 2 below 2^-4 | 3 + i, i < 32: the eight octaves [2^-4, 2^4) in four
// sub-bins each, lower edge 2^(-4 + i / 4) (1 + (i % 4) / 4) | 35 at or above 2^4 (Inf and NaN patterns included)
FR_HD int rf_ratio_bin(float ratio) {
  uint32_t u;
  __builtin_memcpy(&u, &ratio, 4);
  const uint32_t mag = u & 0x7FFFFFFFu;
  if (mag == 0) return 1;
  if (u >> 31) return 0;
  const int i = (int)(mag >> 21) - ((127 - 4) << 2);
  return i < 0 ? 2 : (i >= 32 ? 35 : 3 + i);
}
// the lower edge of bin 3 + i, 0 <= i <= 32
FR_HD float rf_ratio_edge(int i) {
  const uint32_t u = (uint32_t)(((127 - 4) << 2) + i) << 21;
  float v;
  __builtin_memcpy(&v, &u, 4);
  return v;
}

// Serial reference of one frame's factorisation.  G [K][ldg] (the lower triangle and the diagonal are read), c [K], e0, active [K]
// (0: an empty or inactive slot); L: work space [K][K].  -> y [K] (0 on a slot that is not kept), d [K] (the pivots' roots, 0 on a
// slot that is not kept), e [K + 1], dep [K] (1: active and dependent), a [K]; returns the number of kept slots.
FR_HD int rf_row_serial(int K, const float* G, int ldg, const float* c, float e0, const uint8_t* active, float* L, float* y, float* d,
                        float* e, uint8_t* dep, float* a) {
  int kept = 0;
  e[0] = e0;
  for (int s = 0; s < K; ++s) {
    dep[s] = 0;
    y[s] = 0.f;
    d[s] = 0.f;
    e[s + 1] = e[s];
    if (!active[s]) continue;
    float* Ls = L + (int64_t)s * K;
    for (int t = 0; t < s; ++t) {
      if (!(d[t] > 0.f)) continue;
      float v = G[(int64_t)s * ldg + t];
      for (int u = 0; u < t; ++u)
        if (d[u] > 0.f) v = fmaf(-Ls[u], L[(int64_t)t * K + u], v);
      Ls[t] = rf_div(v, d[t]);
    }
    const float g = G[(int64_t)s * ldg + s];
    float piv = g;
    for (int u = 0; u < s; ++u)
      if (d[u] > 0.f) piv = fmaf(-Ls[u], Ls[u], piv);
    if (rf_dependent(piv, g)) {
      dep[s] = 1;
      continue;
    }
    d[s] = rf_sqrt(piv);
    float v = c[s];
    for (int u = 0; u < s; ++u)
      if (d[u] > 0.f) v = fmaf(-Ls[u], y[u], v);
    y[s] = rf_div(v, d[s]);
    e[s + 1] = rf_err_step(e[s], y[s]);
    ++kept;
  }
  for (int s = K - 1; s >= 0; --s) {
    a[s] = 0.f;
    if (!(d[s] > 0.f)) continue;
    float v = y[s];
    for (int u = K - 1; u > s; --u)
      if (d[u] > 0.f) v = fmaf(-L[(int64_t)u * K + s], a[u], v);
    a[s] = rf_div(v, d[s]);
  }
  return kept;
}

// Serial reference of a whole frame.  w [K][d_p]: the operand row of every slot (bf16 values as fp32; the row of an inactive slot
// is not read); x [d_p], b [d_p] (or null: 0), zero in the padding columns; d_p a multiple of 128, d_p <= FR_MAX_D.  The Gram matrix
// is accumulated here in column order with one fmaf per column (the MFMA's own order differs; both lie within the Gram bound).
// -> G [K + 1][K] (row K: c), y, d, e [K + 1], dep, a, *e_final; returns the number of kept slots.  Host only.
FR_H int rf_frame_serial(int K, const float* w, const uint8_t* active, const float* x, const float* b, int d_p, float* G, float* L, float* y,
                         float* d, float* e, uint8_t* dep, float* a, float* e_final) {
  const int C = d_p / 64;
  float r[FR_MAX_D], q[64];
  for (int i = 0; i < d_p; ++i) r[i] = fr_add(x[i], b ? -b[i] : -0.f);
  for (int l = 0; l < 64; ++l) q[l] = fr_lane_sq(r + l * C, C);
  const float e0 = fr_wave_sum(q);
  for (int s = 0; s < K; ++s) {
    const float* ws = w + (int64_t)s * d_p;
    for (int t = 0; t < K; ++t) {
      float g = 0.f;
      if (active[s] && active[t]) {
        const float* wt = w + (int64_t)t * d_p;
        if (t <= s) for (int i = 0; i < d_p; ++i) g = fmaf(ws[i], wt[i], g);
        else for (int i = 0; i < d_p; ++i) g = fmaf(wt[i], ws[i], g);
      }
      G[(int64_t)s * K + t] = g;
    }
    float cs = 0.f;
    if (active[s]) {
      for (int l = 0; l < 64; ++l) {
        float p = 0.f;
        for (int i = 0; i < C; ++i) p = fmaf(r[l * C + i], ws[l * C + i], p);
        q[l] = p;
      }
      cs = fr_wave_sum(q);
    }
    G[(int64_t)K * K + s] = cs;
  }
  const int kept = rf_row_serial(K, G, K, G + (int64_t)K * K, e0, active, L, y, d, e, dep, a);
  for (int s = 0; s < K; ++s)
    if (d[s] > 0.f) {
      const float na = -a[s];
      for (int i = 0; i < d_p; ++i) r[i] = fmaf(na, w[(int64_t)s * d_p + i], r[i]);
    }
  for (int l = 0; l < 64; ++l) q[l] = fr_lane_sq(r + l * C, C);
  *e_final = fr_wave_sum(q);
  return kept;
}
