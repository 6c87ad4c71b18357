// The arithmetic of dead-latent resampling (resample.h; include/freud_sae.h, sae_resample_*), free of any HIP type so that the SAME
// functions compile for the host: tests/test_resample_cpu.py builds them with g++ -ffp-contract=off.
//
// The rule (Bricken et al. 2023, "Towards Monosemanticity", neuron resampling; every choice that lets host and device agree to the bit):
//   dead set    latent j < n with a firing count of 0 over the counted frames, taken in ascending order r = 0 .. |D| - 1
//   row loss    l_i >= 0, fp32, one per row i = file * T + frame (0 on rows that do not count)
//   weight      l_max = the maximum (of the bit patterns: the losses are non-negative), e = its frexp exponent,
//               q_i = floor(l_i 2^(16 - e)) in [0, 65535], w_i = q_i^2 as uint64: p proportional to the loss squared
//   prefix      c_i = w_0 + .. + w_i (inclusive, uint64; rows < 2^31 cannot overflow it), total = c_last; total == 0: nothing is drawn
//   draw        h = rs_hash(seed, round, r), t = mulhi64(h, total) in [0, total), row = the first i with c_i > t
//   owner       of the latents that drew one row the lowest r owns it (an integer minimum: order-free); the others stay dead
//   column      x = the drawn row in fp32: s = fmaf-accumulated sum x_k^2 (k ascending), nrm = sqrt(s) correctly rounded, u_k = x_k / nrm,
//               b = -((1 - alpha) nrm); s == 0 or not finite: the row is degenerate and the latent stays dead
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(__HIPCC__)
#include <vector>
#endif

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

constexpr int RS_QBITS = 16;                 // q_i < 2^16: w_i < 2^32, 2^31 rows of it stay below 2^63
constexpr int64_t RS_MAX_ROWS = 0x7FFFFFFFll;
constexpr int RS_MAX_N = 1 << 24;
// counts of sae_resample_select (int64 [RS_NCOUNTS])
enum { RS_DEAD = 0, RS_PAIRS = 1, RS_SKIPPED_DUPLICATE = 2, RS_TOTAL = 3, RS_LMAX_BITS = 4, RS_NCOUNTS = 8 };

// the bit pattern a loss is ordered by: the sign is dropped (a sum of squares has none; a NaN may)
RS_HD uint32_t rs_loss_bits(uint32_t bits) { return bits & 0x7FFFFFFFu; }

// frexp exponent of the non-negative float with these bits: l = m 2^e, m in [0.5, 1); 0 for l == 0.  Subnormals included.
RS_HD int rs_frexp_exp(uint32_t bits) {
  const int E = (int)(bits >> 23);
  if (E != 0) return E - 126;
  const uint32_t mant = bits & 0x7FFFFFu;
  if (mant == 0) return 0;
  return (31 - __builtin_clz(mant)) - 148;
}

// q = floor(l 2^(RS_QBITS - e)) in integers: l = M 2^x exactly (M the significand, 24 bits), so q = M shifted by x + RS_QBITS - e.
// With l <= l_max < 2^e the result is below 2^RS_QBITS; it is clamped there all the same (an l above l_max is the caller's error).
RS_HD uint32_t rs_weight_q(uint32_t bits, int e) {
  const int E = (int)(bits >> 23);
  const uint64_t M = E != 0 ? (uint64_t)((bits & 0x7FFFFFu) | 0x800000u) : (uint64_t)(bits & 0x7FFFFFu);
  const int x = E != 0 ? E - 150 : -149;
  const int sh = x + RS_QBITS - e;
  uint64_t q;
  if (sh >= 0) q = sh > 30 ? ~(uint64_t)0 : M << sh;
  else q = -sh > 63 ? 0 : M >> -sh;
  const uint64_t cap = ((uint64_t)1 << RS_QBITS) - 1;
  return (uint32_t)(q > cap ? cap : q);
}

// the weight word of a row
RS_HD uint64_t rs_weight(uint32_t loss_bits, int e) {
  const uint64_t q = rs_weight_q(rs_loss_bits(loss_bits), e);
  return q * q;
}

// splitmix64's finaliser (with its increment), and the counter-based hash of (seed, round, r)
RS_HD uint64_t rs_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
RS_HD uint64_t rs_hash(uint64_t seed, uint64_t round, uint64_t r) { return rs_mix(rs_mix(rs_mix(seed) ^ round) ^ r); }

// the high 64 bits of a b
RS_HD uint64_t rs_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// the first i in [0, rows) with c[i] > t; c is non-decreasing and t < c[rows - 1] (else rows - 1)
RS_HD int64_t rs_search(const uint64_t* c, int64_t rows, uint64_t t) {
  int64_t lo = 0, hi = rows - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (c[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

RS_HD int64_t rs_draw(const uint64_t* c, int64_t rows, uint64_t total, uint64_t seed, uint64_t round, uint64_t r) {
  return rs_search(c, rows, rs_mulhi64(rs_hash(seed, round, r), total));
}

// ---- the column arithmetic: every operation is one correctly rounded fp32 operation, on both sides
RS_HD float rs_norm_sq(const float* x, int d) {
  float s = 0.f;
  for (int k = 0; k < d; ++k) s = fmaf(x[k], x[k], s);
  return s;
}
RS_HD bool rs_degenerate(float s) {
  const uint32_t b = __builtin_bit_cast(uint32_t, s);
  return s == 0.f || (b & 0x7F800000u) == 0x7F800000u;
}
// (sqrtf on both sides: compiled for the device it is the correctly rounded root -- hipcc's default,
// -fhip-fp32-correctly-rounded-divide-sqrt -- where this toolchain's __fsqrt_rn is the native approximation unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined)
RS_HD float rs_norm(float s) { return sqrtf(s); }
RS_HD float rs_unit(float xk, float nrm) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(xk, nrm);
#else
  return xk / nrm;
#endif
}
RS_HD float rs_bias(float alpha, float nrm) {
#if defined(__HIP_DEVICE_COMPILE__)
  return -__fmul_rn(__fsub_rn(1.0f, alpha), nrm);
#else
  const float one_minus = 1.0f - alpha;
  return -(one_minus * nrm);
#endif
}

// ---- the serial reference of the selection (host only: it allocates)
#if !defined(__HIPCC__)
// the inclusive prefix of one batch of rows, continued from `carry` (the prefix before the batch); returns the new carry
inline uint64_t rs_prefix_batch(const float* loss, int64_t rows, int e, uint64_t carry, uint64_t* c) {
  for (int64_t i = 0; i < rows; ++i) {
    carry += rs_weight(__builtin_bit_cast(uint32_t, loss[i]), e);
    c[i] = carry;
  }
  return carry;
}

inline uint32_t rs_max_bits(const float* loss, int64_t rows) {
  uint32_t m = 0;
  for (int64_t i = 0; i < rows; ++i) {
    const uint32_t b = rs_loss_bits(__builtin_bit_cast(uint32_t, loss[i]));
    m = b > m ? b : m;
  }
  return m;
}

// loss [rows], fire [n] -> the applying (latent, row) pairs in ascending latent order and counts [RS_NCOUNTS]; returns the pairs.
// batch_rows > 0: the prefix is formed in batches of that many rows (the same words: only the carry crosses a batch).
inline int64_t rs_select_ref(const float* loss, int64_t rows, const uint64_t* fire, int n, uint64_t seed, uint64_t round, int32_t* latents_out,
                             int64_t* rows_out, int64_t* counts, int64_t batch_rows = 0) {
  for (int i = 0; i < RS_NCOUNTS; ++i) counts[i] = 0;
  const uint32_t lmax = rs_max_bits(loss, rows);
  const int e = rs_frexp_exp(lmax);
  std::vector<uint64_t> c((size_t)rows);
  uint64_t total = 0;
  const int64_t step = batch_rows > 0 ? batch_rows : rows;
  for (int64_t r0 = 0; r0 < rows; r0 += step) total = rs_prefix_batch(loss + r0, (rows - r0 < step ? rows - r0 : step), e, total, c.data() + r0);
  std::vector<int32_t> dead;
  for (int j = 0; j < n; ++j)
    if (fire[j] == 0) dead.push_back(j);
  counts[RS_DEAD] = (int64_t)dead.size();
  counts[RS_TOTAL] = (int64_t)total;
  counts[RS_LMAX_BITS] = (int64_t)lmax;
  if (total == 0) return 0;
  std::vector<int64_t> draw(dead.size());
  std::vector<uint32_t> owner((size_t)rows, 0xFFFFFFFFu);
  for (size_t r = 0; r < dead.size(); ++r) {
    draw[r] = rs_draw(c.data(), rows, total, seed, round, (uint64_t)r);
    if ((uint32_t)r < owner[(size_t)draw[r]]) owner[(size_t)draw[r]] = (uint32_t)r;
  }
  int64_t np = 0;
  for (size_t r = 0; r < dead.size(); ++r) {
    if (owner[(size_t)draw[r]] == (uint32_t)r) {
      latents_out[np] = dead[r];
      rows_out[np] = draw[r];
      ++np;
    } else {
      counts[RS_SKIPPED_DUPLICATE] += 1;
    }
  }
  counts[RS_PAIRS] = np;
  return np;
}
#endif
