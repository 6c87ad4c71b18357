// Pursuit frontier (include/freud_sae.h, sae_pursuit_files): non-negative matching pursuit of every counted frame on the decoder
// directions -- the decoder's own error at every budget s = 0 .. K, without the trained encoder.  Per frame
//   r_0 = float(x) - b;   step s: rho = bf16(r_s), sc_j = fp32_acc(rho . w_j) * z_j (the bf16 MFMA product: it only CHOOSES),
//   j* = argmax_j sc_j (ties to the lower j), stop if sc_j* <= 0; a = fp32 dot(r_s, w_j*) / q_j*, stop if not (a > 0);
//   r_{s+1} = fmaf(-a, w_j*, r_s);   e_s = |r_s|^2, held after the stop,
// with w_j the bf16 operand row the frontier uses, q_j = |w_j|^2 and z_j = 1 / sqrt(q_j) in fp32 (q_j == 0: z_j = 0, never chosen).
//
// The first part is free of any HIP type and compiles for the host (tests/test_pursuit_cpu.py): the pick key, the stop predicates,
// the fixed orders of the fp32 sums and a serial reference of the whole rule.  The fixed orders, the same in the kernels:
//   * a LANE owns the C = d_p / 64 contiguous columns from lane * C (frontier.h's layout); its share of a norm or a dot product is
//     the fmaf chain over those columns in column order, starting from 0;
//   * the 64 shares are joined by the xor butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits: an fp32 addition is
//     commutative), as dict_match.h joins its partials.
// Nothing in that order depends on K, the batch, the grid or the row's neighbours.
//
// The pick key is sk_ord(score) << 32 | ~column: a plain unsigned 64-bit max is "largest score, then lower column"; -0.0 is +0.0;
// the key 0 means "not eligible" and no finite score maps to it.
//
// The kernels.  pursuit_const_kernel: q and z, one wave per operand row.  pursuit_init_kernel: r_0 in fp32 and its bf16 image
// [M_p][d_p] (zero in the padding rows and columns), e_0, the row's state, and the whole trace of an uncounted row.  One step is a
// launch pair:
//   * the row x row bf16 GEMM of the tile forms (gemm.h, gemm256.h through launch_gemm; A = rho, B = the operand rows) with the
//     epilogue EpiPursuit: the accumulator times z[col] becomes a key, a thread keeps one running key for each of its 16 rows of the
//     128 x 128 sub-tile (apply_it: registers), tile_end folds the 32 threads that share a row through the tile's LDS scratch and
//     thread t < 128 emits ONE key per (row, 128-column sub-tile) with an unsigned 64-bit atomicMax on rowkey[row], as search.h
//     does -- CHOSEN over plain stores into [column tiles][M] plus a fold: n_p / 128 keys per row and step would be written and
//     read again (192 x 8 bytes per row at n = 24 576), the atomic is an integer max (order-free: two runs give the same bytes),
//     and the step kernel that consumes the key resets it.  Nothing of size M x n is ever written.  A score's sum over K does not
//     depend on the tile it is computed in (dict_match.h), so the pick does not depend on the tile edge or the batch.
//   * pursuit_step_kernel: one wave per row, the fp32 residual in registers (frontier.h's with_np forms for d_p).  It decodes the
//     key, applies both stop tests, gathers w_j*, forms a, updates r, writes r, bf16(r), e_{s+1} and the trace, adds PICKS and
//     IN_SUPPORT (integer atomics) and resets rowkey.
// pursuit_finish_kernel turns the rows' e_s into the frontier's partial layout (part / rowinfo / bud of frontier.h) and adds the
// STEPS histogram, so that frontier_dim_kernel and frontier_fold_kernel fold the batch into the caller's block unchanged.  No
// float atomics anywhere.
//
// Measured (tools/bench_pursuit.py, MI355X, 16 files of 1500 frames = 24 000 rows of N(0, 1), K = 64; per step from the engine's brackets):
//   TopK d = 768, n = 24 576   the GEMM with EpiPursuit 1.01 ms per step, the step kernel 0.11 ms, the call 74.4 ms; the context's own
//                              encoder GEMM (which stores its rows x n product) 0.80 ms streaming / 0.87 ms in the tile form; the torch
//                              route (r @ W^T, arg-max, gather, update, K times) 177.9 ms
//   L1   d = 384, n = 12 288   the GEMM 0.37 ms per step, the step kernel 0.15 ms, the call 34.1 ms; encoder GEMM 0.29 ms; torch 86.9 ms
// The epilogue costs 13 % / 27 % over the tile GEMM with plain bf16 stores; whether that is the two-pass fp32 epilogue with the LDS
// fold or the 192 / 96 atomics per row and step is not separated yet.  Not tuned.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dict_match.h"          // dm_bf16_bits / dm_bf16_float (and search_keys.h)
#include "frontier.h"            // fr_add, fr_mul, fr_lane_sq, fr_budget, FR_MAX_*

#define PU_MAX_K FR_MAX_K        // include/freud_sae.h: SAE_PURSUIT_MAX_K
#define PU_MAX_TAU FR_MAX_TAU    // include/freud_sae.h: SAE_PURSUIT_MAX_TAU

// ---- the pick key
FR_HD uint64_t pu_key(float score, uint32_t col) { return ((uint64_t)sk_ord(score) << 32) | (uint64_t)(~col); }
FR_HD float pu_key_score(uint64_t k) { return sk_unord((uint32_t)(k >> 32)); }
FR_HD uint32_t pu_key_col(uint64_t k) { return ~(uint32_t)k; }
// a column's key in a dictionary of n directions: padding columns and directions of norm 0 are never eligible
FR_HD uint64_t pu_col_key(float acc, float z, uint32_t col, uint32_t n) { return (col < n && z > 0.f) ? pu_key(fr_mul(acc, z), col) : 0ull; }

// ---- the stop predicates: the row stops on a key that is not eligible or whose score is <= 0, and on a coefficient that is not > 0
FR_HD bool pu_stops_on_key(uint64_t k) { return k == 0ull || !(pu_key_score(k) > 0.f); }
FR_HD bool pu_stops_on_coef(float a) { return !(a > 0.f); }

// ---- the fixed orders
FR_HD float pu_lane_dot(const float* r, const float* w, int C) {
  float p = 0.f;
  for (int i = 0; i < C; ++i) p = fmaf(r[i], w[i], p);
  return p;
}
// the 64 lane shares by the xor butterfly (q is overwritten)
FR_HD float pu_wave_sum(float* q) {
  for (int o = 32; o > 0; o >>= 1) {
    float t[64];
    for (int l = 0; l < 64; ++l) t[l] = fr_add(q[l], q[l ^ o]);
    for (int l = 0; l < 64; ++l) q[l] = t[l];
  }
  return q[0];
}
FR_HD float pu_norm_sq(const float* r, int d_p) {
  const int C = d_p / 64;
  float q[64];
  for (int l = 0; l < 64; ++l) q[l] = fr_lane_sq(r + l * C, C);
  return pu_wave_sum(q);
}
FR_HD float pu_dot(const float* r, const float* w, int d_p) {
  const int C = d_p / 64;
  float q[64];
  for (int l = 0; l < 64; ++l) q[l] = pu_lane_dot(r + l * C, w + l * C, C);
  return pu_wave_sum(q);
}
// the constants of one direction
FR_HD float pu_z_of(float q) {
#if defined(__HIP_DEVICE_COMPILE__)
  return q > 0.f ? __fdiv_rn(1.f, __fsqrt_rn(q)) : 0.f;
#else
  volatile float s = sqrtf(q);
  volatile float z = 1.f / s;
  return q > 0.f ? z : 0.f;
#endif
}
FR_HD float pu_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  volatile float p = a / b;
  return p;
#endif
}

// Serial reference of one row.  W [n][d_p]: the operand rows (bf16 values as fp32, zero in the padding columns); qz [2][n]: q then
// z (pu_consts_serial); x [d_p], b [d_p] (or null: 0), zero in the padding columns; d_p a multiple of 128, d_p <= FR_MAX_D.  The
// selection product is accumulated in column order with one fmaf per column (the MFMA's own order differs: the product only chooses,
// and the tests bound the difference).  -> idx [K] (-1 after the stop), val [K] (+0.0 after the stop), e [K + 1], budgets [n_tau];
// returns the number of picks.  Host only.
FR_H void pu_consts_serial(const float* W, int n, int d_p, float* qz) {
  for (int j = 0; j < n; ++j) {
    qz[j] = pu_norm_sq(W + (int64_t)j * d_p, d_p);
    qz[n + j] = pu_z_of(qz[j]);
  }
}
FR_H int pu_row_serial(int K, const float* W, int n, const float* qz, const float* x, const float* b, int d_p, const float* taus, int n_tau,
                       int* idx, float* val, float* e, int* budgets) {
  float r[FR_MAX_D], rho[FR_MAX_D];
  for (int i = 0; i < d_p; ++i) r[i] = fr_add(x[i], b ? -b[i] : -0.f);
  e[0] = pu_norm_sq(r, d_p);
  int steps = 0;
  bool live = true;
  for (int s = 0; s < K; ++s) {
    idx[s] = -1;
    val[s] = 0.f;
    e[s + 1] = e[s];
    if (!live) continue;
    for (int i = 0; i < d_p; ++i) rho[i] = dm_bf16_float(dm_bf16_bits(r[i]));
    uint64_t best = 0;
    for (int j = 0; j < n; ++j) {
      float acc = 0.f;
      const float* w = W + (int64_t)j * d_p;
      for (int i = 0; i < d_p; ++i) acc = fmaf(rho[i], w[i], acc);
      const uint64_t k = pu_col_key(acc, qz[n + j], (uint32_t)j, (uint32_t)n);
      if (k > best) best = k;
    }
    if (pu_stops_on_key(best)) { live = false; continue; }
    const int j = (int)pu_key_col(best);
    const float* w = W + (int64_t)j * d_p;
    const float a = pu_div(pu_dot(r, w, d_p), qz[j]);
    if (pu_stops_on_coef(a)) { live = false; continue; }
    for (int i = 0; i < d_p; ++i) r[i] = fmaf(-a, w[i], r[i]);
    idx[s] = j;
    val[s] = a;
    e[s + 1] = pu_norm_sq(r, d_p);
    ++steps;
  }
  for (int t = 0; t < n_tau; ++t) budgets[t] = fr_budget(e, K, taus[t]);
  return steps;
}

#if defined(__HIPCC__)
#include "common.h"
#include "gemm.h"

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
constexpr uint32_t PU_LIVE = 0x80000000u;     // rowstate: the row still picks; PU_COUNTED: it counts; the low bits: its picks so far
constexpr uint32_t PU_COUNTED = 0x40000000u;
constexpr uint32_t PU_STEPS_MASK = 0x0000FFFFu;

__device__ __forceinline__ float pu_wave_sum_dev(float p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p = __fadd_rn(p, __shfl_xor(p, o, 64));
  return p;
}

// ---- q and z: one wave per operand row, 4 per workgroup; grid n_p / 4.  Rows from n on get q = z = 0.
__global__ __launch_bounds__(256) void pursuit_const_kernel(const bf16_t* __restrict__ W, int n, int n_p, int d_p, float* __restrict__ q,
                                                            float* __restrict__ z) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n_p) return;
  const int C = d_p >> 6;
  float p = 0.f;
  if (j < n) {
    const unsigned short* w = reinterpret_cast<const unsigned short*>(W) + (int64_t)j * d_p + lane * C;
    for (int i = 0; i < C; ++i) {
      const float v = __uint_as_float((unsigned)w[i] << 16);
      p = fmaf(v, v, p);
    }
  }
  p = pu_wave_sum_dev(p);
  if (lane == 0) {
    q[j] = p;
    z[j] = pu_z_of(p);
  }
}

struct PuTrace {                // the optional trace of a call (all three or none)
  int* idx;                     // [M][K]
  float* val;                   // [M][K]
};

// ---- r_0, its bf16 image, e_0 and the row's state: one wave per row of the padded batch, 4 per workgroup; grid M_p / 4.
//   r32 [M_p][d_p], rho [M_p][d_p], err [M][K + 1], rowstate [M], rowkey [M_p]
template <typename T>
__global__ __launch_bounds__(256) void pursuit_init_kernel(const T* __restrict__ x, const float* __restrict__ b, int64_t M, int64_t M_p, int Trows,
                                                           float inv_T, const int* __restrict__ lengths, int d, int d_p, int K,
                                                           float* __restrict__ r32, unsigned short* __restrict__ rho, float* __restrict__ err,
                                                           uint32_t* __restrict__ rowstate, unsigned long long* __restrict__ rowkey, PuTrace tr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);                // (wave-uniform)
  if (row >= M_p) return;
  const int C = d_p >> 6, c0 = lane * C;
  const bool counted = recon_row_counts(row, M, Trows, inv_T, lengths);
  float p = 0.f;
  for (int i = 0; i < C; ++i) {
    const int col = c0 + i;
    const float r = (counted && col < d) ? __fsub_rn(load_as_float(x + row * d + col), b ? b[col] : 0.f) : 0.f;
    r32[row * d_p + col] = r;
    rho[row * d_p + col] = dm_bf16_bits(r);
    p = fmaf(r, r, p);
  }
  p = pu_wave_sum_dev(p);
  if (lane == 0) rowkey[row] = 0ull;
  if (row >= M) return;
  if (lane == 0) rowstate[row] = counted ? (PU_LIVE | PU_COUNTED) : 0u;
  if (counted) {
    if (lane == 0) err[row * (K + 1)] = p;
  } else {
    // an uncounted row: its whole trace now, no step touches it
    for (int s = lane; s <= K; s += 64) err[row * (K + 1) + s] = 0.f;
    if (tr.idx)
      for (int s = lane; s < K; s += 64) {
        tr.idx[row * K + s] = -1;
        tr.val[row * K + s] = 0.f;
      }
  }
}

// ---- the row arg-max epilogue of the tile GEMMs (gemm.h's interface; gemm256.h serves 128 x 128 sub-tiles through the same calls).
// Thread t of a 256-thread group owns the columns 4 (t % 32) .. + 3 of the rows t / 32 + 8 it, it < 16.
struct EpiPursuit {
  const float* z;                       // [n_p]
  unsigned long long* rowkey;           // [M_p]
  int64_t M;
  int n;
  uint32_t khi[16], klo[16];            // the running key of row `it`: ord(score), ~column
  int row0_;
  __device__ void tile_begin(int row0, int, int) { row0_ = row0; }
  struct Pre { f32x4 z; };
  __device__ Pre prefetch(int, int col) const { return Pre{*reinterpret_cast<const f32x4*>(z + col)}; }
  __device__ void apply_it(int it, int, int col, f32x4 v, const Pre& pf) {
    uint64_t best = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t k = pu_col_key(v[j], pf.z[j], (uint32_t)(col + j), (uint32_t)n);
      best = k > best ? k : best;
    }
    khi[it] = (uint32_t)(best >> 32);
    klo[it] = (uint32_t)best;
  }
  // scratch: the 128 x 132-float LDS tile of this 256-thread group, free once the apply loop has read it.  Rows of 33 keys (264
  // bytes): the 32 keys of a row, read back by thread t < 128 for row t.
  __device__ void tile_end(float* scratch) {
    constexpr int PITCH = 33;
    unsigned long long* sc = reinterpret_cast<unsigned long long*>(scratch);
    const int t = threadIdx.x & 255;
#pragma unroll
    for (int it = 0; it < 16; ++it) sc[((t >> 5) + 8 * it) * PITCH + (t & 31)] = ((unsigned long long)khi[it] << 32) | klo[it];
    lds_barrier();
    if (t < 128) {
      const unsigned long long* r = sc + t * PITCH;
      unsigned long long best = 0;
#pragma unroll
      for (int q = 0; q < 32; ++q) best = r[q] > best ? r[q] : best;
      const int64_t row = (int64_t)row0_ + t;
      if (row < M && best != 0ull) atomicMax(rowkey + row, best);
    }
  }
};

// ---- one step of every row: one wave per row, 4 per workgroup; grid ceil(M / 4).  NPAIR > 0: d_p == 128 NPAIR at compile time.
//   lat: the L1 latent [.][lat_ld] as bf16 bits (or null: TopK -- top_idx / top_vals [.][k_sel])
struct PuSupport {
  const unsigned short* lat;
  int64_t lat_ld;
  const int* top_idx;
  const unsigned short* top_vals;
  int k_sel;
};

template <int NPAIR>
__global__ __launch_bounds__(256) void pursuit_step_kernel(int s, int K, int64_t M, int n, int d_p, const bf16_t* __restrict__ W,
                                                           const float* __restrict__ q, float* __restrict__ r32, unsigned short* __restrict__ rho,
                                                           float* __restrict__ err, uint32_t* __restrict__ rowstate,
                                                           unsigned long long* __restrict__ rowkey, PuTrace tr, PuSupport sup,
                                                           unsigned long long* __restrict__ picks, unsigned long long* __restrict__ in_support) {
  constexpr int MAXP = NPAIR > 0 ? NPAIR : FR_MAX_D / 128;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);                // (wave-uniform)
  if (row >= M) return;
  const uint32_t st = rowstate[row];
  const unsigned long long key = rowkey[row];
  if (lane == 0) rowkey[row] = 0ull;
  if (!(st & PU_COUNTED)) return;
  float* e = err + row * (K + 1);
  auto hold = [&]() {           // the stopped row: e is held, the trace says so
    if (lane == 0) {
      e[s + 1] = e[s];
      if (tr.idx) {
        tr.idx[row * K + s] = -1;
        tr.val[row * K + s] = 0.f;
      }
      if (st & PU_LIVE) rowstate[row] = st & ~PU_LIVE;
    }
  };
  if (!(st & PU_LIVE) || pu_stops_on_key(key)) return hold();
  const uint32_t j = pu_key_col(key);
  if (j >= (uint32_t)n) return hold();                   // (cannot come out of the epilogue: defensive, the gather stays inside W)
  const int npair = NPAIR > 0 ? NPAIR : d_p >> 7;
  const int c0 = lane * 2 * npair;
  const unsigned* wr = reinterpret_cast<const unsigned*>(W + (int64_t)j * d_p + c0);
  float* rr = r32 + row * d_p + c0;
  unsigned* ro = reinterpret_cast<unsigned*>(rho + row * d_p + c0);
  // one column pair of the update: the new residual into r32 and rho, its squares into the lane's share of the norm
  auto update = [&](int p, float a, unsigned u, f32x2_t v, float& sq) {
    const float r0 = fmaf(-a, __uint_as_float(u << 16), v[0]), r1 = fmaf(-a, __uint_as_float(u & 0xFFFF0000u), v[1]);
    sq = fmaf(r0, r0, sq);
    sq = fmaf(r1, r1, sq);
    *reinterpret_cast<f32x2_t*>(rr + 2 * p) = f32x2_t{r0, r1};
    ro[p] = (unsigned)dm_bf16_bits(r0) | ((unsigned)dm_bf16_bits(r1) << 16);
  };
  float dot = 0.f, sq = 0.f, a;
  if constexpr (NPAIR > 0) {    // the lane's columns of r and w_j in registers
    unsigned u[MAXP];
    f32x2_t v[MAXP];
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      u[p] = wr[p];
      v[p] = *reinterpret_cast<const f32x2_t*>(rr + 2 * p);
    }
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      dot = fmaf(v[p][0], __uint_as_float(u[p] << 16), dot);
      dot = fmaf(v[p][1], __uint_as_float(u[p] & 0xFFFF0000u), dot);
    }
    a = __fdiv_rn(pu_wave_sum_dev(dot), q[j]);
    if (pu_stops_on_coef(a)) return hold();
#pragma unroll
    for (int p = 0; p < MAXP; ++p) update(p, a, u[p], v[p], sq);
  } else {                      // any d_p: two sweeps over the lane's columns (the second one hits the cache), no register array
    for (int p = 0; p < npair; ++p) {
      const unsigned u = wr[p];
      const f32x2_t v = *reinterpret_cast<const f32x2_t*>(rr + 2 * p);
      dot = fmaf(v[0], __uint_as_float(u << 16), dot);
      dot = fmaf(v[1], __uint_as_float(u & 0xFFFF0000u), dot);
    }
    a = __fdiv_rn(pu_wave_sum_dev(dot), q[j]);
    if (pu_stops_on_coef(a)) return hold();
    for (int p = 0; p < npair; ++p) update(p, a, wr[p], *reinterpret_cast<const f32x2_t*>(rr + 2 * p), sq);
  }
  sq = pu_wave_sum_dev(sq);
  // the encoder's own active set of the row: the stored L1 latent is > 0, or the latent is among top_idx with a positive value
  bool in = false;
  if (sup.lat) {
    in = (short)sup.lat[row * sup.lat_ld + j] > 0;
  } else {
    for (int t0 = 0; t0 < sup.k_sel; t0 += 64) {
      const int t = t0 + lane;
      const bool hit = t < sup.k_sel && sup.top_idx[row * sup.k_sel + t] == (int)j && (short)sup.top_vals[row * sup.k_sel + t] > 0;
      in = in || __ballot(hit) != 0ull;
    }
  }
  if (lane == 0) {
    e[s + 1] = sq;
    if (tr.idx) {
      tr.idx[row * K + s] = (int)j;
      tr.val[row * K + s] = a;
    }
    rowstate[row] = st + 1u;
    atomicAdd(picks + j, 1ull);
    if (in) atomicAdd(in_support + s, 1ull);
  }
}

// ---- the rows' norms into the frontier's partial layout (frontier.h: part / rowinfo / bud), and the STEPS histogram.  One workgroup
// per FR_UNIT rows: thread m adds e_m of the unit's counted rows in row order; thread i < FR_UNIT takes row i's budgets.
__global__ __launch_bounds__(256) void pursuit_finish_kernel(const float* __restrict__ err, const uint32_t* __restrict__ rowstate, int64_t M, int K,
                                                             FrTau tau, float* __restrict__ part, uint32_t* __restrict__ rowinfo,
                                                             unsigned short* __restrict__ bud, unsigned long long* __restrict__ steps) {
  const int64_t row0 = (int64_t)blockIdx.x * FR_UNIT;
  const int tid = threadIdx.x;
  for (int m = tid; m <= K; m += 256) {
    float sum = 0.f;
    for (int i = 0; i < FR_UNIT; ++i) {
      const int64_t row = row0 + i;
      if (row < M && (rowstate[row] & PU_COUNTED)) sum = __fadd_rn(sum, err[row * (K + 1) + m]);
    }
    part[(int64_t)blockIdx.x * FR_PART_LD + m] = sum;
  }
  const int64_t row = row0 + tid;
  if (tid < FR_UNIT && row < M) {
    const uint32_t st = rowstate[row];
    if (!fr_row_finish((st & PU_COUNTED) != 0, row, err + row * (K + 1), K, tau, rowinfo, bud)) return;
    const uint32_t ns = st & PU_STEPS_MASK;
    atomicAdd(steps + (ns <= (uint32_t)K ? ns : (uint32_t)K), 1ull);
  }
}
#endif
