// Refit frontier (include/freud_sae.h, sae_refit_files): the least-squares code of every counted frame on the support its encoder
// chose (or on a support the caller gives), at EVERY prefix of the support's slots, from one progressive Cholesky factorisation per
// frame.  The rule and its serial form are in refit_chol.h; this header holds the kernels.
//
// refit_kernel: one wave per frame, RF_WAVES(Kp) frames per workgroup, Kp = K rounded up to the MFMA tile edge 32.  Per frame:
//   1. the frame's slots into registers (lane l keeps slots l and 64 + l); r_0 = float(x) - b in registers in the frontier's lane
//      layout (lane l owns the d_p / 64 contiguous columns from l d_p / 64); e_0 by the frontier's order.
//   2. c[s] = dot(r_0, w_{i_s}): the lane's columns of the gathered row in column order, then the 64 shares by the frontier's order
//      (each half of 32 in lane order, then half 0 + half 1) -- 32 slots at a time through the wave's transposed LDS tile [32][65],
//      as frontier_walk_kernel reduces its norms.
//   3. G = W_s W_s^T on v_mfma_f32_32x32x16_bf16: the tiles (I, J >= I) of 32 x 32, one accumulator tile each (10 at K = 128), all
//      advanced together over the d_p / 16 k-steps in ascending order -- the order of an element's sum depends on d_p alone.  Both
//      operands of a tile are row blocks of the same gathered matrix, and the instruction's A and B fragments have the same lane map
//      (lane (r, h) holds k = 8 h .. 8 h + 7 of row / column r), so lane (r, h) loads 16 bytes of row i_{32 I + r} straight from the
//      operand table and that one fragment serves as A of the tiles (I, .) and as B of the tiles (., I): nothing is staged in LDS.
//      An inactive or padding slot contributes a zero fragment (its index is replaced by 0 and masked), so its row and column of G
//      are exactly 0 and the slot is dependent by the rule.
//   4. G into the wave's LDS region, both triangles from the computed upper one, row pitch Kp + 1 dwords (odd: lanes that walk a
//      column hit distinct banks); the trace copies it out before it is overwritten.
//   5. the factorisation in place, right-looking: lane s owns row s (and 64 + s).  Column u: the pivot test, d_u, y_u and e_{u+1} are
//      wave-uniform; every lane divides its element of the column and applies it to its row's elements t = u + 1 .. s, four at a
//      time, with L[t][u] read from lane t's register (v_readlane) -- the chain of every element runs over the kept u in ascending
//      order, which is the order refit_chol.h defines.
//   6. back-substitution by columns in descending order (registers and one row read of L per column), the final residual
//      r = fmaf(-a_s, w_{i_s}, r_0 ..) over the kept slots, e_final, the per-latent counters (integer atomics) and the shrinkage
//      histogram (per workgroup in LDS, then integer atomics).
// refit_finish_kernel turns the rows' e_s into the frontier's partial layout (frontier.h: part / rowinfo / bud), so that
// frontier_dim_kernel and frontier_fold_kernel fold the batch into the caller's block unchanged; it adds the KEPT histogram and the
// per-unit sums of e_final, which refit_final_kernel folds in unit order.  No float atomics anywhere: two runs give the same bytes.
//
// LDS per frame: Kp (Kp + 1) + 3 Kp + 4 dwords (at least the 32 x 65 tile): 8.7 / 17.4 / 38.4 / 67.6 KB at Kp = 32 / 64 / 96 / 128;
// four frames per workgroup up to Kp = 64, two above.  108 / 144 / 200 / 256 VGPRs at NT = 1 .. 4, no scratch.
//
// Measured (tools/bench_refit.py, MI355X, 16 files of 1500 frames = 24 000 rows of N(0, 1), K = 64 and every slot active, medians of 3
// rounds of 3 calls, the passes interleaved in one process; the kernel alone from the engine's refit_chol bracket):
//   TopK d = 768, n = 24 576, k = K = 64   the refit kernel 3.93 ms, the collect kernels 0.23 ms, finish + dimension sums + fold 0.67 ms,
//                                          the whole call 6.76 ms beside 2.98 ms for sae_frontier_files; the torch route (gather, bmm in
//                                          bf16, cholesky_ex, two solve_triangular; no dependence rule, no histograms) 34.1 ms
//   L1   d = 384, n = 12 288, K = 64       the kernel 3.29 ms, collect 0.89 ms, fold 0.65 ms, the call 4.98 ms beside 1.59 ms; torch 31.8 ms
// Halving d_p takes 16 % off the kernel: its time is the factorisation's column loop (2016 row-update steps per frame at K = 64, each
// an LDS read, an fmaf and an LDS write, a wave-level fence per column, one wave per SIMD), not the Gram product or the gathers.
// Not tuned.
#pragma once
#include "refit_chol.h"

#if defined(__HIPCC__)
#include "common.h"
#include "recon.h"       // recon_row_counts

constexpr int RF_TILE_PITCH = 65;
constexpr int RF_TILE_FLOATS = 32 * RF_TILE_PITCH;
__host__ __device__ constexpr int rf_mat_floats(int Kp) { return Kp * (Kp + 1) < RF_TILE_FLOATS ? RF_TILE_FLOATS : Kp * (Kp + 1); }
__host__ __device__ constexpr int rf_region_floats(int Kp) { return rf_mat_floats(Kp) + 2 * Kp + Kp + 4; }   // A | g0 | cv | ev
__host__ __device__ constexpr int rf_waves(int Kp) { return Kp <= 64 ? 4 : 2; }

struct RfSupport {
  const float* vals;            // [M][K] the slots of collect.h (the default support)
  const int* idx;
  const int* given;             // [M][K] the caller's support, or null
};
struct RfTrace {                // each nullable
  float* coef;                  // [M][K]
  unsigned char* dep;           // [M][K]
  float* gram;                  // [M][K + 1][K]
};
struct RfCount {                // the caller's block (include/freud_sae.h, SAE_REFIT_*)
  unsigned long long *slots, *neg, *dep, *ratio, *bad_index;
};

// the values 0 .. 31 of a tile whose 64 lane shares lie at tile[j][lane]: lane (j, h) returns value j, in fr_wave_sum's order
__device__ __forceinline__ float rf_tile_reduce(const float* tile, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  const int j = lane & 31, h = lane >> 5;
  const float* tr = tile + j * RF_TILE_PITCH + 32 * h;
  float s = tr[0];
#pragma unroll
  for (int t = 1; t < 32; ++t) s = __fadd_rn(s, tr[t]);
  const float o = __shfl_xor(s, 32, 64);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  return h ? __fadd_rn(o, s) : __fadd_rn(s, o);
}

__device__ __forceinline__ float rf_lane_get(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// ---- the refit of every row.  Grid: ceil(M / rf_waves(32 NT)) workgroups of 64 rf_waves threads; dynamic LDS rf_waves x
// rf_region_floats(32 NT) floats.  W [n_p][d_p]: the bf16 operand rows; b: fp32 [d] or null; n: the dictionary's size.
//   err [M][K + 1], efin [M], keptn [M] (-1: the row does not count)
template <typename T, int NT>
__global__ __launch_bounds__(256) void refit_kernel(const T* __restrict__ x, const float* __restrict__ b, RfSupport sup, int K,
                                                    const bf16_t* __restrict__ W, int64_t M, int Trows, float inv_T,
                                                    const int* __restrict__ lengths, int d, int d_p, int n, float* __restrict__ err,
                                                    float* __restrict__ efin, int* __restrict__ keptn, RfTrace tr, RfCount cnt) {
  constexpr int Kp = 32 * NT, NB = NT > 2 ? 2 : 1, LDA = Kp + 1, NW = rf_waves(Kp);
  constexpr int MAXP = FR_MAX_D / 128, NTILE = NT * (NT + 1) / 2;
  extern __shared__ float rf_smem[];
  __shared__ unsigned hist[RF_RATIO_BINS];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* A = rf_smem + w * rf_region_floats(Kp);
  float* g0 = A + rf_mat_floats(Kp);
  float* cv = g0 + Kp;
  float* ev = cv + Kp;
  if (threadIdx.x < RF_RATIO_BINS) hist[threadIdx.x] = 0u;
  __syncthreads();

  const int64_t row = (int64_t)blockIdx.x * NW + w;                                // (wave-uniform)
  if (row < M && !recon_row_counts(row, M, Trows, inv_T, lengths)) {
    for (int m = lane; m <= K; m += 64) err[row * (K + 1) + m] = 0.f;
    if (lane == 0) {
      efin[row] = 0.f;
      keptn[row] = -1;
    }
    for (int s = lane; s < K; s += 64) {
      if (tr.coef) tr.coef[row * K + s] = 0.f;
      if (tr.dep) tr.dep[row * K + s] = 0;
    }
    if (tr.gram)
      for (int q = lane; q < (K + 1) * K; q += 64) tr.gram[row * (K + 1) * K + q] = 0.f;
  } else if (row < M) {
    // 1. the slots: lane l keeps slots l and 64 + l; an inactive slot keeps the index 0 and the value 0
    int si[NB];
    float sv[NB];
    unsigned long long am[NB];
    int nbad = 0;
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
      const int s = 64 * bk + lane;
      int ii = 0;
      float vv = 0.f;
      bool act = false;
      if (s < K) {
        if (sup.given) {
          ii = sup.given[row * K + s];
          act = (unsigned)ii < (unsigned)n;
          nbad += (!act && ii != -1) ? 1 : 0;
          vv = 1.f;
        } else {
          ii = sup.idx[row * K + s];
          vv = sup.vals[row * K + s];
          act = vv != 0.f && (unsigned)ii < (unsigned)n;
        }
      }
      si[bk] = act ? ii : 0;
      sv[bk] = act ? vv : 0.f;
      am[bk] = __ballot(act);
    }
    if (sup.given) {
      const unsigned long long bm0 = __ballot(nbad > 0), bm1 = __ballot(nbad > 1);
      const int tot = __popcll(bm0) + __popcll(bm1);
      if (tot && lane == 0) atomicAdd(cnt.bad_index, (unsigned long long)tot);
    }
    auto is_active = [&](int s) -> bool { return (am[NB > 1 ? (s >> 6) : 0] >> (s & 63)) & 1ull; };
    auto slot_idx = [&](int s) -> int {
      int a = __builtin_amdgcn_readlane(si[0], s & 63);
      if constexpr (NB > 1) {
        const int o = __builtin_amdgcn_readlane(si[1], s & 63);
        a = (s >> 6) ? o : a;
      }
      return a;
    };
    auto pick = [&](const float (&reg)[NB], int s) -> float {
      float a = rf_lane_get(reg[0], s & 63);
      if constexpr (NB > 1) {
        const float o = rf_lane_get(reg[1], s & 63);
        a = (s >> 6) ? o : a;
      }
      return a;
    };

    // r_0 in the frontier's lane layout, e_0 in its order
    const int npair = d_p >> 7, c0 = lane * 2 * npair;
    float r[2 * MAXP];
#pragma unroll
    for (int c = 0; c < 2 * MAXP; ++c) {
      const int col = c0 + c;
      r[c] = (c < 2 * npair && col < d) ? __fsub_rn(load_as_float(x + row * d + col), b ? b[col] : 0.f) : 0.f;
    }
    auto lane_sq = [&]() {
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < 2 * MAXP; ++c)
        if (c < 2 * npair) q = fmaf(r[c], r[c], q);
      return q;
    };
    A[lane] = lane_sq();
    float ee = rf_lane_get(rf_tile_reduce(A, lane), 0);                            // e_0, then the running e_s

    // 2. the projections, 32 slots per reduction
#pragma unroll 1
    for (int ck = 0; ck < NT; ++ck) {
#pragma unroll 1
      for (int j = 0; j < 32; ++j) {
        const int s = 32 * ck + j;
        float p = 0.f;
        if (s < K && is_active(s)) {                     // (wave-uniform)
          const unsigned* wr = reinterpret_cast<const unsigned*>(W + (int64_t)slot_idx(s) * d_p + c0);
#pragma unroll
          for (int q = 0; q < MAXP; ++q)
            if (q < npair) {
              const unsigned u = wr[q];
              p = fmaf(r[2 * q], __uint_as_float(u << 16), p);
              p = fmaf(r[2 * q + 1], __uint_as_float(u & 0xFFFF0000u), p);
            }
        }
        A[j * RF_TILE_PITCH + lane] = p;
      }
      const float v = rf_tile_reduce(A, lane);
      if (lane < 32) cv[32 * ck + lane] = v;
    }

    // 3. the Gram matrix: lane (rr, h) feeds row i_{32 I + rr}, k = 16 kk + 8 h .. + 7, to tile row / column I
    {
      f32x16 acc[NTILE];
#pragma unroll
      for (int t = 0; t < NTILE; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
      const int rr = lane & 31, h = lane >> 5;
      const u32x4* base[NT];
      bool ract[NT];
#pragma unroll
      for (int I = 0; I < NT; ++I) {
        const int src = ((I & 1) << 5) + rr;
        const int ii = __shfl(si[NB > 1 ? (I >> 1) : 0], src, 64);
        ract[I] = (am[NB > 1 ? (I >> 1) : 0] >> src) & 1ull;
        base[I] = reinterpret_cast<const u32x4*>(W + (int64_t)ii * d_p + 8 * h);
      }
      const int ksteps = d_p >> 4;
#pragma unroll 1
      for (int kk = 0; kk < ksteps; ++kk) {
        bf16x8 f[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I) {
          u32x4 v = base[I][2 * kk];
          if (!ract[I]) v = u32x4{0u, 0u, 0u, 0u};
          f[I] = __builtin_bit_cast(bf16x8, v);
        }
        int t = 0;
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
          for (int J = I; J < NT; ++J, ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[I], f[J], acc[t], 0, 0, 0);
      }
      // 4. into LDS, both triangles from the upper one (accumulator register i of lane (rr, h): row (i & 3) + 8 (i >> 2) + 4 h, column rr)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      int t = 0;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int tr_ = (i & 3) + 8 * (i >> 2) + 4 * h;
            const int gs = 32 * I + tr_, gt = 32 * J + rr;
            if (I < J || tr_ <= rr) {
              A[gs * LDA + gt] = acc[t][i];
              A[gt * LDA + gs] = acc[t][i];
            }
          }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
      const int s = 64 * bk + lane;
      if (s < Kp) g0[s] = A[s * LDA + s];
    }
    if (tr.gram) {
      float* gr = tr.gram + row * (K + 1) * K;
      for (int q = lane; q < K * K; q += 64) gr[q] = A[(q / K) * LDA + (q % K)];
      for (int s = lane; s < K; s += 64) gr[K * K + s] = cv[s];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // 5. the factorisation, right-looking.  dreg / yreg: d_s and y_s of the lane's own slots (0: not kept)
    float dreg[NB], yreg[NB], l[NB];
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) dreg[bk] = yreg[bk] = l[bk] = 0.f;
    if (lane == 0) ev[0] = ee;
#pragma unroll 1
    for (int u = 0; u < K; ++u) {
      const float piv = A[u * LDA + u], g = g0[u];
      const bool keep = is_active(u) && !rf_dependent(piv, g);                     // (wave-uniform)
      if (keep) {
        const float dd = rf_sqrt(piv);
        const float yu = rf_div(cv[u], dd);
        ee = rf_err_step(ee, yu);
#pragma unroll
        for (int bk = 0; bk < NB; ++bk) {
          const int s = 64 * bk + lane;
          l[bk] = 0.f;
          if (s == u) {
            dreg[bk] = dd;
            yreg[bk] = yu;
          }
          if (s > u && s < K) {
            l[bk] = rf_div(A[s * LDA + u], dd);
            A[s * LDA + u] = l[bk];
            cv[s] = fmaf(-l[bk], yu, cv[s]);
          }
        }
        // the column applied to every later row: element (s, t), t = u + 1 .. s, with L[t][u] from lane t's register
#pragma unroll 1
        for (int t0 = u + 1; t0 < K; t0 += 4) {
          float lt[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int t = t0 + q < K ? t0 + q : K - 1;
            lt[q] = pick(l, t);
          }
#pragma unroll
          for (int bk = 0; bk < NB; ++bk) {
            const int s = 64 * bk + lane;
            float av[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (t0 + q <= s && s < K) av[q] = A[s * LDA + t0 + q];
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (t0 + q <= s && s < K) A[s * LDA + t0 + q] = fmaf(-l[bk], lt[q], av[q]);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      }
      if (lane == 0) ev[u + 1] = ee;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // 6. back-substitution by columns, descending: lane s keeps its running y_s; a_u is wave-uniform
    float yy[NB], a[NB];
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
      yy[bk] = yreg[bk];
      a[bk] = 0.f;
    }
#pragma unroll 1
    for (int u = K - 1; u >= 0; --u) {
      const float dd = pick(dreg, u);
      if (!(dd > 0.f)) continue;                                                   // (wave-uniform)
      const float au = rf_div(pick(yy, u), dd);
#pragma unroll
      for (int bk = 0; bk < NB; ++bk) {
        const int s = 64 * bk + lane;
        if (s == u) a[bk] = au;
        if (s < u) yy[bk] = fmaf(-A[u * LDA + s], au, yy[bk]);
      }
    }
    // the final residual over the kept slots in slot order, e_final
#pragma unroll 1
    for (int s = 0; s < K; ++s) {
      if (!(pick(dreg, s) > 0.f)) continue;                                        // (wave-uniform)
      const float na = -pick(a, s);
      const unsigned* wr = reinterpret_cast<const unsigned*>(W + (int64_t)slot_idx(s) * d_p + c0);
#pragma unroll
      for (int q = 0; q < MAXP; ++q)
        if (q < npair) {
          const unsigned u = wr[q];
          r[2 * q] = fmaf(na, __uint_as_float(u << 16), r[2 * q]);
          r[2 * q + 1] = fmaf(na, __uint_as_float(u & 0xFFFF0000u), r[2 * q + 1]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    A[lane] = lane_sq();
    const float ef = rf_lane_get(rf_tile_reduce(A, lane), 0);

    // the row's outputs
    for (int m = lane; m <= K; m += 64) err[row * (K + 1) + m] = ev[m];
    int nkept = 0;
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) nkept += __popcll(__ballot(dreg[bk] > 0.f));
    if (lane == 0) {
      efin[row] = ef;
      keptn[row] = nkept;
    }
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
      const int s = 64 * bk + lane;
      const bool act = s < K && ((am[bk] >> lane) & 1ull);
      const bool kept = dreg[bk] > 0.f;
      if (s < K) {
        if (tr.coef) tr.coef[row * K + s] = a[bk];
        if (tr.dep) tr.dep[row * K + s] = (act && !kept) ? 1 : 0;
      }
      // a latent counts once per frame in SLOTS: a repeated index (a given support only) counts at its first active slot
      bool first = true;
      if (sup.given)
        for (int t = 0; t < K; ++t) {
          const int it = slot_idx(t);
          if (is_active(t) && t < s && it == si[bk]) first = false;
        }
      if (act) {
        if (first) atomicAdd(cnt.slots + si[bk], 1ull);
        if (a[bk] < 0.f) atomicAdd(cnt.neg + si[bk], 1ull);
        if (!kept) atomicAdd(cnt.dep + si[bk], 1ull);
        if (kept && !sup.given) atomicAdd(&hist[rf_ratio_bin(rf_div(a[bk], sv[bk]))], 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < RF_RATIO_BINS && hist[threadIdx.x]) atomicAdd(cnt.ratio + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// ---- the rows' curves into the frontier's partial layout (frontier.h: part / rowinfo / bud), the KEPT histogram and the per-unit
// sums of e_final.  One workgroup per FR_UNIT rows: thread m adds e_m of the unit's counted rows (thread K + 1: e_final).
__global__ __launch_bounds__(256) void refit_finish_kernel(const float* __restrict__ err, const float* __restrict__ efin,
                                                           const int* __restrict__ keptn, int64_t M, int K, FrTau tau,
                                                           float* __restrict__ part, uint32_t* __restrict__ rowinfo,
                                                           unsigned short* __restrict__ bud, float* __restrict__ finpart,
                                                           unsigned long long* __restrict__ kept_hist) {
  const int64_t row0 = (int64_t)blockIdx.x * FR_UNIT;
  const int tid = threadIdx.x;
  for (int m = tid; m <= K + 1; m += 256) {
    // (the order of frontier_walk_kernel's unit sums -- rows 4 i + w per wave w, then the four waves in order -- so that sse[0] is
    // bit-equal to the frontier's)
    float sw[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < FR_UNIT; ++i) {
      const int64_t row = row0 + i;
      if (row < M && keptn[row] >= 0) sw[i & 3] = __fadd_rn(sw[i & 3], m <= K ? err[row * (K + 1) + m] : efin[row]);
    }
    const float sum = __fadd_rn(__fadd_rn(__fadd_rn(sw[0], sw[1]), sw[2]), sw[3]);
    if (m <= K) part[(int64_t)blockIdx.x * FR_PART_LD + m] = sum;
    else finpart[blockIdx.x] = sum;
  }
  const int64_t row = row0 + tid;
  if (tid < FR_UNIT && row < M) {
    const int nk = keptn[row];
    if (!fr_row_finish(nk >= 0, row, err + row * (K + 1), K, tau, rowinfo, bud)) return;
    atomicAdd(kept_hist + (nk <= K ? nk : K), 1ull);
  }
}

// ---- the per-unit sums of e_final in unit order into the block (one thread)
__global__ void refit_final_kernel(const float* __restrict__ finpart, int n_units, double* __restrict__ sse_final) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = 0.0;
  for (int u = 0; u < n_units; ++u) s += (double)finpart[u];
  *sse_final += s;
}
#endif
