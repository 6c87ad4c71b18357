// Feature manipulation (include/freud_sae.h, sae_manipulate_files; the reference's manipulate_latent, utils/activations.py:243-272):
// edit chosen latents of every frame and decode both ways -- the standard reconstruction, and for every variant (one row of edit
// values, e.g. one factor of a sweep) the manipulated one -- from ONE encode and ONE decode.
//
// A decode is linear in the latent, so the manipulated reconstruction is the standard one plus a rank-one term per edited latent:
//
//   manipulated[v][t][c] = fmaf(delta_{v,E-1}, w_{E-1}[c], ... fmaf(delta_{v,0}, w_0[c], standard[t][c]))
//
// edits in the order given, all in fp32.  a = the value encode() returns for (frame, latent), widened exactly from bf16; new and
// delta are ONE fp32 rounding each (sm_new, sm_delta); w_e = row latent_e of the bf16 decoder operand the standard decode
// multiplies by, widened exactly.  An edit whose delta is zero is SKIPPED instead of added as fmaf(0, w, acc): the two differ only
// in the sign of a zero (fmaf(0, w, -0.0) = +0.0), and a frame on which nothing changes must come out bit for bit as standard.
// The result is what a decode of the edited latent gives when the edited value is not rounded back to bf16 as a GEMM operand.
//
// Four kernels: the series (the edited latents' values per frame: a strided read of the stored L1 latent, a search of the TopK
// row's k indices), the operand rows (w_e gathered once into E x d floats), the TopK standard decode straight from the compact
// selection (no dense row, no GEMM; the L1 one is the decoder GEMM of sae_decode), and the apply rule for all variants in one pass.
//
// The first part is free of any HIP type and compiles for the host as search_keys.h does (tests/test_manipulate_cpu.py);
// sm_apply_serial DEFINES the apply kernel's answer, as ft_select_serial defines the file-features select.
#pragma once
#include <math.h>
#include "search_keys.h"

enum { SM_SCALE = 0, SM_SET = 1 };      // include/freud_sae.h: SAE_MANIP_*
#define SM_MAX_EDITS 16                 // SAE_MANIP_MAX_EDITS
#define SM_MAX_VARIANTS 16              // SAE_MANIP_MAX_VARIANTS

// one fp32 rounding each; on the device the intrinsics keep the compiler from contracting the pair into an fma
SK_HD float sm_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(a, b);
#else
  return a * b;
#endif
}
SK_HD float sm_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsub_rn(a, b);
#else
  return a - b;
#endif
}
// SM_SCALE: the reference's a * factor (activations.py:247-249, 261); SM_SET: the latent clamped to `value` on every frame
SK_HD float sm_new(int op, float a, float value) { return op == SM_SET ? value : sm_mul(a, value); }
SK_HD float sm_delta(int op, float a, float value) { return sm_sub(sm_new(op, a, value), a); }

// One frame of one variant on the host: standard [d], a [n_edits] (the frame's values of the edited latents), ops / values
// [n_edits], w [n_edits][w_stride] (operand rows, d used) -> out [d].
inline void sm_apply_serial(const float* standard, int64_t d, int n_edits, const int32_t* ops, const float* a, const float* values,
                            const float* w, int64_t w_stride, float* out) {
  for (int64_t c = 0; c < d; ++c) out[c] = standard[c];
  for (int e = 0; e < n_edits; ++e) {
    const float delta = sm_delta(ops[e], a[e], values[e]);
    if (delta == 0.f) continue;
    for (int64_t c = 0; c < d; ++c) out[c] = fmaf(delta, w[e * w_stride + c], out[c]);
  }
}

#if defined(__HIPCC__)
#include "common.h"

// the edits of one call, by value in the kernel arguments (1.2 KB): no host-to-device copy, nothing to keep alive
struct ManipEdits {
  int n_edits, n_variants;
  int latents[SM_MAX_EDITS];
  int ops[SM_MAX_EDITS];
  float values[SM_MAX_VARIANTS][SM_MAX_EDITS];
};

// ---- series, L1: series[e][t] = lat[t][latent_e] (bf16 [M][ld]) widened.  One thread per (e, t).
__global__ __launch_bounds__(256) void manip_series_kernel(const bf16_t* __restrict__ lat, int64_t ld, int64_t M, ManipEdits ed,
                                                           float* __restrict__ series) {
  const int64_t total = M * ed.n_edits;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int e = (int)(i / M);
    const int64_t t = i - (int64_t)e * M;
    series[i] = (float)lat[t * ld + ed.latents[e]];
  }
}

// ---- series, TopK: one wave per row (4 per workgroup) walks the row's k (index, value) pairs; lane e looks for latent_e.  The
// indices of a row are distinct, so at most one pair matches; no match = 0 (activation_tensor_from_indexed, activations.py:41-58).
__global__ __launch_bounds__(256) void manip_series_topk_kernel(const int* __restrict__ idx, const bf16_t* __restrict__ vals, int k,
                                                                int64_t M, ManipEdits ed, float* __restrict__ series) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                     // (wave-uniform)
  int want = -2;                            // (no index is -2: -1 marks a padding slot)
#pragma unroll
  for (int e = 0; e < SM_MAX_EDITS; ++e)
    if (lane == e && e < ed.n_edits) want = ed.latents[e];
  float got = 0.f;
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int jj = j0 + lane;
    const int my_i = jj < k ? idx[row * k + jj] : -1;
    const float my_a = jj < k ? (float)vals[row * k + jj] : 0.f;
    const int cnt = k - j0 < 64 ? k - j0 : 64;
    for (int j = 0; j < cnt; ++j) {
      const int ii = __shfl(my_i, j, 64);
      const float av = __shfl(my_a, j, 64);
      if (ii == want) got = av;
    }
  }
  if (lane < ed.n_edits) series[(int64_t)lane * M + row] = got;
}

// ---- operand rows: wrows[e][c] = W[latent_e * rs + c * cs] widened, c < d.  L1: the bf16 copy of W [d_p][n_p], rs = 1, cs = n_p;
// TopK: the bf16 copy of W_dec [n_p][d_p], rs = d_p, cs = 1.  Grid (ceil(d / 256), n_edits).
__global__ __launch_bounds__(256) void manip_rows_kernel(const bf16_t* __restrict__ W, int64_t rs, int64_t cs, int d, ManipEdits ed,
                                                         float* __restrict__ wrows, int w_stride) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int e = blockIdx.y;
  if (c < d) wrows[(int64_t)e * w_stride + c] = (float)W[(int64_t)ed.latents[e] * rs + (int64_t)c * cs];
}

// ---- TopK standard decode: x_hat[t] = b_dec + sum_i vals[t][i] * Wd[idx[t][i]] in fp32, in stored list order, with fmaf.  The
// access pattern of topk_decode_kernel: one wave per row, lane l owns the d_p / 64 contiguous columns from l * d_p / 64, so every
// gathered row is one coalesced line; NPAIR > 0: d_p == 128 * NPAIR at compile time and two gathered rows in flight.
template <int NPAIR>
__global__ __launch_bounds__(256) void manip_topk_decode_kernel(const bf16_t* __restrict__ vals, const int* __restrict__ idx, int k,
                                                                const bf16_t* __restrict__ Wd, const float* __restrict__ b_dec,
                                                                float* __restrict__ out, int64_t M, int d, int d_p, int n_p) {
  constexpr int MAXP = NPAIR > 0 ? NPAIR : 12;   // column pairs per lane: d_p <= 64 * 2 * MAXP
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                          // (wave-uniform)
  const int npair = NPAIR > 0 ? NPAIR : d_p >> 7;
  const int c0 = lane * 2 * npair;
  float acc[2 * MAXP];
#pragma unroll
  for (int i = 0; i < 2 * MAXP; ++i) acc[i] = 0.f;
  const int* ri = idx + row * k;
  const bf16_t* rv = vals + row * k;
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int jj = j0 + lane;
    const int my_i = jj < k ? ri[jj] : -1;
    const float my_a = jj < k ? (float)rv[jj] : 0.f;
    const int cnt = k - j0 < 64 ? k - j0 : 64;
    if constexpr (NPAIR > 0) {
      for (int j = 0; j < cnt; j += 2) {
        float av[2];
        const unsigned* wp[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int jr = j + r < 64 ? j + r : 63;                // (wave-uniform)
          const int ir = __shfl(my_i, jr, 64);
          const bool ok = j + r < cnt && ir >= 0 && ir < n_p;    // a padding slot reads row 0 and is not added
          av[r] = ok ? __shfl(my_a, jr, 64) : 0.f;
          wp[r] = reinterpret_cast<const unsigned*>(Wd + (int64_t)(ok ? ir : 0) * d_p + c0);
        }
        unsigned u[2][NPAIR];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int p = 0; p < NPAIR; ++p) u[r][p] = wp[r][p];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int p = 0; p < NPAIR; ++p) {
            acc[2 * p] = fmaf(av[r], __uint_as_float(u[r][p] << 16), acc[2 * p]);
            acc[2 * p + 1] = fmaf(av[r], __uint_as_float(u[r][p] & 0xFFFF0000u), acc[2 * p + 1]);
          }
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        const int ii = __shfl(my_i, j, 64);
        const float av = __shfl(my_a, j, 64);
        if (ii < 0 || ii >= n_p) continue;      // wave-uniform
        const unsigned* wr = reinterpret_cast<const unsigned*>(Wd + (int64_t)ii * d_p + c0);
#pragma unroll
        for (int p = 0; p < MAXP; ++p)
          if (p < npair) {
            const unsigned u = wr[p];
            acc[2 * p] = fmaf(av, __uint_as_float(u << 16), acc[2 * p]);
            acc[2 * p + 1] = fmaf(av, __uint_as_float(u & 0xFFFF0000u), acc[2 * p + 1]);
          }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 2 * MAXP; ++p)
    if (p < 2 * npair && c0 + p < d) out[row * d + c0 + p] = acc[p] + b_dec[c0 + p];
}

// ---- the apply rule, all variants in one pass.  A HALF wave (32 lanes) owns a slab of 32 x VW columns and walks frames: its
// lanes keep the slab's part of the E operand rows in registers (VW x 16 floats, loaded once), read standard[t] once (16 bytes
// per lane with VW = 4), and write one row part per variant.  VW = 4 needs d % 4 == 0 and 16-byte aligned buffers; VW = 1 is the
// form for everything else.  Grid: x = groups of 8 half waves, a multiple of the number of slabs.
template <int VW>
struct ManipVec { float v[VW]; };
template <int VW>
__device__ __forceinline__ ManipVec<VW> manip_load(const float* p) {
  ManipVec<VW> r;
  if constexpr (VW == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    r.v[0] = q[0]; r.v[1] = q[1]; r.v[2] = q[2]; r.v[3] = q[3];
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int VW>
__device__ __forceinline__ void manip_store(float* p, const ManipVec<VW>& r) {
  if constexpr (VW == 4) *reinterpret_cast<f32x4*>(p) = f32x4{r.v[0], r.v[1], r.v[2], r.v[3]};
  else *p = r.v[0];
}

template <int VW>
__global__ __launch_bounds__(256) void manip_apply_kernel(const float* __restrict__ standard, const float* __restrict__ series,
                                                          const float* __restrict__ wrows, int w_stride, int64_t M, int d, int nslab,
                                                          ManipEdits ed, float* __restrict__ manipulated) {
  const int hl = threadIdx.x & 31;
  const int64_t unit = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int slab = (int)(unit % nslab);
  const int64_t t0 = unit / nslab, tstep = (int64_t)gridDim.x * 8 / nslab;
  const int c = (slab * 32 + hl) * VW;
  if (c >= d) return;                       // (d % VW == 0: the lane's VW columns are all inside or all outside)
  ManipVec<VW> w[SM_MAX_EDITS];
  static_for<0, SM_MAX_EDITS>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    if (e < ed.n_edits) w[e] = manip_load<VW>(wrows + (int64_t)e * w_stride + c);
    else
#pragma unroll
      for (int i = 0; i < VW; ++i) w[e].v[i] = 0.f;
  });
  const int64_t Md = M * (int64_t)d;
  for (int64_t t = t0; t < M; t += tstep) {
    const ManipVec<VW> s = manip_load<VW>(standard + t * d + c);
    float a[SM_MAX_EDITS];
    static_for<0, SM_MAX_EDITS>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      a[e] = e < ed.n_edits ? series[(int64_t)e * M + t] : 0.f;
    });
    for (int v = 0; v < ed.n_variants; ++v) {
      ManipVec<VW> o = s;
      static_for<0, SM_MAX_EDITS>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < ed.n_edits) {
          const float delta = sm_delta(ed.ops[e], a[e], ed.values[v][e]);
#pragma unroll
          for (int i = 0; i < VW; ++i) o.v[i] = delta != 0.f ? fmaf(delta, w[e].v[i], o.v[i]) : o.v[i];
        }
      });
      manip_store<VW>(manipulated + (int64_t)v * Md + t * d + c, o);
    }
  }
}
#endif
