// The decoder-norm constraint of TopK training (sae_set_decoder_constraint): the two functions the reference model defines for it,
// topkautoencoder.py:153-175, as two kernels over the fp32 master W_dec[n_p][d_p] (row j = latent j's decoder direction).
//
//   topk_dec_project_kernel   remove_gradient_parallel_to_decoder_directions:  g_j <- g_j - (g_j . w_j) w_j   (no division by |w_j|^2:
//                             the rows are unit because the renorm below ran after the last update)
//   topk_dec_renorm_kernel    set_decoder_norm_to_unit_norm:  w_j <- w_j / (||w_j||_2 + eps),  eps = 2^-23 (torch.finfo(float32).eps),
//                             and the bf16 row of Wd_b from the renormalised values
//
// One wave per row, four rows per 256-thread workgroup, grid n_p / 4 (n_p is a multiple of 128).  A row is d_p / 4 float4s, d_p a
// multiple of 128: lane l holds the float4s l, l + 64, ... in a register array of NV = ceil(d_p / 256) entries with compile-time
// indexing, so that a wave reads contiguous 1 KB segments; the last entry is absent in the upper lanes when d_p / 4 is no multiple
// of 64 (d_p = 128: half the lanes idle; 384: one and a half per lane).  The dot and the sum of squares are a per-lane fp32 partial in
// index order followed by the xor-butterfly of wave_sum: a fixed order, the same bits on every replica.  No LDS, no atomics.
// Padding: a zero row stays +0.0 (0 - 0 * 0 and 0 / (0 + eps)), so do the zero columns of a live row.
#pragma once
#include <type_traits>

#include "common.h"

constexpr float DEC_NORM_EPS = 1.1920928955078125e-07f;      // 2^-23
constexpr int DEC_NORM_MAX_NV = 6;                            // d_p <= 1536, the largest d a TopK context accepts (sae_create)

template <int NV>
__global__ __launch_bounds__(256) void topk_dec_project_kernel(float* __restrict__ g, const float* __restrict__ w, int d_p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, nv = d_p >> 2;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  f32x4* const g4 = reinterpret_cast<f32x4*>(g + row * d_p);
  const f32x4* const w4 = reinterpret_cast<const f32x4*>(w + row * d_p);
  f32x4 gv[NV], wv[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int i = q * 64 + lane;
    const bool in = i < nv;
    gv[q] = in ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    wv[q] = in ? w4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float dot = 0.f;
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) dot = dot + gv[q][j] * wv[q][j];
  dot = wave_sum(dot);
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int i = q * 64 + lane;
    if (i < nv) g4[i] = gv[q] - dot * wv[q];
  }
}

template <int NV>
__global__ __launch_bounds__(256) void topk_dec_renorm_kernel(float* __restrict__ w, bf16_t* __restrict__ wb, int d_p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, nv = d_p >> 2;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  f32x4* const w4 = reinterpret_cast<f32x4*>(w + row * d_p);
  bf16x4* const b4 = reinterpret_cast<bf16x4*>(wb + row * d_p);
  f32x4 wv[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int i = q * 64 + lane;
    wv[q] = i < nv ? w4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) ss = ss + wv[q][j] * wv[q][j];
  const float den = sqrtf(wave_sum(ss)) + DEC_NORM_EPS;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int i = q * 64 + lane;
    if (i < nv) {
      const f32x4 o = wv[q] / den;
      w4[i] = o;
      b4[i] = bf16x4{(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
    }
  }
}

// the one dispatch of both kernels on NV = ceil(d_p / 256): f(integral_constant<NV>)
template <class F>
static bool with_dec_nv(int d_p, F&& f) {
  switch ((d_p + 255) / 256) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    default: return false;
  }
}
