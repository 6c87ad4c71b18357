// Dictionary comparison (include/freud_sae.h, sae_dict_pack / sae_dict_sim_keys): the cosines between the unit decoder directions of
// two dictionaries (or of one with itself), and per direction of A the keys from which file_top.h selects its nearest directions
// of B.
//
// A dictionary is n directions of length d in fp32 with an element stride and a direction stride (TopK: the rows of W_dec [n][d];
// L1: the columns of the tied decoder.weight [d][n]), read in place.  u = w / ||w|| with ||w|| = sqrt_rn of an fp32 sum of squares
// in ONE fixed order -- 64 partial sums, partial l takes the elements l, l + 64, ... in order with one fmaf each, then the xor
// butterfly 32, 16, 8, 4, 2, 1 over the partials -- and an IEEE division, so both read patterns give the same bits.  A direction of
// norm 0 stays the zero vector.
//
// The cosine runs on the bf16 MFMA with fp32 accumulation.  Bf16 operands alone are a few 1e-4 off, too coarse to tell a duplicate
// from a neighbour, so a unit vector is split as hi = bf16(u), lo = bf16(u - hi) and the product is hi.hi + hi.lo + lo.hi (the
// dropped lo.lo is at most 2^-18 relative).  Concatenated along K that is an ordinary row x row bf16 GEMM with K = 3 d_p: the left
// operand packs [hi | hi | lo], the right one [hi | lo | hi]; every segment is d rounded up to DM_K_ALIGN, the rows are n rounded up
// to DM_ROW_ALIGN, all padding is zero.  Three kernels:
//   * the pack: fp32 directions -> the operand and norms [n].  Directions contiguous (element stride 1): one wave per direction.
//     Otherwise (the L1 layout, direction stride 1): 64 directions per workgroup, read along the directions and transposed through
//     LDS so that reads and writes both stay coalesced, as coact.h's mask pack does.
//   * the similarity keys: gemm256.h's OP_ROW x OP_ROW tile GEMM over the 256-aligned cover of A's rows [row0, row0 + n_rows)
//     against all of B with the epilogue functor EpiDictKeys: keys[n_rows][n_b] = ord(S) << 32 (search_keys.h), 0 on the diagonal
//     in self mode; rows and columns of the padding are dropped.  One kernel whatever the row block: an element's sum over K does
//     not depend on the block it is computed in, so any blocking gives the same bits.
//   * the select is file_top.h's, with flags 0: signed cosines, key 0 = not eligible, ties towards the lower column.
//
// The first part is free of any HIP type and compiles for the host as search_keys.h does (tests/test_dictionary_match_cpu.py).
#pragma once
#include "search_keys.h"

enum { DM_LEFT = 0, DM_RIGHT = 1 };      // the `side` of sae_dict_pack
#define DM_MAX_D 8192                    // include/freud_sae.h: SAE_DICT_MAX_D
#define DM_MAX_N (1 << 24)               // file_top.h: FT_MAX_COLS
#define DM_ROW_ALIGN 256                 // gemm256.h's tile edge
#define DM_K_ALIGN 64                    // its K tile

// bf16 of a finite fp32, round to nearest even, as its 16 bits
SK_HD uint16_t dm_bf16_bits(float v) {
  uint32_t b = sk_bits(v);
  b += 0x7FFFu + ((b >> 16) & 1u);
  return (uint16_t)(b >> 16);
}
SK_HD float dm_bf16_float(uint16_t h) { return sk_float((uint32_t)h << 16); }
// u = hi + lo up to 2^-18 |u|; u - hi is exact in fp32, and lo == 0 whenever u is a bf16 number
SK_HD uint16_t dm_split_hi(float u) { return dm_bf16_bits(u); }
SK_HD uint16_t dm_split_lo(float u) { return dm_bf16_bits(u - dm_bf16_float(dm_split_hi(u))); }

// the key of a cosine: order-preserving on signed values, -0.0 as +0.0, never 0 for a finite value (0 = not eligible)
SK_HD uint64_t dm_key(float s) { return (uint64_t)sk_ord(s) << 32; }
SK_HD float dm_key_cosine(uint64_t k) { return sk_unord((uint32_t)(k >> 32)); }

// the packed operand: [dm_rows_p(n)][dm_ld(d)] bf16
SK_HD int64_t dm_rows_p(int64_t n) { return (n + DM_ROW_ALIGN - 1) / DM_ROW_ALIGN * DM_ROW_ALIGN; }
SK_HD int64_t dm_d_p(int64_t d) { return (d + DM_K_ALIGN - 1) / DM_K_ALIGN * DM_K_ALIGN; }
SK_HD int64_t dm_ld(int64_t d) { return 3 * dm_d_p(d); }
SK_HD int64_t dm_pack_bytes(int64_t n, int64_t d) { return dm_rows_p(n) * dm_ld(d) * 2; }

#if defined(__HIPCC__)
#include "common.h"

typedef unsigned long long dm_u64x2 __attribute__((ext_vector_type(2)));

// segment of the hi copy beside segment 0, and of lo
__device__ __forceinline__ int dm_seg_hi(int side) { return side == DM_LEFT ? 1 : 2; }
__device__ __forceinline__ int dm_seg_lo(int side) { return side == DM_LEFT ? 2 : 1; }

__device__ __forceinline__ float dm_unit(float w, float nrm) { return nrm > 0.f ? __fdiv_rn(w, nrm) : 0.f; }

// ---- pack, directions contiguous: one wave per direction, 4 per workgroup; grid rows_p / 4.  Lane l owns partial l.
__global__ __launch_bounds__(256) void dict_pack_rows_kernel(const float* __restrict__ w, int64_t n, int d, int64_t dir_stride, int side,
                                                             unsigned short* __restrict__ packed, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t dir = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int d_p = (int)dm_d_p(d);
  const bool live = dir < n;
  const float* src = w + (live ? dir : 0) * dir_stride;
  float p = 0.f;
  if (live)
    for (int e = lane; e < d; e += 64) {
      const float x = src[e];
      p = __fmaf_rn(x, x, p);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p = __fadd_rn(p, __shfl_xor(p, o));
  const float nrm = __fsqrt_rn(p);
  if (live && lane == 0) norms[dir] = nrm;
  unsigned short* dst = packed + dir * (3 * (int64_t)d_p);
  const int sh = dm_seg_hi(side) * d_p, sl = dm_seg_lo(side) * d_p;
  for (int e0 = lane * 8; e0 < d_p; e0 += 512) {
    u32x4 vh, vl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t h[2], l[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int e = e0 + 2 * q + t;
        const float u = (live && e < d) ? dm_unit(src[e], nrm) : 0.f;
        h[t] = dm_split_hi(u);
        l[t] = dm_split_lo(u);
      }
      vh[q] = h[0] | (h[1] << 16);
      vl[q] = l[0] | (l[1] << 16);
    }
    *reinterpret_cast<u32x4*>(dst + e0) = vh;
    *reinterpret_cast<u32x4*>(dst + sh + e0) = vh;
    *reinterpret_cast<u32x4*>(dst + sl + e0) = vl;
  }
}

// ---- pack, directions strided: 64 directions per workgroup; grid rows_p / 64.  Thread (direction t & 63, q = t >> 6) reads the
// elements 64 c + q + 4 i (i = 0..15) of chunk c along the directions and owns the partials l = q + 4 i; the butterfly's steps 32 .. 4
// pair partials of one thread, its steps 2 and 1 the four threads of a direction.  The split goes through LDS [direction][element]
// and leaves along the elements, 32 bytes per thread and segment.
__global__ __launch_bounds__(256) void dict_pack_cols_kernel(const float* __restrict__ w, int64_t n, int d, int64_t dir_stride,
                                                             int64_t elem_stride, int side, unsigned short* __restrict__ packed,
                                                             float* __restrict__ norms) {
  __shared__ float red[4][64];
  __shared__ __attribute__((aligned(16))) unsigned short thi[64][72];      // rows of 144 bytes keep the 16-byte reads aligned
  __shared__ __attribute__((aligned(16))) unsigned short tlo[64][72];
  const int tid = threadIdx.x, dl = tid & 63, q = tid >> 6;
  const int64_t dir0 = (int64_t)blockIdx.x * 64, dir = dir0 + dl;
  const int d_p = (int)dm_d_p(d), nchunk = d_p / 64;
  const bool live = dir < n;
  const float* src = w + (live ? dir : 0) * dir_stride;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = 64 * c + q + 4 * i;
      if (live && e < d) {
        const float x = src[(int64_t)e * elem_stride];
        acc[i] = __fmaf_rn(x, x, acc[i]);
      }
    }
  }
#pragma unroll
  for (int h = 8; h > 0; h >>= 1)
#pragma unroll
    for (int i = 0; i < h; ++i) acc[i] = __fadd_rn(acc[i], acc[i + h]);
  red[q][dl] = acc[0];
  __syncthreads();
  const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(red[0][dl], red[2][dl]), __fadd_rn(red[1][dl], red[3][dl])));
  if (live && q == 0) norms[dir] = nrm;

  const int r = tid >> 2, part = (tid & 3) * 16;
  unsigned short* dst = packed + (dir0 + r) * (3 * (int64_t)d_p) + part;
  const int sh = dm_seg_hi(side) * d_p, sl = dm_seg_lo(side) * d_p;
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int el = q + 4 * i, e = 64 * c + el;
      const float u = (live && e < d) ? dm_unit(src[(int64_t)e * elem_stride], nrm) : 0.f;
      thi[dl][el] = dm_split_hi(u);
      tlo[dl][el] = dm_split_lo(u);
    }
    __syncthreads();
    const u32x4 h0 = *reinterpret_cast<const u32x4*>(&thi[r][part]), h1 = *reinterpret_cast<const u32x4*>(&thi[r][part + 8]);
    const u32x4 l0 = *reinterpret_cast<const u32x4*>(&tlo[r][part]), l1 = *reinterpret_cast<const u32x4*>(&tlo[r][part + 8]);
    unsigned short* o = dst + 64 * c;
    *reinterpret_cast<u32x4*>(o) = h0;
    *reinterpret_cast<u32x4*>(o + 8) = h1;
    *reinterpret_cast<u32x4*>(o + sh) = h0;
    *reinterpret_cast<u32x4*>(o + sh + 8) = h1;
    *reinterpret_cast<u32x4*>(o + sl) = l0;
    *reinterpret_cast<u32x4*>(o + sl + 8) = l1;
    __syncthreads();
  }
}

// ---- the similarity keys: the epilogue functor of the row x row tile GEMM (gemm.h's interface).  GEMM row `row` is direction
// row_base + row of A (row_base = row0 rounded down to DM_ROW_ALIGN); the wanted rows are [row_lo, row_lo + n_rows) with
// row_lo = row0 - row_base.  The accumulator is used as it is: no rounding, no clamp.
struct EpiDictKeys {
  uint64_t* keys;       // [n_rows][n_b]
  int64_t n_b, n_rows;
  int64_t self_base;    // self mode: row_base, so that GEMM row r meets itself in column self_base + r; otherwise -2^40 (no column)
  int row_lo;
  __device__ void tile_begin(int, int, int) {}
  struct Pre {};
  __device__ Pre prefetch(int, int) const { return Pre{}; }
  __device__ void apply(int row, int col, f32x4 v, const Pre&) {
    const int64_t r = (int64_t)row - row_lo;
    if (r < 0 || r >= n_rows || col >= n_b) return;
    const int64_t self_col = self_base + row;
    uint64_t k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = col + j == self_col ? 0ull : dm_key(v[j]);
    uint64_t* p = keys + r * n_b + col;
    if (col + 3 < n_b && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<dm_u64x2*>(p) = dm_u64x2{k[0], k[1]};
      *reinterpret_cast<dm_u64x2*>(p + 2) = dm_u64x2{k[2], k[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col + j < n_b) p[j] = k[j];
    }
  }
  __device__ void tile_end(float*) {}
};
#endif
