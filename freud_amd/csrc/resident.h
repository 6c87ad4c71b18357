// The kernels of the HBM-resident activation store (freud_amd/resident.py; include/freud_sae.h, sae_store_convert / sae_store_gather):
// the one-time fp32 -> bf16 conversion of uploaded shard rows and the per-step gather of a batch's files out of the store.  Both are
// pure memory traffic; every offset is 64-bit; neither uses LDS or scratch.
//
// Gather: one workgroup of RS_THREADS threads copies one piece (RS_PIECE_BYTES, resident_index.h) of one batch row.  A thread issues
// RS_UNROLL independent loads -- lane-contiguous, so a wave's load is one 1 KiB run -- before its first store.  V is the widest unit
// that divides every address and extent of the launch (16, 4 or 2 bytes; chosen on the host, once per launch); the narrow forms walk the
// piece in rounds of RS_UNROLL loads.  The store is read with the non-temporal policy (each byte is read once per epoch and the
// store is far larger than any cache), the batch is written with the default one (the train step reads it next).  Measured on the
// kernel alone the read policy makes no difference; it is kept for what it says about the data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_guard.h"
#include "resident_index.h"

typedef uint32_t rs_u32x4 __attribute__((ext_vector_type(4)));

template <typename V>
__device__ __forceinline__ V rs_load(const V* p) { return __builtin_nontemporal_load(p); }

template <typename V>
__global__ __launch_bounds__(RS_THREADS) void store_gather_kernel(const char* __restrict__ store, int64_t n_files, int64_t row_bytes,
                                                                  const int32_t* __restrict__ idx, int64_t pieces, char* __restrict__ out,
                                                                  int64_t out_stride, unsigned int* __restrict__ err) {
  int64_t j, p, byte0, len;
  rs_block_of((int64_t)blockIdx.x, pieces, &j, &p);
  bool bad;
  const int64_t file = rs_clamp_index(idx[j], n_files, &bad);
  if (bad && p == 0 && threadIdx.x == 0) atomicAdd(err, 1u);
  rs_piece_span(row_bytes, p, &byte0, &len);
  const V* __restrict__ src = reinterpret_cast<const V*>(store + rs_src_offset(file, row_bytes) + byte0);
  V* __restrict__ dst = reinterpret_cast<V*>(out + rs_dst_offset(j, out_stride) + byte0);
  const int n = (int)(len / (int64_t)sizeof(V));
  for (int e0 = (int)threadIdx.x; e0 < n; e0 += RS_THREADS * RS_UNROLL) {
    V v[RS_UNROLL] = {};
#pragma unroll
    for (int u = 0; u < RS_UNROLL; ++u)
      if (e0 + u * RS_THREADS < n) v[u] = rs_load(src + e0 + u * RS_THREADS);
#pragma unroll
    for (int u = 0; u < RS_UNROLL; ++u)
      if (e0 + u * RS_THREADS < n) dst[e0 + u * RS_THREADS] = v[u];
  }
}

// Convert: VEC (source and destination 16-byte aligned) -- a thread takes 8 values with two 16-byte loads and leaves them with one
// 16-byte store, the workgroups stride over the groups of 8, and the n % 8 values of the tail go through the scalar rule; otherwise the
// scalar rule for every value.
template <bool VEC>
__global__ __launch_bounds__(256) void store_convert_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(src);
  int64_t done = 0;
  if (VEC) {
    const int64_t groups = n >> 3;
    const rs_u32x4* __restrict__ s4 = reinterpret_cast<const rs_u32x4*>(src);
    rs_u32x4* __restrict__ d4 = reinterpret_cast<rs_u32x4*>(dst);
    for (int64_t g = tid; g < groups; g += stride) {
      const rs_u32x4 a = s4[2 * g], b = s4[2 * g + 1];
      rs_u32x4 o;
      o.x = bg_f32_bits_to_bf16(a.x) | (bg_f32_bits_to_bf16(a.y) << 16);
      o.y = bg_f32_bits_to_bf16(a.z) | (bg_f32_bits_to_bf16(a.w) << 16);
      o.z = bg_f32_bits_to_bf16(b.x) | (bg_f32_bits_to_bf16(b.y) << 16);
      o.w = bg_f32_bits_to_bf16(b.z) | (bg_f32_bits_to_bf16(b.w) << 16);
      d4[g] = o;
    }
    done = groups << 3;
  }
  for (int64_t i = done + tid; i < n; i += stride) dst[i] = (uint16_t)bg_f32_bits_to_bf16(s[i]);
}
