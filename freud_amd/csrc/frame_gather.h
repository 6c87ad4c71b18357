// The kernel of frame batches (include/freud_sae.h, sae_store_gather_frames): row j of the destination = the frame of the resident
// store that position pos0 + j * pos_stride of the epoch's permutation holds.  Pure memory traffic beside one evaluation of the
// permutation per FRAME; every offset is 64-bit; no scratch, FP_MAX_ROWS * 8 bytes of LDS.
//
// A workgroup serves the rows and units that fp_block_span (frame_perm.h) gives it.  Lane i < nrows evaluates row i's permutation
// and locate -- once per frame, not per thread -- and leaves the frame's byte offset in LDS; then unit e = tid + u * FP_THREADS of
// the workgroup is unit e % n of row e / n: lane-contiguous, so a wave's load is whole frames end to end (768-byte frames: 21 to a
// workgroup, no idle lane but in the last wave), and a thread issues its FP_UNROLL independent loads before its first store.  V is
// the copy unit of the launch (16, 4 or 2 bytes; chosen on the host).  As in resident.h the store is read with the non-temporal
// policy (each frame is read once per epoch, the store is far larger than any cache) and the batch is written with the default one
// (the train step reads it next).  The error word is the only atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_perm.h"
#include "resident.h"

template <typename V>
__global__ __launch_bounds__(FP_THREADS) void frame_gather_kernel(const char* __restrict__ store, const int64_t* __restrict__ prefix,
                                                                  int64_t n_files, int64_t T, int64_t frame_bytes, uint64_t N, uint64_t key,
                                                                  uint64_t pos0, uint64_t pos_stride, int64_t rows, fp_plan plan,
                                                                  char* __restrict__ out, int64_t out_stride, int64_t* __restrict__ ordinals,
                                                                  unsigned int* __restrict__ err) {
  __shared__ int64_t src_off[FP_MAX_ROWS];
  int64_t row0, unit0;
  int nrows, n;
  fp_block_span(plan, rows, (int64_t)blockIdx.x, &row0, &nrows, &unit0, &n);
  const int tid = (int)threadIdx.x;
  if (tid < nrows) {
    const int64_t j = row0 + tid;
    const uint64_t g = fp_permute(key, N, pos0 + (uint64_t)j * pos_stride);
    int64_t file, t;
    const bool bad = fp_locate(prefix, n_files, T, (int64_t)g, &file, &t);
    const int64_t row = fp_store_row(file, T, t);
    src_off[tid] = row * frame_bytes;
    if (unit0 == 0) {                                            // the workgroup of the row's first piece speaks for the row
      if (bad) atomicAdd(err, 1u);
      if (ordinals) ordinals[j] = row;
    }
  }
  __syncthreads();
  const uint32_t total = (uint32_t)nrows * (uint32_t)n;
  const int64_t byte0 = unit0 * (int64_t)sizeof(V);
  V v[FP_UNROLL] = {};
  uint32_t r[FP_UNROLL], c[FP_UNROLL];
#pragma unroll
  for (int u = 0; u < FP_UNROLL; ++u) {
    const uint32_t e = (uint32_t)(tid + u * FP_THREADS);
    r[u] = c[u] = 0;
    if (e < total) {
      fp_unit_of(e, (uint32_t)n, &r[u], &c[u]);
      v[u] = rs_load(reinterpret_cast<const V*>(store + src_off[r[u]] + byte0) + c[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < FP_UNROLL; ++u)
    if ((uint32_t)(tid + u * FP_THREADS) < total)
      reinterpret_cast<V*>(out + (row0 + r[u]) * out_stride + byte0)[c[u]] = v[u];
}
