// Feature search (the reference's `top_activations`, utils/activations.py:61-132, for every latent in one pass): per (file, latent)
// the maximum of the trimmed series and its first frame as ONE 64-bit key (search_keys.h), then a per-latent top-N merge.
// The latent itself is never written on the fused L1 path.
//
// Files are the rows [f T, f T + T) of the batch; only the first L[f] of them count (L = min(length, T), at least 1: the trim to the
// audio's duration, activations.py:19-29).  Every combination of partial results is an unsigned 64-bit max (vector atomics), so
// the keys do not depend on the order the workgroups run in, and the merge is one thread per latent over the files in order:
// the whole search is deterministic.
#pragma once
#include "common.h"
#include "search_keys.h"

__device__ __forceinline__ int search_len(const int* lengths, int f, int T) {
  int L = lengths ? lengths[f] : T;
  return L < 1 ? 1 : (L > T ? T : L);
}

__global__ __launch_bounds__(256) void search_fill_kernel(uint64_t* __restrict__ p, int64_t n, uint64_t v) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

// Segmented column reduction of a row-major [n_files T][ld] matrix: grid (column blocks of 256, files, row chunks).  Raw mode
// (x itself, no rounding) and the unfused L1 path (the stored bf16 latent).  ABS: keys get max |a| (first frame), aux the max of
// the SIGNED series (first frame); search_abs_fixup_kernel then turns aux into the side word of search_keys.h.
template <typename T, bool ABS>
__global__ __launch_bounds__(256) void search_colreduce_kernel(const T* __restrict__ x, int64_t ld, int ncols, int Trows,
                                                               const int* __restrict__ lengths, int chunk, uint64_t* __restrict__ keys,
                                                               uint64_t* __restrict__ aux) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  const int f = blockIdx.y;
  const int L = search_len(lengths, f, Trows);
  const int r0 = blockIdx.z * chunk;
  if (r0 >= L) return;
  const int r1 = r0 + chunk < L ? r0 + chunk : L;
  const T* p = x + ((int64_t)f * Trows) * ld + col;
  uint64_t best = 0, sbest = 0;
  for (int r = r0; r < r1; ++r) {
    const float v = (float)p[(int64_t)r * ld];
    if (ABS) {
      const uint64_t a = sk_key(fabsf(v), (uint32_t)r), sg = sk_key(v, (uint32_t)r);
      best = a > best ? a : best;
      sbest = sg > sbest ? sg : sbest;
    } else {
      const uint64_t k = sk_key(v, (uint32_t)r);
      best = k > best ? k : best;
    }
  }
  const int64_t o = (int64_t)f * ncols + col;
  atomicMax(reinterpret_cast<unsigned long long*>(keys + o), (unsigned long long)best);
  if (ABS) atomicMax(reinterpret_cast<unsigned long long*>(aux + o), (unsigned long long)sbest);
}

template <typename T>
__global__ __launch_bounds__(256) void search_abs_fixup_kernel(const T* __restrict__ x, int64_t ld, int ncols, int Trows, int64_t n_files,
                                                               const uint64_t* __restrict__ keys, uint64_t* __restrict__ aux) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_files * ncols) return;
  const int64_t f = i / ncols;
  const int col = (int)(i - f * ncols);
  const uint32_t fr = sk_key_frame(keys[i]);
  const float v = (float)x[(f * Trows + fr) * ld + col];
  aux[i] = sk_aux(v, sk_key_frame(aux[i]));
}

// TopK: the dense scatter of the selection (activation_tensor_from_indexed, activations.py:41-58) reduced per file -- frames where a
// latent is not selected are 0, which the keys' start value (0 at frame 0, SK_KEY_ZERO_FRAME0) stands for.
__global__ __launch_bounds__(256) void search_topk_scatter_kernel(const int* __restrict__ idx, const bf16_t* __restrict__ vals, int k,
                                                                  int64_t M, int Trows, const int* __restrict__ lengths, int ncols,
                                                                  uint64_t* __restrict__ keys) {
  const int64_t total = M * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / k;
    const int64_t f = r / Trows;
    const int fr = (int)(r - f * Trows);
    if (fr >= search_len(lengths, (int)f, Trows)) continue;
    const int j = idx[i];
    if (j < 0 || j >= ncols) continue;
    atomicMax(reinterpret_cast<unsigned long long*>(keys + f * ncols + j), (unsigned long long)sk_key((float)vals[i], (uint32_t)fr));
  }
}

// L1 search epilogue of the streaming encoder GEMM (gemm256s.h's s_* interface): EpiEnc's arithmetic to the bf16 latent
// (l1_kernels.h: fmaxf(bf16(acc) + b, 0), then bf16), reduced on the fly and never stored.  A lane keeps, per column of its 8, a
// 32-bit partial key of its rows of the current file: the latent's bf16 bits (>= 0: the magnitude bits order them) over
// 0xFFFF - frame (T <= 65535, checked on the host).  A file change inside a lane's rows (row blocks straddle files: T = 1500 is no
// multiple of 128, and T may be smaller than a block) flushes the lane's partials; at the end of the wave's 128 x 64 block a
// wave that stayed in one file folds its 8 row groups together first, so that the common case is ONE vector atomicMax per
// (file, column) segment.
struct EpiSearch {
  static constexpr bool STREAM = true;
  const float* bias;   // [n_p]
  uint64_t* keys;      // [n_files][n]
  const int* lengths;  // [n_files] or null
  int64_t M;           // n_files T
  int T, n;
  struct SPre {};
  float b[8];
  uint32_t acc[8];
  int cur_f, cur_base, cur_len;
  __device__ void s_begin() { cur_f = -1; cur_base = 0; cur_len = 0; }
  __device__ int64_t s_rows() const { return M; }
  __device__ void s_tile(int, int col) {
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + col), b1 = *reinterpret_cast<const f32x4*>(bias + col + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { b[j] = b0[j]; b[4 + j] = b1[j]; }
  }
  __device__ SPre s_prefetch(int, int) const { return SPre{}; }
  __device__ void flush(int col) {
    if (cur_f < 0) return;
    uint64_t* o = keys + (int64_t)cur_f * n + col;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (acc[j] != 0 && col + j < n)
        atomicMax(reinterpret_cast<unsigned long long*>(o + j),
                  (unsigned long long)sk_key(sk_float((acc[j] >> 16) << 16), 0xFFFFu - (acc[j] & 0xFFFFu)));
  }
  template <bool PARTIAL>
  __device__ void s_apply(int row, int col, f32x4 v0, f32x4 v1, const SPre&) {
    if (PARTIAL && row >= M) return;
    if (cur_f < 0 || row >= cur_base + T) {   // (a lane's rows ascend within a block)
      flush(col);
      cur_f = row / T;
      cur_base = cur_f * T;
      cur_len = search_len(lengths, cur_f, T);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0;
    }
    const int fr = row - cur_base;
    if (fr >= cur_len) return;
    const uint32_t lo = 0xFFFFu - (uint32_t)fr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cv = fmaxf((j < 4 ? v0[j] : v1[j - 4]) + b[j], 0.f);
      const uint32_t bits = (uint32_t)__builtin_bit_cast(unsigned short, (bf16_t)cv) & 0x7FFFu;
      const uint32_t kk = (bits << 16) | lo;
      acc[j] = kk > acc[j] ? kk : acc[j];
    }
  }
  __device__ void s_tile_end(int, int col) {
    const int lane = threadIdx.x & 63;
    const int f0 = __shfl(cur_f, 0);
    if (__all(cur_f == f0)) {
      if (f0 >= 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int m = 8; m < 64; m <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)acc[j], m);
            acc[j] = o > acc[j] ? o : acc[j];
          }
        }
        if (lane < 8) flush(col);
      }
    } else {
      flush(col);
    }
    cur_f = -1;
  }
  __device__ void s_end(float*) {}
};

// Merge of one batch of file keys into the running per-latent top-N table (rank keys / frames, [n_top][ncols]: latent-minor, so
// that the threads of a wave touch consecutive words).  One thread per latent walks the batch's files in order.
__global__ __launch_bounds__(256) void search_merge_kernel(const uint64_t* __restrict__ fk, const uint64_t* __restrict__ aux, int64_t n_files,
                                                           int64_t ncols, int64_t file0, int n_top, int flags, double mn, double mx,
                                                           uint64_t* __restrict__ top, int32_t* __restrict__ frames) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols) return;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t o = f * ncols + j;
    sk_merge_file(top + j, frames + j, ncols, n_top, fk[o], aux ? aux + o : nullptr, flags, mn, mx, file0 + f);
  }
}

// return_max_per_file (activations.py:111-117): the per-file value (the signed one in abs mode) of chosen latents,
// out[l out_stride + file0 + f].
__global__ __launch_bounds__(256) void search_values_kernel(const uint64_t* __restrict__ fk, const uint64_t* __restrict__ aux, int64_t n_files,
                                                            int64_t ncols, int flags, const int* __restrict__ latents, int64_t n_lat,
                                                            int64_t file0, int64_t out_stride, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_lat * n_files) return;
  const int64_t l = i / n_files, f = i - l * n_files;
  const int j = latents[l];
  if (j < 0 || j >= ncols) return;
  const int64_t o = f * ncols + j;
  out[l * out_stride + file0 + f] = sk_candidate(fk[o], aux ? aux + o : nullptr, flags).filt;
}
