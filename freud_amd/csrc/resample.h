// Dead-latent resampling for L1 training (include/freud_sae.h, sae_resample_*): the kernels of the rule in resample_draw.h.
//
//   sae_resample_files   after the encoder (stored latent), the count reduction of stats.h, the decode and the residual sweep of
//                        recon.h: rs_fire_fold_kernel adds the batch's firing counts, rs_rowloss_kernel folds the sweep's row partials
//   sae_resample_select  rs_max_kernel (l_max), rs_blocksum_kernel / rs_blockscan_kernel / rs_prefix_kernel (the uint64 prefix: blocks
//                        of RS_SCAN_ROWS rows, their sums scanned by one workgroup whose carry crosses its chunks), rs_dead_kernel (the
//                        dead latents in order), rs_draw_kernel (hash, search, owner), rs_emit_kernel (the owning pairs in order)
//   sae_resample_apply   rs_apply_kernel: one workgroup per pair rewrites its column of W, b and both moments
//
// Determinism: the only float sum is the fixed-order fp32 sum of a row's partials; everything else is integer.  The atomics are an
// integer maximum (l_max), an integer minimum (the owner word) and integer adds of the apply counters: none returns a value, none
// depends on order.  The selection's outputs come out in ascending latent order from single-workgroup compactions.
#pragma once
#include "common.h"
#include "resample_draw.h"

constexpr int RS_SCAN_ROWS = 256;        // rows per workgroup of the prefix (one per thread)
constexpr int RS_HDR_BYTES = 64;         // the head of the workspace: RsHeader

struct RsHeader {                        // zeroed by the call
  uint32_t lmax_bits;
  uint32_t n_dead;
  unsigned long long total;
};

// l_i = the fp32 sum, chunks ascending, of the sum-r^2 partials of row i (recon_resid_kernel wrote 0 on rows that do not count)
__global__ __launch_bounds__(256) void rs_rowloss_kernel(const float* __restrict__ rowpart, int nch, int64_t M, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  float s = 0.f;
  for (int ch = 0; ch < nch; ++ch) s = __fadd_rn(s, rowpart[(i * nch + ch) * 2]);
  out[i] = s;
}

// fire[j] += the batch's counts of latent j: the slab rows of stats_colreduce_kernel in row-block order
__global__ __launch_bounds__(256) void rs_fire_fold_kernel(const uint32_t* __restrict__ cnt, int nrb, int n, unsigned long long* __restrict__ fire) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  unsigned long long c = 0;
  for (int rb = 0; rb < nrb; ++rb) c += cnt[(int64_t)rb * n + j];
  fire[j] += c;
}

__global__ __launch_bounds__(256) void rs_max_kernel(const uint32_t* __restrict__ loss_bits, int64_t rows, RsHeader* __restrict__ hdr) {
  __shared__ uint32_t red[4];
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256) {
    const uint32_t b = rs_loss_bits(loss_bits[i]);
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)m, o, 64);
    m = other > m ? other : m;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    if (m) atomicMax(&hdr->lmax_bits, m);
  }
}

// blocksum[b] = the sum of the weights of rows [b RS_SCAN_ROWS, ...)
__global__ __launch_bounds__(RS_SCAN_ROWS) void rs_blocksum_kernel(const uint32_t* __restrict__ loss_bits, int64_t rows,
                                                                   const RsHeader* __restrict__ hdr, unsigned long long* __restrict__ blocksum) {
  __shared__ unsigned long long buf[RS_SCAN_ROWS];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * RS_SCAN_ROWS + t;
  const int e = rs_frexp_exp(hdr->lmax_bits);
  buf[t] = i < rows ? rs_weight(loss_bits[i], e) : 0ull;
  __syncthreads();
  for (int o = RS_SCAN_ROWS / 2; o > 0; o >>= 1) {
    if (t < o) buf[t] += buf[t + o];
    __syncthreads();
  }
  if (t == 0) blocksum[blockIdx.x] = buf[0];
}

// the inclusive scan of a workgroup's RS_SCAN_ROWS words through LDS (Hillis-Steele, two buffers); every thread calls it
__device__ __forceinline__ unsigned long long rs_scan_incl(unsigned long long v, unsigned long long (*buf)[RS_SCAN_ROWS]) {
  const int t = threadIdx.x;
  int cur = 0;
  buf[0][t] = v;
  __syncthreads();
  for (int o = 1; o < RS_SCAN_ROWS; o <<= 1) {
    const unsigned long long s = buf[cur][t] + (t >= o ? buf[cur][t - o] : 0ull);
    buf[cur ^ 1][t] = s;
    __syncthreads();
    cur ^= 1;
  }
  const unsigned long long r = buf[cur][t];
  __syncthreads();
  return r;
}

// one workgroup: blocksum -> its exclusive prefix, in place, chunk after chunk with the carry of the chunks before; total -> header
__global__ __launch_bounds__(RS_SCAN_ROWS) void rs_blockscan_kernel(unsigned long long* __restrict__ blocksum, int64_t nblk,
                                                                    RsHeader* __restrict__ hdr) {
  __shared__ unsigned long long buf[2][RS_SCAN_ROWS];
  const int t = threadIdx.x;
  unsigned long long carry = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += RS_SCAN_ROWS) {
    const int64_t b = b0 + t;
    const unsigned long long v = b < nblk ? blocksum[b] : 0ull;
    const unsigned long long incl = rs_scan_incl(v, buf);
    if (b < nblk) blocksum[b] = carry + incl - v;
    // (the chunk's sum: the last thread's inclusive word, read by all through LDS)
    if (t == RS_SCAN_ROWS - 1) buf[0][0] = incl;
    __syncthreads();
    carry += buf[0][0];
    __syncthreads();
  }
  if (t == 0) hdr->total = carry;
}

// c[i] = the inclusive prefix of the weights
__global__ __launch_bounds__(RS_SCAN_ROWS) void rs_prefix_kernel(const uint32_t* __restrict__ loss_bits, int64_t rows,
                                                                 const RsHeader* __restrict__ hdr,
                                                                 const unsigned long long* __restrict__ block_off,
                                                                 unsigned long long* __restrict__ c) {
  __shared__ unsigned long long buf[2][RS_SCAN_ROWS];
  const int64_t i = (int64_t)blockIdx.x * RS_SCAN_ROWS + threadIdx.x;
  const int e = rs_frexp_exp(hdr->lmax_bits);
  const unsigned long long w = i < rows ? rs_weight(loss_bits[i], e) : 0ull;
  const unsigned long long incl = rs_scan_incl(w, buf);
  if (i < rows) c[i] = block_off[blockIdx.x] + incl;
}

// the position of a flagged thread among the flagged threads of its workgroup of 256, and their number; every thread calls it
__device__ __forceinline__ uint32_t rs_block_rank(bool flag, uint32_t* wsum /* LDS [4] */, uint32_t* n_flagged) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const uint32_t pre = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int k = 0; k < 4; ++k) {
    off += k < w ? wsum[k] : 0u;
    tot += wsum[k];
  }
  __syncthreads();
  *n_flagged = tot;
  return off + pre;
}

// one workgroup: dead[r] = the r-th latent j < n with fire[j] == 0; their number -> header
__global__ __launch_bounds__(256) void rs_dead_kernel(const unsigned long long* __restrict__ fire, int n, int* __restrict__ dead,
                                                      RsHeader* __restrict__ hdr) {
  __shared__ uint32_t wsum[4];
  uint32_t base = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    const bool is_dead = j < n && fire[j] == 0ull;
    uint32_t cnt;
    const uint32_t rank = rs_block_rank(is_dead, wsum, &cnt);
    if (is_dead) dead[base + rank] = j;
    base += cnt;
  }
  if (threadIdx.x == 0) hdr->n_dead = base;
}

// draw[r] = the row dead latent r draws; owner[row] = the lowest r that drew it (owner starts at 0xFFFFFFFF)
__global__ __launch_bounds__(256) void rs_draw_kernel(const RsHeader* __restrict__ hdr, const unsigned long long* __restrict__ c, int64_t rows,
                                                      unsigned long long seed, unsigned long long round, int* __restrict__ draw,
                                                      uint32_t* __restrict__ owner) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long total = hdr->total;
  if (r >= hdr->n_dead || total == 0ull) return;
  int64_t row = rs_draw(reinterpret_cast<const uint64_t*>(c), rows, (uint64_t)total, (uint64_t)seed, (uint64_t)round, (uint64_t)r);
  row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);
  draw[r] = (int)row;
  atomicMin(&owner[row], r);
}

// one workgroup: the pairs whose latent owns its row, in ascending r; the counts
__global__ __launch_bounds__(256) void rs_emit_kernel(const RsHeader* __restrict__ hdr, const int* __restrict__ dead, const int* __restrict__ draw,
                                                      const uint32_t* __restrict__ owner, int* __restrict__ latents_out,
                                                      long long* __restrict__ rows_out, long long* __restrict__ counts) {
  __shared__ uint32_t wsum[4];
  const uint32_t nd = hdr->n_dead;
  const bool any = hdr->total != 0ull;
  uint32_t base = 0;
  if (any) {
    for (uint32_t r0 = 0; r0 < nd; r0 += 256) {
      const uint32_t r = r0 + threadIdx.x;
      const bool owns = r < nd && owner[draw[r]] == r;
      uint32_t cnt;
      const uint32_t rank = rs_block_rank(owns, wsum, &cnt);
      if (owns) {
        latents_out[base + rank] = dead[r];
        rows_out[base + rank] = (long long)draw[r];
      }
      base += cnt;
    }
  }
  if (threadIdx.x == 0) {
    counts[RS_DEAD] = (long long)nd;
    counts[RS_PAIRS] = (long long)base;
    counts[RS_SKIPPED_DUPLICATE] = any ? (long long)(nd - base) : 0ll;
    counts[RS_TOTAL] = (long long)hdr->total;
    counts[RS_LMAX_BITS] = (long long)hdr->lmax_bits;
    for (int i = RS_LMAX_BITS + 1; i < RS_NCOUNTS; ++i) counts[i] = 0ll;
  }
}

// ---- the column rewrite: workgroup i takes pair i -- latent j = latents[i], x = x_rows[i][0 .. d).  P, Mom, Var are the flat buffers
// [W [d_p][n_p] | b [n_p]].  A degenerate row (resample_draw.h) leaves the column as it is.  stats: [0] revived, [1] degenerate,
// [2 + i] = 1 iff pair i was applied (zeroed by the call).
__global__ __launch_bounds__(256) void rs_apply_kernel(const int* __restrict__ latents, const float* __restrict__ x_rows, int d, int d_p,
                                                       int n_p, float alpha, float* __restrict__ P, float* __restrict__ Mom,
                                                       float* __restrict__ Var, unsigned long long* __restrict__ stats) {
  __shared__ float s_sh;
  const int i = blockIdx.x, j = latents[i];
  const float* x = x_rows + (int64_t)i * d;
  if (threadIdx.x == 0) s_sh = rs_norm_sq(x, d);
  __syncthreads();
  const float s = s_sh;
  if (rs_degenerate(s)) {                                // (uniform over the workgroup)
    if (threadIdx.x == 0) atomicAdd(&stats[1], 1ull);
    return;
  }
  const float nrm = rs_norm(s);
  for (int k = threadIdx.x; k < d_p; k += 256) {
    const int64_t o = (int64_t)k * n_p + j;
    P[o] = k < d ? rs_unit(x[k], nrm) : 0.f;
    Mom[o] = 0.f;
    Var[o] = 0.f;
  }
  if (threadIdx.x == 0) {
    const int64_t o = (int64_t)d_p * n_p + j;
    P[o] = rs_bias(alpha, nrm);
    Mom[o] = 0.f;
    Var[o] = 0.f;
    atomicAdd(&stats[0], 1ull);
    stats[2 + i] = 1ull;
  }
}
