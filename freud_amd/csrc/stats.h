// Feature statistics (include/freud_sae.h, sae_stats_files): per latent the number of frames where it is active (> 0), the sum
// and sum of squares of its value, its maximum, and per frame the number of active latents (the L0 histogram), in one pass over
// a batch of files.  The latent is encode()'s: the bf16 L1 latent of the training kernels, or the scatter of the TopK selection.
//
// Determinism: every float sum is a fixed-order fp32 partial per (row block, latent) -- a SLAB row, written with plain stores --
// and stats_fold_kernel adds a batch's slab rows in row-block order into the fp64 running totals, one thread per latent.  Counts
// and the L0 histogram are integers (atomics there do not depend on order), maxima are maxima of non-negative bf16 bit patterns.
//
// "Active" compares the MAGNITUDE bits of the bf16 latent (bits & 0x7FFF != 0): a -0.0 left by max(x, 0) is not active.
#pragma once
#include "common.h"
#include "search.h"      // search_len: the trimmed length of a file

constexpr int STATS_RB = 128;        // rows per slab row of the L1 paths (the streaming GEMM's wave block)
constexpr int STATS_TK_RB = 256;     // rows per slab row of the TopK path
constexpr int STATS_TK_SEG = 4096;   // latents per LDS segment of the TopK column kernel (4 x 16 KiB)
constexpr int STATS_HIST_LDS = 8192; // L0 bins privatised in LDS by stats_l0_kernel; larger L0s go straight to the global histogram

struct StatsSlab {                   // [nrb][n] each
  uint32_t* cnt;
  uint32_t* mx;                      // bf16 bit patterns (>= 0: ordered as the values)
  float* sum;
  float* sq;
};

__device__ __forceinline__ uint32_t stats_mag(float cv) {
  return (uint32_t)__builtin_bit_cast(unsigned short, (bf16_t)cv) & 0x7FFFu;
}
// row / T without an integer division: a float estimate, corrected by one step either way -- exact while the estimate is within
// 1 of the quotient, which holds for quotients below 2^16 (files per batch: at most 65535, search_shape_check)
__device__ __forceinline__ int stats_file_of(int row, int T, float inv_T) {
  int f = (int)((float)row * inv_T);
  const int base = f * T;
  f += row >= base + T ? 1 : 0;
  f -= row < base ? 1 : 0;
  return f;
}
__device__ __forceinline__ float stats_val(uint32_t mag) { return __uint_as_float(mag << 16); }

// L1 statistics epilogue of the streaming encoder GEMM (gemm256s.h's s_* interface): EpiEnc's arithmetic to the bf16 latent
// (fmaxf(bf16(acc) + b, 0), then bf16), reduced on the fly and never stored.  Lane l owns columns col .. col + 7 and 16 rows of its
// wave's 128 x 64 block (gemm256s.h).  Per column it keeps count / sum / sum of squares / max over its rows; s_tile_end folds the
// 8 row groups (lanes l ^ 8, ^ 16, ^ 32) as a reduce-scatter -- afterwards every lane holds ONE column of the 64 -- and writes the
// slab row of the wave's 128-row block.  Per row, the 8 lanes of the row add their active counts (three DPP steps) and store one
// byte per (row, 64-column tile): l0b[row][col / 64], summed per row by stats_l0_kernel.  Rows beyond the trimmed length of their
// file count nowhere (the L0 kernel skips them as well); rows >= M store a 0 byte.  Per lane: 217 VGPRs, no VGPR spill (EpiSearch: 222).
struct EpiStats {
  static constexpr bool STREAM = true;
  const float* bias;       // [n_p]
  StatsSlab slab;          // [M_p / 128][n]
  uint8_t* l0b;            // [M_p][n_p / 64]
  const int* lengths;      // [n_files] or null
  int64_t M;               // n_files T
  int T, n, ncb;           // ncb = n_p / 64
  float inv_T;             // 1 / T (the file of a row without an integer division: stats_file_of)
  struct SPre {};
  float b[8];
  uint32_t cmask;          // bit j: column col + j < n
  typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
  uint32_t cnt2[4];        // two 16-bit counts per word: columns 2 p, 2 p + 1 (a lane counts at most 16 rows per tile)
  u16x2 mx2[4];            // the same pairs of maxima (bf16 magnitudes, 15 bits)
  uint32_t cnt[8], mx[8];  // (unpacked for the fold at the end of a tile)
  float sum[8], sq[8];
  uint32_t vmask;          // bit 4 i + q: the lane's row row0 + 32 i + 8 q + lane / 8 of this tile counts (< M, within its file's length)
  int row0_;
  __device__ void zero() {     // (at the start and after each tile's stores: zeroing in s_tile kept 32 registers live over the
#pragma unroll                //  last K tile, and the kernel spilled)
    for (int j = 0; j < 8; ++j) sum[j] = sq[j] = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) { cnt2[p] = 0; mx2[p] = u16x2{0, 0}; }
  }
  __device__ void s_begin() { zero(); }
  __device__ int64_t s_rows() const { return M; }
  __device__ void s_tile(int row0, int col) {
    // the row mask: loads of the lengths and arithmetic under the last K tile's MFMAs, so that s_apply has no branch (a branch
    // there, or this loop unrolled, pushed the kernel over 256 registers)
    row0_ = row0;
    const int rr = (threadIdx.x & 63) >> 3;
    uint32_t vm = 0;
#pragma unroll 1
    for (int t = 0; t < 16; ++t) {
      const int row = row0 + 8 * t + rr;
      bool ok = row < M;
      if (lengths) {
        const int rc = ok ? row : (int)M - 1;
        const int f = stats_file_of(rc, T, inv_T);
        ok = ok && rc - f * T < search_len(lengths, f, T);
      }
      vm |= (ok ? 1u : 0u) << t;
    }
    vmask = vm;
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bias + col), b1 = *reinterpret_cast<const f32x4*>(bias + col + 4);
    cmask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { b[j] = b0[j]; b[4 + j] = b1[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) cmask |= (col + j < n ? 1u : 0u) << j;
  }
  __device__ SPre s_prefetch(int, int) const { return SPre{}; }
  template <bool PARTIAL>
  __device__ void s_apply(int row, int col, f32x4 v0, f32x4 v1, const SPre&) {
    const uint32_t m = ((vmask >> ((row - row0_) >> 3)) & 1u) ? cmask : 0u;
    uint32_t rc = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      uint32_t mg[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * p + h;
        const float cv = fmaxf((j < 4 ? v0[j] : v1[j - 4]) + b[j], 0.f);
        mg[h] = ((m >> j) & 1u) ? stats_mag(cv) : 0u;
        const float a = stats_val(mg[h]);
        sum[j] += a;
        sq[j] = fmaf(a, a, sq[j]);
      }
      const uint32_t act = (mg[0] != 0u ? 1u : 0u) | (mg[1] != 0u ? 0x10000u : 0u);
      cnt2[p] += act;
      rc += act;
      mx2[p] = __builtin_elementwise_max(mx2[p], u16x2{(unsigned short)mg[0], (unsigned short)mg[1]});
    }
    rc = (rc & 0xFFFFu) + (rc >> 16);
    // the row's 64 columns: the 8 lanes rr * 8 .. + 7 (quad swaps, then the other quad of the 8 via row_half_mirror)
    int r = (int)rc;
    r += __builtin_amdgcn_update_dpp(r, r, 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]
    r += __builtin_amdgcn_update_dpp(r, r, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
    r += __builtin_amdgcn_update_dpp(r, r, 0x141, 0xF, 0xF, false);    // row_half_mirror
    // (no lane predicate: the 8 lanes store the same byte to the same address; rows < M_p are inside the buffer)
    l0b[(int64_t)row * ncb + (col >> 6)] = (uint8_t)r;
  }
  // one step of the reduce-scatter: lanes with `mask` set keep slots H .. 2H - 1, the others 0 .. H - 1; both add their partner's
  template <int H, int MASK>
  __device__ __forceinline__ void fold_step(bool up) {
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const uint32_t c_send = up ? cnt[j] : cnt[j + H], c_keep = up ? cnt[j + H] : cnt[j];
      const uint32_t m_send = up ? mx[j] : mx[j + H], m_keep = up ? mx[j + H] : mx[j];
      const float s_send = up ? sum[j] : sum[j + H], s_keep = up ? sum[j + H] : sum[j];
      const float q_send = up ? sq[j] : sq[j + H], q_keep = up ? sq[j + H] : sq[j];
      const uint32_t c_o = (uint32_t)__shfl_xor((int)c_send, MASK, 64), m_o = (uint32_t)__shfl_xor((int)m_send, MASK, 64);
      const float s_o = __shfl_xor(s_send, MASK, 64), q_o = __shfl_xor(q_send, MASK, 64);
      cnt[j] = c_keep + c_o;
      mx[j] = m_keep > m_o ? m_keep : m_o;
      sum[j] = s_keep + s_o;
      sq[j] = q_keep + q_o;
    }
  }
  __device__ void s_tile_end(int row_w, int col) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      cnt[2 * p] = cnt2[p] & 0xFFFFu;
      cnt[2 * p + 1] = cnt2[p] >> 16;
      mx[2 * p] = mx2[p][0];
      mx[2 * p + 1] = mx2[p][1];
    }
    fold_step<4, 32>((lane & 32) != 0);
    fold_step<2, 16>((lane & 16) != 0);
    fold_step<1, 8>((lane & 8) != 0);
    // (lane >> 3: bit 2 = the lane kept columns 4-7 at the first step, bit 1 the upper pair at the second, bit 0 the odd one)
    const int c = col + ((lane >> 3) & 7);
    if (c < n) {
      const int64_t o = (int64_t)(row_w / STATS_RB) * n + c;
      slab.cnt[o] = cnt[0];
      slab.mx[o] = mx[0];
      slab.sum[o] = sum[0];
      slab.sq[o] = sq[0];
    }
    zero();
  }
  __device__ void s_end(float*) {}
};

// Unfused L1 path: column statistics of the stored bf16 latent [M_p][ld] -- grid (column blocks of 256, 128-row blocks); each
// thread walks its column's rows of the block in order.
__global__ __launch_bounds__(256) void stats_colreduce_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t M, int T,
                                                              const int* __restrict__ lengths, StatsSlab slab) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= n) return;
  const int64_t r0 = (int64_t)blockIdx.y * STATS_RB;
  const int64_t r1 = r0 + STATS_RB < M ? r0 + STATS_RB : M;
  uint32_t cnt = 0, mx = 0;
  float sum = 0.f, sq = 0.f;
  int64_t base = -1;
  int len = T;
  for (int64_t r = r0; r < r1; ++r) {
    if (lengths) {
      if (base < 0 || r >= base + T) {
        const int64_t f = r / T;
        base = f * T;
        len = search_len(lengths, (int)f, T);
      }
      if (r - base >= len) continue;
    }
    const uint32_t mag = lat[r * ld + col] & 0x7FFFu;
    const float a = stats_val(mag);
    cnt += mag != 0u ? 1u : 0u;
    sum += a;
    sq = fmaf(a, a, sq);
    mx = mag > mx ? mag : mx;
  }
  const int64_t o = (int64_t)blockIdx.y * n + col;
  slab.cnt[o] = cnt;
  slab.mx[o] = mx;
  slab.sum[o] = sum;
  slab.sq[o] = sq;
}

// TopK: column statistics of the selection (idx / vals [M][k]).  One wave per (block of STATS_TK_RB rows, segment of STATS_TK_SEG
// latents) walks its rows IN ORDER and adds each selected value of its segment to LDS accumulators: the indices of one row are
// distinct, so the lanes of one step never meet, and the LDS operations of a wave execute in program order -- the fp32 partials do
// not depend on timing.  The segment's accumulators are then written to its slab row with plain stores.
__global__ __launch_bounds__(64) void stats_topk_cols_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals, int k,
                                                             int64_t M, int T, const int* __restrict__ lengths, int n, StatsSlab slab) {
  __shared__ uint32_t l_cnt[STATS_TK_SEG], l_mx[STATS_TK_SEG];
  __shared__ float l_sum[STATS_TK_SEG], l_sq[STATS_TK_SEG];
  const int lane = threadIdx.x;
  const int seg0 = blockIdx.y * STATS_TK_SEG, segn = min(STATS_TK_SEG, n - seg0);
  for (int i = lane; i < segn; i += 64) { l_cnt[i] = 0; l_mx[i] = 0; l_sum[i] = 0.f; l_sq[i] = 0.f; }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * STATS_TK_RB;
  const int64_t r1 = r0 + STATS_TK_RB < M ? r0 + STATS_TK_RB : M;
  for (int64_t r = r0; r < r1; ++r) {
    if (lengths) {
      const int64_t f = r / T;
      if (r - f * T >= search_len(lengths, (int)f, T)) continue;     // (uniform over the wave)
    }
    for (int s = lane; s < k; s += 64) {
      const int j = idx[r * k + s] - seg0;
      const uint32_t mag = vals[r * k + s] & 0x7FFFu;
      if (j >= 0 && j < segn && mag != 0u) {
        const float a = stats_val(mag);
        l_cnt[j] += 1u;
        l_sum[j] += a;
        l_sq[j] = fmaf(a, a, l_sq[j]);
        l_mx[j] = mag > l_mx[j] ? mag : l_mx[j];
      }
    }
  }
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.x * n + seg0;
  for (int i = lane; i < segn; i += 64) {
    slab.cnt[o + i] = l_cnt[i];
    slab.mx[o + i] = l_mx[i];
    slab.sum[o + i] = l_sum[i];
    slab.sq[o + i] = l_sq[i];
  }
}

// Per-row active counts, one wave per row.  Sources: the bytes of EpiStats, the stored L1 latent, the TopK selection.
struct L0Bytes {
  const uint8_t* b;
  int ncb;
  __device__ uint32_t lane_count(int64_t r, int lane) const {
    uint32_t s = 0;
    for (int i = lane; i < ncb; i += 64) s += b[r * ncb + i];
    return s;
  }
};
struct L0Latent {              // [M_p][ld] bf16 bit patterns, ld a multiple of 8
  const unsigned short* c;
  int64_t ld;
  int n;
  __device__ uint32_t lane_count(int64_t r, int lane) const {
    uint32_t s = 0;
    for (int j0 = 8 * lane; j0 < n; j0 += 512) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(c + r * ld + j0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s += ((w[e] & 0x7FFFu) != 0u && j0 + 2 * e < n) ? 1u : 0u;
        s += ((w[e] & 0x7FFF0000u) != 0u && j0 + 2 * e + 1 < n) ? 1u : 0u;
      }
    }
    return s;
  }
};
struct L0Topk {
  const unsigned short* vals;  // [M][k]
  int k;
  __device__ uint32_t lane_count(int64_t r, int lane) const {
    uint32_t s = 0;
    for (int i = lane; i < k; i += 64) s += (vals[r * k + i] & 0x7FFFu) != 0u ? 1u : 0u;
    return s;
  }
};

// l0_hist[i] += number of counted rows with i active latents; n_frames += counted rows.  The histogram's first STATS_HIST_LDS bins
// are privatised in LDS and flushed once per block (one global atomic per non-empty bin); L0s above go to the global bins directly.
template <class Src>
__global__ __launch_bounds__(256) void stats_l0_kernel(Src src, int64_t M, int T, const int* __restrict__ lengths, int nbins,
                                                       unsigned long long* __restrict__ hist, unsigned long long* __restrict__ n_frames) {
  __shared__ uint32_t h[STATS_HIST_LDS];
  __shared__ uint32_t frames;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int hb = nbins < STATS_HIST_LDS ? nbins : STATS_HIST_LDS;
  for (int i = threadIdx.x; i < hb; i += 256) h[i] = 0;
  if (threadIdx.x == 0) frames = 0;
  __syncthreads();
  uint32_t my_frames = 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < M; r += (int64_t)gridDim.x * 4) {
    if (lengths) {
      const int64_t f = r / T;
      if (r - f * T >= search_len(lengths, (int)f, T)) continue;     // (uniform over the wave)
    }
    uint32_t s = src.lane_count(r, lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
    if (lane == 0) {
      if ((int)s < hb) atomicAdd(&h[s], 1u);
      else atomicAdd(hist + s, 1ull);
      ++my_frames;
    }
  }
  if (lane == 0 && my_frames) atomicAdd(&frames, my_frames);
  __syncthreads();
  for (int i = threadIdx.x; i < hb; i += 256)
    if (h[i]) atomicAdd(hist + i, (unsigned long long)h[i]);
  if (threadIdx.x == 0 && frames) atomicAdd(n_frames, (unsigned long long)frames);
}

// Fold of a batch's slab rows [nrb][n] into the running totals, one thread per latent, row blocks in order.
__global__ __launch_bounds__(256) void stats_fold_kernel(StatsSlab slab, int nrb, int n, unsigned long long* __restrict__ fire,
                                                         double* __restrict__ asum, double* __restrict__ asq, float* __restrict__ amax) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  unsigned long long c = 0;
  uint32_t m = 0;
  double s = 0.0, q = 0.0;
  for (int rb = 0; rb < nrb; ++rb) {
    const int64_t o = (int64_t)rb * n + j;
    c += slab.cnt[o];
    s += (double)slab.sum[o];
    q += (double)slab.sq[o];
    m = slab.mx[o] > m ? slab.mx[o] : m;
  }
  fire[j] += c;
  asum[j] += s;
  asq[j] += q;
  amax[j] = fmaxf(amax[j], stats_val(m));
}
