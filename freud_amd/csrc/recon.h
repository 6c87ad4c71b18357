// Reconstruction report (include/freud_sae.h, sae_recon_files): how well the dictionary reconstructs a batch of files -- the
// residual r = x - x_hat per frame, its energy per file and per model dimension -- and what every latent is worth to that
// reconstruction.  Both decoders are linear in the latent, so zeroing latent j changes a frame's squared error by
// 2 a_j (r . w_j) + a_j^2 |w_j|^2: the pass accumulates P_j = sum a_j (r . w_j) and sum a_j^2 over the counted frames and leaves
// |w_j|^2 beside them.  The latent is encode()'s, x_hat the decode of exactly that latent (sae_decode's GEMM for L1, the sparse
// fp32 decode of manip.h for TopK).
//
// Kernels: the residual sweep (both variants), EpiAttr (L1: P for all latents as the epilogue of the backward's dpre-shaped GEMM
// r_b [M_p][d_p] x Wt [n_p][d_p] in all three GEMM kernels, nothing of size M x n is stored), the TopK pair (one dot per selected slot with r in registers,
// then the column walk of stats_topk_cols_kernel), the decoder norms and the fold.
//
// Determinism: every float sum is a fixed-order fp32 partial written with plain stores -- per (row, 64 columns) for the row
// energies, per (128-row block, column) for the model dimensions and the L1 latents, per (256-row block, latent) for TopK -- and
// recon_fold_kernel adds a batch's partials in a fixed order into fp64.  The only atomic is the integer frame count.
#pragma once
#include "common.h"
#include "stats.h"       // stats_file_of, stats_val, the row blocks of the slabs

constexpr int RC_CW = 64;            // columns of x per workgroup of the residual sweep (one lane each)

// does `row` count: below M and within the trimmed length of its file (the file without an integer division: stats_file_of)
__device__ __forceinline__ bool recon_row_counts(int64_t row, int64_t M, int T, float inv_T, const int* lengths) {
  if (row >= M) return false;
  if (!lengths) return true;
  const int f = stats_file_of((int)row, T, inv_T);
  return (int)row - f * T < search_len(lengths, f, T);
}

// ---- the residual sweep.  Grid (128-row blocks, d_p / 64 column chunks), 4 waves: wave w takes rows r0 + 4 i + w, lane l column
// 64 chunk + l.  xr holds x_hat [M][d] on entry and r on exit (r = 0 on rows that do not count); r = float(x) - x_hat is ONE fp32
// subtraction on the delivered x.
//   rb      [M_p][d_p] bf16 (or null): the GEMM operand r_b = bf16(r), zero in the padding columns and on rows that do not count;
//           the grid covers M_p rows then
//   resid   [M][d] (or null): a copy of r for the caller
//   lat     [M_p][n_p] bf16 (or null): the stored L1 latent; its rows < M that do not count are ZEROED (chunk 0's waves), so that
//           the attribution epilogue needs no row mask
//   rowpart [M][nch][2]: sum of r^2 and of x^2 over the row's 64 columns of this chunk (0 on rows that do not count)
//   dimpart [row blocks][3][d_p]: per column the sums of x, x^2 and r^2 over the block's 128 rows -- per wave over its 32 rows in
//           order, then the four waves in order
template <typename T>
__global__ __launch_bounds__(256) void recon_resid_kernel(const T* __restrict__ x, float* __restrict__ xr, float* __restrict__ resid,
                                                          bf16_t* __restrict__ rb, bf16_t* __restrict__ lat, int n_p, int64_t M, int Trows,
                                                          float inv_T, const int* __restrict__ lengths, int d, int d_p,
                                                          float* __restrict__ rowpart, float* __restrict__ dimpart) {
  __shared__ float red[4][3][RC_CW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int chunk = blockIdx.y, nch = gridDim.y;
  const int col = chunk * RC_CW + lane;
  const int64_t r0 = (int64_t)blockIdx.x * STATS_RB;
  float sx = 0.f, sxx = 0.f, srr = 0.f;
  for (int i = 0; i < STATS_RB / 4; ++i) {
    const int64_t row = r0 + 4 * i + w;                                        // (wave-uniform)
    const bool counted = recon_row_counts(row, M, Trows, inv_T, lengths);
    float xv = 0.f, r = 0.f;
    if (counted && col < d) {
      xv = load_as_float(x + row * d + col);
      r = __fsub_rn(xv, xr[row * d + col]);
    }
    if (row < M && col < d) {
      xr[row * d + col] = r;
      if (resid) resid[row * d + col] = r;
    }
    if (rb) rb[row * d_p + col] = (bf16_t)r;
    sx += xv;
    sxx = fmaf(xv, xv, sxx);
    srr = fmaf(r, r, srr);
    if (row < M) {
      const float rr = wave_sum(r * r), xx = wave_sum(xv * xv);
      if (lane == 0) {
        rowpart[(row * nch + chunk) * 2] = rr;
        rowpart[(row * nch + chunk) * 2 + 1] = xx;
      }
      if (lat && chunk == 0 && !counted)
        for (int j = 8 * lane; j < n_p; j += 512) *reinterpret_cast<u32x4*>(lat + row * n_p + j) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  red[w][0][lane] = sx;
  red[w][1][lane] = sxx;
  red[w][2][lane] = srr;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      dimpart[((int64_t)blockIdx.x * 3 + q) * d_p + col] = ((red[0][q][lane] + red[1][q][lane]) + red[2][q][lane]) + red[3][q][lane];
  }
}

// ---- L1 attribution: epilogue of the tile GEMMs (gemm.h, gemm256.h) over A = r_b, B = Wt.  v = r_b . w_j as the MFMA accumulated it
// in fp32 -- NOT rounded to bf16 (no ROUNDS_BF16_FIRST: the tile reaches the functor through fp32 LDS).  A thread owns 4 columns and
// 16 rows of a 128 x 128 sub-tile; per column it adds a v (one fp32 product, then the add) and a^2 over its rows, tile_end folds the
// 8 row groups through LDS in order and writes the slab row of the 128-row block.  The latent tile is prefetched as in EpiDpre.
// Rows that do not count carry a = 0 (rows >= M: EpiEnc; the others: recon_resid_kernel), so there is no mask here.
// Registers: the 256 x 256 kernel is at its 256-register limit with ANY functor.  What keeps this one out of scratch there:
//   * the row index of prefetch() is opaque to the optimiser -- otherwise the sixteen 64-bit latent addresses of a thread are
//     hoisted out of gemm256.h's loop over the two column passes (32 registers live across the whole epilogue: 29 spilled);
//   * the slab position is one 32-bit index instead of a row tile and a column;
//   * NO_PERSIST: the instantiation whose workgroups walk several tiles carries the functor's state over its tile loop and
//     spilled 15 registers; launch_gemm starts one workgroup per tile for this functor instead.
struct EpiAttr {
  static constexpr int PREFETCH_BATCH = EPI_BATCH_HEAVY;
  static constexpr bool NO_PERSIST = true;
  const bf16_t* c;      // [M_p][n_p]
  float* slab_p;        // [M_p / 128][n_p]
  float* slab_q;        // [M_p / 128][n_p]
  int n_p;
  float ps[4], qs[4];
  int slab_o;            // index of the tile's first column in its slab row (slabs stay below 2^31 floats: the host checks)
  __device__ void tile_begin(int row0, int col0, int) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ps[j] = qs[j] = 0.f;
    slab_o = (row0 / GEMM_BM) * n_p + col0;
  }
  struct Pre { bf16x4 cv; };
  __device__ Pre prefetch(int row, int col) const {
    asm volatile("" : "+v"(row));
    return Pre{EPI_LOAD(reinterpret_cast<const bf16x4*>(c + (int64_t)row * n_p + col))};
  }
  __device__ void apply(int, int, f32x4 v, const Pre& pre) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = (float)pre.cv[j];
      ps[j] += __fmul_rn(a, v[j]);
      qs[j] = fmaf(a, a, qs[j]);
    }
  }
  __device__ void tile_end(float* scratch) {
    // thread t owns columns 4 (t & 31) .. of row group t >> 5: the 8 row groups through LDS, added in order
    const int t = threadIdx.x & 255;
    *reinterpret_cast<f32x4*>(scratch + (t >> 5) * 128 + (t & 31) * 4) = f32x4{ps[0], ps[1], ps[2], ps[3]};
    *reinterpret_cast<f32x4*>(scratch + 1024 + (t >> 5) * 128 + (t & 31) * 4) = f32x4{qs[0], qs[1], qs[2], qs[3]};
    lds_barrier();
    if (t < 128) {
      float sp = 0.f, sq = 0.f;
#pragma unroll
      for (int gidx = 0; gidx < 8; ++gidx) {
        sp += scratch[gidx * 128 + t];
        sq += scratch[1024 + gidx * 128 + t];
      }
      const int o = slab_o + t;
      slab_p[o] = sp;
      slab_q[o] = sq;
    }
  }

  // ---- streaming form (gemm256s.h).  The sum must see the UNROUNDED accumulators, so this is the fp32 epilogue of that kernel
  // (STREAM_F32, the TopK encoder's: one 32 x 32 block of the wave's 128 x 64 at a time through its 4 KiB of LDS), not the bf16 one
  // EpiDpre uses -- and that interface has no prefetch slot: the latent's 16 bytes per (row, 8 columns) are loaded inside s_apply,
  // where the unrolled epilogue lets the compiler issue them ahead as the accumulators retire.  Lane (rq = lane / 4, cp = lane % 4)
  // owns rows rq + 16 q + 32 i and columns 32 j + 8 cp .. + 7: 16 columns, 8 rows each.  The first element of a column ASSIGNS its
  // sums (e = 4 i + 2 j + q is a compile-time constant), so nothing is zeroed or kept live over the K loop.  s_tile_end folds the 16
  // row lanes of a column as a reduce-scatter in the fixed order lanes ^ 32, ^ 16, ^ 8, ^ 4 -- afterwards every lane holds ONE of the
  // wave's 64 columns -- and writes the slab row of the wave's 128-row block.  217 VGPRs, no scratch.
  static constexpr bool STREAM = true;
  static constexpr bool STREAM_F32 = true;
  struct SPre {};
  float sp[16], sq[16];
  __device__ void s_begin() {}
  __device__ int64_t s_rows() const { return (int64_t)1 << 62; }
  __device__ void s_tile(int, int) {}
  __device__ void s_apply(int e, int row, int col, f32x4 v0, f32x4 v1) {
    const int j = (e >> 1) & 1;
    const bool first = (e >> 2) == 0 && (e & 1) == 0;
    const u32x4 cw = EPI_LOAD(reinterpret_cast<const u32x4*>(c + (int64_t)row * n_p + col));
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float a = __uint_as_float((m & 1) ? (cw[m >> 1] & 0xFFFF0000u) : (cw[m >> 1] << 16));
      const float t = __fmul_rn(a, m < 4 ? v0[m] : v1[m - 4]);
      sp[8 * j + m] = first ? t : sp[8 * j + m] + t;
      sq[8 * j + m] = first ? __fmul_rn(a, a) : fmaf(a, a, sq[8 * j + m]);
    }
  }
  template <int H, int MASK>
  __device__ __forceinline__ void s_fold(bool up) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float p_send = up ? sp[i] : sp[i + H], p_keep = up ? sp[i + H] : sp[i];
      const float q_send = up ? sq[i] : sq[i + H], q_keep = up ? sq[i + H] : sq[i];
      sp[i] = p_keep + __shfl_xor(p_send, MASK, 64);
      sq[i] = q_keep + __shfl_xor(q_send, MASK, 64);
    }
  }
  __device__ void s_tile_end(int row_w, int col_w) {
    const int lane = threadIdx.x & 63;
    s_fold<8, 32>((lane & 32) != 0);
    s_fold<4, 16>((lane & 16) != 0);
    s_fold<2, 8>((lane & 8) != 0);
    s_fold<1, 4>((lane & 4) != 0);
    const int col = col_w + 32 * ((lane >> 5) & 1) + 8 * (lane & 3) + 4 * ((lane >> 4) & 1) + 2 * ((lane >> 3) & 1) + ((lane >> 2) & 1);
    const int64_t o = (int64_t)(row_w / STATS_RB) * n_p + col;
    slab_p[o] = sp[0];
    slab_q[o] = sq[0];
  }
  __device__ void s_end(float*) {}
};

// ---- TopK attribution, step 1: p[row][i] = a_i * (r . Wd[idx_i]) for the row's k slots.  One wave per row (4 per workgroup) in the
// access pattern of manip_topk_decode_kernel: lane l owns the d_p / 64 contiguous columns from l d_p / 64, r stays in its registers
// and every gathered row is one coalesced line.  The dot is fp32 fmaf over the lane's columns, then the wave's butterfly; a padding
// slot (index outside [0, n_p)) gives 0.  NPAIR > 0: d_p == 128 NPAIR at compile time.
template <int NPAIR>
__global__ __launch_bounds__(256) void recon_topk_attr_kernel(const float* __restrict__ r, const bf16_t* __restrict__ vals,
                                                              const int* __restrict__ idx, int k, const bf16_t* __restrict__ Wd,
                                                              float* __restrict__ p, int64_t M, int d, int d_p, int n_p) {
  constexpr int MAXP = NPAIR > 0 ? NPAIR : 12;   // column pairs per lane: d_p <= 64 * 2 * MAXP
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                          // (wave-uniform)
  const int npair = NPAIR > 0 ? NPAIR : d_p >> 7;
  const int c0 = lane * 2 * npair;
  float rv[2 * MAXP];
#pragma unroll
  for (int i = 0; i < 2 * MAXP; ++i) rv[i] = (i < 2 * npair && c0 + i < d) ? r[row * d + c0 + i] : 0.f;
  const int* ri = idx + row * k;
  const bf16_t* rva = vals + row * k;
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int jj = j0 + lane;
    const int my_i = jj < k ? ri[jj] : -1;
    const float my_a = jj < k ? (float)rva[jj] : 0.f;
    const int cnt = k - j0 < 64 ? k - j0 : 64;
    float mine = 0.f;
    for (int j = 0; j < cnt; ++j) {
      const int ii = __shfl(my_i, j, 64);
      float s = 0.f;
      if (ii >= 0 && ii < n_p) {                 // (wave-uniform)
        const unsigned* wr = reinterpret_cast<const unsigned*>(Wd + (int64_t)ii * d_p + c0);
#pragma unroll
        for (int q = 0; q < MAXP; ++q)
          if (q < npair) {
            const unsigned u = wr[q];
            s = fmaf(rv[2 * q], __uint_as_float(u << 16), s);
            s = fmaf(rv[2 * q + 1], __uint_as_float(u & 0xFFFF0000u), s);
          }
        s = wave_sum(s);
      }
      if (lane == j) mine = __fmul_rn(my_a, s);
    }
    if (jj < k) p[row * k + jj] = mine;
  }
}

// ---- TopK attribution, step 2: stats_topk_cols_kernel's walk -- one wave per (block of STATS_TK_RB rows, segment of STATS_TK_SEG
// latents) goes through its rows IN ORDER and adds p and a^2 of each selected latent of its segment to LDS accumulators (the
// indices of a row are distinct and a wave's LDS operations execute in program order), then writes its slab row.  A selected zero
// and a row that does not count add nothing.
__global__ __launch_bounds__(64) void recon_topk_cols_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals,
                                                             const float* __restrict__ p, int k, int64_t M, int T,
                                                             const int* __restrict__ lengths, int n, int ld, float* __restrict__ slab_p,
                                                             float* __restrict__ slab_q) {
  __shared__ float l_p[STATS_TK_SEG], l_q[STATS_TK_SEG];
  const int lane = threadIdx.x;
  const int seg0 = blockIdx.y * STATS_TK_SEG, segn = min(STATS_TK_SEG, n - seg0);
  for (int i = lane; i < segn; i += 64) { l_p[i] = 0.f; l_q[i] = 0.f; }
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
        const float a = __uint_as_float((uint32_t)vals[r * k + s] << 16);
        l_p[j] += p[r * k + s];
        l_q[j] = fmaf(a, a, l_q[j]);
      }
    }
  }
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.x * ld + seg0;
  for (int i = lane; i < segn; i += 64) {
    slab_p[o + i] = l_p[i];
    slab_q[o + i] = l_q[i];
  }
}

// ---- |w_j|^2 of the bf16 decoder operand: w_j[c] = W[j rs + c cs], c < d -- L1: Wb [d_p][n_p], rs = 1, cs = n_p; TopK: Wd_b
// [n_p][d_p], rs = d_p, cs = 1.  One thread per latent; the fp32 products of bf16 values are exact, the sum is fp64 in order.
__global__ __launch_bounds__(256) void recon_wnorm_kernel(const bf16_t* __restrict__ W, int64_t rs, int64_t cs, int d, int n,
                                                          float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const float w = (float)W[(int64_t)j * rs + (int64_t)c * cs];
    s += (double)(w * w);
  }
  out[j] = (float)s;
}

// ---- the fold of one batch into the caller's block.  Three kinds of workgroups:
//   [0, nb_lat)             one thread per latent: the slab rows in row-block order into attr_sum / act_sq_sum
//   [nb_lat, nb_lat+nb_dim) one thread per model dimension: the 128-row partials in order into sum_x / sum_x_sq / sum_r_sq
//   the rest                one wave per file: its counted rows' partials (row chunks in order, lane t takes rows t, t + 64, ..,
//                           then the butterfly) WRITTEN to file_out[f] = {sse, energy}; the frame count by an integer atomic
struct ReconOut {               // the caller's block (include/freud_sae.h, SAE_RECON_*)
  unsigned long long* n_frames;
  double *attr, *asq, *sx, *sxx, *srr;
  float* wnorm;
};

__global__ __launch_bounds__(256) void recon_fold_kernel(const float* __restrict__ slab_p, const float* __restrict__ slab_q, int nrb_lat,
                                                         int n, int ld, const float* __restrict__ dimpart, int nrb_dim, int d, int d_p,
                                                         const float* __restrict__ rowpart, int nch, int n_files, int T,
                                                         const int* __restrict__ lengths, ReconOut o, double* __restrict__ file_out,
                                                         int nb_lat, int nb_dim) {
  const int b = blockIdx.x;
  if (b < nb_lat) {
    const int j = b * 256 + threadIdx.x;
    if (j >= n) return;
    double sp = 0.0, sq = 0.0;
    for (int rb = 0; rb < nrb_lat; ++rb) {
      sp += (double)slab_p[(int64_t)rb * ld + j];
      sq += (double)slab_q[(int64_t)rb * ld + j];
    }
    o.attr[j] += sp;
    o.asq[j] += sq;
  } else if (b < nb_lat + nb_dim) {
    const int i = (b - nb_lat) * 256 + threadIdx.x;
    if (i >= d) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int rb = 0; rb < nrb_dim; ++rb) {
      s0 += (double)dimpart[((int64_t)rb * 3 + 0) * d_p + i];
      s1 += (double)dimpart[((int64_t)rb * 3 + 1) * d_p + i];
      s2 += (double)dimpart[((int64_t)rb * 3 + 2) * d_p + i];
    }
    o.sx[i] += s0;
    o.sxx[i] += s1;
    o.srr[i] += s2;
  } else {
    const int lane = threadIdx.x & 63;
    const int f = (b - nb_lat - nb_dim) * 4 + (threadIdx.x >> 6);
    if (f >= n_files) return;                    // (wave-uniform)
    const int L = search_len(lengths, f, T);
    double e = 0.0, en = 0.0;
    for (int t = lane; t < L; t += 64) {
      const float* rp = rowpart + ((int64_t)f * T + t) * nch * 2;
      for (int ch = 0; ch < nch; ++ch) {
        e += (double)rp[2 * ch];
        en += (double)rp[2 * ch + 1];
      }
    }
    e = wave_sum_d(e);
    en = wave_sum_d(en);
    if (lane == 0) {
      file_out[2 * (int64_t)f] = e;
      file_out[2 * (int64_t)f + 1] = en;
      atomicAdd(o.n_frames, (unsigned long long)L);
    }
  }
}
