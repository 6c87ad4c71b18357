// Activation histograms (include/freud_sae.h, sae_hist_files): per latent the histogram of its value over the counted frames
// (frame_hist [n][NB]), the histogram of each file's maximum (file_max_hist [n][NB]) and, for up to HIST_MAX_SEL chosen latents, the
// frame histogram split by the frames' labels (label_hist [n_sel][C + 1][NB]).  Bins are hist_bins.h's, on the bf16 bit pattern of
// the value encode() returns; frames count as in stats.h (search_len).  Every output is an int64 running total and every sum an
// integer: two runs give bitwise identical arrays.
//
// L1 (hist_l1_kernel) reads the stored latent [M_p][ld].  One thread owns one column and walks a chunk of whole files in row order;
// a workgroup is blockDim.x adjacent columns.  The regular bins of a column are counted in LDS, two 16-bit counters per dword:
// h[q][thread] holds bins 2 + 2q (low half) and 2 + 2q + 1 (high half), so the dword of lane l is on bank l % 32 whatever the bin and a
// 32-lane group never conflicts.  A thread owns its column, so the update is a plain read-modify-write and no barrier is needed
// anywhere.  A zero costs no LDS update: bin 0 is the counted rows minus the non-zero ones; underflow and overflow are registers.
// The counters are flushed -- one global integer add per non-empty bin -- at the end of the chunk and whenever the next segment of
// rows would take the rows since the last flush past HIST_FLUSH_ROWS = 65535: a column that stays in one bin cannot wrap its 16-bit
// counter, and the low half never carries into the high one.  The maximum of a file is a register; one global add per (file, column).
//
// TopK reads the selection idx / vals [M][k]: integer global adds straight into frame_hist, a scatter-max of the magnitudes into
// scratch [n_files][n], then hist_topk_finish_kernel (one thread per latent, plain adds: it owns the latent's rows) bins the file
// maxima and sets bin 0 to the frames counted so far minus the other bins -- frame_hist and n_frames are running totals of the
// same calls.
#pragma once
#include "common.h"
#include "hist_bins.h"
#include "search.h"      // search_len: the trimmed length of a file

constexpr int HIST_MAX_SEL = 64;
constexpr int HIST_FLUSH_ROWS = 65535;     // rows between two flushes of the 16-bit LDS counters, at most
constexpr int HIST_UNROLL = 16;            // rows of a column in flight

__device__ __forceinline__ void hist_add(int64_t* p, uint32_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// n_frames += the batch's counted frames; label_count[C] as well when the label part runs.  One workgroup.
__global__ __launch_bounds__(256) void hist_frames_kernel(int64_t n_files, int T, const int* __restrict__ lengths, int64_t* __restrict__ n_frames,
                                                          int64_t* __restrict__ label_count_any) {
  __shared__ unsigned long long part[4];
  unsigned long long s = 0;
  for (int64_t f = threadIdx.x; f < n_files; f += 256) s += (unsigned long long)search_len(lengths, (int)f, T);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = part[0] + part[1] + part[2] + part[3];
    *n_frames += (int64_t)total;
    if (label_count_any) *label_count_any += (int64_t)total;
  }
}

// ---- L1.  Grid (column blocks of blockDim.x, chunks of files_per_chunk files); dynamic LDS ((O P + 1) / 2) * blockDim.x dwords.
__global__ __launch_bounds__(256) void hist_l1_kernel(const unsigned short* __restrict__ lat, int64_t ld, int n, int64_t n_files, int T,
                                                      const int* __restrict__ lengths, int files_per_chunk, HistSpec sp,
                                                      int64_t* __restrict__ frame_hist, int64_t* __restrict__ file_max_hist) {
  extern __shared__ uint32_t hist_lds[];
  const int nt = blockDim.x, tid = threadIdx.x;
  const int col = blockIdx.x * nt + tid;
  if (col >= n) return;                    // (no barrier below: a thread owns its column and its LDS dwords)
  const int reg = hist_regular(sp), nb = reg + 3, nq = (reg + 1) >> 1;
  uint32_t* h = hist_lds + tid;
  for (int q = 0; q < nq; ++q) h[q * nt] = 0;
  int64_t* fh = frame_hist + (int64_t)col * nb;
  int64_t* mh = file_max_hist + (int64_t)col * nb;
  uint32_t since = 0, nz = 0, under = 0, over = 0;

  auto flush = [&]() {
    for (int q = 0; q < nq; ++q) {
      const uint32_t w = h[q * nt];
      if (w) {
        if (w & 0xFFFFu) hist_add(fh + 2 + 2 * q, w & 0xFFFFu);
        if (w >> 16) hist_add(fh + 3 + 2 * q, w >> 16);
        h[q * nt] = 0;
      }
    }
    if (since != nz) hist_add(fh, since - nz);
    if (under) hist_add(fh + 1, under);
    if (over) hist_add(fh + nb - 1, over);
    since = nz = under = over = 0;
  };
  auto count = [&](uint32_t mag) {
    if (mag == 0) return;
    ++nz;
    const int i = hist_index(mag, sp);
    if (i < 0) ++under;
    else if (i >= reg) ++over;
    else h[(i >> 1) * nt] += 1u << ((i & 1) << 4);
  };

  const int64_t f0 = (int64_t)blockIdx.y * files_per_chunk;
  const int64_t f1 = f0 + files_per_chunk < n_files ? f0 + files_per_chunk : n_files;
  for (int64_t f = f0; f < f1; ++f) {
    const int len = search_len(lengths, (int)f, T);
    const unsigned short* p = lat + f * T * ld + col;
    uint32_t fmax = 0;
    for (int s0 = 0; s0 < len; s0 += HIST_FLUSH_ROWS) {
      const int seg = len - s0 < HIST_FLUSH_ROWS ? len - s0 : HIST_FLUSH_ROWS;
      if (since + (uint32_t)seg > (uint32_t)HIST_FLUSH_ROWS) flush();
      since += (uint32_t)seg;
      int r = s0;
      for (; r + HIST_UNROLL <= s0 + seg; r += HIST_UNROLL) {
        uint32_t v[HIST_UNROLL];
#pragma unroll
        for (int e = 0; e < HIST_UNROLL; ++e) v[e] = p[(int64_t)(r + e) * ld] & 0x7FFFu;
#pragma unroll
        for (int e = 0; e < HIST_UNROLL; ++e) {
          count(v[e]);
          fmax = v[e] > fmax ? v[e] : fmax;
        }
      }
      for (; r < s0 + seg; ++r) {
        const uint32_t mag = p[(int64_t)r * ld] & 0x7FFFu;
        count(mag);
        fmax = mag > fmax ? mag : fmax;
      }
    }
    hist_add(mh + hist_bin(fmax, sp), 1u);
  }
  flush();
}

// ---- TopK: one thread per entry of the selection
__global__ __launch_bounds__(256) void hist_topk_scatter_kernel(const int* __restrict__ idx, const unsigned short* __restrict__ vals, int k, int64_t M,
                                                                int T, const int* __restrict__ lengths, int n, HistSpec sp,
                                                                int64_t* __restrict__ frame_hist, uint32_t* __restrict__ file_max) {
  const int nb = hist_nbins(sp);
  const int64_t total = M * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const uint32_t mag = vals[e] & 0x7FFFu;
    if (mag == 0) continue;
    const int64_t r = e / k, f = r / T;
    if (r - f * T >= search_len(lengths, (int)f, T)) continue;
    const int j = idx[e];
    if (j < 0 || j >= n) continue;
    hist_add(frame_hist + (int64_t)j * nb + hist_bin(mag, sp), 1u);
    atomicMax(file_max + f * n + j, mag);
  }
}

// one thread per latent: the file maxima of the batch binned, then bin 0 of frame_hist from the running frame count
__global__ __launch_bounds__(256) void hist_topk_finish_kernel(const uint32_t* __restrict__ file_max, int64_t n_files, int n, HistSpec sp,
                                                               const int64_t* __restrict__ n_frames, int64_t* __restrict__ frame_hist,
                                                               int64_t* __restrict__ file_max_hist) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int nb = hist_nbins(sp);
  int64_t* mh = file_max_hist + (int64_t)j * nb;
  for (int64_t f = 0; f < n_files; ++f) mh[hist_bin(file_max[f * n + j], sp)] += 1;
  int64_t* fh = frame_hist + (int64_t)j * nb;
  int64_t active = 0;
  for (int b = 1; b < nb; ++b) active += fh[b];
  fh[0] = *n_frames - active;
}

// ---- the label-conditional part: one thread per (row, chosen latent); the thread of the first chosen latent also counts the row's
// labels.  TOPK: `lat` is vals and the row's k selected entries are searched for the latent (idx / vals [M][k]; work rows x n_sel x
// k, small next to the encoder); else lat [M_p][ld].  The "any" row C is not counted here: hist_label_any_kernel copies it.
template <bool TOPK>
__global__ __launch_bounds__(256) void hist_label_kernel(const unsigned short* __restrict__ lat, int64_t ld, const int* __restrict__ idx, int k, int n,
                                                         int64_t M, int T, const int* __restrict__ lengths, const int* __restrict__ labels, int S,
                                                         int C, const int* __restrict__ sel, int n_sel, HistSpec sp,
                                                         int64_t* __restrict__ label_hist, int64_t* __restrict__ label_count) {
  const int nb = hist_nbins(sp);
  const int64_t total = M * n_sel;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / n_sel, f = r / T;
    const int s = (int)(e - r * n_sel);
    if (r - f * T >= search_len(lengths, (int)f, T)) continue;
    if (s == 0)
      for (int q = 0; q < S; ++q) {
        const int id = labels[r * S + q];
        if (id >= 0 && id < C) hist_add(label_count + id, 1u);
      }
    const int j = sel[s];
    if (j < 0 || j >= n) continue;
    uint32_t mag = 0;
    if (TOPK) {
      for (int q = 0; q < k; ++q)
        if (idx[r * k + q] == j) mag = lat[r * k + q] & 0x7FFFu;
    } else {
      mag = lat[r * ld + j] & 0x7FFFu;
    }
    const int b = hist_bin(mag, sp);
    for (int q = 0; q < S; ++q) {
      const int id = labels[r * S + q];
      if (id >= 0 && id < C) hist_add(label_hist + ((int64_t)s * (C + 1) + id) * nb + b, 1u);
    }
  }
}

// label_hist[s][C][:] = frame_hist[sel[s]][:] -- both are running totals of the same calls.  Grid n_sel.
__global__ __launch_bounds__(256) void hist_label_any_kernel(const int64_t* __restrict__ frame_hist, const int* __restrict__ sel, int n, int C, int nb,
                                                             int64_t* __restrict__ label_hist) {
  const int s = blockIdx.x, j = sel[s];
  if (j < 0 || j >= n) return;
  for (int b = threadIdx.x; b < nb; b += 256) label_hist[((int64_t)s * (C + 1) + C) * nb + b] = frame_hist[(int64_t)j * nb + b];
}
