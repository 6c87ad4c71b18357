// Input statistics (sae_input_moments, sae_input_median): what the data looks like before a dictionary exists.  No SAE, no context.
// The sample is resident as x[n_files][T][d] (fp32 / fp16 / bf16); file f counts its first cnt_f = clamp(length_f, 1, T) frames.
//
// Units.  Every partial sum belongs to a fixed unit u = f * ceil(T / 256) + b: file f, frames [256 b, min(256 b + 256, cnt_f)) (an
// empty unit holds zeros, and +inf / -inf for min / max).  One 256-thread workgroup computes one unit in an order that depends on
// (d, dtype) alone; in_fold_kernel then adds the units of a column in ascending u.  So every result is a function of
// (x, lengths, iterations): not of the grid, not of the CU count.  No atomics anywhere.
//
//   in_count_kernel        N = sum of cnt_f (int64, one workgroup)
//   in_moments_kernel<T,0> per unit and column: sum x, sum x^2 (fp64: the square of an fp32 value is exact), min, max
//   in_moments_kernel<T,1> per unit and column: sum (x - mean)^2 with the fp64 mean, the centred second sweep
//   in_weiszfeld_kernel    per unit: sum w x per column, sum w, sum dist (fp64) for the current estimate m (fp64 [d]):
//                            diff = float(double(x) - m)        one rounding: |m| ~ 10^3 against a difference of order 1 keeps its bits
//                            s    = sum diff^2                  fp32: a per-lane partial in column order (mul, add: no contraction),
//                                                               then the xor-butterfly of wave_sum
//                            dist = sqrtf(s), w = 1.f / fmaxf(dist, floor)
//                          One wave per row.  Column c belongs to the 16-byte vector c / EPV of its row, that vector to lane
//                          (c / EPV) % 64, slot (c / EPV) / 64: the <T, NV> form reads each vector once into a register array of NV
//                          slots with compile-time indices (the loads of the next one to three rows are in flight under the current row's arithmetic) and
//                          keeps m and the column sums in registers; the <T, 0> form (rows that are not 16-byte aligned: odd d with a
//                          2-byte dtype, an odd base pointer) walks the same ownership with scalar loads, reads the row a second time
//                          for the weighted sum (an L1 / L2 hit) and keeps the sums in LDS.  Both forms add the same numbers in
//                          the same order: the bits do not depend on which one ran.
//   in_fold_kernel         columns of part[U][ncols] folded in ascending unit order (tiles of IN_TILE_U units through LDS, 32 columns
//                          per workgroup); the Weiszfeld form also folds sum w and sum dist in every workgroup, divides, writes
//                          m_{k+1} into the path and J_k = sum dist / N
//   in_finish_kernel       the moments' output block from the folded sums
#pragma once
#include <float.h>
#include <type_traits>

#include "common.h"

constexpr int IN_MAX_D = 2048;
constexpr int IN_UNIT = 256;       // frames per unit
constexpr int IN_MAX_NV = 8;       // 16-byte vectors per lane: d <= 2048 in fp32
constexpr int IN_FOLD_COLS = 32;   // columns per fold workgroup
constexpr int IN_TILE_U = 128;     // units per fold tile

__device__ __forceinline__ int in_count_of(const int32_t* lengths, int64_t f, int T) {
  if (!lengths) return T;
  const int l = lengths[f];
  return l < 1 ? 1 : (l > T ? T : l);
}

__global__ __launch_bounds__(256) void in_count_kernel(const int32_t* __restrict__ lengths, int64_t n_files, int T, int64_t* __restrict__ n_out) {
  __shared__ long long red[256];
  long long s = 0;
  for (int64_t f = threadIdx.x; f < n_files; f += 256) s += in_count_of(lengths, f, T);
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int i = 0; i < 256; ++i) t += red[i];
    *n_out = t;
  }
}

// part: PASS 0 [U][4 d] (sum x | sum x^2 | min | max), PASS 1 [U][d].  Threads (rg, cl): columns cl, cl + CW, ...; rows rg, rg + RG, ...
// with CW = min(256, the power of two >= d) and RG = 256 / CW; the row groups are added in ascending rg.
template <typename T, int PASS>
__global__ __launch_bounds__(256) void in_moments_kernel(const T* __restrict__ x, int Trows, int d, int units_per_file,
                                                          const int32_t* __restrict__ lengths, const double* __restrict__ mean,
                                                          double* __restrict__ part) {
  __shared__ double sh_a[256], sh_b[256];
  __shared__ float sh_mn[256], sh_mx[256];
  const int64_t u = blockIdx.x, f = u / units_per_file;
  const int r0 = (int)(u % units_per_file) * IN_UNIT;
  const int cnt = in_count_of(lengths, f, Trows);
  const int nrows = cnt - r0 < IN_UNIT ? (cnt - r0 < 0 ? 0 : cnt - r0) : IN_UNIT;
  int cw = 256;
  while (cw / 2 >= d) cw >>= 1;
  const int rgs = 256 / cw, rg = threadIdx.x / cw, cl = threadIdx.x % cw;
  const T* const base = x + ((int64_t)f * Trows + r0) * d;
  double* const out = part + u * (int64_t)(PASS == 0 ? 4 * d : d);
  for (int c0 = 0; c0 < d; c0 += cw) {
    const int c = c0 + cl;
    double a = 0.0, b = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    if (c < d) {
      const double mu = PASS == 1 ? mean[c] : 0.0;
#pragma unroll 4
      for (int r = rg; r < nrows; r += rgs) {
        const float v = load_as_float(base + (int64_t)r * d + c);
        if (PASS == 0) {
          a += (double)v;
          b = fma((double)v, (double)v, b);
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
        } else {
          const double e = (double)v - mu;
          a = fma(e, e, a);
        }
      }
    }
    __syncthreads();
    sh_a[threadIdx.x] = a;
    sh_b[threadIdx.x] = b;
    sh_mn[threadIdx.x] = mn;
    sh_mx[threadIdx.x] = mx;
    __syncthreads();
    if (rg == 0 && c < d) {
      for (int g = 1; g < rgs; ++g) {
        a += sh_a[g * cw + cl];
        b += sh_b[g * cw + cl];
        mn = fminf(mn, sh_mn[g * cw + cl]);
        mx = fmaxf(mx, sh_mx[g * cw + cl]);
      }
      out[c] = a;
      if (PASS == 0) {
        out[d + c] = b;
        out[2 * d + c] = (double)mn;
        out[3 * d + c] = (double)mx;
      }
    }
  }
}

// element e of a 16-byte vector as fp32
template <typename T, int E>
__device__ __forceinline__ float in_elem(const u32x4& v) {
  if constexpr (std::is_same<T, float>::value) {
    return __uint_as_float(v[E]);
  } else if constexpr (std::is_same<T, bf16_t>::value) {
    return __uint_as_float((E & 1) ? (v[E >> 1] & 0xFFFF0000u) : (v[E >> 1] << 16));
  } else {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)((E & 1) ? (v[E >> 1] >> 16) : (v[E >> 1] & 0xFFFFu)));
  }
}

// the scalars of a unit's tail: the four waves' sum w and sum dist (wsc [4][2] in LDS) added in wave order
__device__ __forceinline__ void in_weiszfeld_scalars(const double* wsc, int d, double* __restrict__ out) {
  if (threadIdx.x < 2) out[d + threadIdx.x] = ((wsc[threadIdx.x] + wsc[2 + threadIdx.x]) + wsc[4 + threadIdx.x]) + wsc[6 + threadIdx.x];
}

// part [U][d + 2]: sum w x | sum w | sum dist; the four waves' column sums are added in wave order, ((w0 + w1) + w2) + w3, in both
// forms.  Dynamic LDS: NV > 0: d doubles; NV == 0: 4 d doubles (above 64 KB in all: the launcher raises the kernel's limit).
template <typename T, int NV>
__global__ __launch_bounds__(256) void in_weiszfeld_kernel(const T* __restrict__ x, int Trows, int d, int units_per_file,
                                                           const int32_t* __restrict__ lengths, const double* __restrict__ m,
                                                           float floor_w, double* __restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ double in_lds[];
  __shared__ double wsc[8];
  constexpr int EPV = 16 / (int)sizeof(T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t u = blockIdx.x, f = u / units_per_file;
  const int r0 = (int)(u % units_per_file) * IN_UNIT;
  const int cnt = in_count_of(lengths, f, Trows);
  const int nrows = cnt - r0 < IN_UNIT ? (cnt - r0 < 0 ? 0 : cnt - r0) : IN_UNIT;
  const T* const base = x + ((int64_t)f * Trows + r0) * d;
  double sw = 0.0, sd = 0.0;
  if constexpr (NV > 0) {
    const int nvec = d / EPV;
    double mr[NV][EPV], acc[NV][EPV];
    static_for<0, NV>([&](auto q) {
      static_for<0, EPV>([&](auto e) {
        const int c = (q * 64 + lane) * EPV + e;
        mr[q][e] = c < d ? m[c] : 0.0;
        acc[q][e] = 0.0;
      });
    });
    // the row in flight and the PF rows behind it: a narrow row (few vectors per lane) needs more of them to cover the memory latency
    constexpr int PF = NV <= 2 ? 3 : (NV <= 4 ? 2 : 1);
    u32x4 buf[PF + 1][NV];
    auto load_row = [&](u32x4 (&dst)[NV], int r) {
      const u32x4* const p = reinterpret_cast<const u32x4*>(base + (int64_t)r * d);
      static_for<0, NV>([&](auto q) {
        const int i = q * 64 + lane;
        dst[q] = (r < nrows && i < nvec) ? p[i] : u32x4{0u, 0u, 0u, 0u};
      });
    };
    static_for<0, PF>([&](auto j) { load_row(buf[j], wave + 4 * j); });
    for (int r = wave; r < nrows; r += 4) {
      u32x4 (&cur)[NV] = buf[0];
      load_row(buf[PF], r + 4 * PF);
      float ss = 0.f;
      static_for<0, NV>([&](auto q) {
        static_for<0, EPV>([&](auto e) {
          const float diff = (float)((double)in_elem<T, decltype(e)::value>(cur[q]) - mr[q][e]);
          ss = ss + diff * diff;
        });
      });
      const float dist = sqrtf(wave_sum(ss));
      const float w = 1.f / fmaxf(dist, floor_w);
      const double wd = (double)w;
      static_for<0, NV>([&](auto q) {
        static_for<0, EPV>([&](auto e) { acc[q][e] = fma(wd, (double)in_elem<T, decltype(e)::value>(cur[q]), acc[q][e]); });
      });
      sw += wd;
      sd += (double)dist;
      static_for<0, PF>([&](auto j) { static_for<0, NV>([&](auto q) { buf[j][q] = buf[j + 1][q]; }); });
    }
    for (int wv = 0; wv < 4; ++wv) {
      if (wave == wv) {
        static_for<0, NV>([&](auto q) {
          static_for<0, EPV>([&](auto e) {
            const int c = (q * 64 + lane) * EPV + e;
            if (c < d) in_lds[c] = wv == 0 ? acc[q][e] : in_lds[c] + acc[q][e];
          });
        });
      }
      __syncthreads();
    }
    for (int c = threadIdx.x; c < d; c += 256) part[u * (int64_t)(d + 2) + c] = in_lds[c];
  } else {
    double* const acc = in_lds + wave * d;
    for (int c = lane; c < d; c += 64) acc[c] = 0.0;
    const int nslots = (d + 64 * EPV - 1) / (64 * EPV);
    for (int r = wave; r < nrows; r += 4) {
      const T* const row = base + (int64_t)r * d;
      float ss = 0.f;
      for (int q = 0; q < nslots; ++q) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          const int c = (q * 64 + lane) * EPV + e;
          // (an absent column adds 0.f * 0.f like the register form's zero vector: s + 0 == s)
          const float diff = c < d ? (float)((double)load_as_float(row + c) - m[c]) : 0.f;
          ss = ss + diff * diff;
        }
      }
      const float dist = sqrtf(wave_sum(ss));
      const float w = 1.f / fmaxf(dist, floor_w);
      const double wd = (double)w;
      for (int q = 0; q < nslots; ++q) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          const int c = (q * 64 + lane) * EPV + e;
          if (c < d) acc[c] = fma(wd, (double)load_as_float(row + c), acc[c]);
        }
      }
      sw += wd;
      sd += (double)dist;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256)
      part[u * (int64_t)(d + 2) + c] = ((in_lds[c] + in_lds[d + c]) + in_lds[2 * d + c]) + in_lds[3 * d + c];
  }
  if (lane == 0) {
    wsc[wave * 2] = sw;
    wsc[wave * 2 + 1] = sd;
  }
  __syncthreads();
  in_weiszfeld_scalars(wsc, d, part + u * (int64_t)(d + 2));
}

enum { IN_FOLD_MOMENTS0 = 0, IN_FOLD_SUM = 1, IN_FOLD_WEISZFELD = 2 };

// Folds the columns [32 b, 32 b + 32) of part[U][ncols] in ascending unit order into folded[ncols].
//   IN_FOLD_MOMENTS0   ncols = 4 d: columns < 2 d are sums, [2 d, 3 d) minima, [3 d, 4 d) maxima
//   IN_FOLD_SUM        sums
//   IN_FOLD_WEISZFELD  ncols = d + 2, grid over the d columns: every workgroup also folds sum w and sum dist (the same bits in each),
//                      writes m_next[c] = sum w x / sum w unless m_next is null, and workgroup 0 writes *objective = sum dist / N
template <int MODE>
__global__ __launch_bounds__(256) void in_fold_kernel(const double* __restrict__ part, int64_t U, int ncols, int d,
                                                      double* __restrict__ folded, double* __restrict__ m_next,
                                                      double* __restrict__ objective, const int64_t* __restrict__ n_frames) {
  constexpr int W = IN_FOLD_COLS + 2;
  __shared__ double tile[IN_TILE_U * W];
  __shared__ double sh_w;
  const int c0 = blockIdx.x * IN_FOLD_COLS, j = threadIdx.x;
  const int fold_cols = MODE == IN_FOLD_WEISZFELD ? d : ncols;
  // slot j of the tile -> its column of part, or -1
  auto col_of = [&](int s) {
    if (s < IN_FOLD_COLS) return c0 + s < fold_cols ? c0 + s : -1;
    return MODE == IN_FOLD_WEISZFELD ? d + (s - IN_FOLD_COLS) : -1;
  };
  const int mycol = j < W ? col_of(j) : -1;
  const int op = (MODE == IN_FOLD_MOMENTS0 && mycol >= 2 * d) ? (mycol >= 3 * d ? 2 : 1) : 0;
  double acc = op == 0 ? 0.0 : (op == 1 ? INFINITY : -INFINITY);
  // a tile's loads are issued one tile ahead, into registers, and land in LDS when the tile before it has been added
  constexpr int PER = IN_TILE_U * W / 256;
  static_assert(IN_TILE_U * W % 256 == 0, "the fold tile is a whole number of elements per thread");
  double pre[PER];
  auto fetch = [&](int64_t u0) {
    const int64_t left = (U - u0) * W;
    static_for<0, PER>([&](auto n) {
      const int i = j + 256 * n, col = col_of(i % W);
      pre[n] = (i < left && col >= 0) ? part[(u0 + i / W) * ncols + col] : 0.0;
    });
  };
  fetch(0);
  for (int64_t u0 = 0; u0 < U; u0 += IN_TILE_U) {
    const int nu = U - u0 < IN_TILE_U ? (int)(U - u0) : IN_TILE_U;
    __syncthreads();
    static_for<0, PER>([&](auto n) { tile[j + 256 * n] = pre[n]; });
    __syncthreads();
    if (u0 + IN_TILE_U < U) fetch(u0 + IN_TILE_U);
    if (mycol >= 0) {
      if (op == 0) {
        for (int k = 0; k < nu; ++k) acc += tile[k * W + j];
      } else if (op == 1) {
        for (int k = 0; k < nu; ++k) acc = fmin(acc, tile[k * W + j]);
      } else {
        for (int k = 0; k < nu; ++k) acc = fmax(acc, tile[k * W + j]);
      }
    }
  }
  if (MODE != IN_FOLD_WEISZFELD) {
    if (mycol >= 0) folded[mycol] = acc;
  } else {
    if (j == IN_FOLD_COLS) sh_w = acc;
    __syncthreads();
    if (j < IN_FOLD_COLS && mycol >= 0 && m_next) m_next[mycol] = acc / sh_w;
    if (j == IN_FOLD_COLS + 1 && blockIdx.x == 0) *objective = acc / (double)*n_frames;
  }
}

// out: mean [d] | centred sum of squares [d] | min [d] | max [d] | sum |x|^2 | N.  PASS 0 (folded [4 d]) writes all but the second
// block; PASS 1 (folded [d]) writes that.  sum |x|^2 adds the columns' sums of squares in ascending column order.
template <int PASS>
__global__ __launch_bounds__(256) void in_finish_kernel(const double* __restrict__ folded, int d, const int64_t* __restrict__ n_frames,
                                                         double* __restrict__ out) {
  const double N = (double)*n_frames;
  for (int c = threadIdx.x; c < d; c += 256) {
    if (PASS == 0) {
      out[c] = folded[c] / N;
      out[2 * d + c] = folded[2 * d + c];
      out[3 * d + c] = folded[3 * d + c];
    } else {
      out[d + c] = folded[c];
    }
  }
  if (PASS == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) s += folded[d + c];
    out[4 * d] = s;
    out[4 * d + 1] = N;
  }
}

// the one dispatch of the Weiszfeld form on the 16-byte vectors per lane: f(integral_constant<NV>), NV = 0 for the scalar form
template <class F>
static bool with_in_nv(int nv, F&& f) {
  switch (nv) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
  }
}
