// The launchers of the bf16 GEMM kernels (gemm.h, gemm256.h, gemm256s.h): which kernel a shape and an epilogue functor get, its
// grid and its LDS.  Templates over the functor: every translation unit that brings epilogues of its own includes this header and
// instantiates the kernels it launches -- engine.hip the training paths', passes.hip the file passes'.
#pragma once
#include "engine_internal.h"
#include "gemm256.h"
#include "gemm256s.h"

constexpr int G2_PERSIST_STATIC = 512;      // resident workgroups of the big static 256x256 GEMM launches (0: one workgroup per tile)

// The output tile launch_gemm's tile form gives an [nbm x nbn] grid of 128x128 tiles: 256 (gemm256.h) when both output dimensions are
// multiples of 256, else 128 (gemm.h).  The one statement of that rule: whoever sizes a grid, a split-K factor or a slab layout for a
// launch_gemm call asks here.
static int gemm_tile_edge(int nbm, int nbn) { return (!g_force_gemm128 && nbm % 2 == 0 && nbn % 2 == 0) ? 256 : 128; }
static int gemm_tile_edge(const GemmArgs& g) { return gemm_tile_edge(g.nbm, g.nbn); }

// true: launch_gemm runs this GEMM in the streaming form of gemm256s.h (the K = d GEMMs: row-major x row-major, one K segment,
// thousands of static output tiles) -- callers that size a per-workgroup output of the functor ask first
template <int AM, int BM_, class Epi>
static bool gemm_streams(const GemmArgs& g) {
  if constexpr (!(epi_stream<Epi>::value && AM == OP_ROW && BM_ == OP_ROW)) return false;
  if (g_no_stream || gemm_tile_edge(g) != 256) return false;
  if (g.ktiles % 2 != 0) return false;                     // (the static-stage K loop walks the K tiles in pairs: gemm256s.h)
  return !g.dyn && g.splits == 1 && g.tail_tiles == 0 && g.ktiles == g.ktiles0 && g.ktiles >= 2 && g.seg1_gate == nullptr && g.lda == g.ldb &&
         (g.nbm / 2) * (g.nbn / 2) >= 4 * G2_PERSIST_STATIC;
}

// the streaming form itself, for a GEMM that gemm_streams() accepted (the file passes launch it with epilogues that have only the
// streaming interface, so they cannot go through launch_gemm, whose tile-form branches would be instantiated with them)
template <class Epi>
static int launch_gemm_stream(const GemmArgs& g, const Epi& epi, hipStream_t s) {
  auto kerns = gemm256s_bf16_kernel<Epi>;
  LDS_ATTR(kerns, G2S_LDS_BYTES, g_device);
  GemmArgs g2 = g;
  g2.nbm = g.nbm / 2;
  g2.nbn = g.nbn / 2;
  hipLaunchKernelGGL(kerns, dim3(G2_PERSIST_STATIC), dim3(512), G2S_LDS_BYTES, s, g2, epi);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// functors that opt out of gemm256.h's tile-walking (PERSIST) instantiation: static constexpr bool NO_PERSIST = true
template <class E, class = void>
struct epi_no_persist { static constexpr bool value = false; };
template <class E>
struct epi_no_persist<E, std::void_t<decltype(E::NO_PERSIST)>> { static constexpr bool value = E::NO_PERSIST; };

template <int AM, int BM_, class Epi>
static int launch_gemm(const GemmArgs& g, const Epi& epi, hipStream_t s) {
  if constexpr (epi_stream<Epi>::value && AM == OP_ROW && BM_ == OP_ROW) {
    if (gemm_streams<AM, BM_, Epi>(g)) return launch_gemm_stream(g, epi, s);
  }
  if (gemm_tile_edge(g) == 256) {
    auto kern256 = gemm256_bf16_kernel<AM, BM_, Epi>;
    constexpr bool a3 = epi_deep_a_ring<Epi>::value;     // (gemm256.h: three A slots + two B slots)
    constexpr int lds256 = a3 ? G2_A3_LDS_BYTES : (epi_rounds_first<Epi>::value && G2_BF16_LDS_BYTES > G2_LDS_BYTES) ? G2_BF16_LDS_BYTES : G2_LDS_BYTES;
    static_assert(G2_A3_LDS_BYTES >= G2_BF16_LDS_BYTES && G2_A3_LDS_BYTES >= G2_LDS_BYTES, "the epilogues reuse the ring's LDS");
    LDS_ATTR(kern256, lds256, g_device);
    GemmArgs g2 = g;
    g2.nbm = g.nbm / 2;
    g2.nbn = g.nbn / 2;
    const int grid_max = (g.dyn && g.grid_cover > 0) ? g.grid_cover
                         : g2.tail_tiles > 0    ? g2.nbm * g2.nbn + g2.tail_tiles * (g2.tail_pieces - 1)
                                                : g2.nbm * g2.nbn * g2.splits;
    const int grid_est = (((g.grid_hint + 3) / 4 + 7) / 8) * 8;          // 256x256 tiles, a multiple of 8
    // (the caller sets grid_hint only for a SMALL estimated extent: the persistent instantiation's tile loop costs the K loop
    // ~10 %, while the workgroups that start only to exit are cheap until they are the great majority)
    if constexpr (epi_no_persist<Epi>::value) {              // (a functor whose state does not fit the tile-walking instantiation)
      hipLaunchKernelGGL(kern256, dim3(grid_max), dim3(512), lds256, s, g2, epi);
    } else
    if (G2_PERSIST_STATIC > 0 && !g.dyn && g2.splits == 1 && g2.tail_tiles == 0 && grid_max >= 4 * G2_PERSIST_STATIC) {
      // big static launches (the K = d GEMMs: tens of thousands of tiles) as G2_PERSIST_STATIC resident workgroups that walk
      // the tiles: encoder / dpre -2 %, TopK encoder -2.5 % against one workgroup per tile (same box; 256 / 512 / 1024 measure alike)
      auto kernp = gemm256_bf16_kernel<AM, BM_, Epi, true>;
      LDS_ATTR(kernp, lds256, g_device);
      hipLaunchKernelGGL(kernp, dim3(G2_PERSIST_STATIC), dim3(512), lds256, s, g2, epi);
    } else if (g.dyn && g.grid_hint > 0 && grid_est < grid_max) {
      auto kernp = gemm256_bf16_kernel<AM, BM_, Epi, true>;
      LDS_ATTR(kernp, lds256, g_device);
      hipLaunchKernelGGL(kernp, dim3(grid_est < 256 ? 256 : grid_est), dim3(512), lds256, s, g2, epi);
    } else {
      hipLaunchKernelGGL(kern256, dim3(grid_max), dim3(512), lds256, s, g2, epi);
    }
    HIP_TRY(hipGetLastError());
    return SAE_OK;
  }
  auto kern = gemm_bf16_kernel<AM, BM_, Epi>;
  LDS_ATTR(kern, GEMM_LDS_BYTES, g_device);
  const int grid = (g.dyn && g.grid_cover > 0) ? g.grid_cover : g.nbm * g.nbn * g.splits;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), GEMM_LDS_BYTES, s, g, epi);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}
