// The decomposition of the input covariance (input_cov.h; include/freud_sae.h, sae_input_cov), free of any HIP type so that the SAME
// functions compile for the host: tests/test_input_pca_cpu.py builds them with g++.  Everything here is a function of
// (n_files, T, d) alone: never of the grid, the CU count or the device.
//
//   tiles     the output S [d][d] in tiles of ICV_TILE x ICV_TILE; only the tiles (ti, tj) with ti <= tj are computed, enumerated row by
//             row: t = 0 is (0, 0), then (0, 1) .. (0, ntd - 1), (1, 1), ..  The last step mirrors them.
//   units     the 256-frame units of input_stats.h: u = f * ceil(T / 256) + b, file f, frames [256 b, min(256 b + 256, cnt_f))
//   segments  segment s holds the units [s ups, min((s + 1) ups, U)): consecutive, ascending, none empty.  One workgroup adds the
//             frames of one (segment, tile) in ascending order; the fold adds a tile's segments in ascending s.
//   count     the most segments with tiles x segments <= ICV_TARGET_GROUPS (d = 384: 21 tiles x 97 -> 96 segments of 16 units at
//             256 files x 1500 frames: 2016 workgroups, two full rounds of four per CU on 256 CUs and no third), at least one and at
//             most one per unit.  So the partials, one ICV_TILE^2 block of doubles per (segment, tile), take at most
//             ICV_TARGET_GROUPS x 32 KiB = 64 MiB.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ICV_HD __host__ __device__ __forceinline__
#else
#define ICV_HD inline
#endif

constexpr int ICV_TILE = 64;               // edge of an output tile: four waves of 32 x 32
constexpr int ICV_UNIT = 256;              // frames per unit (input_stats.h: IN_UNIT)
constexpr int ICV_TARGET_GROUPS = 2048;    // workgroups at most: eight per CU of a 256-CU device (d <= 2048: 528 tiles fit)
constexpr int64_t ICV_MAX_PARTIAL_BYTES = (int64_t)ICV_TARGET_GROUPS * ICV_TILE * ICV_TILE * 8;

struct IcvPlan {
  int ntd;                 // tiles per dimension
  int tiles;               // ntd (ntd + 1) / 2
  int64_t units_per_file;  // ceil(T / ICV_UNIT)
  int64_t units;           // U
  int64_t units_per_seg;   // ups
  int64_t segments;        // ceil(U / ups)
};

ICV_HD IcvPlan icv_plan(int64_t n_files, int64_t T, int64_t d) {
  IcvPlan p;
  p.ntd = (int)((d + ICV_TILE - 1) / ICV_TILE);
  p.tiles = p.ntd * (p.ntd + 1) / 2;
  p.units_per_file = (T + ICV_UNIT - 1) / ICV_UNIT;
  p.units = n_files * p.units_per_file;
  int64_t want = ICV_TARGET_GROUPS / p.tiles;
  if (want > p.units) want = p.units;
  if (want < 1) want = 1;
  p.units_per_seg = (p.units + want - 1) / want;
  p.segments = (p.units + p.units_per_seg - 1) / p.units_per_seg;
  return p;
}

// tile t of the enumeration -> (ti, tj), ti <= tj
ICV_HD void icv_tile_of(int t, int ntd, int* ti, int* tj) {
  int i = 0;
  while (t >= ntd - i) {
    t -= ntd - i;
    ++i;
  }
  *ti = i;
  *tj = i + t;
}

// the units [u0, u1) of segment s
ICV_HD void icv_segment_units(const IcvPlan& p, int64_t s, int64_t* u0, int64_t* u1) {
  *u0 = s * p.units_per_seg;
  const int64_t e = *u0 + p.units_per_seg;
  *u1 = e < p.units ? e : p.units;
}

// partials [segments][tiles][ICV_TILE][ICV_TILE] doubles
ICV_HD int64_t icv_partial_bytes(const IcvPlan& p) { return p.segments * p.tiles * (int64_t)(ICV_TILE * ICV_TILE) * 8; }
