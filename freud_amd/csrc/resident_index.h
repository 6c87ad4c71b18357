// The arithmetic of the resident store's gather (resident.h; include/freud_sae.h, sae_store_gather), free of any HIP type so that the
// SAME functions compile for the host: tests/test_resident_cpu.py builds them with g++.  Everything is 64-bit: a store of 200 000
// files x 1500 x 384 values is 1.2e11 elements, and idx * row_bytes leaves 32 bits at the 1865th bf16 file of that shape.
//
//   pieces    a row of row_bytes is cut into pieces of RS_PIECE_BYTES (the last one shorter); one workgroup copies one piece of one
//             batch row.  Workgroup w of the 1-D grid serves batch row w / pieces and piece w % pieces.
//   index     idx[j] is clamped into [0, n_files): a bad index can never address outside the store.  It is also COUNTED (by the
//             workgroup of the row's piece 0, once per batch row), so that it cannot pass unnoticed either.  The host validates index
//             lists before they are uploaded (freud_amd/resident.py: check_indices); the clamp is the second line, not the check.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

constexpr int RS_THREADS = 256;
constexpr int RS_UNROLL = 4;                                          // independent 16-byte loads per thread before its first store
constexpr int64_t RS_PIECE_BYTES = (int64_t)RS_THREADS * RS_UNROLL * 16;   // 16 KiB (measured: 8 KiB the same, 32 KiB 35 % slower)

RS_HD int64_t rs_pieces(int64_t row_bytes) { return (row_bytes + RS_PIECE_BYTES - 1) / RS_PIECE_BYTES; }

// workgroup w -> (batch row j, piece p)
RS_HD void rs_block_of(int64_t w, int64_t pieces, int64_t* j, int64_t* p) {
  *j = w / pieces;
  *p = w % pieces;
}

// piece p of a row -> its first byte and its length (0 < len <= RS_PIECE_BYTES for p < rs_pieces(row_bytes))
RS_HD void rs_piece_span(int64_t row_bytes, int64_t p, int64_t* byte0, int64_t* len) {
  *byte0 = p * RS_PIECE_BYTES;
  const int64_t rest = row_bytes - *byte0;
  *len = rest < RS_PIECE_BYTES ? rest : RS_PIECE_BYTES;
}

// idx -> a file inside the store; *bad = whether it had to be moved there
RS_HD int64_t rs_clamp_index(int32_t idx, int64_t n_files, bool* bad) {
  const int64_t i = idx;
  *bad = i < 0 || i >= n_files;
  return i < 0 ? 0 : (i >= n_files ? n_files - 1 : i);
}

// byte offsets of a file in the store and of a batch row in the destination
RS_HD int64_t rs_src_offset(int64_t file, int64_t row_bytes) { return file * row_bytes; }
RS_HD int64_t rs_dst_offset(int64_t j, int64_t out_stride_bytes) { return j * out_stride_bytes; }

// the widest of 16, 4, 2 bytes that divides every address and extent of a launch (0: not even 2).  `bits` = the OR of both base
// addresses, the row size and the destination stride.
RS_HD int rs_copy_width(uint64_t bits) { return (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : (bits & 1) == 0 ? 2 : 0; }
