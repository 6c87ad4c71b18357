// Fused forward of the tied-weight L1 SAE for d_model (padded) == 384 on gfx950, third decomposition: the two products of
// fwd_fused2.h on TWO waves per SIMD.  Same arguments, same LDS images (4-slot W^T ring, two pair buffers, bias ring:
// FF_LDS_BYTES), same LDS-DMA source swizzles, same arithmetic in the same order, bit-identical outputs.
//
// Why: fwd_fused2's four waves (one per SIMD) each issue in order through one port: while a wave issues an LDS-DMA piece, a
// fragment read, a v_cvt or waits at the hand-over, its SIMD's matrix pipe has nobody else to take an MFMA from.  Here a
// workgroup is 512 threads; a SIMD holds one wave of each role and the matrix pipe takes from whichever is ready:
//
//   encoder role (waves 0-3): wave w is fwd_fused2's wave w without its decoder MFMAs -- x fragments of rows 32 w .. 32 w + 31
//           in registers, the 24-MFMA chain S(j+1) = W^T tile . x^T, S(j) -> c(j) (bf16 round, fp32 bias, ReLU, L1 sum), the
//           16-byte chunks into the pair buffer, the six LDS-DMA pieces and the bias piece, the drain of the finished pair;
//   decoder role (waves 4-7): wave 4 + w owns x_hat^T[96 w .. 96 w + 95][128 rows] in 12 accumulator tiles and runs the 24
//           decoder MFMAs of tile j-1, m = 12 ks + 3 mb + dtl, from transposed reads of the ring slot and ds_read_b128 of the
//           pair buffer.  No vector arithmetic in its loop.
//
// Each role is a function of its own, called under a wave-uniform branch, and the barriers sit INSIDE the two functions -- the
// same number in each, listed one by one below.  With one barrier statement shared by both roles every register of both roles
// is live at it (96 x + 32 S + 32 ring + ... AND 192 accumulators): the union is ~400 registers against the 256 a wave of a
// 512-thread workgroup owns, whatever the VGPR / AGPR split.  As two functions a wave's registers are its role's only.
// s_barrier counts arrivals, not program addresses.
//
// Barriers, in order (E = encoder wave, D = decoder wave); every wave meets 1 + ntiles + 3 or 4 of them:
//   P      E: its prologue DMA pieces and x have landed (the warm-up pieces keep fwd_fused2's plan, six per encoder wave and
//          tile: the decoder waves have no DMA offsets).  D: ring slot 3 and the staging image are cleared, accumulators zero.
//   L(j)   one per tile j = 0 .. ntiles-1.  E arrives after the counted wait `vmcnt(1) lgkmcnt(2)` of fwd_fused2 (its six pieces
//          of W^T tile j+2 have landed, its chunks of c(j) are written); D arrives after `lgkmcnt(0)` (every read it has asked
//          for -- ring slot (j-1) % 4 and c(j-1) -- is in its registers).
//   E0     E: last latent pair drained, every DMA piece landed.  D: final decoder tile multiplied, nothing of the ring or the
//          pair buffers left to read: the epilogue's staging image may overlay them.
//   E1     (16-bit x on the vector path only) E has staged x and its -1.0 flag; D reads them behind it.
//   E2     D has turned the staging image into dx_hat in place; E stores it behind this barrier.
//   E3     the wave sums are in the bias ring; thread 0 adds them in block_sum_256's order.
//
// Hazards of the tile loop (the list at fwd_fused2.h "pipeline", now ACROSS waves):
//   - ring slot (j-1) % 4 is refilled with tile j+3 by pieces that E issues BEHIND L(j) (two) and in iteration j+1 (four).  D
//     reads that slot for the decoder of tile j-1: k-step 0 behind L(j-1), k-step 1 before its MFMA 12; all of it is in D's
//     registers at its lgkmcnt(0) in front of L(j).  E read the slot last for S(j-1), in iteration j-2.
//   - ring slot (j+1) % 4: tile j+1 was published by L(j-1); E reads it between L(j-1) and L(j+1) (three fragments of it
//     ahead), its refill (tile j+5) is issued behind L(j+2).  D asks for k-step 0 of tile j (slot j % 4, published by L(j-2))
//     behind L(j) and has used it before L(j+1); that slot's refill is issued behind L(j+1).
//   - c(j) is written by E before L(j) and read by D only behind L(j).  Its place in the pair buffers held c(j-4), which D
//     finished reading before L(j-3).  The drain of a pair reads the wave's own rows: program order.
//
// The epilogue keeps the residual where the accumulators are: decoder wave 4 + w does what fwd_fused2's wave w does (same
// lanes, same rows, same d-slice, same order of additions), from x that the encoder waves stage out of their fragment
// registers.  x_hat does not fit next to x in LDS (two [128][784 B] images are 196 KiB), so handing x_hat to the encoder waves
// is not possible without a second pass; sq_part / cnt_part come out of the same additions as before.
//
// Arbitration between the two waves of a SIMD, measured on the bench step (d = 384, n = 3072, M = 65 536; three alternating runs
// each, per-kernel HIP events; profiles/fwd_split_ab.txt): fwd_fused2 241.2-241.7 us; this form, equal priority, encoder on waves
// 0-3: 228.8-229.3 us; `s_setprio 1` in front of the decoder waves' loop: 239.0-239.7 us; the roles swapped (decoder on waves 0-3):
// 239.0-240.5 us.  Either way of putting the decoder first gives back nearly all of the gain: the encoder waves own the latency
// chain (DMA pieces, S -> c, the staging write every decoder waits for), and a decoder that wins every arbitration delays it.
#pragma once
#include "fwd_fused2.h"

constexpr int FS_THREADS = 512;

__device__ __forceinline__ int fs_swz(int row) { return (row & 7) ^ ((row >> 1) & 1) ^ ((row >> 4) & 1); }

// ---------------------------------------------------------------------------------------------------------------- encoder role
template <typename T, bool PAD>
__device__ __forceinline__ void fs_encoder_wave(const FwdFusedArgs& a, char* smem, const int w, const int lane) {
  const int arow = lane & 31, ah = lane >> 5;
  const int wg = blockIdx.x + a.block_offset;
  const int64_t m0 = (int64_t)wg * FF_BM + 32 * w;             // first row of this wave's row block
  const int64_t mrow = m0 + arow;
  const bool row_ok = mrow < a.M;
  char* cst = smem + FF_RING_BYTES;                             // two pair buffers [128 rows][128 B]
  float* bias_s = reinterpret_cast<float*>(smem + FF_FIXED_LDS);

  typedef __attribute__((ext_vector_type(2))) unsigned short us2_t;
  constexpr unsigned MASK_BITS2 = std::is_same<T, bf16_t>::value ? 0xBF80BF80u : 0xBC00BC00u;     // -1.0 twice, bf16 / fp16
  constexpr bool SCAN_EARLY = !PAD && std::is_same<T, bf16_t>::value;
  bool wany_early = false;     // (wave-uniform) some 16-bit word of this wave's 32 x 384 block of a.xb reads -1.0

  bf16x8 xfrag[24];
  // ---- LDS-DMA plan of a W^T tile (as in fwd_fused.h): 24 pieces, six per encoder wave
  unsigned voff_t[6], loff_t[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int inst = w + 4 * i, sub = inst >> 3, row = 4 * (inst & 7) + (lane >> 4), pc = lane & 15;
    const int ch = pc ^ (((row & 3) << 2) | ((row >> 2) & 3));
    voff_t[i] = (unsigned)(row * (FF_D * 2) + (sub * 16 + ch) * 16);
    loff_t[i] = (unsigned)__builtin_amdgcn_readfirstlane(sub * 8192 + (inst & 7) * 1024);
  }
  typedef __attribute__((address_space(3))) char* lptr_t;
  const unsigned smem_base = (unsigned)(uintptr_t)(lptr_t)smem;
  auto dma_pair = [&](int p, int jt, int st) {
    const bf16_t* src = a.Wt + (int64_t)jt * FF_BN * FF_D;
    const unsigned dst = smem_base + st * FF_WT_BYTES;
    glds16_x2(src, src, voff_t[2 * p], voff_t[2 * p + 1], (unsigned)__builtin_amdgcn_readfirstlane((int)(dst + loff_t[2 * p])),
              (unsigned)__builtin_amdgcn_readfirstlane((int)(dst + loff_t[2 * p + 1])));
  };
  auto dma_one = [&](int k, int jt, int st) {       // piece k (0..5) of this wave's share of W^T tile jt into ring slot st
    const bf16_t* src = a.Wt + (int64_t)jt * FF_BN * FF_D;
    glds16(src, voff_t[k], (unsigned)__builtin_amdgcn_readfirstlane((int)(smem_base + st * FF_WT_BYTES + loff_t[k])));
  };
  const int last = a.ntiles - 1;
#pragma unroll
  for (int q = 0; q < 3; ++q)                       // prologue: W^T tiles 0, 1, 2 into slots 0, 1, 2
#pragma unroll
    for (int p = 0; p < 3; ++p) dma_pair(p, q <= last ? q : last, q);
  static_assert(2 * FF_BN == 64, "one 4-byte piece per lane of wave 0");
  if (w == 0) glds4(a.bias, (unsigned)(lane * 4), (unsigned)__builtin_amdgcn_readfirstlane((int)(smem_base + FF_FIXED_LDS)));
  {
    const bf16_t* xp = a.xb + mrow * FF_D + 8 * ah;
#pragma unroll
    for (int kk = 0; kk < 24; ++kk) xfrag[kk] = *reinterpret_cast<const bf16x8*>(xp + 16 * kk);
  }
  // the -1.0 scan of x used in place, on each fragment as it arrives (fwd_fused2.h)
  if (SCAN_EARLY) {
    us2_t mz = {0xFFFFu, 0xFFFFu};
#pragma unroll
    for (int kk = 0; kk < 24; ++kk) {
      const u32x4 xw = __builtin_bit_cast(u32x4, xfrag[kk]);
#pragma unroll
      for (int c = 0; c < 4; ++c) mz = __builtin_elementwise_min(mz, __builtin_bit_cast(us2_t, xw[c] ^ MASK_BITS2));
    }
    wany_early = __builtin_amdgcn_ballot_w64((mz[0] == 0) | (mz[1] == 0)) != 0ull;
  }
#pragma unroll
  for (int kk = 0; kk < 24; ++kk) asm volatile("" : "+v"(xfrag[kk]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                                                                   // barrier P

  // ---- loop-invariant per-lane LDS offsets
  int roff[8];                       // row reads of a W^T tile
#pragma unroll
  for (int i = 0; i < 8; ++i) roff[i] = dual_off(arow, 2 * i + ah);
  // staging image: byte offset of chunk (tile half hf, k-step s, this lane's h) in row `arow` of a 32-row block (swizzle: fwd_fused2.h)
  int boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) boff[i] = arow * 128 + (((4 * (i >> 1) + 2 * (i & 1) + ah) ^ fs_swz(arow)) << 4);
  const int wrow = w * 4096;                                     // this wave's row block inside a pair buffer
  // drain: piece p = rows 8 p .. 8 p + 7 of the row block; lane -> row 8 p + lane / 8, 16 output bytes = columns 8 o .. 8 o + 7
  const int drow_l = lane >> 3, dch = lane & 7;
  int doff0, doff1;
  {
    const int tl = dch >> 2, s = (dch & 3) >> 1, u = dch & 1;
    doff0 = drow_l * 128 + (((4 * tl + 2 * s + 0) ^ fs_swz(drow_l)) << 4) + 8 * u;
    doff1 = drow_l * 128 + (((4 * tl + 2 * s + 1) ^ fs_swz(drow_l)) << 4) + 8 * u;
  }
  auto dpiece = [](int off, int p) { return (p & 2) ? (off ^ 16) : off; };
  bf16_t* cdrain = a.c + (m0 + drow_l) * a.n_p + dch * 8;

  float l1_acc = 0.f;

  // ---- S(0): encoder product of tile 0 (outside the pipeline)
  f32x16 Sn;
#pragma unroll
  for (int r = 0; r < 16; ++r) Sn[r] = 0.f;
#pragma unroll
  for (int kk = 0; kk < 24; ++kk) {
    const bf16x8 fa = *reinterpret_cast<const bf16x8*>(smem + (kk >> 3) * 8192 + roff[kk & 7]);
    Sn = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, xfrag[kk], Sn, 0, 0, 0);
  }

  constexpr int RING = 8;
  const char *rlo[8], *rhi[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    rlo[i] = smem + roff[i];
    rhi[i] = smem + 2 * FF_WT_BYTES + roff[i];
  }
  auto enc_frag = [&](int slot, int kk) -> bf16x8 {
    const int off = (slot & 1) * FF_WT_BYTES + (kk >> 3) * 8192;
    return *reinterpret_cast<const bf16x8*>((slot < 2 ? rlo : rhi)[kk & 7] + off);
  };

  bf16x8 ring[RING];
  f32x16 SA = Sn, SB;
#pragma unroll
  for (int r = 0; r < 16; ++r) SB[r] = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) ring[k] = enc_frag(1, k);      // the first three fragments of tile 1

  u32x4 dr[2];
  bf16_t* const dummy_line = a.c + (int64_t)a.c_rows * a.n_p + lane * 8;
  // Iteration j in fwd_fused2's 48 gaps, of which this role fills the ODD ones with the encoder MFMA i / 2 of tile j+1; everything
  // else -- the latent arithmetic of tile j in gaps 4..35, the staging writes in gaps 18 and 34, the hand-over in gap 40, the DMA
  // pieces in gaps 41, 45 and 1, 5, 9, 13 of the next iteration, the drain -- stands where it stood, so the counted wait of the
  // hand-over counts the same operations.
  auto body = [&](auto ph_tag, int j) {
    constexpr int PH = decltype(ph_tag)::value;          // == j % 4
    constexpr int SLOT_E = (PH + 1) & 3, SLOT_EN = (PH + 2) & 3, SLOT_DMA = (PH + 3) & 3;
    constexpr int PB_W = (PH >> 1) & 1, HF_W = PH & 1;               // where c(j) goes
    f32x16& Scur = (PH & 1) ? SB : SA;
    f32x16& Snxt = (PH & 1) ? SA : SB;
    const int jt = j + 3 <= last ? j + 3 : last;                     // DMA source (clamped in the tail)
    const float* bj = bias_s + (j & (FF_BIAS_RING_TILES - 1)) * FF_BN;
    const char* cst_r = cst + (PB_W ^ 1) * 16384 + wrow;             // pair buffer drained (tiles 2t-2, 2t-1), this wave's rows
    bf16_t* dst_pair = j >= 2 ? cdrain + 64 * ((j >> 1) - 1) : dummy_line;
    const int64_t dst_rstride = j >= 2 ? (int64_t)a.n_p : 0;
    f32x4 bq[4];
    float l1_it = 0.f;
    unsigned se_u = 0u;
    float se_t0 = 0.f, se_t1 = 0.f;
    bf16x8 cw;
    const f32x16 S = Scur;

    static_for<0, 48>([&](auto slot_tag) {
      constexpr int i = decltype(slot_tag)::value;
      // encoder fragments k = i/2 + 3 and i/2 + 4 together, every fourth gap, the later one first (fwd_fused2.h)
      if ((i & 3) == 0 && i <= 40) {
        if (i / 2 + 4 <= 23) ring[(i / 2 + 4) % RING] = enc_frag(SLOT_E, i / 2 + 4);
        ring[(i / 2 + 3) % RING] = enc_frag(SLOT_E, i / 2 + 3);
      }
      if constexpr (i == 42 || i == 44 || i == 46) ring[(i - 42) / 2] = enc_frag(SLOT_EN, (i - 42) / 2);      // k = 0..2 of the NEXT iteration
      if constexpr (i < 4) bq[i] = *reinterpret_cast<const f32x4*>(bj + 8 * i + 4 * ah);
      if (i == 40) {
        // L(j).  <= 1 VMEM operation outstanding (this iteration's first latent store): the six DMA pieces of tile j+2 are done;
        // <= 2 LDS operations outstanding (three fragment reads follow the staging write of gap 34): that write is done
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(1) lgkmcnt(2)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
      if (i == 41 || i == 45) dma_one((i - 41) / 4, jt, SLOT_DMA);
      if (i == 1 || i == 5 || i == 9 || i == 13) dma_one(2 + (i - 1) / 4, j + 2 <= last ? j + 2 : last, (PH + 2) & 3);
      if ((PH & 1) == 0 && i == 46 && w == 0) {
        const int jb = j + 2 <= a.ntiles - 2 ? j + 2 : a.ntiles - 2;
        glds4(a.bias + (int64_t)jb * FF_BN, (unsigned)(lane * 4),
              (unsigned)__builtin_amdgcn_readfirstlane((int)(smem_base + FF_FIXED_LDS + ((j + 2) & (FF_BIAS_RING_TILES - 1)) * FF_BN * 4)));
      }
      // S(j) -> c(j): a pair of elements over four consecutive gaps, the L1 additions e = 0, 1, 2, ... as opaque v_add_f32 (fwd_fused2.h)
      if constexpr (i >= 4 && i <= 35) {
        const int p = (i - 4) >> 2, ph = (i - 4) & 3, e0 = 2 * p;       // pair p = elements e0, e0 + 1 (S register e <-> column n = (e&3) + 8 (e>>2) + 4 h)
        if (ph == 0) {
          se_u = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{S[e0], S[e0 + 1]}, bf16x2));      // rounded to bf16 BEFORE the fp32 bias add (CPU autocast)
        } else if (ph == 1) {
          se_t0 = __uint_as_float(se_u << 16) + bq[e0 >> 2][e0 & 3];
          se_t1 = __uint_as_float(se_u & 0xFFFF0000u);
        } else if (ph == 2) {
          se_t1 = se_t1 + bq[e0 >> 2][(e0 & 3) + 1];
          se_t0 = fmaxf(se_t0, 0.f);
          se_t1 = fmaxf(se_t1, 0.f);
          if (PAD) { se_t0 = row_ok ? se_t0 : 0.f; se_t1 = row_ok ? se_t1 : 0.f; }
        } else {
          asm volatile("v_add_f32 %0, %0, %1\n\tv_add_f32 %0, %0, %2" : "+v"(l1_it) : "v"(se_t0), "v"(se_t1));
          cw[e0 & 7] = (bf16_t)se_t0;
          cw[(e0 & 7) + 1] = (bf16_t)se_t1;
          if ((e0 & 7) == 6)      // the eight values of k-step e0 >> 3: one 16-byte chunk of this lane's row
            *reinterpret_cast<bf16x8*>(cst + PB_W * 16384 + wrow + boff[2 * HF_W + (e0 >> 3)]) = cw;
        }
      }
      // two full-line pieces of the finished pair per iteration: LDS reads in one gap, global store 8 gaps later
      if (i == 29 || i == 33) {
        const int p = 2 * (PH & 1) + (i == 33);
        const uint2 lo = *reinterpret_cast<const uint2*>(cst_r + p * 1024 + dpiece(doff0, p));
        const uint2 hi = *reinterpret_cast<const uint2*>(cst_r + p * 1024 + dpiece(doff1, p));
        dr[i == 33] = u32x4{lo.x, lo.y, hi.x, hi.y};
      }
      if (i == 37 || i == 42) {
        const int p = 2 * (PH & 1) + (i == 42);
        __builtin_nontemporal_store(dr[i == 42], reinterpret_cast<u32x4*>(dst_pair + (int64_t)(8 * p) * dst_rstride));
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (i == 1) {
        f32x16 zero;
#pragma unroll
        for (int r = 0; r < 16; ++r) zero[r] = 0.f;
        Snxt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[0], xfrag[0], zero, 0, 0, 0);
      } else if constexpr ((i & 1) == 1) {
        Snxt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ring[(i / 2) % RING], xfrag[i / 2], Snxt, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    l1_acc += l1_it + 0.0f;      // (as in fwd_fused2.h: the same two additions)
  };
  for (int j4 = 0; j4 < a.ntiles; j4 += 4) {            // ntiles is a multiple of 4 (n_p is a multiple of 128)
    body(std::integral_constant<int, 0>{}, j4);
    body(std::integral_constant<int, 1>{}, j4 + 1);
    body(std::integral_constant<int, 2>{}, j4 + 2);
    body(std::integral_constant<int, 3>{}, j4 + 3);
  }
  // drain the last pair of latent tiles (this wave's own rows)
  {
    const char* cst_r = cst + (((a.ntiles >> 1) - 1) & 1) * 16384 + wrow;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const uint2 lo = *reinterpret_cast<const uint2*>(cst_r + p * 1024 + dpiece(doff0, p));
      const uint2 hi = *reinterpret_cast<const uint2*>(cst_r + p * 1024 + dpiece(doff1, p));
      __builtin_nontemporal_store(u32x4{lo.x, lo.y, hi.x, hi.y},
                                  reinterpret_cast<u32x4*>(cdrain + (int64_t)(8 * p) * a.n_p + 64 * ((a.ntiles >> 1) - 1)));
    }
  }
  // everything but the four latent stores just above must be done: the last DMA pieces still write ring slots that the
  // epilogue's staging image overlays
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                                                                      // barrier E0
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: stage x for the decoder waves' residual, store dx_hat, hand in the L1 sum
  const bool vec_ok = (a.d == FF_D) && ((reinterpret_cast<uintptr_t>(a.x) & (sizeof(T) * 4 - 1)) == 0);
  constexpr int FF_DXH_PITCH = FF_D * 2 + 16;                    // 784 B
  static_assert(128 * FF_DXH_PITCH <= FF_FIXED_LDS, "the dx_hat staging must fit the idle LDS");
  char* stg = smem;                                              // [128 rows][784 B]
  constexpr bool X_VIA_LDS = !PAD && sizeof(T) == 2;
  constexpr bool X_FROM_FRAGS = X_VIA_LDS && std::is_same<T, bf16_t>::value;
  unsigned* mflag = reinterpret_cast<unsigned*>(smem + FF_FIXED_LDS + 64);                         // bias ring: idle since the tile loop
  if (X_FROM_FRAGS && vec_ok && reinterpret_cast<const void*>(a.x) == reinterpret_cast<const void*>(a.xb)) {
    // bf16 activations used in place are still in this wave's B-fragment registers: lane (arow, ah) holds x[m0 + arow][16 kk + 8 ah .. + 7]
    char* srow_w = stg + (32 * w + arow) * FF_DXH_PITCH + 16 * ah;
    us2_t mz = {0xFFFFu, 0xFFFFu};
#pragma unroll
    for (int kk = 0; kk < 24; ++kk) {
      *reinterpret_cast<bf16x8*>(srow_w + 32 * kk) = xfrag[kk];
      if (!SCAN_EARLY) {
        const u32x4 xw = __builtin_bit_cast(u32x4, xfrag[kk]);
#pragma unroll
        for (int c = 0; c < 4; ++c) mz = __builtin_elementwise_min(mz, __builtin_bit_cast(us2_t, xw[c] ^ MASK_BITS2));
      }
    }
    const bool wany = SCAN_EARLY ? wany_early : __builtin_amdgcn_ballot_w64((mz[0] == 0) | (mz[1] == 0)) != 0ull;
    if (lane == 0) mflag[w] = wany ? 1u : 0u;
    __syncthreads();                                                                                 // barrier E1
  } else if (X_VIA_LDS && vec_ok) {     // the wave's 32 x rows are one contiguous 24 KiB block: 24 coalesced 16-byte loads per lane
    const char* xblk = reinterpret_cast<const char*>(reinterpret_cast<const T*>(a.x) + m0 * FF_D);
    us2_t mz = {0xFFFFu, 0xFFFFu};
#pragma unroll
    for (int p0 = 0; p0 < 24; p0 += 4) {
      u32x4 xr[4];
#pragma unroll
      for (int pc = 0; pc < 4; ++pc) xr[pc] = *reinterpret_cast<const u32x4*>(xblk + (p0 + pc) * 1024 + lane * 16);
#pragma unroll
      for (int pc = 0; pc < 4; ++pc) {
        const int off = (p0 + pc) * 1024 + lane * 16, r = off / (FF_D * 2), cb = off - r * (FF_D * 2);
        *reinterpret_cast<u32x4*>(stg + (32 * w + r) * FF_DXH_PITCH + cb) = xr[pc];
#pragma unroll
        for (int c = 0; c < 4; ++c) mz = __builtin_elementwise_min(mz, __builtin_bit_cast(us2_t, xr[pc][c] ^ MASK_BITS2));
      }
    }
    const bool wany = __builtin_amdgcn_ballot_w64((mz[0] == 0) | (mz[1] == 0)) != 0ull;
    if (lane == 0) mflag[w] = wany ? 1u : 0u;
    __syncthreads();                                                                                 // barrier E1
  }
  __syncthreads();                                                                                   // barrier E2: dx_hat is in the staging image
  {   // the wave's 32 rows of dx_hat are one contiguous 24 KiB block: 24 fully coalesced 16-byte stores per lane
    char* gblk = reinterpret_cast<char*>(a.dxh + m0 * FF_D);
#pragma unroll
    for (int pc = 0; pc < 24; ++pc) {
      const int off = pc * 1024 + lane * 16, r = off / (FF_D * 2), cb = off - r * (FF_D * 2);
      *reinterpret_cast<u32x4*>(gblk + off) = *reinterpret_cast<const u32x4*>(stg + (32 * w + r) * FF_DXH_PITCH + cb);
    }
  }
  float* red = reinterpret_cast<float*>(smem + FF_FIXED_LDS);     // [4 waves][l1, sq, plain, nmask]
  {
    const float v0 = wave_sum(l1_acc);
    if (lane == 0) red[4 * w] = v0;
  }
  lds_barrier();                                                                                     // barrier E3
  if (w == 0 && lane == 0) {
    const float l1s = ((red[0] + red[4]) + red[8]) + red[12];
    const float sqs = ((red[1] + red[5]) + red[9]) + red[13];
    const float pls = ((red[2] + red[6]) + red[10]) + red[14];
    const float nms = ((red[3] + red[7]) + red[11]) + red[15];
    a.cnt_part[wg] = nms;
    a.l1_part[wg] = l1s;
    a.sq_part[2 * wg] = sqs;
    a.sq_part[2 * wg + 1] = pls;
  }
}

// ---------------------------------------------------------------------------------------------------------------- decoder role
// w = 0..3: the d-slice [96 w, 96 w + 96); dt = thread index among the 256 decoder threads
template <typename T, bool PAD>
__device__ __forceinline__ void fs_decoder_wave(const FwdFusedArgs& a, char* smem, const int w, const int lane) {
  const int arow = lane & 31, ah = lane >> 5;
  const int wg = blockIdx.x + a.block_offset;
  char* cst = smem + FF_RING_BYTES;
  const int dt = 64 * w + lane;
  // ring slot 3 and the staging image are read (times zero / as zeros) by the first iteration's decoder phase
  for (int i = dt; i < FF_WT_BYTES / 16; i += 256) reinterpret_cast<u32x4*>(smem + 3 * FF_WT_BYTES)[i] = u32x4{0u, 0u, 0u, 0u};
  for (int i = dt; i < FF_CST_BYTES / 16; i += 256) reinterpret_cast<u32x4*>(cst)[i] = u32x4{0u, 0u, 0u, 0u};

  f32x16 acc[12];                       // acc[4 dtl + mb]: rows d = 96 w + 32 dtl + ..., columns = row block mb
#pragma unroll
  for (int i = 0; i < 12; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  __syncthreads();                                                                                   // barrier P

  // the six W fragments (k-step ks, slice tile dtl) of this wave's d-slice: two transposed 8-byte reads each (fwd_fused2.h)
  int aoff0[6], aoff1[6];
  {
    const int g = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const int ks = f / 3, dtile = 3 * w + f % 3;
      const int col = 32 * (dtile & 3) + 16 * g + 4 * p;
      const int r0 = 4 * ah + q, r1 = r0 + 8;
      const int base = (dtile >> 2) * 8192 + ks * 4096;
      aoff0[f] = base + dual_off(r0, col >> 3) + (col & 7) * 2;
      aoff1[f] = base + dual_off(r1, col >> 3) + (col & 7) * 2;
    }
  }
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  auto tr_pair = [&](const char* p0, const char* p1) -> bf16x8 {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p1));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };
  int boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) boff[i] = arow * 128 + (((4 * (i >> 1) + 2 * (i & 1) + ah) ^ fs_swz(arow)) << 4);
  auto dec_a = [&](int slot, int f) -> bf16x8 {          // W fragment f = 3 ks + dtl of ring slot `slot`
    const char* b = smem + slot * FF_WT_BYTES;
    return tr_pair(b + aoff0[f], b + aoff1[f]);
  };
  auto dec_b = [&](int pb, int hf, int b) -> bf16x8 {    // c^T fragment b = 4 ks + mb of pair buffer pb, tile half hf
    const int ks = b >> 2, mb = b & 3;
    return *reinterpret_cast<const bf16x8*>(cst + boff[2 * hf + ks] + pb * 16384 + mb * 4096);
  };

  // Three W fragments and four c^T fragments in registers (192 accumulators leave 64): fragment (ks, dtl) sits in Afr[dtl] -- k-step
  // 1 replaces k-step 0 fragment by fragment behind its last MFMA (9, 10, 11), the next tile's k-step 0 behind MFMAs 21, 22, 23.
  bf16x8 Afr[3], Bq[4];
  // decoder of "tile -1": zeros from pair buffer 1, half 1 times the cleared ring slot 3
#pragma unroll
  for (int f = 0; f < 3; ++f) Afr[f] = dec_a(3, f);
  Bq[0] = dec_b(1, 1, 0);
  Bq[1] = dec_b(1, 1, 1);

  // The 24 decoder MFMAs of one tile: W fragments out of ring slot SLOT_D, c^T out of (PB_D, HF_D).  HANDOVER: this is iteration j
  // of the loop -- L(j) stands in front of MFMA 20, and behind it the first fragments of tile j (ring slot SLOT_DN, c(j) in
  // (PB_W, HF_W)) are asked for while MFMAs 20..23 issue from registers.
  auto mfmas = [&](auto ph_tag, auto handover_tag) {
    constexpr int PH = decltype(ph_tag)::value;          // == j % 4
    constexpr bool HANDOVER = decltype(handover_tag)::value;
    constexpr int SLOT_D = (PH + 3) & 3, SLOT_DN = PH;
    constexpr int PB_W = (PH >> 1) & 1, HF_W = PH & 1;                     // where c(j) is
    constexpr int PB_D = (((PH + 3) & 3) >> 1) & 1, HF_D = (PH + 3) & 1;   // where c(j-1) is
    static_for<0, 24>([&](auto m_tag) {
      constexpr int m = decltype(m_tag)::value;
      constexpr int ks = m / 12, mb = (m % 12) / 3, dtl = m % 3;
      // c^T fragment b feeds MFMAs 3 b .. 3 b + 2: asked for in front of MFMA 3 b - 4
      if constexpr (m >= 2 && m <= 17 && (m - 2) % 3 == 0) Bq[((m + 4) / 3) & 3] = dec_b(PB_D, HF_D, (m + 4) / 3);
      if constexpr (m == 10 || m == 11 || m == 12) Afr[m - 10] = dec_a(SLOT_D, 3 + m - 10);       // k-step 1
      if constexpr (HANDOVER && m == 20) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                                                // barrier L(j)
        __builtin_amdgcn_sched_barrier(0);
        Bq[0] = dec_b(PB_W, HF_W, 0);
      }
      if constexpr (HANDOVER && m == 22) {
        Bq[1] = dec_b(PB_W, HF_W, 1);
        Afr[0] = dec_a(SLOT_DN, 0);
      }
      if constexpr (HANDOVER && m == 23) Afr[1] = dec_a(SLOT_DN, 1);
      __builtin_amdgcn_sched_barrier(0);
      acc[4 * dtl + mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Afr[dtl], Bq[(4 * ks + mb) & 3], acc[4 * dtl + mb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (HANDOVER) Afr[2] = dec_a(SLOT_DN, 2);
  };
  for (int j4 = 0; j4 < a.ntiles; j4 += 4) {            // ntiles is a multiple of 4
    mfmas(std::integral_constant<int, 0>{}, std::true_type{});
    mfmas(std::integral_constant<int, 1>{}, std::true_type{});
    mfmas(std::integral_constant<int, 2>{}, std::true_type{});
    mfmas(std::integral_constant<int, 3>{}, std::true_type{});
  }
  // final half iteration: decoder of the last tile (slot 3, pair buffer 1, half 1): "iteration ntiles", phase 0, no hand-over
  mfmas(std::integral_constant<int, 0>{}, std::false_type{});
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                                                                      // barrier E0
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue: x_hat^T accumulators -> residual / dx_hat / squared-error sums, as fwd_fused2.h's wave w does it.
  // acc[4 dtl + mb][r] <-> d = 96 w + 32 dtl + (r&3) + 8 (r>>2) + 4 h, row 128 wg + 32 mb + arow.
  float sq = 0.f, plain = 0.f, nmask = 0.f;
  float msq = 0.f;               // lean epilogue: squared error of the MASKED entries (masked MSE numerator = plain - msq)
  f32x2_t plain2 = {0.f, 0.f};   // packed form of the lean epilogue: the squared-error sum of the even / odd elements
  typedef __attribute__((ext_vector_type(4))) T Tx4;
  const bool vec_ok = (a.d == FF_D) && ((reinterpret_cast<uintptr_t>(a.x) & (sizeof(T) * 4 - 1)) == 0);
  constexpr int FF_DXH_PITCH = FF_D * 2 + 16;                    // 784 B
  char* stg = smem;                                              // [128 rows][784 B]
  constexpr bool X_VIA_LDS = !PAD && sizeof(T) == 2;
  const unsigned* mflag = reinterpret_cast<const unsigned*>(smem + FF_FIXED_LDS + 64);
  bool blk_masked = true;
  if (X_VIA_LDS && vec_ok) {            // (block-uniform, and the encoder waves' condition for staging x: both roles meet E1 or neither)
    __syncthreads();                                                                                 // barrier E1
    const u32x4 f = *reinterpret_cast<const u32x4*>(mflag);
    blk_masked = (f[0] | f[1] | f[2] | f[3]) != 0u;
  }
  auto residual = [&](auto notest_tag) {
  constexpr bool NOTEST = decltype(notest_tag)::value;      // (implies vec_ok: the scan that clears a block runs only on the vector path)
  // the groups are software-pipelined by hand (fwd_fused2.h): group g + 1's reads before group g's arithmetic, a fence per group
  constexpr bool FENCE = NOTEST && X_VIA_LDS;
  constexpr bool PIPE = FENCE && std::is_same<T, bf16_t>::value;
  Tx4 xq[2][4];
  auto xload = [&](int g, Tx4 (&dst)[4]) {
    const char* sr = stg + (32 * (g / 3) + arow) * FF_DXH_PITCH + (96 * w + 32 * (g % 3) + 4 * ah) * 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = *reinterpret_cast<const Tx4*>(sr + 16 * k);
  };
  if constexpr (PIPE) xload(0, xq[0]);
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int64_t grow = (int64_t)wg * FF_BM + 32 * mb + arow;   // global activation row of this lane in row block mb
    const bool ok = !PAD || grow < a.M;
    const float rmask = ok ? 1.f : 0.f;
    const T* xrow = reinterpret_cast<const T*>(a.x) + (ok ? grow : a.M - 1) * a.d;
    char* srow = stg + (32 * mb + arow) * FF_DXH_PITCH;
#pragma unroll
    for (int dtl = 0; dtl < 3; ++dtl) {
      const int dbase = 96 * w + 32 * dtl + 4 * ah;
      if (NOTEST || vec_ok) {
        const int g = 3 * mb + dtl;
        if constexpr (FENCE) {
          if (g > 0) __builtin_amdgcn_sched_barrier(0);
          if (PIPE && g + 1 < 12) xload(g + 1, xq[(g + 1) & 1]);
        }
        Tx4 xv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          xv[k] = PIPE ? xq[g & 1][k]
                       : (X_VIA_LDS ? *reinterpret_cast<const Tx4*>(srow + (dbase + 8 * k) * 2) : *reinterpret_cast<const Tx4*>(xrow + dbase + 8 * k));
        if (!PAD) {
          if constexpr (NOTEST && X_VIA_LDS) {      // the block holds no masked entry (scanned while x was staged): no test, no branch
            if constexpr (std::is_same<T, bf16_t>::value) {
              uint2 ow[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const uint2 xw = __builtin_bit_cast(uint2, xv[k]);
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                  const unsigned xd = pp ? xw.y : xw.x;
                  const unsigned rb = __builtin_bit_cast(unsigned, __builtin_convertvector(
                      f32x2_t{acc[4 * dtl + mb][4 * k + 2 * pp], acc[4 * dtl + mb][4 * k + 2 * pp + 1]}, bf16x2));
                  const f32x2_t rf = {__uint_as_float(rb << 16), __uint_as_float(rb & 0xFFFF0000u)};
                  const f32x2_t xf = {__uint_as_float(xd << 16), __uint_as_float(xd & 0xFFFF0000u)};
                  f32x2_t e2, d2;
                  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(e2) : "v"(rf), "v"(xf));
                  asm("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(plain2) : "v"(e2));
                  asm("v_pk_add_f32 %0, %1, %1" : "=v"(d2) : "v"(e2));
                  const unsigned ob = __builtin_bit_cast(unsigned, __builtin_convertvector(d2, bf16x2));
                  if (pp) ow[k].y = ob; else ow[k].x = ob;
                }
              }
#pragma unroll
              for (int k = 0; k < 4; ++k) *reinterpret_cast<uint2*>(srow + (dbase + 8 * k) * 2) = ow[k];
              continue;
            }
            bf16x4 o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const float xf = (float)xv[k][q];
                const float e = bf16_round(acc[4 * dtl + mb][4 * k + q]) - xf;
                plain = __builtin_fmaf(e, e, plain);
                o[k][q] = (bf16_t)(e + e);
              }
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<bf16x4*>(srow + (dbase + 8 * k) * 2) = o[k];
            continue;
          }
          // a block WITH masked entries: selects, no branch
          bf16x4 o[4];
          unsigned nm_i = 0u;
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float xf = (float)xv[k][q];
              const float e = bf16_round(acc[4 * dtl + mb][4 * k + q]) - xf;
              const bool mk = xf == -1.0f;
              const float em = mk ? e : 0.0f, ek = mk ? 0.0f : e;
              plain = __builtin_fmaf(e, e, plain);
              msq = __builtin_fmaf(em, em, msq);
              nm_i += mk ? 1u : 0u;
              o[k][q] = (bf16_t)(ek + ek);
            }
          nmask += (float)nm_i;
#pragma unroll
          for (int k = 0; k < 4; ++k) *reinterpret_cast<bf16x4*>(srow + (dbase + 8 * k) * 2) = o[k];
          continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bf16x4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xf = (float)xv[k][q];
            const float e = bf16_round(acc[4 * dtl + mb][4 * k + q]) - xf;
            const float e2 = e * e;
            plain += rmask * e2;
            const float keep = (xf != -1.0f) ? rmask : 0.f;
            nmask += rmask - keep;
            sq += keep * e2;
            o[q] = (bf16_t)(keep * (e * 2.0f));
          }
          *reinterpret_cast<bf16x4*>(srow + (dbase + 8 * k) * 2) = o;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bf16x4 o;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int dd = dbase + 8 * k + q;
            const bool valid = dd < a.d;
            const float xf = (float)xrow[valid ? dd : a.d - 1];
            const float e = bf16_round(acc[4 * dtl + mb][4 * k + q]) - xf;
            const float e2 = valid ? e * e : 0.f;
            plain += rmask * e2;
            const float keep = (valid && xf != -1.0f) ? rmask : 0.f;
            nmask += (valid ? rmask : 0.f) - keep;
            sq += keep * e2;
            o[q] = (bf16_t)(keep * (e * 2.0f));
          }
          *reinterpret_cast<bf16x4*>(srow + (dbase + 8 * k) * 2) = o;
        }
      }
    }
  }
  };
  if (X_VIA_LDS && vec_ok && !blk_masked) residual(std::true_type{}); else residual(std::false_type{});
  __syncthreads();                                                                                   // barrier E2
  plain += plain2[0] + plain2[1];
  if (!PAD && vec_ok) sq = plain - msq;          // (vec_ok is block-uniform)
  float* red = reinterpret_cast<float*>(smem + FF_FIXED_LDS);     // [4 waves][l1, sq, plain, nmask]
  {
    const float v1 = wave_sum(sq), v2 = wave_sum(plain), v3 = wave_sum(nmask);
    if (lane == 0) { red[4 * w + 1] = v1; red[4 * w + 2] = v2; red[4 * w + 3] = v3; }
  }
  lds_barrier();                                                                                     // barrier E3
}

template <typename T, bool PAD>
__global__ __launch_bounds__(FS_THREADS, 1) void fwd_split_d384_kernel(FwdFusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (wv < 4) fs_encoder_wave<T, PAD>(a, smem, wv, lane);
  else fs_decoder_wave<T, PAD>(a, smem, wv - 4, lane);
}
