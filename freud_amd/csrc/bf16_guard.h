// fp32 -> bf16 as the activation loader delivers it (host_convert.c: f32_to_bf16), as ONE scalar rule that compiles for the device
// (resident.h: sae_store_convert) and for the host (tests/test_resident_cpu.py builds it with g++ and holds it to
// freud_f32_to_bf16_portable of libfreud_host.so):
//   round to nearest even on the bit pattern;
//   a NaN stays a quiet NaN: (u >> 16) | 0x40;
//   -1.0 is the reference's mask value (mse_loss, src/models/l1autoencoder.py:31): a value that is not -1.0 but would round to
//   0xBF80 goes to the neighbouring bf16 on its own side, 0xBF81 (below -1.0) or 0xBF7F (above), and stays unmasked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BG_HD __host__ __device__ __forceinline__
#else
#define BG_HD inline
#endif

// the bits of an fp32 value -> the bits of its bf16 (in the low half of the result); selects only, no branch
BG_HD uint32_t bg_f32_bits_to_bf16(uint32_t u) {
  uint32_t b = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  const bool nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
  b = nan ? ((u >> 16) | 0x0040u) : b;
  const bool guard = (b == 0xBF80u) && (u != 0xBF800000u);
  b = guard ? ((u > 0xBF800000u) ? 0xBF81u : 0xBF7Fu) : b;
  return b;
}
