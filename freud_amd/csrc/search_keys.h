// Key and merge arithmetic of the feature search (search.h; utils/activations.py:61-132 of the reference, `top_activations`),
// free of any HIP type so that the SAME functions compile for the host: tests/test_search_keys_cpu.py builds them with g++ and
// replays the reference's own answers (tests/golden/search_raw.npz) through them.
//
// Per (file, latent) the kernels leave ONE 64-bit key: ord(value) << 32 | (0xFFFFFFFF - frame).  An unsigned max over a file's
// frames then gives the largest value and, among equal values, the FIRST frame -- torch's max() / argmax() of the trimmed series.
// Per latent the merge keeps a top-N list of rank keys ord(value) << 32 | (0xFFFFFFFF - file): the reference's stable sort by value
// (descending) over files appended in dataset order is the order (value descending, file ascending), and a file that ties the
// N-th entry is dropped (it sorts after it).  A rank key of 0 marks an empty slot (no real value maps to ord 0).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SK_HD __host__ __device__ __forceinline__
#else
#define SK_HD inline
#endif

enum { SK_ABS = 1, SK_HAS_MIN = 2, SK_HAS_MAX = 4 };      // the flags of the merge (include/freud_sae.h: SAE_SEARCH_*)

SK_HD uint32_t sk_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
SK_HD float sk_float(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

// Order-preserving float -> u32: a < b (as floats) <=> sk_ord(a) < sk_ord(b).  -0.0 maps to +0.0's code (torch's max / argmax
// treat them as equal, so must the key); -inf -> 0x007FFFFF, +inf -> 0xFF800000.  NaNs are not ordered (the shards hold none).
SK_HD uint32_t sk_ord(float v) {
  uint32_t u = sk_bits(v);
  if ((u & 0x7FFFFFFFu) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SK_HD float sk_unord(uint32_t o) { return sk_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

SK_HD uint64_t sk_key(float v, uint32_t frame) { return ((uint64_t)sk_ord(v) << 32) | (uint64_t)(0xFFFFFFFFu - frame); }
SK_HD float sk_key_value(uint64_t k) { return sk_unord((uint32_t)(k >> 32)); }
SK_HD uint32_t sk_key_frame(uint64_t k) { return 0xFFFFFFFFu - (uint32_t)k; }
// the key every TopK file starts from: value 0 at frame 0 (a latent that is never selected in a file)
#define SK_KEY_ZERO_FRAME0 ((uint64_t)0x80000000u << 32 | 0xFFFFFFFFull)

// The abs-mode side word of a raw search: the signed value at the frame of max |a| (high half) and the frame of the signed
// max (low half: the reference returns a.argmax() of the SIGNED series as the time even in abs mode, activations.py:120-121).
SK_HD uint64_t sk_aux(float signed_value, uint32_t signed_argmax) { return ((uint64_t)sk_bits(signed_value) << 32) | signed_argmax; }

// activations.py:86-91: value > max_val or value < min_val rejects (Python floats: the fp32 value compared in double)
SK_HD bool sk_pass(float value, int flags, double min_val, double max_val) {
  if ((flags & SK_HAS_MAX) && (double)value > max_val) return false;
  if ((flags & SK_HAS_MIN) && (double)value < min_val) return false;
  return true;
}

// One file's candidate for one latent.  key: the file key; aux: its abs-mode side word or null (SAE latents are >= 0, so
// argmax |a| = argmax a and the abs mode equals the plain one).  -> the value that is filtered and reported per file (signed),
// the value that is ranked, the frame that is returned.
struct SkCand { float filt, rank; uint32_t frame; };
SK_HD SkCand sk_candidate(uint64_t key, const uint64_t* aux, int flags) {
  SkCand c;
  c.rank = sk_key_value(key);
  c.filt = c.rank;
  c.frame = sk_key_frame(key);
  if ((flags & SK_ABS) && aux) {
    c.filt = sk_float((uint32_t)(*aux >> 32));
    c.frame = (uint32_t)*aux;
  }
  return c;
}

// Insert (rank key r, frame) into the list rk[0], rk[stride], ... rk[(n_top - 1) stride] (descending; 0 = empty).  Files arrive in
// ascending order, so an equal value never displaces an earlier file.
SK_HD void sk_insert(uint64_t* rk, int32_t* frames, int64_t stride, int n_top, uint64_t r, int32_t frame) {
  if (r <= rk[(int64_t)(n_top - 1) * stride]) return;
  int i = n_top - 1;
  while (i > 0 && rk[(int64_t)(i - 1) * stride] < r) {
    rk[(int64_t)i * stride] = rk[(int64_t)(i - 1) * stride];
    frames[(int64_t)i * stride] = frames[(int64_t)(i - 1) * stride];
    --i;
  }
  rk[(int64_t)i * stride] = r;
  frames[(int64_t)i * stride] = frame;
}

// The reference's loop body for one (file, latent): filter, then append + stable sort + truncate.
SK_HD void sk_merge_file(uint64_t* rk, int32_t* frames, int64_t stride, int n_top, uint64_t key, const uint64_t* aux, int flags,
                         double min_val, double max_val, int64_t file) {
  const SkCand c = sk_candidate(key, aux, flags);
  if (!sk_pass(c.filt, flags, min_val, max_val)) return;
  const float rv = (flags & SK_ABS) ? (c.rank < 0.f ? -c.rank : c.rank) : c.rank;
  sk_insert(rk, frames, stride, n_top, ((uint64_t)sk_ord(rv) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)file), (int32_t)c.frame);
}
SK_HD int64_t sk_rank_file(uint64_t r) { return r == 0 ? -1 : (int64_t)(0xFFFFFFFFu - (uint32_t)r); }
SK_HD float sk_rank_value(uint64_t r) { return sk_unord((uint32_t)(r >> 32)); }
