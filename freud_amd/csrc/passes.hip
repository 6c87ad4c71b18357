// libfreud_sae.so -- the analysis layer of the C ABI declared in include/freud_sae.h: the file passes (one batch of files encoded
// with the training kernels of engine.hip, then the pass's own kernels) and the context-free utilities on their outputs.
// What it calls of engine.hip is declared in engine_internal.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <utility>

#include "engine_internal.h"
#include "gemm_launch.h"
#include "search.h"
#include "file_top.h"
#include "stats.h"
#include "coact.h"
#include "labels.h"
#include "cross.h"
#include "hist.h"
#include "timing.h"
#include "collect.h"
#include "findex.h"
#include "manip.h"
#include "dict_match.h"
#include "recon.h"
#include "frontier.h"
#include "pursuit.h"
#include "refit.h"
#include "resample.h"
#include "input_stats.h"
#include "input_cov_plan.h"
#include "input_cov.h"
#include "resident.h"
#include "frame_gather.h"

// ---- feature search (search.h; the reference's top_activations, utils/activations.py:61-132, for every latent at once)
static int search_launch_colreduce(const void* x, int x_dtype, int64_t ld, int ncols, int Trows, int64_t n_files, const int* lengths,
                                   bool absolute, uint64_t* keys, uint64_t* aux, hipStream_t s) {
  const int chunk = 128;
  const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)n_files, (unsigned)((Trows + chunk - 1) / chunk));
  const int64_t pairs = n_files * ncols;
  const unsigned fgrid = (unsigned)((pairs + 255) / 256);
  int rc = with_x_type(x_dtype, x, [&](auto* xt) {
    using T = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
    if (absolute) {
      hipLaunchKernelGGL((search_colreduce_kernel<T, true>), grid, dim3(256), 0, s, xt, ld, ncols, Trows, lengths, chunk, keys, aux);
      hipLaunchKernelGGL(search_abs_fixup_kernel<T>, dim3(fgrid), dim3(256), 0, s, xt, ld, ncols, Trows, n_files, keys, aux);
    } else {
      hipLaunchKernelGGL((search_colreduce_kernel<T, false>), grid, dim3(256), 0, s, xt, ld, ncols, Trows, lengths, chunk, keys, nullptr);
    }
    return (int)SAE_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- what the file passes share (FilePassKind, engine_internal.h): one batch of files encoded with the training kernels
static int search_shape_check(int64_t n_files, int64_t rows_per_file) {
  if (n_files <= 0 || rows_per_file <= 0) return fail(SAE_ERR_INVALID, "n_files=%lld and rows_per_file=%lld must be positive", (long long)n_files, (long long)rows_per_file);
  if (n_files > 65535) return fail(SAE_ERR_INVALID, "n_files=%lld > 65535 in one call", (long long)n_files);
  // (the column reduction launches one grid z-slice per 128 rows of a file: at most 65535 of them)
  if (rows_per_file > 65535ll * 128) return fail(SAE_ERR_INVALID, "rows_per_file=%lld > %lld", (long long)rows_per_file, 65535ll * 128);
  return SAE_OK;
}

// the front door of every file pass: argument checks (nothing is enqueued when one fails), then the context's device
static int file_pass_begin(const FilePassKind& kind, sae_ctx* c, const void* x, const void* out, int64_t n_files, int64_t rows_per_file,
                           int x_dtype, int flags, int64_t* M) {
  if (!c || !x || !out) return fail(SAE_ERR_INVALID, "null argument");
  if (c->fp8) return fail(SAE_ERR_INVALID, "%s: fp8 contexts are not supported (%s)", kind.fn, kind.fp8_advice);
  if (int rc = search_shape_check(n_files, rows_per_file)) return rc;
  *M = n_files * rows_per_file;
  if (*M > c->cfg.max_rows) return fail(SAE_ERR_INVALID, "n_files * rows_per_file = %lld > max_rows=%lld", (long long)*M, (long long)c->cfg.max_rows);
  if (x_dtype != SAE_DTYPE_F32 && x_dtype != SAE_DTYPE_F16 && x_dtype != SAE_DTYPE_BF16) return fail(SAE_ERR_INVALID, "unknown x_dtype %d", x_dtype);
  if (flags & ~kind.flags_mask) return fail(SAE_ERR_INVALID, "unknown %s flags 0x%x", kind.flags_noun, flags);
  USE_DEVICE(c);
  return SAE_OK;
}

// The passes' one scratch (c->pass_scratch, grow-only): a pass names the bytes of each area it needs and gets their bases, each
// aligned to 256 bytes.  The areas hold whatever the last pass left there -- a pass clears what its kernels assume clear.
static int pass_scratch(sae_ctx* c, std::initializer_list<int64_t> bytes, char** base) {
  int64_t total = 0;
  for (const int64_t b : bytes) total += round_up(b, 256);
  CTX_MEM(grow, pass_scratch, total, DM_DEVICE);     // (a grow frees first: hipFree waits for the work that still reads the old block)
  char* p = c->pass_scratch;
  for (const int64_t b : bytes) {
    *base++ = p;
    p += round_up(b, 256);
  }
  return SAE_OK;
}

// L1: the training forward's (l1_prepare) weights preparation and bf16 copy of x, then the GEMM arguments of its encoder -- for the epilogue the pass
// brings (EpiSearch, EpiStats) where the GEMM streams, for file_pass_l1_encode and a reduction of the stored latent where it does not
template <typename T>
static GemmArgs file_pass_l1_front(sae_ctx* c, const T* x, int64_t M, hipStream_t s) {
  int64_t Mp = round_up(M, 128);
  if (round_up(M, 256) <= c->max_rows_p) Mp = round_up(M, 256);    // (an even number of row blocks: the streaming GEMM's condition)
  prep_weights_l1(c, s);
  launch_prep_x_dtype(c, x, x_dtype_of<T>(), M, Mp, s);
  return enc_gemm_args(c, c->xb, Mp);
}

// the pass's own epilogue in the streaming GEMM, inside the encoder's event bracket
template <class Epi>
static int file_pass_l1_fused(sae_ctx* c, const GemmArgs& g, const Epi& e, hipStream_t s) {
  ev_begin(c, KID_ENC_FWD, s);
  const int rc = launch_gemm_stream(g, e, s);
  ev_end(c, KID_ENC_FWD, s);
  return rc;
}

// L1: the batch's latent as encode() returns it, stored as bf16 rows in c->c -- the front (the caller's own `front` where it has run
// one to decide on its fused form), then the ordinary encoder.  Mp: the rows the front padded to.
template <typename T>
static int file_pass_l1_encode(sae_ctx* c, const T* x, int64_t M, hipStream_t s, const GemmArgs* front = nullptr, int64_t* Mp = nullptr) {
  const GemmArgs g = front ? *front : file_pass_l1_front(c, x, M, s);
  if (Mp) *Mp = (int64_t)g.nbm * 128;
  return launch_encoder_l1(c, g, M, s);
}

// The encoder as encode() runs it: the stored L1 latent, or c->top_idx / c->top_vals of the eval forward (encoder GEMM + top-k
// selection, the k of encode())
static int file_pass_encode(sae_ctx* c, const void* x, int64_t M, int x_dtype, hipStream_t s) {
  if (c->topk) return dispatch_fwd_bwd(c, x, M, x_dtype, s, false);
  return with_x_type(x_dtype, x, [&](auto* xt) { return file_pass_l1_encode(c, xt, M, s); });
}

// L1 search: where the streaming GEMM does not apply (small or odd shapes, FREUD_GEMM_STREAM=0, force_gemm128) or `unfused` is asked
// for (the baseline of tools/bench_search.py), the latent is stored by the ordinary encoder and reduced by the column kernel.
template <typename T>
static int search_l1_impl(sae_ctx* c, const T* x, int64_t M, int Trows, int64_t n_files, const int* lengths, uint64_t* keys, bool unfused,
                          hipStream_t s) {
  const GemmArgs g = file_pass_l1_front(c, x, M, s);
  HIP_TRY(hipMemsetAsync(keys, 0, (size_t)n_files * c->n * 8, s));
  if (!unfused && Trows <= 65535 && gemm_streams<OP_ROW, OP_ROW, EpiSearch>(g)) {
    EpiSearch e{};
    e.bias = c->P + c->nW; e.keys = keys; e.lengths = lengths; e.M = M; e.T = Trows; e.n = c->n;
    return file_pass_l1_fused(c, g, e, s);
  }
  if (int rc = file_pass_l1_encode(c, x, M, s, &g)) return rc;
  return search_launch_colreduce(c->c, SAE_DTYPE_BF16, c->n_p, c->n, Trows, n_files, lengths, false, keys, nullptr, s);
}

extern "C" int sae_search_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                int flags, uint64_t* file_keys, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kSearchPass, c, x, file_keys, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  if (c->topk) {
    // the keys filled, then the selection of encode() scattered into them
    const int64_t nk = n_files * c->n;
    hipLaunchKernelGGL(search_fill_kernel, dim3(grid_for(nk, 4096)), dim3(256), 0, s, file_keys, nk, (uint64_t)SK_KEY_ZERO_FRAME0);
    if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
    hipLaunchKernelGGL(search_topk_scatter_kernel, dim3(grid_for(M * c->k, 4096)), dim3(256), 0, s, c->top_idx, c->top_vals, c->k, M, Trows,
                       lengths, c->n, file_keys);
    HIP_TRY(hipGetLastError());
  } else {
    const bool unfused = (flags & SAE_SEARCH_UNFUSED) != 0;
    if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return search_l1_impl(c, xt, M, Trows, n_files, lengths, file_keys, unfused, s); }))
      return rc;
  }
  file_pass_end(kSearchPass, c);
  return SAE_OK;
}

extern "C" int sae_search_raw_files(const void* x, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths,
                                    int absolute, uint64_t* file_keys, uint64_t* aux, void* stream) {
  if (!x || !file_keys || (absolute && !aux)) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = search_shape_check(n_files, rows_per_file)) return rc;
  if (d <= 0 || d > (1 << 24)) return fail(SAE_ERR_INVALID, "d=%lld outside (0, 2^24]", (long long)d);
  if (x_dtype != SAE_DTYPE_F32 && x_dtype != SAE_DTYPE_F16 && x_dtype != SAE_DTYPE_BF16) return fail(SAE_ERR_INVALID, "unknown x_dtype %d", x_dtype);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(file_keys, 0, (size_t)(n_files * d) * 8, s));
  if (absolute) HIP_TRY(hipMemsetAsync(aux, 0, (size_t)(n_files * d) * 8, s));
  return search_launch_colreduce(x, x_dtype, d, (int)d, (int)rows_per_file, n_files, lengths, absolute != 0, file_keys, aux, s);
}

extern "C" int sae_search_merge(const uint64_t* file_keys, const uint64_t* aux, int64_t n_files, int64_t ncols, int64_t file0, int n_top,
                                int flags, double min_val, double max_val, uint64_t* top_keys, int32_t* top_frames, void* stream) {
  if (!file_keys || !top_keys || !top_frames) return fail(SAE_ERR_INVALID, "null argument");
  if (n_files <= 0 || ncols <= 0 || file0 < 0) return fail(SAE_ERR_INVALID, "n_files=%lld, ncols=%lld, file0=%lld", (long long)n_files, (long long)ncols, (long long)file0);
  if (file0 + n_files >= 0xFFFFFFFFll) return fail(SAE_ERR_INVALID, "file indices beyond 2^32 - 2");
  if (n_top < 1 || n_top > SAE_SEARCH_MAX_TOP) return fail(SAE_ERR_INVALID, "n_top=%d outside [1, %d]", n_top, SAE_SEARCH_MAX_TOP);
  if (flags & ~(SAE_SEARCH_ABS | SAE_SEARCH_MIN | SAE_SEARCH_MAX)) return fail(SAE_ERR_INVALID, "unknown merge flags 0x%x", flags);
  hipLaunchKernelGGL(search_merge_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, file_keys, aux, n_files,
                     ncols, file0, n_top, flags, min_val, max_val, top_keys, top_frames);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_search_file_values(const uint64_t* file_keys, const uint64_t* aux, int64_t n_files, int64_t ncols, int flags,
                                      const int32_t* latents, int64_t n_latents, int64_t file0, int64_t out_stride, float* out, void* stream) {
  if (!file_keys || !latents || !out) return fail(SAE_ERR_INVALID, "null argument");
  if (n_files <= 0 || ncols <= 0 || n_latents <= 0 || file0 < 0) return fail(SAE_ERR_INVALID, "empty or negative extent");
  if (out_stride < file0 + n_files) return fail(SAE_ERR_INVALID, "out_stride=%lld < file0 + n_files=%lld", (long long)out_stride, (long long)(file0 + n_files));
  const int64_t total = n_latents * n_files;
  hipLaunchKernelGGL(search_values_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, file_keys, aux, n_files,
                     ncols, flags, latents, n_latents, file0, out_stride, out);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- file features (file_top.h): the top-N latents of every file of a batch, selected from its file keys
static_assert(SAE_FILE_TOP_POSITIVE == FT_POSITIVE && SAE_FILE_TOP_MAX == FT_MAX_TOP, "freud_sae.h and file_top.h disagree");

extern "C" int sae_file_top_features(const uint64_t* file_keys, int64_t n_files, int64_t ncols, int n_top, int flags, int32_t* top_latents,
                                     uint64_t* top_keys, void* stream) {
  if (!file_keys || !top_latents || !top_keys) return fail(SAE_ERR_INVALID, "null argument");
  if (n_files < 1 || ncols < 1) return fail(SAE_ERR_INVALID, "n_files=%lld, ncols=%lld", (long long)n_files, (long long)ncols);
  if (n_files > 0x7FFFFFFFll || ncols > FT_MAX_COLS) return fail(SAE_ERR_INVALID, "n_files=%lld > 2^31 - 1 or ncols=%lld > 2^24", (long long)n_files, (long long)ncols);
  if (n_top < 1 || n_top > SAE_FILE_TOP_MAX) return fail(SAE_ERR_INVALID, "n_top=%d outside [1, %d]", n_top, SAE_FILE_TOP_MAX);
  if (flags & ~SAE_FILE_TOP_POSITIVE) return fail(SAE_ERR_INVALID, "unknown file-top flags 0x%x", flags);
  hipLaunchKernelGGL(file_top_kernel, dim3((unsigned)n_files), dim3(FT_THREADS), 0, (hipStream_t)stream, file_keys, ncols, n_top, flags,
                     top_latents, top_keys);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- feature statistics (stats.h): per-latent firing counts, sums, maxima and the L0 histogram of one batch of files
// its scratch area: the slab [max_rows_p / STATS_RB][n] x 4 words of 4 bytes, then (L1) one L0 byte per row and 64 latents.  Every
// slab row and L0 byte a call reads it has written with plain stores first: nothing to clear.
static int64_t stats_slab_words(const sae_ctx* c) { return (c->max_rows_p / STATS_RB) * (int64_t)c->n; }
static uint8_t* stats_l0_bytes(const sae_ctx* c, char* base) { return (uint8_t*)base + stats_slab_words(c) * 16; }
static int64_t stats_scratch_bytes(const sae_ctx* c) {
  return stats_slab_words(c) * 16 + (c->topk ? 0 : c->max_rows_p * (int64_t)(c->n_p / 64));
}

static StatsSlab stats_slab(const sae_ctx* c, char* base) {
  const int64_t words = stats_slab_words(c);
  StatsSlab sl;
  sl.cnt = (uint32_t*)base;
  sl.mx = sl.cnt + words;
  sl.sum = (float*)(sl.mx + words);
  sl.sq = sl.sum + words;
  return sl;
}

struct StatsOut {               // the caller's block (include/freud_sae.h, SAE_STATS_*)
  unsigned long long *n_frames, *fire, *hist;
  double *asum, *asq;
  float* amax;
};

static StatsOut stats_out(void* block, int n) {
  char* b = (char*)block;
  StatsOut o;
  o.n_frames = (unsigned long long*)(b + SAE_STATS_N_FRAMES(n));
  o.fire = (unsigned long long*)(b + SAE_STATS_FIRE_COUNT(n));
  o.asum = (double*)(b + SAE_STATS_ACT_SUM(n));
  o.asq = (double*)(b + SAE_STATS_ACT_SQ_SUM(n));
  o.hist = (unsigned long long*)(b + SAE_STATS_L0_HIST(n));
  o.amax = (float*)(b + SAE_STATS_ACT_MAX(n));
  return o;
}

template <class Src>
static void stats_launch_l0(Src src, int64_t M, int T, const int* lengths, int n, const StatsOut& o, hipStream_t s) {
  hipLaunchKernelGGL(stats_l0_kernel<Src>, dim3(grid_for(M, 1024, 4)), dim3(256), 0, s, src, M, T, lengths, n + 1, o.hist, o.n_frames);
}

static void stats_launch_fold(sae_ctx* c, const StatsSlab& sl, int nrb, const StatsOut& o, hipStream_t s) {
  hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, sl, nrb, c->n, o.fire, o.asum, o.asq, o.amax);
}

// L1 statistics: where the streaming GEMM does not apply, or `unfused` is asked for, the ordinary encoder stores the latent and two
// kernels reduce it (column statistics into the slab, row counts into the histogram).
template <typename T>
static int stats_l1_impl(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, const StatsOut& o, bool unfused, char* scratch,
                         hipStream_t s) {
  const int n_p = c->n_p;
  const GemmArgs g = file_pass_l1_front(c, x, M, s);
  const StatsSlab sl = stats_slab(c, scratch);
  const int nrb = (int)((M + STATS_RB - 1) / STATS_RB);
  if (!unfused && gemm_streams<OP_ROW, OP_ROW, EpiStats>(g)) {
    uint8_t* l0b = stats_l0_bytes(c, scratch);
    EpiStats e{};
    e.bias = c->P + c->nW; e.slab = sl; e.l0b = l0b; e.lengths = lengths; e.M = M; e.T = Trows; e.n = c->n; e.ncb = n_p / 64;
    e.inv_T = 1.0f / (float)Trows;
    if (int rc = file_pass_l1_fused(c, g, e, s)) return rc;
    stats_launch_l0(L0Bytes{l0b, n_p / 64}, M, Trows, lengths, c->n, o, s);
  } else {
    if (int rc = file_pass_l1_encode(c, x, M, s, &g)) return rc;
    const unsigned short* lat = (const unsigned short*)c->c;
    hipLaunchKernelGGL(stats_colreduce_kernel, dim3((unsigned)((c->n + 255) / 256), (unsigned)nrb), dim3(256), 0, s, lat, (int64_t)n_p, c->n,
                       M, Trows, lengths, sl);
    stats_launch_l0(L0Latent{lat, n_p, c->n}, M, Trows, lengths, c->n, o, s);
  }
  stats_launch_fold(c, sl, nrb, o, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_stats_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                               int flags, void* stats, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kStatsPass, c, x, stats, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(stats, 8)) return fail(SAE_ERR_INVALID, "the stats block must be 8-byte aligned");
  char* scratch;
  if (int rc = pass_scratch(c, {stats_scratch_bytes(c)}, &scratch)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  const StatsOut o = stats_out(stats, c->n);
  if (c->topk) {
    // the statistics of encode()'s selection
    if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
    const int nrb = (int)((M + STATS_TK_RB - 1) / STATS_TK_RB);
    const unsigned short* vals = (const unsigned short*)c->top_vals;
    hipLaunchKernelGGL(stats_topk_cols_kernel, dim3((unsigned)nrb, (unsigned)((c->n + STATS_TK_SEG - 1) / STATS_TK_SEG)), dim3(64), 0, s,
                       c->top_idx, vals, c->k, M, Trows, lengths, c->n, stats_slab(c, scratch));
    stats_launch_l0(L0Topk{vals, c->k}, M, Trows, lengths, c->n, o, s);
    stats_launch_fold(c, stats_slab(c, scratch), nrb, o, s);
    HIP_TRY(hipGetLastError());
  } else {
    const bool unfused = (flags & SAE_STATS_UNFUSED) != 0;
    if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return stats_l1_impl(c, xt, M, Trows, lengths, o, unfused, scratch, s); })) return rc;
  }
  file_pass_end(kStatsPass, c);
  return SAE_OK;
}

// ---- feature co-activation (coact.h): C += Zt Zt^T of one batch of files on the i8 MFMA, and the neighbour keys of rows of C
static_assert(SAE_COACT_JACCARD == CO_JACCARD && SAE_COACT_COND == CO_COND && SAE_COACT_COUNT == CO_COUNT, "freud_sae.h and coact.h disagree");

// its scratch area: the int8 mask Zt [n_p][round_up(max_rows_p, CO_BK)], every byte of a call's [n_p][Kp] written by its pack (L1)
// or cleared before the scatter (TopK)
static int64_t coact_zt_bytes(const sae_ctx* c) { return (int64_t)c->n_p * round_up(c->max_rows_p, CO_BK); }

// the K split of coact.h's header: enough slices of the Kp / CO_BK steps that `tiles` output tiles fill CO_MIN_WGS workgroups, `per` steps each
struct KSplit { int ksplit, per; };
static KSplit coact_ksplit(int64_t tiles, int64_t Kp) {
  const int nsteps = (int)(Kp / CO_BK);
  const int want = (int)std::min<int64_t>(std::max<int64_t>((CO_MIN_WGS + tiles - 1) / tiles, 1), nsteps);
  const int per = (nsteps + want - 1) / want;
  return {(nsteps + per - 1) / per, per};
}

// the update of one batch's mask Zt [n_p][Kp] (n_p a multiple of CO_BM)
static int coact_launch_update(sae_ctx* c, const int8_t* zt, int64_t Kp, int n_p, int n, int32_t* counts, hipStream_t s) {
  const int nt = n_p / CO_BM;
  const int64_t ntiles = (int64_t)nt * (nt + 1) / 2;
  const KSplit ks = coact_ksplit(ntiles, Kp);
  const dim3 grid((unsigned)nt, (unsigned)nt, (unsigned)ks.ksplit);
  ev_begin(c, KID_COACT_UPDATE, s);
  if (ks.ksplit > 1) hipLaunchKernelGGL(coact_update_kernel<true>, grid, dim3(256), 0, s, zt, Kp, n, ks.per, counts);
  else hipLaunchKernelGGL(coact_update_kernel<false>, grid, dim3(256), 0, s, zt, Kp, n, ks.per, counts);
  ev_end(c, KID_COACT_UPDATE, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// the batch's activity mask into zt: the encoder as encode() runs it, then the mask pack (sae_coact_files, sae_label_files)
static int coact_encode_pack(sae_ctx* c, const void* x, int64_t M, int Trows, int x_dtype, const int32_t* lengths, int8_t* zt, int64_t Kp,
                             void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
  ev_begin(c, KID_COACT_PACK, s);
  hipError_t memset_zt = hipSuccess;
  if (c->topk) {                            // the selection scattered into the zeroed mask
    memset_zt = hipMemsetAsync(zt, 0, (size_t)((int64_t)c->n_p * Kp), s);
    if (memset_zt == hipSuccess)
      hipLaunchKernelGGL(coact_pack_topk_kernel, dim3(grid_for(M * c->k, 4096)), dim3(256), 0, s, c->top_idx, (const unsigned short*)c->top_vals,
                         c->k, M, Trows, lengths, c->n, zt, Kp);
  } else {
    hipLaunchKernelGGL(coact_pack_l1_kernel, dim3((unsigned)(Kp / 64), (unsigned)(c->n_p / 64)), dim3(256), 0, s, (const unsigned short*)c->c,
                       (int64_t)c->n_p, c->n, M, Trows, lengths, zt, Kp);
  }
  ev_end(c, KID_COACT_PACK, s);             // (the bracket closes whatever the memset answered)
  HIP_TRY(memset_zt);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_coact_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                               int flags, int32_t* counts, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kCoactPass, c, x, counts, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(counts, 4)) return fail(SAE_ERR_INVALID, "the count table must be 4-byte aligned");
  char* zt;
  if (int rc = pass_scratch(c, {coact_zt_bytes(c)}, &zt)) return rc;
  const int64_t Kp = round_up(M, CO_BK);
  if (int rc = coact_encode_pack(c, x, M, (int)rows_per_file, x_dtype, lengths, (int8_t*)zt, Kp, stream)) return rc;
  if (int rc = coact_launch_update(c, (int8_t*)zt, Kp, c->n_p, c->n, counts, (hipStream_t)stream)) return rc;
  file_pass_end(kCoactPass, c);
  return SAE_OK;
}

extern "C" int sae_coact_neighbor_keys(const int32_t* counts, int64_t n, int64_t row0, int64_t n_rows, int measure, uint64_t* keys, void* stream) {
  if (!counts || !keys) return fail(SAE_ERR_INVALID, "null argument");
  if (n < 1 || n > FT_MAX_COLS) return fail(SAE_ERR_INVALID, "n=%lld outside [1, 2^24]", (long long)n);
  if (n_rows < 1 || row0 < 0 || row0 + n_rows > n)
    return fail(SAE_ERR_INVALID, "rows [%lld, %lld) are empty or outside [0, %lld)", (long long)row0, (long long)(row0 + n_rows), (long long)n);
  if (measure != SAE_COACT_JACCARD && measure != SAE_COACT_COND && measure != SAE_COACT_COUNT) return fail(SAE_ERR_INVALID, "unknown measure %d", measure);
  hipLaunchKernelGGL(coact_keys_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<int64_t>(n_rows, 65535)), dim3(256), 0,
                     (hipStream_t)stream, counts, (int)n, row0, n_rows, measure, keys);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- feature labels (labels.h): A += Lt Zt^T of one batch of files -- co-activation's mask against the frames' labels -- and the keys
// of a block of rows of A in either orientation
static_assert(SAE_LABEL_F1 == LB_F1 && SAE_LABEL_PRECISION == LB_PRECISION && SAE_LABEL_RECALL == LB_RECALL && SAE_LABEL_COUNT == LB_COUNT &&
              SAE_LABEL_MAX_CLASSES == LB_MAX_CLASSES && SAE_LABEL_MAX_SLOTS == LB_MAX_SLOTS, "freud_sae.h and labels.h disagree");

extern "C" int sae_label_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                               const int32_t* labels, int n_slots, int n_classes, int flags, int32_t* counts, int64_t* label_count,
                               void* stream) {
  int64_t M;
  if (!labels || !label_count) return fail(SAE_ERR_INVALID, "null argument");
  if (n_slots < 1 || n_slots > SAE_LABEL_MAX_SLOTS) return fail(SAE_ERR_INVALID, "n_slots=%d outside [1, %d]", n_slots, SAE_LABEL_MAX_SLOTS);
  if (n_classes < 1 || n_classes > SAE_LABEL_MAX_CLASSES) return fail(SAE_ERR_INVALID, "n_classes=%d outside [1, %d]", n_classes, SAE_LABEL_MAX_CLASSES);
  if (misaligned(counts, 4) || misaligned(label_count, 8))
    return fail(SAE_ERR_INVALID, "the count table must be 4-byte aligned and label_count 8-byte aligned");
  if (int rc = file_pass_begin(kLabelPass, c, x, counts, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  const int C_p = (int)round_up(n_classes + 1, CO_BM);
  // two scratch areas: co-activation's mask and the int8 label pack Lt [C_p][round_up(max_rows_p, CO_BK)] (its [C_p][Kp] cleared below)
  char* area[2];
  if (int rc = pass_scratch(c, {coact_zt_bytes(c), (int64_t)C_p * round_up(c->max_rows_p, CO_BK)}, area)) return rc;
  int8_t *zt = (int8_t*)area[0], *lt = (int8_t*)area[1];
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  const int64_t Kp = round_up(M, CO_BK);
  if (int rc = coact_encode_pack(c, x, M, Trows, x_dtype, lengths, zt, Kp, stream)) return rc;

  ev_begin(c, KID_LABEL_PACK, s);
  const hipError_t memset_lt = hipMemsetAsync(lt, 0, (size_t)((int64_t)C_p * Kp), s);
  if (memset_lt == hipSuccess) {
    hipLaunchKernelGGL(label_pack_kernel, dim3(grid_for(M * n_slots, 4096)), dim3(256), 0, s, labels, n_slots, n_classes, M, Trows, lengths,
                       lt, Kp);
    hipLaunchKernelGGL(label_count_kernel, dim3((unsigned)(n_classes + 1)), dim3(256), 0, s, lt, Kp, (unsigned long long*)label_count);
  }
  ev_end(c, KID_LABEL_PACK, s);             // (the bracket closes whatever the memset answered)
  HIP_TRY(memset_lt);
  HIP_TRY(hipGetLastError());

  // the K split of coact.h's header over the rectangle's tiles
  const int ntr = C_p / CO_BM, ntc = c->n_p / CO_BM;
  const KSplit ks = coact_ksplit(ntr * ntc, Kp);
  const dim3 grid((unsigned)ntc, (unsigned)ntr, (unsigned)ks.ksplit);
  ev_begin(c, KID_LABEL_UPDATE, s);
  if (ks.ksplit > 1) hipLaunchKernelGGL(label_update_kernel<true>, grid, dim3(256), 0, s, lt, zt, Kp, n_classes + 1, c->n, ks.per, counts);
  else hipLaunchKernelGGL(label_update_kernel<false>, grid, dim3(256), 0, s, lt, zt, Kp, n_classes + 1, c->n, ks.per, counts);
  ev_end(c, KID_LABEL_UPDATE, s);
  HIP_TRY(hipGetLastError());
  file_pass_end(kLabelPass, c);
  return SAE_OK;
}

extern "C" int sae_label_keys(const int32_t* counts, const int64_t* label_count, int64_t n_classes, int64_t n, int measure, int by_latent,
                              int64_t row0, int64_t n_rows, uint64_t* keys, void* stream) {
  if (!counts || !label_count || !keys) return fail(SAE_ERR_INVALID, "null argument");
  if (n_classes < 1 || n_classes > SAE_LABEL_MAX_CLASSES) return fail(SAE_ERR_INVALID, "n_classes=%lld outside [1, %d]", (long long)n_classes, SAE_LABEL_MAX_CLASSES);
  if (n < 1 || n > FT_MAX_COLS) return fail(SAE_ERR_INVALID, "n=%lld outside [1, 2^24]", (long long)n);
  if (by_latent != 0 && by_latent != 1) return fail(SAE_ERR_INVALID, "by_latent=%d is neither 0 nor 1", by_latent);
  const int64_t rows_all = by_latent ? n : n_classes, ncols = by_latent ? n_classes : n;
  if (n_rows < 1 || row0 < 0 || row0 + n_rows > rows_all)
    return fail(SAE_ERR_INVALID, "rows [%lld, %lld) are empty or outside [0, %lld)", (long long)row0, (long long)(row0 + n_rows), (long long)rows_all);
  if (measure != SAE_LABEL_F1 && measure != SAE_LABEL_PRECISION && measure != SAE_LABEL_RECALL && measure != SAE_LABEL_COUNT)
    return fail(SAE_ERR_INVALID, "unknown measure %d", measure);
  hipLaunchKernelGGL(label_keys_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)std::min<int64_t>(n_rows, 65535)), dim3(256), 0,
                     (hipStream_t)stream, counts, label_count, (int)n_classes, (int)n, measure, by_latent, row0, n_rows, keys);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- cross-activation (cross.h): the lag-aware masks of one batch of files into caller-owned memory, then -- without a context --
// X += source x target^T of two such masks on label_update_kernel, and the keys of a block of rows of X in either orientation
static_assert(SAE_CROSS_JACCARD == CX_JACCARD && SAE_CROSS_COND == CX_COND && SAE_CROSS_LIFT == CX_LIFT && SAE_CROSS_COUNT == CX_COUNT &&
              SAE_CROSS_SOURCE == CX_SOURCE && SAE_CROSS_TARGET == CX_TARGET && SAE_CROSS_MAX_LAG == CX_MAX_LAG &&
              SAE_CROSS_MAX_LAGS == CX_MAX_LAGS, "freud_sae.h and cross.h disagree");

static bool cross_dims_ok(int64_t n, int64_t rows) { return n >= 1 && n <= CX_MAX_N && rows >= 1 && rows <= 65535ll * CO_BK; }
static int64_t cross_rows_p(int64_t n) { return round_up(n + 1, CO_BM); }

extern "C" int64_t sae_cross_mask_bytes(int64_t n_dict, int64_t rows) {
  return cross_dims_ok(n_dict, rows) ? cross_rows_p(n_dict) * round_up(rows, CO_BK) : 0;
}

extern "C" int sae_cross_mask_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                    int sides, const int32_t* lags_host, int n_lags, void* masks, int64_t masks_bytes, void* stream) {
  int64_t M;
  if (sides < 1 || sides > (CX_SOURCE | CX_TARGET)) return fail(SAE_ERR_INVALID, "sides=%d is not SAE_CROSS_SOURCE, SAE_CROSS_TARGET or both", sides);
  const bool targets = (sides & CX_TARGET) != 0;
  if (targets ? (n_lags < 1 || n_lags > CX_MAX_LAGS || !lags_host) : n_lags != 0)
    return fail(SAE_ERR_INVALID, "n_lags=%d: target masks take 1 to %d lags, a source mask alone none", n_lags, CX_MAX_LAGS);
  for (int a = 0; a < n_lags; ++a) {
    if (lags_host[a] < 0 || lags_host[a] >= CX_MAX_LAG) return fail(SAE_ERR_INVALID, "lag %d outside [0, %d)", lags_host[a], CX_MAX_LAG);
    for (int b = 0; b < a; ++b)
      if (lags_host[a] == lags_host[b]) return fail(SAE_ERR_INVALID, "lag %d is given twice", lags_host[a]);
  }
  if (misaligned(masks, 16)) return fail(SAE_ERR_INVALID, "the masks must be 16-byte aligned");
  if (int rc = file_pass_begin(kCrossPass, c, x, masks, n_files, rows_per_file, x_dtype, 0, &M)) return rc;
  if (!cross_dims_ok(c->n, M)) return fail(SAE_ERR_INVALID, "n_dict=%d > 2^21 or %lld rows > %lld", c->n, (long long)M, 65535ll * CO_BK);
  const int64_t Kp = round_up(M, CO_BK), one = cross_rows_p(c->n) * Kp;
  const int n_masks = ((sides & CX_SOURCE) ? 1 : 0) + n_lags;
  if (masks_bytes < n_masks * one)
    return fail(SAE_ERR_INVALID, "masks_bytes=%lld < %d masks of %lld bytes", (long long)masks_bytes, n_masks, (long long)one);
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;

  ev_begin(c, KID_CROSS_PACK, s);
  hipError_t memset_zt = hipSuccess;
  for (int m = 0; m < n_masks && memset_zt == hipSuccess; ++m) {
    int8_t* zt = (int8_t*)masks + m * one;
    const int lag = (sides & CX_SOURCE) ? (m == 0 ? 0 : lags_host[m - 1]) : lags_host[m];      // (the source mask: the target mask at lag 0)
    if (c->topk) {                            // the selection scattered into the zeroed mask
      memset_zt = hipMemsetAsync(zt, 0, (size_t)one, s);
      if (memset_zt == hipSuccess)
        hipLaunchKernelGGL(cross_pack_topk_kernel, dim3(grid_for(M * c->k, 4096)), dim3(256), 0, s, c->top_idx, (const unsigned short*)c->top_vals,
                           c->k, M, Trows, lengths, c->n, lag, zt, Kp);
    } else {
      hipLaunchKernelGGL(cross_pack_l1_kernel, dim3((unsigned)(Kp / 64), (unsigned)(cross_rows_p(c->n) / 64)), dim3(256), 0, s,
                         (const unsigned short*)c->c, (int64_t)c->n_p, c->n, M, Trows, lengths, lag, zt, Kp);
    }
  }
  ev_end(c, KID_CROSS_PACK, s);             // (the bracket closes whatever the memset answered)
  HIP_TRY(memset_zt);
  HIP_TRY(hipGetLastError());
  file_pass_end(kCrossPass, c);
  return SAE_OK;
}

extern "C" int sae_cross_update(const void* mask_a, int64_t n_a, const void* mask_b, int64_t n_b, int64_t rows, int32_t* counts, void* stream) {
  if (!mask_a || !mask_b || !counts) return fail(SAE_ERR_INVALID, "null argument");
  if (!cross_dims_ok(n_a, rows) || !cross_dims_ok(n_b, rows))
    return fail(SAE_ERR_INVALID, "n_a=%lld or n_b=%lld outside [1, 2^21], or rows=%lld outside [1, %lld]", (long long)n_a, (long long)n_b,
                (long long)rows, 65535ll * CO_BK);
  if (misaligned(mask_a, 16) || misaligned(mask_b, 16) || misaligned(counts, 4))
    return fail(SAE_ERR_INVALID, "the masks must be 16-byte aligned and the count table 4-byte aligned");
  const int64_t Kp = round_up(rows, CO_BK);
  // the K split of coact.h's header over the rectangle's tiles
  const int64_t ntr = cross_rows_p(n_a) / CO_BM, ntc = cross_rows_p(n_b) / CO_BM;
  const KSplit ks = coact_ksplit(ntr * ntc, Kp);
  const dim3 grid((unsigned)ntc, (unsigned)ntr, (unsigned)ks.ksplit);
  hipStream_t s = (hipStream_t)stream;
  const int8_t *za = (const int8_t*)mask_a, *zb = (const int8_t*)mask_b;
  if (ks.ksplit > 1) hipLaunchKernelGGL(label_update_kernel<true>, grid, dim3(256), 0, s, za, zb, Kp, (int)n_a + 1, (int)n_b + 1, ks.per, counts);
  else hipLaunchKernelGGL(label_update_kernel<false>, grid, dim3(256), 0, s, za, zb, Kp, (int)n_a + 1, (int)n_b + 1, ks.per, counts);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_cross_keys(const int32_t* counts, int64_t n_a, int64_t n_b, int measure, int by_b, int exclude_diagonal, int64_t row0,
                              int64_t n_rows, uint64_t* keys, void* stream) {
  if (!counts || !keys) return fail(SAE_ERR_INVALID, "null argument");
  if (n_a < 1 || n_a > CX_MAX_N || n_b < 1 || n_b > CX_MAX_N) return fail(SAE_ERR_INVALID, "n_a=%lld or n_b=%lld outside [1, 2^21]", (long long)n_a, (long long)n_b);
  if ((by_b != 0 && by_b != 1) || (exclude_diagonal != 0 && exclude_diagonal != 1))
    return fail(SAE_ERR_INVALID, "by_b=%d and exclude_diagonal=%d must each be 0 or 1", by_b, exclude_diagonal);
  const int64_t rows_all = by_b ? n_b : n_a, ncols = by_b ? n_a : n_b;
  if (n_rows < 1 || row0 < 0 || row0 + n_rows > rows_all)
    return fail(SAE_ERR_INVALID, "rows [%lld, %lld) are empty or outside [0, %lld)", (long long)row0, (long long)(row0 + n_rows), (long long)rows_all);
  if (measure != SAE_CROSS_JACCARD && measure != SAE_CROSS_COND && measure != SAE_CROSS_LIFT && measure != SAE_CROSS_COUNT)
    return fail(SAE_ERR_INVALID, "unknown measure %d", measure);
  hipLaunchKernelGGL(cross_keys_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)std::min<int64_t>(n_rows, 65535)), dim3(256), 0,
                     (hipStream_t)stream, counts, (int)n_a, (int)n_b, measure, by_b, exclude_diagonal, row0, n_rows, keys);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- activation histograms (hist.h): per latent the histogram of its value on every counted frame and of every file's maximum,
// and the frame histogram of a few chosen latents split by label
static_assert(SAE_HIST_MAX_BINS == HB_MAX_BINS && SAE_HIST_MAX_SEL == HIST_MAX_SEL, "freud_sae.h, hist_bins.h and hist.h disagree");

// the stored latent of file_pass_encode binned by hist_l1_kernel.  Chunks of whole files: the fewest files per chunk that still give
// HIST_MIN_WGS workgroups (every chunk flushes its non-empty bins with global adds, so fewer chunks are cheaper).  Columns per
// workgroup: 256 while the counters fit 48 KiB of LDS (O P <= 96), else 128.
constexpr int HIST_MIN_WGS = 1024;
static void hist_launch_l1(sae_ctx* c, int64_t n_files, int Trows, const int* lengths, HistSpec sp, int64_t* frame_hist, int64_t* file_max_hist,
                           hipStream_t s) {
  const int reg = hist_regular(sp);
  const int nt = reg <= 96 ? 256 : 128;
  const int colblocks = (c->n + nt - 1) / nt;
  const int64_t want = std::min<int64_t>(n_files, (HIST_MIN_WGS + colblocks - 1) / colblocks);
  const int fpc = (int)(n_files / want);
  const int64_t chunks = (n_files + fpc - 1) / fpc;
  hipLaunchKernelGGL(hist_l1_kernel, dim3((unsigned)colblocks, (unsigned)chunks), dim3(nt), (size_t)((reg + 1) / 2) * nt * 4, s,
                     (const unsigned short*)c->c, (int64_t)c->n_p, c->n, n_files, Trows, lengths, fpc, sp, frame_hist, file_max_hist);
}

extern "C" int sae_hist_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                              int lo_exp, int octaves, int sub_bits, int flags, int64_t* frame_hist, int64_t* file_max_hist,
                              int64_t* n_frames, const int32_t* labels, int n_slots, int n_classes, const int32_t* sel_latents, int n_sel,
                              int64_t* label_hist, int64_t* label_count, void* stream) {
  int64_t M;
  const HistSpec sp{lo_exp, octaves, sub_bits};
  if (!hist_spec_ok(sp))
    return fail(SAE_ERR_INVALID, "histogram spec lo_exp=%d octaves=%d sub_bits=%d: -126 <= lo_exp, octaves >= 1, lo_exp + octaves <= 128, "
                "sub_bits in 0..3, octaves << sub_bits <= %d", lo_exp, octaves, sub_bits, HB_MAX_REGULAR);
  if (!file_max_hist || !n_frames) return fail(SAE_ERR_INVALID, "null argument");
  if (n_sel < 0 || n_sel > SAE_HIST_MAX_SEL) return fail(SAE_ERR_INVALID, "n_sel=%d outside [0, %d]", n_sel, SAE_HIST_MAX_SEL);
  if (n_sel > 0) {
    if (!labels || !sel_latents || !label_hist || !label_count) return fail(SAE_ERR_INVALID, "n_sel=%d needs labels, sel_latents, label_hist and label_count", n_sel);
    if (n_slots < 1 || n_slots > SAE_LABEL_MAX_SLOTS) return fail(SAE_ERR_INVALID, "n_slots=%d outside [1, %d]", n_slots, SAE_LABEL_MAX_SLOTS);
    if (n_classes < 1 || n_classes > SAE_LABEL_MAX_CLASSES) return fail(SAE_ERR_INVALID, "n_classes=%d outside [1, %d]", n_classes, SAE_LABEL_MAX_CLASSES);
  }
  for (const void* p : {(const void*)frame_hist, (const void*)file_max_hist, (const void*)n_frames, (const void*)label_hist, (const void*)label_count})
    if (misaligned(p, 8)) return fail(SAE_ERR_INVALID, "the histogram arrays must be 8-byte aligned");
  if (int rc = file_pass_begin(kHistPass, c, x, frame_hist, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  // TopK scratch: the file maxima [n_files][n] of this batch (cleared below: the scatter takes maxima into it)
  char* scratch = nullptr;
  if (c->topk)
    if (int rc = pass_scratch(c, {n_files * c->n * 4}, &scratch)) return rc;
  uint32_t* fmax = (uint32_t*)scratch;
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;

  ev_begin(c, KID_HIST, s);
  hipError_t memset_fmax = hipSuccess;
  hipLaunchKernelGGL(hist_frames_kernel, dim3(1), dim3(256), 0, s, n_files, Trows, lengths, n_frames, n_sel > 0 ? label_count + n_classes : nullptr);
  if (c->topk) {
    memset_fmax = hipMemsetAsync(fmax, 0, (size_t)(n_files * c->n) * 4, s);
    if (memset_fmax == hipSuccess) {
      hipLaunchKernelGGL(hist_topk_scatter_kernel, dim3(grid_for(M * c->k, 4096)), dim3(256), 0, s, c->top_idx, (const unsigned short*)c->top_vals,
                         c->k, M, Trows, lengths, c->n, sp, frame_hist, fmax);
      hipLaunchKernelGGL(hist_topk_finish_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, fmax, n_files, c->n, sp, n_frames,
                         frame_hist, file_max_hist);
    }
  } else {
    hist_launch_l1(c, n_files, Trows, lengths, sp, frame_hist, file_max_hist, s);
  }
  if (n_sel > 0 && memset_fmax == hipSuccess) {
    const dim3 grid(grid_for(M * n_sel, 4096));
    if (c->topk)
      hipLaunchKernelGGL(hist_label_kernel<true>, grid, dim3(256), 0, s, (const unsigned short*)c->top_vals, (int64_t)0, c->top_idx, c->k, c->n, M,
                         Trows, lengths, labels, n_slots, n_classes, sel_latents, n_sel, sp, label_hist, label_count);
    else
      hipLaunchKernelGGL(hist_label_kernel<false>, grid, dim3(256), 0, s, (const unsigned short*)c->c, (int64_t)c->n_p, (const int*)nullptr, 0, c->n,
                         M, Trows, lengths, labels, n_slots, n_classes, sel_latents, n_sel, sp, label_hist, label_count);
    hipLaunchKernelGGL(hist_label_any_kernel, dim3((unsigned)n_sel), dim3(256), 0, s, frame_hist, sel_latents, c->n, n_classes, hist_nbins(sp),
                       label_hist);
  }
  ev_end(c, KID_HIST, s);                   // (the bracket closes whatever the memset answered)
  HIP_TRY(memset_fmax);
  HIP_TRY(hipGetLastError());
  file_pass_end(kHistPass, c);
  return SAE_OK;
}

// ---- feature timing (timing.h): per latent the histograms of its run durations and of the gaps between its runs, and six totals
static_assert(SAE_TIMING_ACTIVE == TB_ACTIVE && SAE_TIMING_SPAN == TB_SPAN && SAE_TIMING_RUNS == TB_RUNS && SAE_TIMING_FILES == TB_FILES &&
              SAE_TIMING_LONGEST == TB_LONGEST && SAE_TIMING_CENSORED == TB_CENSORED && SAE_TIMING_NTOTALS == TB_NTOTALS &&
              SAE_TIMING_MAX_BINS == TB_MAX_BINS && SAE_TIMING_MAX_BRIDGE == TB_MAX_BRIDGE && TM_MAX_K == SAE_COLLECT_MAX_K,
              "freud_sae.h, timing_bins.h and timing.h disagree");

// the stored latent of file_pass_encode walked by timing_l1_kernel.  Chunks of whole files as in hist_launch_l1.  Columns per
// workgroup from the LDS the spec needs: 2 ((NB + 1) / 2) dwords per column -- 256 while that fits 48 KiB (NB <= 48), else 128 (NB = 111:
// 56 KiB).  one_chunk (SAE_TIMING_ONE_CHUNK): every file of the call in one chunk -- the same arrays from another geometry.
static void timing_launch_l1(sae_ctx* c, int64_t n_files, int Trows, const int* lengths, int sub_bits, int bridge, uint32_t threshold,
                             bool one_chunk, int64_t* run_hist, int64_t* gap_hist, int64_t* totals, hipStream_t s) {
  const int nq = (timing_nbins(sub_bits, Trows) + 1) / 2;
  const int nt = nq <= 24 ? 256 : 128;
  const int colblocks = (c->n + nt - 1) / nt;
  const int64_t want = std::min<int64_t>(n_files, (HIST_MIN_WGS + colblocks - 1) / colblocks);
  const int fpc = one_chunk ? (int)n_files : (int)(n_files / want);
  const int64_t chunks = (n_files + fpc - 1) / fpc;
  hipLaunchKernelGGL(timing_l1_kernel, dim3((unsigned)colblocks, (unsigned)chunks), dim3(nt), (size_t)2 * nq * nt * 4, s,
                     (const unsigned short*)c->c, (int64_t)c->n_p, c->n, n_files, Trows, lengths, fpc, sub_bits, bridge, threshold, run_hist,
                     gap_hist, totals);
}

extern "C" int sae_timing_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                int sub_bits, int bridge, uint32_t threshold_bits, int flags, int64_t* run_hist, int64_t* gap_hist,
                                int64_t* totals, int64_t* n_frames, void* stream) {
  int64_t M;
  if (!timing_spec_ok(sub_bits, bridge, threshold_bits, rows_per_file))
    return fail(SAE_ERR_INVALID, "timing sub_bits=%d bridge=%d threshold_bits=0x%x rows_per_file=%lld: sub_bits in 0..3, bridge in 0..%d, "
                "threshold_bits <= 0x%x, 1 <= rows_per_file <= %d", sub_bits, bridge, threshold_bits, (long long)rows_per_file, TB_MAX_BRIDGE,
                TB_MAX_THRESHOLD, TB_MAX_ROWS);
  if (!gap_hist || !totals || !n_frames) return fail(SAE_ERR_INVALID, "null argument");
  for (const void* p : {(const void*)run_hist, (const void*)gap_hist, (const void*)totals, (const void*)n_frames})
    if (misaligned(p, 8)) return fail(SAE_ERR_INVALID, "the timing arrays must be 8-byte aligned");
  if (int rc = file_pass_begin(kTimingPass, c, x, run_hist, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (c->topk && (c->k < 1 || c->k > TM_MAX_K)) return fail(SAE_ERR_INVALID, "sae_timing_files: k=%d outside [1, %d]", c->k, TM_MAX_K);
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;

  ev_begin(c, KID_TIMING, s);
  hipLaunchKernelGGL(hist_frames_kernel, dim3(1), dim3(256), 0, s, n_files, Trows, lengths, n_frames, (int64_t*)nullptr);
  if (c->topk) {
    const dim3 grid((unsigned)n_files, (unsigned)((c->n + TM_SEG - 1) / TM_SEG));
    if (c->k <= 64)
      hipLaunchKernelGGL(timing_topk_kernel<true>, grid, dim3(64), 0, s, c->top_idx, (const unsigned short*)c->top_vals, c->k, Trows, lengths,
                         c->n, sub_bits, bridge, threshold_bits, run_hist, gap_hist, totals);
    else
      hipLaunchKernelGGL(timing_topk_kernel<false>, grid, dim3(64), 0, s, c->top_idx, (const unsigned short*)c->top_vals, c->k, Trows, lengths,
                         c->n, sub_bits, bridge, threshold_bits, run_hist, gap_hist, totals);
  } else {
    timing_launch_l1(c, n_files, Trows, lengths, sub_bits, bridge, threshold_bits, (flags & SAE_TIMING_ONE_CHUNK) != 0, run_hist, gap_hist,
                     totals, s);
  }
  ev_end(c, KID_TIMING, s);
  HIP_TRY(hipGetLastError());
  file_pass_end(kTimingPass, c);
  return SAE_OK;
}

// ---- dictionary comparison (dict_match.h): unit decoder directions as a K-concatenated hi / lo bf16 operand, and the cosine keys of
// a block of A's rows against all of B through the row x row tile GEMM
static_assert(SAE_DICT_MAX_D == DM_MAX_D && SAE_DICT_LEFT == DM_LEFT && SAE_DICT_RIGHT == DM_RIGHT && DM_MAX_N == FT_MAX_COLS &&
              DM_ROW_ALIGN == G2_BM && DM_ROW_ALIGN == G2_BN && DM_K_ALIGN == GEMM_BK, "freud_sae.h, dict_match.h and gemm256.h disagree");

static bool dict_dims_ok(int64_t n, int64_t d) { return n >= 1 && n <= DM_MAX_N && d >= 1 && d <= DM_MAX_D; }

extern "C" int64_t sae_dict_pack_bytes(int64_t n, int64_t d) { return dict_dims_ok(n, d) ? dm_pack_bytes(n, d) : 0; }

extern "C" int sae_dict_pack(const float* w, int64_t n, int64_t d, int64_t dir_stride, int64_t elem_stride, int side, void* packed,
                             float* norms, void* stream) {
  if (!w || !packed || !norms) return fail(SAE_ERR_INVALID, "null argument");
  if (!dict_dims_ok(n, d)) return fail(SAE_ERR_INVALID, "n=%lld outside [1, 2^24] or d=%lld outside [1, %d]", (long long)n, (long long)d, DM_MAX_D);
  if (dir_stride < 1 || elem_stride < 1) return fail(SAE_ERR_INVALID, "dir_stride=%lld, elem_stride=%lld: strides are positive element counts", (long long)dir_stride, (long long)elem_stride);
  if (side != DM_LEFT && side != DM_RIGHT) return fail(SAE_ERR_INVALID, "side=%d is neither 0 nor 1", side);
  if (misaligned(packed, 16) || misaligned(w, 4) || misaligned(norms, 4))
    return fail(SAE_ERR_INVALID, "the packed operand must be 16-byte aligned, the weights and norms 4-byte aligned");
  const int64_t rows_p = dm_rows_p(n);
  hipStream_t s = (hipStream_t)stream;
  if (elem_stride == 1)
    hipLaunchKernelGGL(dict_pack_rows_kernel, dim3((unsigned)(rows_p / 4)), dim3(256), 0, s, w, n, (int)d, dir_stride, side, (unsigned short*)packed, norms);
  else
    hipLaunchKernelGGL(dict_pack_cols_kernel, dim3((unsigned)(rows_p / 64)), dim3(256), 0, s, w, n, (int)d, dir_stride, elem_stride, side,
                       (unsigned short*)packed, norms);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_dict_sim_keys(const void* packed_a, int64_t n_a, const void* packed_b, int64_t n_b, int64_t d, int64_t row0, int64_t n_rows,
                                 int self_mode, uint64_t* keys, void* stream) {
  if (!packed_a || !packed_b || !keys) return fail(SAE_ERR_INVALID, "null argument");
  if (!dict_dims_ok(n_a, d) || !dict_dims_ok(n_b, d))
    return fail(SAE_ERR_INVALID, "n_a=%lld, n_b=%lld outside [1, 2^24] or d=%lld outside [1, %d]", (long long)n_a, (long long)n_b, (long long)d, DM_MAX_D);
  if (self_mode != 0 && self_mode != 1) return fail(SAE_ERR_INVALID, "self_mode=%d is neither 0 nor 1", self_mode);
  if (self_mode && n_a != n_b) return fail(SAE_ERR_INVALID, "self mode with n_a=%lld != n_b=%lld", (long long)n_a, (long long)n_b);
  if (n_rows < 1 || row0 < 0 || row0 + n_rows > n_a)
    return fail(SAE_ERR_INVALID, "rows [%lld, %lld) are empty or outside [0, %lld)", (long long)row0, (long long)(row0 + n_rows), (long long)n_a);
  if (misaligned(packed_a, 16) || misaligned(packed_b, 16) || misaligned(keys, 8))
    return fail(SAE_ERR_INVALID, "the packed operands must be 16-byte aligned and the keys 8-byte aligned");
  const int64_t ld = dm_ld(d);
  const int64_t row_base = row0 / DM_ROW_ALIGN * DM_ROW_ALIGN;                   // (the cover stays inside dm_rows_p(n_a))
  const int64_t nbm = (dm_rows_p(row0 + n_rows) - row_base) / DM_ROW_ALIGN, nbn = dm_rows_p(n_b) / DM_ROW_ALIGN;
  if (nbm * nbn > (1 << 30)) return fail(SAE_ERR_INVALID, "a row block of %lld x %lld tiles: split it", (long long)nbm, (long long)nbn);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  GemmArgs g{};
  g.A0 = (const bf16_t*)packed_a + row_base * ld; g.lda = ld; g.B0 = (const bf16_t*)packed_b; g.ldb = ld;
  g.nbm = (int)nbm; g.nbn = (int)nbn;                                            // (256 x 256 tiles: the kernel is launched directly)
  g.ktiles0 = g.ktiles = (int)(ld / GEMM_BK); g.splits = 1;
  EpiDictKeys e{};
  e.keys = keys; e.n_b = n_b; e.n_rows = n_rows; e.row_lo = (int)(row0 - row_base);
  e.self_base = self_mode ? row_base : -((int64_t)1 << 40);
  auto kern = gemm256_bf16_kernel<OP_ROW, OP_ROW, EpiDictKeys>;
  LDS_ATTR(kern, G2_LDS_BYTES, dev);
  hipLaunchKernelGGL(kern, dim3((unsigned)(nbm * nbn)), dim3(512), G2_LDS_BYTES, (hipStream_t)stream, g, e);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- feature manipulation (manip.h): one encode, one decode, then a rank-one term per edit and variant
static_assert(SAE_MANIP_SCALE == SM_SCALE && SAE_MANIP_SET == SM_SET && SAE_MANIP_MAX_EDITS == SM_MAX_EDITS &&
              SAE_MANIP_MAX_VARIANTS == SM_MAX_VARIANTS, "freud_sae.h and manip.h disagree");

static void manip_decode_topk(sae_ctx* c, int64_t M, float* x_hat, hipStream_t s) {
  const float* bd = c->P + 2 * c->nW + c->n_p;
  const dim3 grid((unsigned)((M + 3) / 4));
  with_np(c->d_p, [&](auto np_tag) {
    constexpr int NP = decltype(np_tag)::value;
    hipLaunchKernelGGL(manip_topk_decode_kernel<NP>, grid, dim3(256), 0, s, c->top_vals, c->top_idx, c->k, c->Wd_b, bd, x_hat, M, c->d,
                       c->d_p, c->n_p);
  });
}

extern "C" int sae_manipulate_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* latents,
                                    const int32_t* ops, int n_edits, const float* values, int n_variants, int flags, float* standard,
                                    float* manipulated, float* series, void* stream) {
  if (!latents || !ops || !values || !manipulated || !series) return fail(SAE_ERR_INVALID, "null argument");
  if (n_edits < 1 || n_edits > SAE_MANIP_MAX_EDITS) return fail(SAE_ERR_INVALID, "n_edits=%d outside [1, %d]", n_edits, SAE_MANIP_MAX_EDITS);
  if (n_variants < 1 || n_variants > SAE_MANIP_MAX_VARIANTS)
    return fail(SAE_ERR_INVALID, "n_variants=%d outside [1, %d]", n_variants, SAE_MANIP_MAX_VARIANTS);
  ManipEdits ed{};
  ed.n_edits = n_edits; ed.n_variants = n_variants;
  for (int e = 0; e < n_edits; ++e) {
    if (c && (latents[e] < 0 || latents[e] >= c->n)) return fail(SAE_ERR_INVALID, "edit %d: latent %d outside [0, %d)", e, latents[e], c->n);
    for (int f = 0; f < e; ++f)
      if (latents[f] == latents[e]) return fail(SAE_ERR_INVALID, "edits %d and %d name the same latent %d", f, e, latents[e]);
    if (ops[e] != SAE_MANIP_SCALE && ops[e] != SAE_MANIP_SET) return fail(SAE_ERR_INVALID, "edit %d: unknown op %d", e, ops[e]);
    ed.latents[e] = latents[e]; ed.ops[e] = ops[e];
    for (int v = 0; v < n_variants; ++v) {
      const float val = values[v * n_edits + e];
      if (!std::isfinite(val)) return fail(SAE_ERR_INVALID, "variant %d, edit %d: the value is not finite", v, e);
      ed.values[v][e] = val;
    }
  }
  int64_t M;
  if (int rc = file_pass_begin(kManipPass, c, x, standard, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (c->topk && c->d_p > 1536) return fail(SAE_ERR_INVALID, "sae_manipulate_files: the TopK decode serves d_model <= 1536");
  // scratch: the operand rows [SM_MAX_EDITS][d_p] (manip_rows_kernel writes every element the apply reads)
  char* scratch;
  if (int rc = pass_scratch(c, {(int64_t)SM_MAX_EDITS * c->d_p * 4}, &scratch)) return rc;
  float* wrows = (float*)scratch;
  hipStream_t s = (hipStream_t)stream;
  const int d = c->d;
  // the bf16 eval forward: encode() -- and the state sae_eval leaves (latent rows, indices, metrics)
  if (int rc = dispatch_fwd_bwd(c, x, M, x_dtype, stream, false)) return rc;

  ev_begin(c, KID_MANIP_DECODE, s);
  int rc = SAE_OK;
  if (c->topk) manip_decode_topk(c, M, standard, s);
  else rc = decode_l1_latent(c, c->c, c->last_M_p / 128, M, standard, s);    // (the forward's own padded latent: no pad_latent copy)
  ev_end(c, KID_MANIP_DECODE, s);
  if (rc) return rc;

  ev_begin(c, KID_MANIP_SERIES, s);
  if (c->topk) {
    hipLaunchKernelGGL(manip_series_topk_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, c->top_idx, c->top_vals, c->k, M, ed, series);
    hipLaunchKernelGGL(manip_rows_kernel, dim3((d + 255) / 256, n_edits), dim3(256), 0, s, c->Wd_b, (int64_t)c->d_p, (int64_t)1, d, ed,
                       wrows, c->d_p);
  } else {
    hipLaunchKernelGGL(manip_series_kernel, dim3(grid_for(M * n_edits, 4096)), dim3(256), 0, s, c->c, (int64_t)c->n_p, M, ed, series);
    hipLaunchKernelGGL(manip_rows_kernel, dim3((d + 255) / 256, n_edits), dim3(256), 0, s, c->Wb, (int64_t)1, (int64_t)c->n_p, d, ed,
                       wrows, c->d_p);
  }
  ev_end(c, KID_MANIP_SERIES, s);

  ev_begin(c, KID_MANIP_APPLY, s);
  {
    const bool vec = d % 4 == 0 && !misaligned(standard, 16) && !misaligned(manipulated, 16);
    const int vw = vec ? 4 : 1;
    const int nslab = (d + 32 * vw - 1) / (32 * vw);
    // groups of 8 half waves, a multiple of the slabs: every frame x slab once, at most ~4096 groups striding over the frames
    const int64_t per_slab = std::min<int64_t>((M + 7) / 8, std::max<int64_t>(4096 / nslab, 1));
    const dim3 grid((unsigned)(per_slab * nslab));
    if (vec) hipLaunchKernelGGL(manip_apply_kernel<4>, grid, dim3(256), 0, s, standard, series, wrows, c->d_p, M, d, nslab, ed, manipulated);
    else hipLaunchKernelGGL(manip_apply_kernel<1>, grid, dim3(256), 0, s, standard, series, wrows, c->d_p, M, d, nslab, ed, manipulated);
  }
  ev_end(c, KID_MANIP_APPLY, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- reconstruction report (recon.h): the residual of encode() -> decode() per frame, its sums per file and per model dimension,
// and per latent the attribution sums P_j = sum a_j (r . w_j), sum a_j^2 and |w_j|^2
static_assert(SAE_RECON_UNFUSED == 1, "freud_sae.h and passes.hip disagree");

struct ReconScratch {           // its scratch area carved up (floats): x_hat / r, the slabs, the row and dimension partials, TopK's p.
  float *xr, *slab_p, *slab_q, *rowpart, *dimpart, *p;      // All written with plain stores before the call reads them: nothing to clear.
};

static ReconScratch recon_scratch(const sae_ctx* c, char* base) {
  const int64_t rows = c->cfg.max_rows, nrb = c->max_rows_p / STATS_RB, nch = c->d_p / RC_CW;
  ReconScratch r;
  r.xr = (float*)base;
  r.slab_p = r.xr + round_up(rows * c->d, 4);
  r.slab_q = r.slab_p + nrb * c->n_p;
  r.rowpart = r.slab_q + nrb * c->n_p;
  r.dimpart = r.rowpart + rows * nch * 2;
  r.p = r.dimpart + nrb * 3 * c->d_p;
  return r;
}

static int64_t recon_scratch_bytes(const sae_ctx* c) {
  const ReconScratch r = recon_scratch(c, nullptr);        // (offsets from a null base: only their differences are used)
  return ((r.p - r.xr) + (c->topk ? c->cfg.max_rows * (int64_t)c->k : 0)) * 4;
}

static ReconOut recon_out(void* block, int n, int d) {
  char* b = (char*)block;
  ReconOut o;
  o.n_frames = (unsigned long long*)(b + SAE_RECON_N_FRAMES(n, d));
  o.attr = (double*)(b + SAE_RECON_ATTR_SUM(n, d));
  o.asq = (double*)(b + SAE_RECON_ACT_SQ_SUM(n, d));
  o.sx = (double*)(b + SAE_RECON_SUM_X(n, d));
  o.sxx = (double*)(b + SAE_RECON_SUM_X_SQ(n, d));
  o.srr = (double*)(b + SAE_RECON_SUM_R_SQ(n, d));
  o.wnorm = (float*)(b + SAE_RECON_DEC_NORM_SQ(n, d));
  return o;
}

template <typename T>
static void recon_launch_resid(sae_ctx* c, const T* x, const ReconScratch& sc, float* resid, bf16_t* rb, bf16_t* lat, int64_t rows_cover,
                               int64_t M, int Trows, const int* lengths, hipStream_t s) {
  const dim3 grid((unsigned)(rows_cover / STATS_RB), (unsigned)(c->d_p / RC_CW));
  hipLaunchKernelGGL(recon_resid_kernel<T>, grid, dim3(256), 0, s, x, sc.xr, resid, rb, lat, c->n_p, M, Trows, 1.0f / (float)Trows, lengths,
                     c->d, c->d_p, sc.rowpart, sc.dimpart);
}

static void recon_launch_fold(sae_ctx* c, const ReconScratch& sc, int nrb_lat, int nrb_dim, int64_t n_files, int Trows, const int* lengths,
                              const ReconOut& o, double* file_out, hipStream_t s) {
  const int nb_lat = (c->n + 255) / 256, nb_dim = (c->d + 255) / 256, nb_files = (int)((n_files + 3) / 4);
  hipLaunchKernelGGL(recon_fold_kernel, dim3((unsigned)(nb_lat + nb_dim + nb_files)), dim3(256), 0, s, sc.slab_p, sc.slab_q, nrb_lat, c->n,
                     c->n_p, sc.dimpart, nrb_dim, c->d, c->d_p, sc.rowpart, c->d_p / RC_CW, (int)n_files, Trows, lengths, o, file_out, nb_lat,
                     nb_dim);
}

// L1: the stored latent of file_pass_l1_encode; x_hat by decode_l1_latent on that latent; the residual sweep writes r_b into c->dxh
// (free in a file pass) and zeroes the latent rows that do not count;
// the attribution is the backward's dpre-shaped GEMM r_b [M_p][d_p] x Wt [n_p][d_p] with EpiAttr: in the streaming form where
// launch_gemm would take it (gemm_streams), in the tile forms elsewhere and with `unfused` (SAE_RECON_UNFUSED).
template <typename T>
static int recon_l1_impl(sae_ctx* c, const T* x, int64_t M, int64_t n_files, int Trows, const int* lengths, const ReconOut& o,
                         double* file_out, float* resid, bool unfused, const ReconScratch& sc, hipStream_t s) {
  const int n_p = c->n_p;
  int64_t Mp;
  if (int rc = file_pass_l1_encode(c, x, M, s, nullptr, &Mp)) return rc;

  ev_begin(c, KID_RECON_DECODE, s);
  int rc = decode_l1_latent(c, c->c, round_up(M, c->row_pad) / 128, M, sc.xr, s);      // (sae_decode's M_p)
  ev_end(c, KID_RECON_DECODE, s);
  if (rc) return rc;

  ev_begin(c, KID_RECON_RESID, s);
  recon_launch_resid(c, x, sc, resid, c->dxh, c->c, Mp, M, Trows, lengths, s);
  hipLaunchKernelGGL(recon_wnorm_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, c->Wb, (int64_t)1, (int64_t)n_p, c->d, c->n,
                     o.wnorm);
  ev_end(c, KID_RECON_RESID, s);

  const GemmArgs ga = enc_gemm_args(c, c->dxh, Mp);
  EpiAttr ea{};
  ea.c = c->c; ea.slab_p = sc.slab_p; ea.slab_q = sc.slab_q; ea.n_p = n_p;
  const bool no_stream_was = g_no_stream;
  if (unfused) g_no_stream = true;                 // (the tile forms for this launch only)
  const int kid = gemm_streams<OP_ROW, OP_ROW, EpiAttr>(ga) ? KID_RECON_ATTR_STREAM : KID_RECON_ATTR;
  ev_begin(c, kid, s);
  rc = launch_gemm<OP_ROW, OP_ROW>(ga, ea, s);
  g_no_stream = no_stream_was;
  if (!rc) recon_launch_fold(c, sc, (int)(Mp / STATS_RB), (int)(Mp / STATS_RB), n_files, Trows, lengths, o, file_out, s);
  ev_end(c, kid, s);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

template <typename T>
static int recon_topk_impl(sae_ctx* c, const T* x, int64_t M, int64_t n_files, int Trows, const int* lengths, const ReconOut& o,
                           double* file_out, float* resid, const ReconScratch& sc, hipStream_t s) {
  const int64_t rows_cover = round_up(M, STATS_RB);
  ev_begin(c, KID_RECON_DECODE, s);
  manip_decode_topk(c, M, sc.xr, s);
  ev_end(c, KID_RECON_DECODE, s);

  ev_begin(c, KID_RECON_RESID, s);
  recon_launch_resid(c, x, sc, resid, (bf16_t*)nullptr, (bf16_t*)nullptr, rows_cover, M, Trows, lengths, s);
  hipLaunchKernelGGL(recon_wnorm_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, c->Wd_b, (int64_t)c->d_p, (int64_t)1, c->d,
                     c->n, o.wnorm);
  ev_end(c, KID_RECON_RESID, s);

  ev_begin(c, KID_RECON_ATTR, s);
  {
    const dim3 grid((unsigned)((M + 3) / 4));
    with_np(c->d_p, [&](auto np_tag) {
      constexpr int NP = decltype(np_tag)::value;
      hipLaunchKernelGGL(recon_topk_attr_kernel<NP>, grid, dim3(256), 0, s, sc.xr, c->top_vals, c->top_idx, c->k, c->Wd_b, sc.p, M, c->d,
                         c->d_p, c->n_p);
    });
  }
  const int nrb = (int)((M + STATS_TK_RB - 1) / STATS_TK_RB);
  hipLaunchKernelGGL(recon_topk_cols_kernel, dim3((unsigned)nrb, (unsigned)((c->n + STATS_TK_SEG - 1) / STATS_TK_SEG)), dim3(64), 0, s,
                     c->top_idx, (const unsigned short*)c->top_vals, sc.p, c->k, M, Trows, lengths, c->n, c->n_p, sc.slab_p, sc.slab_q);
  recon_launch_fold(c, sc, nrb, (int)(rows_cover / STATS_RB), n_files, Trows, lengths, o, file_out, s);
  ev_end(c, KID_RECON_ATTR, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_recon_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                               int flags, void* block, double* file_out, float* resid, void* stream) {
  int64_t M;
  if (!file_out) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = file_pass_begin(kReconPass, c, x, block, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(block, 8) || misaligned(file_out, 8) || misaligned(resid, 4))
    return fail(SAE_ERR_INVALID, "the report block and file_out must be 8-byte aligned, resid 4-byte aligned");
  if (c->topk && c->d_p > 1536) return fail(SAE_ERR_INVALID, "sae_recon_files: the TopK decode serves d_model <= 1536");
  if ((c->max_rows_p / STATS_RB) * (int64_t)c->n_p >= ((int64_t)1 << 31))
    return fail(SAE_ERR_INVALID, "sae_recon_files: max_rows / 128 x n_dict = %lld slab entries >= 2^31", (long long)((c->max_rows_p / STATS_RB) * (int64_t)c->n_p));
  char* scratch;
  if (int rc = pass_scratch(c, {recon_scratch_bytes(c)}, &scratch)) return rc;
  const ReconScratch sc = recon_scratch(c, scratch);
  hipStream_t s = (hipStream_t)stream;
  const int Trows = (int)rows_per_file;
  const ReconOut o = recon_out(block, c->n, c->d);
  if (c->topk) {
    // the sparse decode and the attribution of encode()'s selection
    if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
    if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return recon_topk_impl(c, xt, M, n_files, Trows, lengths, o, file_out, resid, sc, s); }))
      return rc;
  } else {
    const bool unfused = (flags & SAE_RECON_UNFUSED) != 0;
    if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return recon_l1_impl(c, xt, M, n_files, Trows, lengths, o, file_out, resid, unfused, sc, s); }))
      return rc;
  }
  file_pass_end(kReconPass, c);
  return SAE_OK;
}

// ---- feature collection (collect.h): every row's K slots of the latent encode() returns, in the reference's indexed form
static_assert(SAE_COLLECT_IDX32 == CL_IDX32 && SAE_COLLECT_MAX_K == CL_MAX_K, "freud_sae.h and collect.h disagree");
// Grids of what is resident at once, the kernels stride over the rest of the rows: collect_l1_kernel holds 98 VGPRs (4 waves per SIMD:
// 4 workgroups of 256 threads per CU), collect_topk_kernel 32 KiB of LDS (5 per CU); 256 CUs
constexpr int COLLECT_L1_WGS = 256 * 4, COLLECT_TOPK_WGS = 256 * 5;

// row_nnz (or null): every row's number of active latents, for sae_frontier_files
template <typename IdxT>
static void collect_launch(sae_ctx* c, int64_t M, int K, float* values, IdxT* indices, int64_t* stats, hipStream_t s,
                           uint32_t* row_nnz = nullptr) {
  unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
  if (c->topk)
    hipLaunchKernelGGL(collect_topk_kernel<IdxT>, dim3(grid_for(M, COLLECT_TOPK_WGS, 4)), dim3(CL_THREADS), 0, s, c->top_idx,
                       (const unsigned short*)c->top_vals, c->k, M, K, values, indices, st, row_nnz);
  else
    hipLaunchKernelGGL(collect_l1_kernel<IdxT>, dim3(grid_for(M, COLLECT_L1_WGS, 1)), dim3(CL_THREADS), 0, s, (const unsigned short*)c->c,
                       (int64_t)c->n_p, c->n, M, K, values, indices, st, row_nnz);
}

extern "C" int sae_collect_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, int K, int flags,
                                 float* values, void* indices, int64_t* stats, void* stream) {
  int64_t M;
  if (!indices || !stats) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = file_pass_begin(kCollectPass, c, x, values, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  const bool idx32 = (flags & SAE_COLLECT_IDX32) != 0;
  if (misaligned(stats, 8) || misaligned(values, 4) || misaligned(indices, idx32 ? 4 : 8))
    return fail(SAE_ERR_INVALID, "stats must be 8-byte aligned, values 4-byte aligned, indices aligned to their type");
  const int k_max = c->topk ? c->k : std::min(c->n, (int)SAE_COLLECT_MAX_K);
  if (K < 1 || K > k_max)
    return fail(SAE_ERR_INVALID, "K=%d outside [1, %d] (%s)", K, k_max, c->topk ? "the context's k" : "min(n_dict, SAE_COLLECT_MAX_K)");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
  ev_begin(c, KID_COLLECT, s);
  if (idx32) collect_launch(c, M, K, values, (int32_t*)indices, stats, s);
  else collect_launch(c, M, K, values, (int64_t*)indices, stats, s);
  ev_end(c, KID_COLLECT, s);
  HIP_TRY(hipGetLastError());
  file_pass_end(kCollectPass, c);
  return SAE_OK;
}

// ---- the frontier family: sae_frontier_files (frontier.h), sae_pursuit_files (pursuit.h), sae_refit_files (refit.h).  Each gets the
// squared error of every counted frame at every latent budget 0 .. K its own way, leaves part / rowinfo / bud in context scratch and
// ends in the frontier's fold into the caller's block.  First what the three share on the host.
static_assert(SAE_FRONTIER_MAX_K == FR_MAX_K && SAE_FRONTIER_MAX_TAU == FR_MAX_TAU && FR_MAX_K <= CL_MAX_K && FR_UNIT % 4 == 0,
              "freud_sae.h, frontier.h and collect.h disagree");
static_assert(SAE_PURSUIT_MAX_K == PU_MAX_K && SAE_PURSUIT_MAX_TAU == PU_MAX_TAU, "freud_sae.h and pursuit.h disagree");
static_assert(SAE_REFIT_MAX_K == RF_MAX_K && SAE_REFIT_MAX_TAU == RF_MAX_TAU && SAE_REFIT_RATIO_BINS == RF_RATIO_BINS && RF_MAX_K <= FR_MAX_K &&
                  RF_MAX_K % 32 == 0,
              "freud_sae.h, refit_chol.h and frontier.h disagree");

// the caller's thresholds (a host array) as the kernels' argument
static int frontier_tau(const float* thresholds, int n_tau, int max_tau, FrTau* tau) {
  if (n_tau < 0 || n_tau > max_tau) return fail(SAE_ERR_INVALID, "n_tau=%d outside [0, %d]", n_tau, max_tau);
  if (n_tau > 0 && !thresholds) return fail(SAE_ERR_INVALID, "null argument");
  *tau = FrTau{};
  tau->n = n_tau;
  for (int t = 0; t < n_tau; ++t) {
    if (!(thresholds[t] > 0.f && thresholds[t] < 1.f)) return fail(SAE_ERR_INVALID, "threshold %d = %g is not inside (0, 1)", t, (double)thresholds[t]);
    tau->t[t] = thresholds[t];
  }
  return SAE_OK;
}

// the operand rows [n_p][d_p] and the bias: L1 -- the transposed copy of the normalised bf16 W, no bias; TopK -- W_dec and b_dec
struct FrOperand {
  const bf16_t* W;
  const float* b;
};
static FrOperand frontier_operand(const sae_ctx* c) {
  if (c->topk) return {c->Wd_b, c->P + 2 * c->nW + c->n_p};
  return {c->Wt, nullptr};
}

// The scratch areas are carved piece by piece from a running pointer (from a null base: the size alone).  Apart from cstats every
// piece is written with plain stores before it is read, so the leftovers of another pass do not matter.
static char* take(char*& p, int64_t bytes) { char* q = p; p += round_up(bytes, 16); return q; }
static int64_t frontier_units(const sae_ctx* c) { return (c->cfg.max_rows + FR_UNIT - 1) / FR_UNIT; }

struct FoldScratch {            // what the fold reads
  uint32_t* rowinfo;            // [max_rows]
  unsigned short* bud;          // [max_rows][FR_MAX_TAU]
  float *part, *dimpart;        // [units][FR_PART_LD], [128-row blocks][2][d_p]
};
static FoldScratch fold_scratch(const sae_ctx* c, char*& p) {
  const int64_t rows = c->cfg.max_rows, nrb = (rows + STATS_RB - 1) / STATS_RB;
  FoldScratch f;
  f.rowinfo = (uint32_t*)take(p, rows * 4);
  f.bud = (unsigned short*)take(p, rows * FR_MAX_TAU * 2);
  f.part = (float*)take(p, frontier_units(c) * FR_PART_LD * 4);
  f.dimpart = (float*)take(p, nrb * 2 * c->d_p * 4);
  return f;
}

struct SlotScratch {            // the slots of the collect kernels
  float* vals;                  // [max_rows][kcap], kcap = min(the pass's MAX_K, k or n)
  int* idx;
  int64_t* cstats;              // [8] the collect kernels' totals (not reported)
  uint32_t* row_nnz;            // [max_rows]
};
static SlotScratch slot_scratch(const sae_ctx* c, int64_t max_k, char*& p) {
  const int64_t rows = c->cfg.max_rows, kcap = std::min<int64_t>(max_k, c->topk ? c->k : c->n);
  SlotScratch sl;
  sl.vals = (float*)take(p, rows * kcap * 4);
  sl.idx = (int*)take(p, rows * kcap * 4);
  sl.cstats = (int64_t*)take(p, 64);
  sl.row_nnz = (uint32_t*)take(p, rows * 4);
  return sl;
}

// every row's K slots and its number of active latents into sl, inside the bracket kid
static int collect_slots(sae_ctx* c, int64_t M, int K, const SlotScratch& sl, int kid, hipStream_t s) {
  // the collect kernels ADD their totals to cstats (never reported): cleared, since the area holds another pass's leftovers
  HIP_TRY(hipMemsetAsync(sl.cstats, 0, 64, s));
  ev_begin(c, kid, s);
  collect_launch(c, M, K, sl.vals, sl.idx, sl.cstats, s, sl.row_nnz);
  ev_end(c, kid, s);
  return SAE_OK;
}

// the fields every block of the family has, at their offsets in block; rows_cut / active_cut stay null (the fold skips them)
static FrOut fold_out(void* block, int64_t n_frames, int64_t sse, int64_t sum_x, int64_t sum_x_sq, int64_t budget) {
  char* b = (char*)block;
  FrOut o{};
  o.n_frames = (unsigned long long*)(b + n_frames);
  o.sse = (double*)(b + sse);
  o.sx = (double*)(b + sum_x);
  o.sxx = (double*)(b + sum_x_sq);
  o.budget = (unsigned long long*)(b + budget);
  return o;
}

// the dimension sums of the batch, then the fold of part / rowinfo / bud / dimpart into the block (the caller's KID_*_FOLD bracket)
template <typename T>
static void frontier_fold_launch(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, int K, int n_tau, const FoldScratch& f,
                                 const FrOut& o, hipStream_t s) {
  const int n_units = (int)((M + FR_UNIT - 1) / FR_UNIT), nrb = (int)((M + STATS_RB - 1) / STATS_RB);
  hipLaunchKernelGGL(frontier_dim_kernel<T>, dim3((unsigned)nrb, (unsigned)(c->d_p / 64)), dim3(256), 0, s, x, M, Trows, 1.0f / (float)Trows,
                     lengths, c->d, c->d_p, f.dimpart);
  const int nb_s = (K + 1 + 255) / 256, nb_dim = (c->d + 255) / 256;
  const int n_chunks = (int)((M + FR_FOLD_ROWS - 1) / FR_FOLD_ROWS);
  hipLaunchKernelGGL(frontier_fold_kernel, dim3((unsigned)(nb_s + nb_dim + (n_tau + 1) * n_chunks)), dim3(256), 0, s, f.part, n_units, K,
                     f.dimpart, nrb, c->d, c->d_p, f.rowinfo, f.bud, M, n_tau, o, nb_s, nb_dim, n_chunks);
}

// ---- sparsity frontier (frontier.h): the slots of sae_collect_files into context scratch, one walk of them per row, the fold
struct FrontierScratch {
  SlotScratch slots;
  FoldScratch fold;
  int64_t bytes;
};

static FrontierScratch frontier_scratch(const sae_ctx* c, char* base) {
  char* p = base;
  FrontierScratch f;
  f.slots = slot_scratch(c, FR_MAX_K, p);
  f.fold = fold_scratch(c, p);
  f.bytes = p - base;
  return f;
}

template <typename T>
static int frontier_impl(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, int K, const FrTau& tau, const FrOut& o,
                         const FrontierScratch& f, hipStream_t s) {
  if (int rc = collect_slots(c, M, K, f.slots, KID_FRONTIER_SORT, s)) return rc;
  const FrOperand op = frontier_operand(c);
  ev_begin(c, KID_FRONTIER_WALK, s);
  with_np(c->d_p, [&](auto np_tag) {
    constexpr int NP = decltype(np_tag)::value;
    hipLaunchKernelGGL((frontier_walk_kernel<T, NP>), dim3((unsigned)((M + FR_UNIT - 1) / FR_UNIT)), dim3(256), 0, s, x, op.b, f.slots.vals,
                       f.slots.idx, f.slots.row_nnz, K, op.W, M, Trows, 1.0f / (float)Trows, lengths, c->d, c->d_p, c->n_p, tau, f.fold.part,
                       f.fold.rowinfo, f.fold.bud);
  });
  ev_end(c, KID_FRONTIER_WALK, s);

  ev_begin(c, KID_FRONTIER_FOLD, s);
  frontier_fold_launch(c, x, M, Trows, lengths, K, tau.n, f.fold, o, s);
  ev_end(c, KID_FRONTIER_FOLD, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_frontier_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                  int K, const float* thresholds, int n_tau, int flags, void* block, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kFrontierPass, c, x, block, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(block, 8)) return fail(SAE_ERR_INVALID, "the frontier block must be 8-byte aligned");
  const int k_max = std::min(c->topk ? c->k : c->n, (int)SAE_FRONTIER_MAX_K);
  if (K < 1 || K > k_max)
    return fail(SAE_ERR_INVALID, "K=%d outside [1, %d] (%s)", K, k_max, c->topk ? "min(the context's k, SAE_FRONTIER_MAX_K)" : "min(n_dict, SAE_FRONTIER_MAX_K)");
  FrTau tau;
  if (int rc = frontier_tau(thresholds, n_tau, SAE_FRONTIER_MAX_TAU, &tau)) return rc;
  if (c->d_p > FR_MAX_D) return fail(SAE_ERR_INVALID, "sae_frontier_files: the walk serves d_model <= %d", FR_MAX_D);
  if (c->topk && c->k > CL_MAX_K) return fail(SAE_ERR_INVALID, "sae_frontier_files: k=%d > %d", c->k, CL_MAX_K);
  char* scratch;
  if (int rc = pass_scratch(c, {frontier_scratch(c, nullptr).bytes}, &scratch)) return rc;        // (from a null base: the size alone)
  const FrontierScratch f = frontier_scratch(c, scratch);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
  const int d = c->d;
  FrOut o = fold_out(block, SAE_FRONTIER_N_FRAMES(n_tau, K, d), SAE_FRONTIER_SSE(n_tau, K, d), SAE_FRONTIER_SUM_X(n_tau, K, d),
                     SAE_FRONTIER_SUM_X_SQ(n_tau, K, d), SAE_FRONTIER_BUDGET(n_tau, K, d));
  o.rows_cut = (unsigned long long*)((char*)block + SAE_FRONTIER_ROWS_CUT(n_tau, K, d));
  o.active_cut = (unsigned long long*)((char*)block + SAE_FRONTIER_ACTIVE_CUT(n_tau, K, d));
  if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return frontier_impl(c, xt, M, (int)rows_per_file, lengths, K, tau, o, f, s); })) return rc;
  file_pass_end(kFrontierPass, c);
  return SAE_OK;
}

// ---- pursuit frontier (pursuit.h): every counted frame coded greedily against the decoder directions -- K (selection GEMM, step)
// launch pairs on the caller's stream, then the frontier's own fold
struct PursuitScratch {
  float* r32;                   // [max_rows_p][d_p] the fp32 residual
  unsigned short* rho;          // [max_rows_p][d_p] its bf16 image: the A operand of the selection GEMM
  unsigned long long* rowkey;   // [max_rows_p] the row's best key of the current step
  float *q, *z;                 // [n_p] the per-direction constants
  uint32_t* rowstate;           // [max_rows]
  float* err;                   // [max_rows][K + 1] the rows' e_s (the caller's trace_err instead when a trace is asked for)
  FoldScratch fold;
  int64_t bytes;
};

static PursuitScratch pursuit_scratch(const sae_ctx* c, int K, char* base) {
  const int64_t rows = c->cfg.max_rows, rows_p = c->max_rows_p;
  char* p = base;
  PursuitScratch f;
  f.r32 = (float*)take(p, rows_p * c->d_p * 4);
  f.rho = (unsigned short*)take(p, rows_p * c->d_p * 2);
  f.rowkey = (unsigned long long*)take(p, rows_p * 8);
  f.q = (float*)take(p, (int64_t)c->n_p * 4);
  f.z = (float*)take(p, (int64_t)c->n_p * 4);
  f.rowstate = (uint32_t*)take(p, rows * 4);
  f.err = (float*)take(p, rows * (K + 1) * 4);
  f.fold = fold_scratch(c, p);
  f.bytes = p - base;
  return f;
}

struct PursuitOut {             // the caller's block (include/freud_sae.h, SAE_PURSUIT_*)
  FrOut fold;                   // what the frontier's fold adds: n_frames, sse, sum_x, sum_x_sq, budget
  unsigned long long *steps, *picks, *in_support;
};

static PursuitOut pursuit_out(void* block, int n_tau, int K, int d, int n) {
  char* b = (char*)block;
  PursuitOut o;
  o.fold = fold_out(block, SAE_PURSUIT_N_FRAMES(n_tau, K, d, n), SAE_PURSUIT_SSE(n_tau, K, d, n), SAE_PURSUIT_SUM_X(n_tau, K, d, n),
                    SAE_PURSUIT_SUM_X_SQ(n_tau, K, d, n), SAE_PURSUIT_BUDGET(n_tau, K, d, n));
  o.steps = (unsigned long long*)(b + SAE_PURSUIT_STEPS(n_tau, K, d, n));
  o.picks = (unsigned long long*)(b + SAE_PURSUIT_PICKS(n_tau, K, d, n));
  o.in_support = (unsigned long long*)(b + SAE_PURSUIT_IN_SUPPORT(n_tau, K, d, n));
  return o;
}

template <typename T>
static int pursuit_impl(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, int K, const FrTau& tau, const PursuitOut& o,
                        const PursuitScratch& f, float* err, const PuTrace& tr, hipStream_t s) {
  const FrOperand op = frontier_operand(c);
  const bf16_t* W = op.W;
  const float inv_T = 1.0f / (float)Trows;
  int64_t Mp = round_up(M, 128);
  if (round_up(M, 256) <= c->max_rows_p) Mp = round_up(M, 256);        // (an even number of row blocks: the 256-edge tile grid)
  PuSupport sup{};
  if (c->topk) { sup.top_idx = c->top_idx; sup.top_vals = (const unsigned short*)c->top_vals; sup.k_sel = c->k; }
  else { sup.lat = (const unsigned short*)c->c; sup.lat_ld = c->n_p; }

  // (the constants and the initialiser run once per call: outside the per-step brackets, which then hold K records each)
  hipLaunchKernelGGL(pursuit_const_kernel, dim3((unsigned)((c->n_p + 3) / 4)), dim3(256), 0, s, W, c->n, c->n_p, c->d_p, f.q, f.z);
  hipLaunchKernelGGL(pursuit_init_kernel<T>, dim3((unsigned)((Mp + 3) / 4)), dim3(256), 0, s, x, op.b, M, Mp, Trows, inv_T, lengths, c->d, c->d_p, K,
                     f.r32, f.rho, err, f.rowstate, f.rowkey, tr);
  HIP_TRY(hipGetLastError());

  GemmArgs g{};
  g.A0 = (const bf16_t*)f.rho; g.B0 = W; g.lda = c->d_p; g.ldb = c->d_p;
  g.nbm = (int)(Mp / 128); g.nbn = c->n_p / 128; g.ktiles0 = g.ktiles = c->d_p / 64; g.splits = 1;
  EpiPursuit e{};
  e.z = f.z; e.rowkey = f.rowkey; e.M = M; e.n = c->n;
  for (int step = 0; step < K; ++step) {
    ev_begin(c, KID_PURSUIT_GEMM, s);
    const int rc = launch_gemm<OP_ROW, OP_ROW>(g, e, s);
    ev_end(c, KID_PURSUIT_GEMM, s);
    if (rc) return rc;
    ev_begin(c, KID_PURSUIT_STEP, s);
    with_np(c->d_p, [&](auto np_tag) {
      constexpr int NP = decltype(np_tag)::value;
      hipLaunchKernelGGL(pursuit_step_kernel<NP>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, step, K, M, c->n, c->d_p, W, f.q, f.r32, f.rho, err,
                         f.rowstate, f.rowkey, tr, sup, o.picks, o.in_support);
    });
    ev_end(c, KID_PURSUIT_STEP, s);
  }

  ev_begin(c, KID_PURSUIT_FOLD, s);
  hipLaunchKernelGGL(pursuit_finish_kernel, dim3((unsigned)((M + FR_UNIT - 1) / FR_UNIT)), dim3(256), 0, s, err, f.rowstate, M, K, tau, f.fold.part,
                     f.fold.rowinfo, f.fold.bud, o.steps);
  frontier_fold_launch(c, x, M, Trows, lengths, K, tau.n, f.fold, o.fold, s);
  ev_end(c, KID_PURSUIT_FOLD, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_pursuit_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                 int K, const float* thresholds, int n_tau, int flags, void* block, int32_t* trace_idx, float* trace_val,
                                 float* trace_err, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kPursuitPass, c, x, block, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(block, 8)) return fail(SAE_ERR_INVALID, "the pursuit block must be 8-byte aligned");
  if (K < 1 || K > SAE_PURSUIT_MAX_K) return fail(SAE_ERR_INVALID, "K=%d outside [1, %d] (SAE_PURSUIT_MAX_K)", K, SAE_PURSUIT_MAX_K);
  FrTau tau;
  if (int rc = frontier_tau(thresholds, n_tau, SAE_PURSUIT_MAX_TAU, &tau)) return rc;
  const int n_trace = (trace_idx != nullptr) + (trace_val != nullptr) + (trace_err != nullptr);
  if (n_trace != 0 && n_trace != 3) return fail(SAE_ERR_INVALID, "the trace is three pointers, all or none");
  if (misaligned(trace_idx, 4) || misaligned(trace_val, 4) || misaligned(trace_err, 4)) return fail(SAE_ERR_INVALID, "the trace arrays must be 4-byte aligned");
  if (c->d_p > FR_MAX_D) return fail(SAE_ERR_INVALID, "sae_pursuit_files: the step serves d_model <= %d", FR_MAX_D);
  char* scratch;
  if (int rc = pass_scratch(c, {pursuit_scratch(c, K, nullptr).bytes}, &scratch)) return rc;      // (from a null base: the size alone)
  const PursuitScratch f = pursuit_scratch(c, K, scratch);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;          // (the encoder's own active set, for IN_SUPPORT)
  const PursuitOut o = pursuit_out(block, n_tau, K, c->d, c->n);
  PuTrace tr{trace_idx, trace_val};
  float* err = n_trace ? trace_err : f.err;
  if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return pursuit_impl(c, xt, M, (int)rows_per_file, lengths, K, tau, o, f, err, tr, s); })) return rc;
  file_pass_end(kPursuitPass, c);
  return SAE_OK;
}

// ---- refit frontier (refit.h): the least-squares code of every counted frame on its encoder's support (the slots of the collect
// kernels, in context scratch) or on a support the caller gives, one wave per frame, then the frontier's own fold
struct RefitScratch {
  SlotScratch slots;
  FoldScratch fold;
  float* err;                   // [max_rows][K + 1] the rows' e_s (the caller's trace_err instead when it is given)
  float* efin;                  // [max_rows]
  int* keptn;                   // [max_rows] the row's kept slots, -1 on a row that does not count
  float* finpart;               // [units] sums of e_final
  int64_t bytes;
};

static RefitScratch refit_scratch(const sae_ctx* c, int K, char* base) {
  const int64_t rows = c->cfg.max_rows;
  char* p = base;
  RefitScratch f;
  f.slots = slot_scratch(c, RF_MAX_K, p);
  f.fold = fold_scratch(c, p);
  f.err = (float*)take(p, rows * (K + 1) * 4);
  f.efin = (float*)take(p, rows * 4);
  f.keptn = (int*)take(p, rows * 4);
  f.finpart = (float*)take(p, frontier_units(c) * 4);
  f.bytes = p - base;
  return f;
}

struct RefitOut {               // the caller's block (include/freud_sae.h, SAE_REFIT_*)
  FrOut fold;                   // what the frontier's fold adds: n_frames, sse, sum_x, sum_x_sq, budget
  double* sse_final;
  unsigned long long* kept;
  RfCount cnt;
};

static RefitOut refit_out(void* block, int n_tau, int K, int d, int n) {
  char* b = (char*)block;
  RefitOut o;
  o.fold = fold_out(block, SAE_REFIT_N_FRAMES(n_tau, K, d, n), SAE_REFIT_SSE(n_tau, K, d, n), SAE_REFIT_SUM_X(n_tau, K, d, n),
                    SAE_REFIT_SUM_X_SQ(n_tau, K, d, n), SAE_REFIT_BUDGET(n_tau, K, d, n));
  o.sse_final = (double*)(b + SAE_REFIT_SSE_FINAL(n_tau, K, d, n));
  o.kept = (unsigned long long*)(b + SAE_REFIT_KEPT(n_tau, K, d, n));
  o.cnt.slots = (unsigned long long*)(b + SAE_REFIT_SLOTS(n_tau, K, d, n));
  o.cnt.neg = (unsigned long long*)(b + SAE_REFIT_NEG(n_tau, K, d, n));
  o.cnt.dep = (unsigned long long*)(b + SAE_REFIT_DEP(n_tau, K, d, n));
  o.cnt.ratio = (unsigned long long*)(b + SAE_REFIT_RATIO(n_tau, K, d, n));
  o.cnt.bad_index = (unsigned long long*)(b + SAE_REFIT_BAD_INDEX(n_tau, K, d, n));
  return o;
}

template <typename T, int NT>
static int refit_launch(sae_ctx* c, const T* x, const float* b, const RfSupport& sup, int K, const bf16_t* W, int64_t M, int Trows,
                        const int* lengths, float* err, const RefitScratch& f, const RfTrace& tr, const RfCount& cnt, hipStream_t s) {
  constexpr int Kp = 32 * NT, NW = rf_waves(Kp), lds = NW * rf_region_floats(Kp) * 4;
  auto kern = refit_kernel<T, NT>;
  LDS_ATTR(kern, lds, g_device);
  hipLaunchKernelGGL(kern, dim3((unsigned)((M + NW - 1) / NW)), dim3(64 * NW), lds, s, x, b, sup, K, W, M, Trows, 1.0f / (float)Trows, lengths,
                     c->d, c->d_p, c->n, err, f.efin, f.keptn, tr, cnt);
  return SAE_OK;
}

template <typename T>
static int refit_impl(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, int K, const FrTau& tau, const int* given,
                      const RefitOut& o, const RefitScratch& f, float* err, const RfTrace& tr, hipStream_t s) {
  RfSupport sup{f.slots.vals, f.slots.idx, given};
  if (!given)
    if (int rc = collect_slots(c, M, K, f.slots, KID_REFIT_SORT, s)) return rc;
  const FrOperand op = frontier_operand(c);
  ev_begin(c, KID_REFIT_CHOL, s);
  int rc;
  switch ((K + 31) / 32) {
    case 1: rc = refit_launch<T, 1>(c, x, op.b, sup, K, op.W, M, Trows, lengths, err, f, tr, o.cnt, s); break;
    case 2: rc = refit_launch<T, 2>(c, x, op.b, sup, K, op.W, M, Trows, lengths, err, f, tr, o.cnt, s); break;
    case 3: rc = refit_launch<T, 3>(c, x, op.b, sup, K, op.W, M, Trows, lengths, err, f, tr, o.cnt, s); break;
    default: rc = refit_launch<T, 4>(c, x, op.b, sup, K, op.W, M, Trows, lengths, err, f, tr, o.cnt, s); break;
  }
  ev_end(c, KID_REFIT_CHOL, s);
  if (rc) return rc;

  ev_begin(c, KID_REFIT_FOLD, s);
  const int n_units = (int)((M + FR_UNIT - 1) / FR_UNIT);
  hipLaunchKernelGGL(refit_finish_kernel, dim3((unsigned)n_units), dim3(256), 0, s, err, f.efin, f.keptn, M, K, tau, f.fold.part, f.fold.rowinfo,
                     f.fold.bud, f.finpart, o.kept);
  hipLaunchKernelGGL(refit_final_kernel, dim3(1), dim3(64), 0, s, f.finpart, n_units, o.sse_final);
  frontier_fold_launch(c, x, M, Trows, lengths, K, tau.n, f.fold, o.fold, s);
  ev_end(c, KID_REFIT_FOLD, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_refit_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                               int K, const float* thresholds, int n_tau, int flags, const int32_t* support_idx, void* block,
                               float* trace_coef, float* trace_err, unsigned char* trace_dep, float* trace_gram, void* stream) {
  int64_t M;
  if (int rc = file_pass_begin(kRefitPass, c, x, block, n_files, rows_per_file, x_dtype, flags, &M)) return rc;
  if (misaligned(block, 8)) return fail(SAE_ERR_INVALID, "the refit block must be 8-byte aligned");
  const int k_max = support_idx ? (int)SAE_REFIT_MAX_K : std::min(c->topk ? c->k : c->n, (int)SAE_REFIT_MAX_K);
  if (K < 1 || K > k_max)
    return fail(SAE_ERR_INVALID, "K=%d outside [1, %d] (%s)", K, k_max,
                support_idx ? "SAE_REFIT_MAX_K" : c->topk ? "min(the context's k, SAE_REFIT_MAX_K)" : "min(n_dict, SAE_REFIT_MAX_K)");
  FrTau tau;
  if (int rc = frontier_tau(thresholds, n_tau, SAE_REFIT_MAX_TAU, &tau)) return rc;
  if (misaligned(support_idx, 4) || misaligned(trace_coef, 4) || misaligned(trace_err, 4) || misaligned(trace_gram, 4))
    return fail(SAE_ERR_INVALID, "the support and the trace arrays must be 4-byte aligned");
  if (c->d_p > FR_MAX_D) return fail(SAE_ERR_INVALID, "sae_refit_files: the refit serves d_model <= %d", FR_MAX_D);
  if (!support_idx && c->topk && c->k > CL_MAX_K) return fail(SAE_ERR_INVALID, "sae_refit_files: k=%d > %d", c->k, CL_MAX_K);
  char* scratch;
  if (int rc = pass_scratch(c, {refit_scratch(c, K, nullptr).bytes}, &scratch)) return rc;        // (from a null base: the size alone)
  const RefitScratch f = refit_scratch(c, K, scratch);
  hipStream_t s = (hipStream_t)stream;
  if (support_idx) refresh_decoder_operand(c, s);       // (no encoder runs: the operand rows of the current weights all the same)
  else if (int rc = file_pass_encode(c, x, M, x_dtype, s)) return rc;
  const RefitOut o = refit_out(block, n_tau, K, c->d, c->n);
  const RfTrace tr{trace_coef, trace_dep, trace_gram};
  float* err = trace_err ? trace_err : f.err;
  if (int rc = with_x_type(x_dtype, x, [&](auto* xt) { return refit_impl(c, xt, M, (int)rows_per_file, lengths, K, tau, support_idx, o, f, err, tr, s); }))
    return rc;
  file_pass_end(kRefitPass, c);
  return SAE_OK;
}

// ---- feature index (findex.h): the latent-major postings of an indexed store; context-free, like sae_search_merge
static_assert(SAE_FINDEX_IDX32 == FI_IDX32 && SAE_FINDEX_NSTATS == FI_NSTATS && SAE_COLLECT_MAX_K == FI_MAX_K, "freud_sae.h and findex.h disagree");

static int64_t findex_blocks(int64_t rows) { return (rows + FI_ROWS - 1) / FI_ROWS; }

static int findex_batch_check(const void* values, const void* indices, int64_t rows, int K, int flags, int64_t n_dict) {
  if (!values || !indices) return fail(SAE_ERR_INVALID, "null argument");
  if (flags & ~SAE_FINDEX_IDX32) return fail(SAE_ERR_INVALID, "unknown feature-index flags 0x%x", flags);
  if (rows < 1 || findex_blocks(rows) > 0x7FFFFFFFll) return fail(SAE_ERR_INVALID, "rows=%lld outside [1, 2^31 * %d)", (long long)rows, FI_ROWS);
  if (K < 1 || K > FI_MAX_K) return fail(SAE_ERR_INVALID, "K=%d outside [1, %d]", K, FI_MAX_K);
  if (n_dict < 1 || n_dict > FI_MAX_N) return fail(SAE_ERR_INVALID, "n_dict=%lld outside [1, 2^30]", (long long)n_dict);
  if (misaligned(values, 4) || misaligned(indices, (flags & SAE_FINDEX_IDX32) ? 4 : 8))
    return fail(SAE_ERR_INVALID, "values must be 4-byte aligned, indices aligned to their type");
  return SAE_OK;
}

extern "C" int64_t sae_findex_workspace_bytes(int64_t max_rows, int64_t n_range) {
  if (max_rows < 1 || n_range < 1 || n_range > FI_MAX_N) return -1;
  return findex_blocks(max_rows) * n_range * 4;
}

template <typename IdxT>
static void findex_count_launch(const uint32_t* vb, const IdxT* idx, int64_t rows, int K, int64_t n_dict, int j0, int j1,
                                unsigned long long* totals, unsigned int* counts, unsigned long long* stats, hipStream_t s) {
  const dim3 grid((unsigned)findex_blocks(rows), (unsigned)((j1 - j0 + FI_SEG - 1) / FI_SEG));
  const size_t lds = (size_t)std::min(j1 - j0, FI_SEG) * 4;
  if (K <= 64) hipLaunchKernelGGL((fi_count_kernel<IdxT, true>), grid, dim3(64), lds, s, vb, idx, rows, K, n_dict, j0, j1, totals, counts, stats);
  else hipLaunchKernelGGL((fi_count_kernel<IdxT, false>), grid, dim3(64), lds, s, vb, idx, rows, K, n_dict, j0, j1, totals, counts, stats);
}

template <typename IdxT>
static void findex_fill_launch(const uint32_t* vb, const IdxT* idx, int64_t rows, int K, int64_t n_dict, int j0, int j1, uint64_t pos0,
                               const unsigned int* block_off, uint32_t* positions, uint32_t* values, uint64_t capacity,
                               unsigned long long* err, hipStream_t s) {
  const dim3 grid((unsigned)findex_blocks(rows), (unsigned)((j1 - j0 + FI_SEG - 1) / FI_SEG));
  const size_t lds = (size_t)std::min(j1 - j0, FI_SEG) * 4;
  if (K <= 64)
    hipLaunchKernelGGL((fi_fill_kernel<IdxT, true>), grid, dim3(64), lds, s, vb, idx, rows, K, n_dict, j0, j1, (unsigned long long)pos0, block_off,
                       positions, values, (unsigned long long)capacity, err);
  else
    hipLaunchKernelGGL((fi_fill_kernel<IdxT, false>), grid, dim3(64), lds, s, vb, idx, rows, K, n_dict, j0, j1, (unsigned long long)pos0, block_off,
                       positions, values, (unsigned long long)capacity, err);
}

extern "C" int sae_findex_count(const float* values, const void* indices, int64_t rows, int K, int flags, int64_t n_dict, int64_t* totals,
                                int64_t* stats, void* stream) {
  if (!totals || !stats) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = findex_batch_check(values, indices, rows, K, flags, n_dict)) return rc;
  if (misaligned(totals, 8) || misaligned(stats, 8)) return fail(SAE_ERR_INVALID, "totals and stats must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* vb = reinterpret_cast<const uint32_t*>(values);
  unsigned long long *tt = reinterpret_cast<unsigned long long*>(totals), *st = reinterpret_cast<unsigned long long*>(stats);
  if (flags & SAE_FINDEX_IDX32) findex_count_launch(vb, (const int32_t*)indices, rows, K, n_dict, 0, (int)n_dict, tt, nullptr, st, s);
  else findex_count_launch(vb, (const int64_t*)indices, rows, K, n_dict, 0, (int)n_dict, tt, nullptr, st, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_findex_fill(const float* values, const void* indices, int64_t rows, int K, int flags, int64_t n_dict, int64_t j0, int64_t j1,
                               int64_t pos0, int64_t* cursor, int64_t out_base, uint32_t* positions_out, float* values_out,
                               int64_t capacity, void* workspace, int64_t workspace_bytes, int64_t* err, void* stream) {
  if (!cursor || !positions_out || !values_out || !workspace || !err) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = findex_batch_check(values, indices, rows, K, flags, n_dict)) return rc;
  if (j0 < 0 || j1 <= j0 || j1 > n_dict) return fail(SAE_ERR_INVALID, "latent range [%lld, %lld) outside [0, %lld)", (long long)j0, (long long)j1, (long long)n_dict);
  if (pos0 < 0 || pos0 + rows > 0x100000000ll) return fail(SAE_ERR_INVALID, "positions [%lld, %lld) do not fit 32 bits", (long long)pos0, (long long)(pos0 + rows));
  if (out_base < 0 || capacity < 0 || capacity >= 0xFFFFFFFFll)
    return fail(SAE_ERR_INVALID, "out_base=%lld, capacity=%lld: a range holds fewer than 2^32 - 1 slots", (long long)out_base, (long long)capacity);
  if (workspace_bytes < sae_findex_workspace_bytes(rows, j1 - j0))
    return fail(SAE_ERR_INVALID, "workspace of %lld bytes < sae_findex_workspace_bytes(%lld, %lld)", (long long)workspace_bytes, (long long)rows, (long long)(j1 - j0));
  if (misaligned(cursor, 8) || misaligned(err, 8) || misaligned(workspace, 4) || misaligned(positions_out, 4) || misaligned(values_out, 4))
    return fail(SAE_ERR_INVALID, "cursor and err must be 8-byte aligned, workspace and the outputs 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* vb = reinterpret_cast<const uint32_t*>(values);
  unsigned int* counts = reinterpret_cast<unsigned int*>(workspace);
  unsigned long long* er = reinterpret_cast<unsigned long long*>(err);
  uint32_t* vout = reinterpret_cast<uint32_t*>(values_out);
  const bool i32 = (flags & SAE_FINDEX_IDX32) != 0;
  if (i32) findex_count_launch(vb, (const int32_t*)indices, rows, K, n_dict, (int)j0, (int)j1, nullptr, counts, nullptr, s);
  else findex_count_launch(vb, (const int64_t*)indices, rows, K, n_dict, (int)j0, (int)j1, nullptr, counts, nullptr, s);
  hipLaunchKernelGGL(fi_scan_kernel, dim3((unsigned)((j1 - j0 + 63) / 64)), dim3(1024), 0, s, counts, (int)findex_blocks(rows), (int)j0, (int)j1,
                     reinterpret_cast<long long*>(cursor), (long long)out_base);
  if (i32) findex_fill_launch(vb, (const int32_t*)indices, rows, K, n_dict, (int)j0, (int)j1, (uint64_t)pos0, counts, positions_out, vout, (uint64_t)capacity, er, s);
  else findex_fill_launch(vb, (const int64_t*)indices, rows, K, n_dict, (int)j0, (int)j1, (uint64_t)pos0, counts, positions_out, vout, (uint64_t)capacity, er, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_findex_verify(const int64_t* starts, int64_t n_dict, int64_t j0, int64_t j1, int64_t out_base, const uint32_t* positions,
                                 int64_t capacity, int64_t limit, int64_t* err, void* stream) {
  if (!starts || !positions || !err) return fail(SAE_ERR_INVALID, "null argument");
  if (n_dict < 1 || n_dict > FI_MAX_N || j0 < 0 || j1 <= j0 || j1 > n_dict)
    return fail(SAE_ERR_INVALID, "latent range [%lld, %lld) outside [0, n_dict=%lld)", (long long)j0, (long long)j1, (long long)n_dict);
  if (limit < 1 || limit > 0x100000000ll || out_base < 0 || capacity < 0) return fail(SAE_ERR_INVALID, "limit=%lld outside [1, 2^32], or out_base or capacity < 0", (long long)limit);
  if (misaligned(starts, 8) || misaligned(err, 8) || misaligned(positions, 4)) return fail(SAE_ERR_INVALID, "starts and err must be 8-byte aligned");
  hipLaunchKernelGGL(fi_verify_kernel, dim3((unsigned)((j1 - j0 + FI_VERIFY_WAVES - 1) / FI_VERIFY_WAVES)), dim3(64 * FI_VERIFY_WAVES), 0,
                     (hipStream_t)stream, reinterpret_cast<const long long*>(starts), (int)j0, (int)j1, (long long)out_base, positions,
                     (long long)capacity, (unsigned long long)limit, reinterpret_cast<unsigned long long*>(err));
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- dead-latent resampling (resample.h, resample_draw.h): the row losses and firing counts of one batch of files, the selection of
// (dead latent, high-loss row) pairs, and the rewrite of the chosen columns inside the engine
static int resample_refuse(const sae_ctx* c, const char* fn) {
  if (c->topk) return fail(SAE_ERR_INVALID, "%s: resampling serves L1 contexts; a TopK dictionary revives its dead latents with AuxK (auxk_alpha)", fn);
  if (c->fp8) return fail(SAE_ERR_INVALID, "%s: fp8 contexts are not supported (resample in a bf16 context)", fn);
  return SAE_OK;
}

template <typename T>
static int resample_l1_impl(sae_ctx* c, const T* x, int64_t M, int Trows, const int* lengths, float* row_loss, unsigned long long* fire,
                            const StatsSlab& sl, const ReconScratch& sc, hipStream_t s) {
  if (int rc = file_pass_l1_encode(c, x, M, s)) return rc;
  // the firing counts of the stored latent: the unfused statistics path's column reduction, folded for the counts alone
  const int nrb = (int)((M + STATS_RB - 1) / STATS_RB);
  hipLaunchKernelGGL(stats_colreduce_kernel, dim3((unsigned)((c->n + 255) / 256), (unsigned)nrb), dim3(256), 0, s, (const unsigned short*)c->c,
                     (int64_t)c->n_p, c->n, M, Trows, lengths, sl);
  hipLaunchKernelGGL(rs_fire_fold_kernel, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, sl.cnt, nrb, c->n, fire);
  // x_hat of exactly that latent and the residual sweep, as sae_recon_files runs them -- and no attribution GEMM
  ev_begin(c, KID_RECON_DECODE, s);
  const int rc = decode_l1_latent(c, c->c, round_up(M, c->row_pad) / 128, M, sc.xr, s);
  ev_end(c, KID_RECON_DECODE, s);
  if (rc) return rc;
  ev_begin(c, KID_RECON_RESID, s);
  recon_launch_resid(c, x, sc, (float*)nullptr, (bf16_t*)nullptr, (bf16_t*)nullptr, round_up(M, STATS_RB), M, Trows, lengths, s);
  hipLaunchKernelGGL(rs_rowloss_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, sc.rowpart, c->d_p / RC_CW, M, row_loss);
  ev_end(c, KID_RECON_RESID, s);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_resample_files(sae_ctx* c, const void* x, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths,
                                  float* row_loss, int64_t* fire_count, void* stream) {
  int64_t M;
  if (!fire_count) return fail(SAE_ERR_INVALID, "null argument");
  if (c)
    if (int rc = resample_refuse(c, "sae_resample_files")) return rc;
  if (int rc = file_pass_begin(kResamplePass, c, x, row_loss, n_files, rows_per_file, x_dtype, 0, &M)) return rc;
  if (misaligned(row_loss, 4) || misaligned(fire_count, 8)) return fail(SAE_ERR_INVALID, "row_loss must be 4-byte aligned, fire_count 8-byte aligned");
  if ((c->max_rows_p / STATS_RB) * (int64_t)c->n_p >= ((int64_t)1 << 31))
    return fail(SAE_ERR_INVALID, "sae_resample_files: max_rows / 128 x n_dict = %lld slab entries >= 2^31", (long long)((c->max_rows_p / STATS_RB) * (int64_t)c->n_p));
  char* area[2];                // the statistics pass's slab and the reconstruction report's scratch, side by side
  if (int rc = pass_scratch(c, {stats_scratch_bytes(c), recon_scratch_bytes(c)}, area)) return rc;
  const StatsSlab sl = stats_slab(c, area[0]);
  const ReconScratch sc = recon_scratch(c, area[1]);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = with_x_type(x_dtype, x, [&](auto* xt) {
        return resample_l1_impl(c, xt, M, (int)rows_per_file, lengths, row_loss, reinterpret_cast<unsigned long long*>(fire_count), sl, sc, s);
      }))
    return rc;
  file_pass_end(kResamplePass, c);
  return SAE_OK;
}

// the workspace of sae_resample_select: RsHeader | c [rows] u64 | block sums [blocks] u64 | owner [rows] u32 | dead [n] i32 | draw [n] i32
struct ResampleWs {
  RsHeader* hdr;
  unsigned long long *c, *blocksum;
  uint32_t* owner;
  int *dead, *draw;
  int64_t nblk, bytes;
};

static ResampleWs resample_ws(void* base, int64_t rows, int64_t n) {
  ResampleWs w;
  char* p = (char*)base;
  w.nblk = (rows + RS_SCAN_ROWS - 1) / RS_SCAN_ROWS;
  w.hdr = (RsHeader*)p; p += RS_HDR_BYTES;
  w.c = (unsigned long long*)p; p += rows * 8;
  w.blocksum = (unsigned long long*)p; p += w.nblk * 8;
  w.owner = (uint32_t*)p; p += round_up(rows * 4, 8);
  w.dead = (int*)p; p += round_up(n * 4, 8);
  w.draw = (int*)p; p += round_up(n * 4, 8);
  w.bytes = p - (char*)base;
  return w;
}

static bool resample_dims_ok(int64_t rows, int64_t n) { return rows >= 1 && rows <= RS_MAX_ROWS && n >= 1 && n <= RS_MAX_N; }

extern "C" int64_t sae_resample_workspace_bytes(int64_t rows, int64_t n) {
  return resample_dims_ok(rows, n) ? resample_ws(nullptr, rows, n).bytes : -1;
}

static_assert(sizeof(RsHeader) <= RS_HDR_BYTES && SAE_RESAMPLE_NCOUNTS == RS_NCOUNTS && SAE_RESAMPLE_DEAD == RS_DEAD && SAE_RESAMPLE_PAIRS == RS_PAIRS &&
              SAE_RESAMPLE_SKIPPED_DUPLICATE == RS_SKIPPED_DUPLICATE && SAE_RESAMPLE_TOTAL == RS_TOTAL && SAE_RESAMPLE_LMAX_BITS == RS_LMAX_BITS,
              "freud_sae.h, resample_draw.h and resample.h disagree");

extern "C" int sae_resample_select(const float* row_loss, int64_t rows, const int64_t* fire_count, int64_t n, uint64_t seed, uint64_t round,
                                   int32_t* latents_out, int64_t* rows_out, int64_t* counts_out, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  if (!row_loss || !fire_count || !latents_out || !rows_out || !counts_out || !workspace) return fail(SAE_ERR_INVALID, "null argument");
  if (!resample_dims_ok(rows, n)) return fail(SAE_ERR_INVALID, "rows=%lld outside [1, 2^31) or n=%lld outside [1, 2^24]", (long long)rows, (long long)n);
  if (workspace_bytes < sae_resample_workspace_bytes(rows, n))
    return fail(SAE_ERR_INVALID, "workspace of %lld bytes < sae_resample_workspace_bytes(%lld, %lld)", (long long)workspace_bytes, (long long)rows, (long long)n);
  if (misaligned(row_loss, 4) || misaligned(latents_out, 4) || misaligned(fire_count, 8) || misaligned(rows_out, 8) || misaligned(counts_out, 8) ||
      misaligned(workspace, 8))
    return fail(SAE_ERR_INVALID, "row_loss and latents_out must be 4-byte aligned, fire_count, rows_out, counts_out and the workspace 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const ResampleWs w = resample_ws(workspace, rows, n);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(row_loss);
  HIP_TRY(hipMemsetAsync(w.hdr, 0, RS_HDR_BYTES, s));
  HIP_TRY(hipMemsetAsync(w.owner, 0xFF, (size_t)rows * 4, s));
  hipLaunchKernelGGL(rs_max_kernel, dim3(grid_for(rows, 1024)), dim3(256), 0, s, bits, rows, w.hdr);
  hipLaunchKernelGGL(rs_blocksum_kernel, dim3((unsigned)w.nblk), dim3(RS_SCAN_ROWS), 0, s, bits, rows, w.hdr, w.blocksum);
  hipLaunchKernelGGL(rs_blockscan_kernel, dim3(1), dim3(RS_SCAN_ROWS), 0, s, w.blocksum, w.nblk, w.hdr);
  hipLaunchKernelGGL(rs_prefix_kernel, dim3((unsigned)w.nblk), dim3(RS_SCAN_ROWS), 0, s, bits, rows, w.hdr, w.blocksum, w.c);
  hipLaunchKernelGGL(rs_dead_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(fire_count), (int)n, w.dead, w.hdr);
  hipLaunchKernelGGL(rs_draw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.hdr, w.c, rows, (unsigned long long)seed,
                     (unsigned long long)round, w.draw, w.owner);
  hipLaunchKernelGGL(rs_emit_kernel, dim3(1), dim3(256), 0, s, w.hdr, w.dead, w.draw, w.owner, latents_out, reinterpret_cast<long long*>(rows_out),
                     reinterpret_cast<long long*>(counts_out));
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_resample_apply(sae_ctx* c, const int32_t* latents, int64_t n_latents, const float* x_rows, double alpha, int64_t* out_stats,
                                  void* stream) {
  if (!c || !latents || !x_rows || !out_stats) return fail(SAE_ERR_INVALID, "null argument");
  if (int rc = resample_refuse(c, "sae_resample_apply")) return rc;
  if (n_latents < 1 || n_latents > c->n) return fail(SAE_ERR_INVALID, "n_latents=%lld outside [1, n_dict=%d]", (long long)n_latents, c->n);
  if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(SAE_ERR_INVALID, "alpha=%g outside [0, 1]", alpha);
  if (misaligned(latents, 4) || misaligned(x_rows, 4) || misaligned(out_stats, 8))
    return fail(SAE_ERR_INVALID, "latents and x_rows must be 4-byte aligned, out_stats 8-byte aligned");
  USE_DEVICE(c);
  hipStream_t s = (hipStream_t)stream;
  // the latents are read back and checked before anything is enqueued that writes
  int32_t* host = new int32_t[(size_t)n_latents];
  unsigned char* seen = new unsigned char[(size_t)c->n]();
  int rc = SAE_OK;
  hipError_t e = hipMemcpyAsync(host, latents, (size_t)n_latents * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) rc = fail(SAE_ERR_HIP, "reading the latents failed: %s", hipGetErrorString(e));
  for (int64_t i = 0; i < n_latents && !rc; ++i) {
    if (host[i] < 0 || host[i] >= c->n) rc = fail(SAE_ERR_INVALID, "pair %lld: latent %d outside [0, %d)", (long long)i, host[i], c->n);
    else if (seen[host[i]]) rc = fail(SAE_ERR_INVALID, "pair %lld repeats latent %d", (long long)i, host[i]);
    else seen[host[i]] = 1;
  }
  delete[] host;
  delete[] seen;
  if (rc) return rc;
  // the master as the reference holds it (d_p <= 384: the folded update may have left it un-normalised), then the columns; every
  // derived copy (Wb, Wt, cnorm, cn_part) is rebuilt by the next forward, as after sae_set_params
  settle_weights(c, s);
  c->cn_valid = false;
  HIP_TRY(hipMemsetAsync(out_stats, 0, (size_t)(2 + n_latents) * 8, s));
  hipLaunchKernelGGL(rs_apply_kernel, dim3((unsigned)n_latents), dim3(256), 0, s, latents, x_rows, c->d, c->d_p, c->n_p, (float)alpha, c->P, c->Mom,
                     c->Var, reinterpret_cast<unsigned long long*>(out_stats));
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- input statistics (input_stats.h): moments and the geometric median of a resident sample, no context
static_assert(SAE_INPUT_MAX_D == IN_MAX_D && SAE_INPUT_MAX_ITERATIONS == 1024 && IN_MAX_NV * 64 * 4 >= IN_MAX_D, "freud_sae.h and input_stats.h disagree");

// the workspace: the frame count | the folded sums [4 d + 2] | the units' partials [U][max(4 d, d + 2)]
struct InputWs {
  int64_t* n_frames;
  double *folded, *part;
  int64_t units_per_file, U, bytes;
};

static InputWs input_ws(void* base, int64_t n_files, int64_t rows_per_file, int64_t d) {
  InputWs w;
  char* p = (char*)base;
  w.units_per_file = (rows_per_file + IN_UNIT - 1) / IN_UNIT;
  w.U = n_files * w.units_per_file;
  w.n_frames = (int64_t*)p; p += 64;
  w.folded = (double*)p; p += round_up((4 * d + 2) * 8, 64);
  w.part = (double*)p; p += w.U * std::max<int64_t>(4 * d, d + 2) * 8;
  w.bytes = p - (char*)base;
  return w;
}

static bool input_dims_ok(int64_t n_files, int64_t rows_per_file, int64_t d) {
  return n_files >= 1 && n_files <= 65535 && rows_per_file >= 1 && rows_per_file <= 65535ll * 128 && d >= 1 && d <= IN_MAX_D;
}

extern "C" int64_t sae_input_stats_workspace_bytes(int64_t n_files, int64_t rows_per_file, int64_t d) {
  return input_dims_ok(n_files, rows_per_file, d) ? input_ws(nullptr, n_files, rows_per_file, d).bytes : -1;
}

// the checks that sae_input_moments and sae_input_median share; nothing is enqueued when one fails
static int input_check(const char* fn, const void* x, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const void* out,
                       const void* workspace, int64_t workspace_bytes) {
  if (!x || !out || !workspace) return fail(SAE_ERR_INVALID, "%s: null argument", fn);
  if (int rc = search_shape_check(n_files, rows_per_file)) return rc;
  if (d < 1 || d > IN_MAX_D) return fail(SAE_ERR_INVALID, "%s: d=%lld outside [1, %d]", fn, (long long)d, IN_MAX_D);
  if (x_dtype != SAE_DTYPE_F32 && x_dtype != SAE_DTYPE_F16 && x_dtype != SAE_DTYPE_BF16) return fail(SAE_ERR_INVALID, "unknown x_dtype %d", x_dtype);
  if (workspace_bytes < sae_input_stats_workspace_bytes(n_files, rows_per_file, d))
    return fail(SAE_ERR_INVALID, "%s: workspace of %lld bytes < sae_input_stats_workspace_bytes(%lld, %lld, %lld)", fn, (long long)workspace_bytes,
                (long long)n_files, (long long)rows_per_file, (long long)d);
  if (misaligned(x, x_dtype == SAE_DTYPE_F32 ? 4 : 2) || misaligned(out, 8) || misaligned(workspace, 8))
    return fail(SAE_ERR_INVALID, "%s: x must be aligned to its element, the outputs and the workspace to 8 bytes", fn);
  return SAE_OK;
}

template <int MODE>
static void input_launch_fold(const InputWs& w, int ncols, int d, double* m_next, double* objective, hipStream_t s) {
  const int cols = MODE == IN_FOLD_WEISZFELD ? d : ncols;
  hipLaunchKernelGGL(in_fold_kernel<MODE>, dim3((unsigned)((cols + IN_FOLD_COLS - 1) / IN_FOLD_COLS)), dim3(256), 0, s, w.part, w.U, ncols, d,
                     w.folded, m_next, objective, w.n_frames);
}

extern "C" int sae_input_moments(const void* x, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths,
                                 double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = input_check("sae_input_moments", x, n_files, rows_per_file, d, x_dtype, out, workspace, workspace_bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const InputWs w = input_ws(workspace, n_files, rows_per_file, d);
  const int T = (int)rows_per_file, di = (int)d, upf = (int)w.units_per_file;
  hipLaunchKernelGGL(in_count_kernel, dim3(1), dim3(256), 0, s, lengths, n_files, T, w.n_frames);
  int rc = with_x_type(x_dtype, x, [&](auto* xt) {
    using XT = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
    hipLaunchKernelGGL((in_moments_kernel<XT, 0>), dim3((unsigned)w.U), dim3(256), 0, s, xt, T, di, upf, lengths, (const double*)nullptr, w.part);
    input_launch_fold<IN_FOLD_MOMENTS0>(w, 4 * di, di, nullptr, nullptr, s);
    hipLaunchKernelGGL(in_finish_kernel<0>, dim3(1), dim3(256), 0, s, w.folded, di, w.n_frames, out);
    // the centred sweep reads the mean that the first one left in out
    hipLaunchKernelGGL((in_moments_kernel<XT, 1>), dim3((unsigned)w.U), dim3(256), 0, s, xt, T, di, upf, lengths, (const double*)out, w.part);
    input_launch_fold<IN_FOLD_SUM>(w, di, di, nullptr, nullptr, s);
    hipLaunchKernelGGL(in_finish_kernel<1>, dim3(1), dim3(256), 0, s, w.folded, di, w.n_frames, out);
    return (int)SAE_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// one sweep at the estimate m: the units' partials, then the fold into m_next (null: the objective alone) and *objective
template <typename XT>
static int input_launch_step(const XT* x, int T, int d, const InputWs& w, const int32_t* lengths, const double* m, float floor_w,
                             double* m_next, double* objective, hipStream_t s) {
  constexpr int EPV = 16 / (int)sizeof(XT);
  // the register form needs 16-byte aligned rows; NV = its vectors per lane
  const bool vec = d % EPV == 0 && !misaligned(x, 16);
  const int nv = vec ? (d / EPV + 63) / 64 : 0;
  int rc = SAE_OK;
  const bool known = with_in_nv(nv, [&](auto NV) {
    // (d <= IN_MAX_D: a 2-byte dtype never has more than 4 vectors per lane, and those forms are not compiled)
    constexpr int KNV = (decltype(NV)::value - 1) * 64 * EPV < IN_MAX_D ? decltype(NV)::value : 0;
    auto kern = in_weiszfeld_kernel<XT, KNV>;
    const size_t lds = (size_t)(nv ? d : 4 * d) * 8;
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) { rc = fail(SAE_ERR_HIP, "hipFuncSetAttribute(%zu bytes of LDS) failed: %s", lds, hipGetErrorString(e)); return; }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)w.U), dim3(256), lds, s, x, T, d, (int)w.units_per_file, lengths, m, floor_w, w.part);
  });
  if (!known) return fail(SAE_ERR_INVALID, "no Weiszfeld kernel for %d vectors per lane", nv);
  if (rc) return rc;
  input_launch_fold<IN_FOLD_WEISZFELD>(w, d + 2, d, m_next, objective, s);
  return SAE_OK;
}

extern "C" int sae_input_median(const void* x, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths,
                                const double* start, double floor, int iterations, double* path, double* objective, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  if (!start || !objective) return fail(SAE_ERR_INVALID, "sae_input_median: null argument");
  if (int rc = input_check("sae_input_median", x, n_files, rows_per_file, d, x_dtype, path, workspace, workspace_bytes)) return rc;
  if (iterations < 1 || iterations > SAE_INPUT_MAX_ITERATIONS)
    return fail(SAE_ERR_INVALID, "iterations=%d outside [1, %d]", iterations, SAE_INPUT_MAX_ITERATIONS);
  if (!(floor >= (double)FLT_MIN && floor <= (double)FLT_MAX)) return fail(SAE_ERR_INVALID, "floor=%g outside [FLT_MIN, FLT_MAX]", floor);
  if (misaligned(start, 8) || misaligned(objective, 8)) return fail(SAE_ERR_INVALID, "start and objective must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const InputWs w = input_ws(workspace, n_files, rows_per_file, d);
  const int T = (int)rows_per_file, di = (int)d;
  hipLaunchKernelGGL(in_count_kernel, dim3(1), dim3(256), 0, s, lengths, n_files, T, w.n_frames);
  HIP_TRY(hipMemcpyAsync(path, start, (size_t)d * 8, hipMemcpyDeviceToDevice, s));
  // sweep k at m_k gives J_k and m_{k+1}; the last sweep, at m_I, gives J_I alone.  No host synchronisation in between.
  int rc = with_x_type(x_dtype, x, [&](auto* xt) {
    for (int k = 0; k <= iterations; ++k)
      if (int r = input_launch_step(xt, T, di, w, lengths, path + (int64_t)k * d, (float)floor, k < iterations ? path + (int64_t)(k + 1) * d : nullptr,
                                    objective + k, s))
        return r;
    return (int)SAE_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- input covariance (input_cov.h, input_cov_plan.h): the centred scatter of a resident sample, no context
extern "C" int64_t sae_input_cov_workspace_bytes(int64_t n_files, int64_t rows_per_file, int64_t d) {
  return input_dims_ok(n_files, rows_per_file, d) ? icv_partial_bytes(icv_plan(n_files, rows_per_file, d)) : -1;
}

extern "C" int sae_input_cov_plan(int64_t n_files, int64_t rows_per_file, int64_t d, int64_t out[4]) {
  if (!out) return fail(SAE_ERR_INVALID, "sae_input_cov_plan: null argument");
  if (!input_dims_ok(n_files, rows_per_file, d))
    return fail(SAE_ERR_INVALID, "sae_input_cov_plan: n_files=%lld, rows_per_file=%lld or d=%lld out of range", (long long)n_files,
                (long long)rows_per_file, (long long)d);
  const IcvPlan p = icv_plan(n_files, rows_per_file, d);
  out[0] = ICV_TILE;
  out[1] = p.tiles;
  out[2] = p.segments;
  out[3] = p.units_per_seg;
  return SAE_OK;
}

extern "C" int sae_input_cov(const void* x, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths,
                             const double* center, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const fn = "sae_input_cov";
  if (!x || !out || !workspace) return fail(SAE_ERR_INVALID, "%s: null argument", fn);
  if (int rc = search_shape_check(n_files, rows_per_file)) return rc;
  if (d < 1 || d > IN_MAX_D) return fail(SAE_ERR_INVALID, "%s: d=%lld outside [1, %d]", fn, (long long)d, IN_MAX_D);
  if (x_dtype != SAE_DTYPE_F32 && x_dtype != SAE_DTYPE_F16 && x_dtype != SAE_DTYPE_BF16) return fail(SAE_ERR_INVALID, "unknown x_dtype %d", x_dtype);
  if (workspace_bytes < sae_input_cov_workspace_bytes(n_files, rows_per_file, d))
    return fail(SAE_ERR_INVALID, "%s: workspace of %lld bytes < sae_input_cov_workspace_bytes(%lld, %lld, %lld)", fn, (long long)workspace_bytes,
                (long long)n_files, (long long)rows_per_file, (long long)d);
  if (misaligned(x, x_dtype == SAE_DTYPE_F32 ? 4 : 2) || misaligned(out, 8) || misaligned(workspace, 8) || misaligned(center, 8))
    return fail(SAE_ERR_INVALID, "%s: x must be aligned to its element, the centre, the output and the workspace to 8 bytes", fn);
  hipStream_t s = (hipStream_t)stream;
  const IcvPlan p = icv_plan(n_files, rows_per_file, d);
  double* const part = (double*)workspace;
  int rc = with_x_type(x_dtype, x, [&](auto* xt) {
    using XT = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
    hipLaunchKernelGGL((icv_tile_kernel<XT>), dim3((unsigned)p.tiles, (unsigned)p.segments), dim3(256), 0, s, xt, (int)rows_per_file, (int)d, p,
                       lengths, center, part);
    return (int)SAE_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(icv_fold_kernel, dim3((unsigned)p.tiles, ICV_TILE * ICV_TILE / 256), dim3(256), 0, s, (const double*)part, p, (int)d, out);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- the HBM-resident activation store (resident.h): the one-time fp32 -> bf16 conversion of uploaded rows and the gather of a
// batch's files out of the store
extern "C" int64_t sae_store_piece_bytes(void) { return RS_PIECE_BYTES; }

extern "C" int sae_store_convert(const float* src, void* dst, int64_t n_elems, void* stream) {
  const char* const fn = "sae_store_convert";
  if (!src || !dst) return fail(SAE_ERR_INVALID, "%s: null argument", fn);
  if (n_elems < 0) return fail(SAE_ERR_INVALID, "%s: n_elems=%lld is negative", fn, (long long)n_elems);
  if (misaligned(src, 4) || misaligned(dst, 2)) return fail(SAE_ERR_INVALID, "%s: src must be 4-byte aligned and dst 2-byte aligned", fn);
  if (n_elems == 0) return SAE_OK;
  hipStream_t s = (hipStream_t)stream;
  if (!misaligned(src, 16) && !misaligned(dst, 16))
    hipLaunchKernelGGL(store_convert_kernel<true>, dim3(grid_for(std::max<int64_t>(n_elems >> 3, 1), 8192)), dim3(256), 0, s, src, (uint16_t*)dst, n_elems);
  else
    hipLaunchKernelGGL(store_convert_kernel<false>, dim3(grid_for(n_elems, 8192)), dim3(256), 0, s, src, (uint16_t*)dst, n_elems);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

extern "C" int sae_store_gather(const void* store, int64_t n_files, int64_t row_bytes, const int32_t* idx, int64_t nb, void* out,
                                int64_t out_stride_bytes, uint32_t* err, void* stream) {
  const char* const fn = "sae_store_gather";
  if (!store || !idx || !out || !err) return fail(SAE_ERR_INVALID, "%s: null argument", fn);
  if (n_files < 1 || n_files > 0x7FFFFFFFll) return fail(SAE_ERR_INVALID, "%s: n_files=%lld outside [1, 2^31 - 1]", fn, (long long)n_files);
  if (row_bytes < 1 || nb < 0) return fail(SAE_ERR_INVALID, "%s: row_bytes=%lld, nb=%lld", fn, (long long)row_bytes, (long long)nb);
  if (out_stride_bytes < row_bytes)
    return fail(SAE_ERR_INVALID, "%s: out_stride_bytes=%lld < row_bytes=%lld", fn, (long long)out_stride_bytes, (long long)row_bytes);
  if (misaligned(idx, 4) || misaligned(err, 4)) return fail(SAE_ERR_INVALID, "%s: idx and err must be 4-byte aligned", fn);
  const int width = rs_copy_width((uint64_t)reinterpret_cast<uintptr_t>(store) | (uint64_t)reinterpret_cast<uintptr_t>(out) | (uint64_t)row_bytes |
                                  (uint64_t)out_stride_bytes);
  if (!width) return fail(SAE_ERR_INVALID, "%s: the store, the destination, row_bytes and out_stride_bytes must be multiples of 2 bytes", fn);
  const int64_t pieces = rs_pieces(row_bytes);
  if (nb > 0x7FFFFFFFll / pieces) return fail(SAE_ERR_INVALID, "%s: nb=%lld rows of %lld pieces exceed 2^31 - 1 workgroups", fn, (long long)nb, (long long)pieces);
  if (nb == 0) return SAE_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(nb * pieces));
  const char* const src = (const char*)store;
  char* const dst = (char*)out;
  if (width == 16)
    hipLaunchKernelGGL(store_gather_kernel<rs_u32x4>, grid, dim3(RS_THREADS), 0, s, src, n_files, row_bytes, idx, pieces, dst, out_stride_bytes, err);
  else if (width == 4)
    hipLaunchKernelGGL(store_gather_kernel<uint32_t>, grid, dim3(RS_THREADS), 0, s, src, n_files, row_bytes, idx, pieces, dst, out_stride_bytes, err);
  else
    hipLaunchKernelGGL(store_gather_kernel<uint16_t>, grid, dim3(RS_THREADS), 0, s, src, n_files, row_bytes, idx, pieces, dst, out_stride_bytes, err);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}

// ---- frame batches (frame_gather.h): rows of the destination = the frames that a run of positions of the epoch's permutation holds
extern "C" int sae_store_gather_frames(const void* store, int64_t n_files, int64_t rows_per_file, int64_t frame_bytes, const int64_t* prefix,
                                       int64_t n_frames, uint64_t key, int64_t pos0, int64_t pos_stride, int64_t rows, void* out,
                                       int64_t out_stride_bytes, int64_t* ordinals_out, uint32_t* err, void* stream) {
  const char* const fn = "sae_store_gather_frames";
  if (!store || (!out && rows != 0) || !err) return fail(SAE_ERR_INVALID, "%s: null argument", fn);
  if (n_files < 1 || n_files > 0x7FFFFFFFll || rows_per_file < 1 || rows_per_file > 0x7FFFFFFFll)
    return fail(SAE_ERR_INVALID, "%s: n_files=%lld, rows_per_file=%lld outside [1, 2^31 - 1]", fn, (long long)n_files, (long long)rows_per_file);
  if (frame_bytes < 1 || frame_bytes > 0x7FFFFFFFll) return fail(SAE_ERR_INVALID, "%s: frame_bytes=%lld outside [1, 2^31 - 1]", fn, (long long)frame_bytes);
  if (n_frames < 1 || n_frames > n_files * rows_per_file)
    return fail(SAE_ERR_INVALID, "%s: n_frames=%lld outside [1, n_files * rows_per_file = %lld]", fn, (long long)n_frames,
                (long long)(n_files * rows_per_file));
  if (rows < 0 || rows > n_frames || (rows > 0 && (pos0 < 0 || pos0 >= n_frames || pos_stride < 1)))
    return fail(SAE_ERR_INVALID, "%s: rows=%lld, pos0=%lld, pos_stride=%lld with %lld frames", fn, (long long)rows, (long long)pos0,
                (long long)pos_stride, (long long)n_frames);
  if (rows > 1 && (rows - 1) > (n_frames - 1 - pos0) / pos_stride)       // pos0 + (rows - 1) * pos_stride >= n_frames, without the product
    return fail(SAE_ERR_INVALID, "%s: the last position pos0 + (rows - 1) * pos_stride leaves the %lld frames", fn, (long long)n_frames);
  if (out_stride_bytes < frame_bytes)
    return fail(SAE_ERR_INVALID, "%s: out_stride_bytes=%lld < frame_bytes=%lld", fn, (long long)out_stride_bytes, (long long)frame_bytes);
  if (misaligned(err, 4) || misaligned(prefix, 8) || misaligned(ordinals_out, 8))
    return fail(SAE_ERR_INVALID, "%s: err must be 4-byte, prefix and ordinals_out 8-byte aligned", fn);
  const int width = rs_copy_width((uint64_t)reinterpret_cast<uintptr_t>(store) | (uint64_t)reinterpret_cast<uintptr_t>(out) | (uint64_t)frame_bytes |
                                  (uint64_t)out_stride_bytes);
  if (!width) return fail(SAE_ERR_INVALID, "%s: the store, the destination, frame_bytes and out_stride_bytes must be multiples of 2 bytes", fn);
  const fp_plan plan = fp_plan_of(frame_bytes, width, rows);
  if (plan.blocks > 0x7FFFFFFFll) return fail(SAE_ERR_INVALID, "%s: %lld workgroups exceed 2^31 - 1", fn, (long long)plan.blocks);
  if (rows == 0) return SAE_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)plan.blocks);
  const char* const src = (const char*)store;
  char* const dst = (char*)out;
  const uint64_t N = (uint64_t)n_frames, p0 = (uint64_t)pos0, ps = (uint64_t)pos_stride;
  if (width == 16)
    hipLaunchKernelGGL(frame_gather_kernel<rs_u32x4>, grid, dim3(FP_THREADS), 0, s, src, prefix, n_files, rows_per_file, frame_bytes, N, key, p0, ps,
                       rows, plan, dst, out_stride_bytes, ordinals_out, err);
  else if (width == 4)
    hipLaunchKernelGGL(frame_gather_kernel<uint32_t>, grid, dim3(FP_THREADS), 0, s, src, prefix, n_files, rows_per_file, frame_bytes, N, key, p0, ps,
                       rows, plan, dst, out_stride_bytes, ordinals_out, err);
  else
    hipLaunchKernelGGL(frame_gather_kernel<uint16_t>, grid, dim3(FP_THREADS), 0, s, src, prefix, n_files, rows_per_file, frame_bytes, N, key, p0, ps,
                       rows, plan, dst, out_stride_bytes, ordinals_out, err);
  HIP_TRY(hipGetLastError());
  return SAE_OK;
}
