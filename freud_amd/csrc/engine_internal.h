// What the translation units of libfreud_sae.so share -- engine.hip (the context, the training paths, evaluation, the getters) and
// passes.hip (the file passes and the context-free utilities): the context, the error and launch helpers, the per-call
// thread-locals and the core functions the passes call.  Host code only: no kernel is defined here, so any unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rccl/rccl.h>

#include <type_traits>

#include "../../include/freud_sae.h"
#include "common.h"
#include "dev_mem.h"
#include "gemm.h"
#include "p2p_index.h"

struct CscEntry;                // topk_sparse.h

// (nothing below is part of the C ABI: the library exports the sae_* functions of include/freud_sae.h only)
#pragma GCC visibility push(hidden)

// (__thread, not thread_local: for an extern thread_local the compiler calls a wrapper that tests the address of a WEAK "TLS init
// function" and calls it when that is not null.  Built with this toolchain, hidden, into a shared library, the first access from
// passes.hip crashed there -- the symbol stays undefined in the library and the test did not read null; a two-file program with the
// same declarations does the same.  __thread promises a constant initialiser: plain TLS accesses, no wrapper, hidden or not.)
extern __thread bool g_force_gemm128;   // (the CURRENT call's context: set by use_device, like g_device -- ADVICE r5)
                                        // sae_config.force_gemm128: keep every GEMM on the 128x128 kernel (A/B timing, tests)
extern __thread bool g_no_stream;       // FREUD_GEMM_STREAM=0 / debug_flags 86: the K = d GEMMs in gemm256.h's tile form (A/B timing, tests)
extern __thread int g_device;  // device of the context the current call works on (set by use_device)

// ------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(SAE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                      __FILE__, __LINE__);                                              \
  } while (0)

// dynamic-LDS opt-in (> 64 KiB) is a per-device function attribute: remember (function, device) pairs
int ensure_lds_attr(const void* fn, int bytes, int device);
#define LDS_ATTR(fn, bytes, device)                                           \
  do {                                                                        \
    int rc_ = ensure_lds_attr(reinterpret_cast<const void*>(fn), (bytes), (device)); \
    if (rc_) return rc_;                                                      \
  } while (0)
#pragma GCC visibility pop

// workgroups of `per` items that cover n items, at most `cap` of them (the kernels behind it stride over the rest)
static int grid_for(int64_t n, int cap, int per = 256) {
  const int64_t g = (n + per - 1) / per;
  return (int)(g < cap ? g : cap);
}

// the one dispatch on an activation dtype of include/freud_sae.h: f(typed pointer) -> status
template <class F>
static int with_x_type(int x_dtype, const void* x, F&& f) {
  switch (x_dtype) {
    case SAE_DTYPE_F32: return f((const float*)x);
    case SAE_DTYPE_F16: return f((const _Float16*)x);
    case SAE_DTYPE_BF16: return f((const bf16_t*)x);
    default: return fail(SAE_ERR_INVALID, "unknown x_dtype %d", x_dtype);
  }
}

// ... and its inverse: the dtype code of a typed pointer's element
template <typename T>
static constexpr int x_dtype_of() {
  return std::is_same<T, float>::value ? SAE_DTYPE_F32 : std::is_same<T, _Float16>::value ? SAE_DTYPE_F16 : SAE_DTYPE_BF16;
}

// the one dispatch of the sparse TopK kernels on d_p: f(integral_constant<NP>), NP = d_p / 128 where a kernel is specialised, else 0
template <class F>
static void with_np(int d_p, F&& f) {
  if (d_p == 384) f(std::integral_constant<int, 3>{});
  else if (d_p == 768) f(std::integral_constant<int, 6>{});
  else if (d_p == 1280) f(std::integral_constant<int, 10>{});
  else f(std::integral_constant<int, 0>{});
}

// ... and of the two kernels of the TopK backward that exist for the three trained widths only (sparse_bwd_kernel, topk_dacts_kernel):
// exactly <3>, <6> and <10> -- the caller guarantees d_p in {384, 768, 1280}
template <class F>
static void with_np_trained(int d_p, F&& f) {
  if (d_p == 384) f(std::integral_constant<int, 3>{});
  else if (d_p == 768) f(std::integral_constant<int, 6>{});
  else f(std::integral_constant<int, 10>{});
}

// the entry points' test of a pointer argument against the alignment its kernels need (a null optional pointer passes)
static bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

// ------------------------------------------------------------------------------------------
// kernel ids for profiling
// ------------------------------------------------------------------------------------------
enum KernelId {
  KID_PREP_W = 0,
  KID_PREP_X,
  KID_ENC_FWD,
  KID_DEC_FWD,
  KID_FWD_FUSED,
  KID_DPRE,
  KID_DW,
  KID_BWD_FUSED,
  KID_REDUCE,
  KID_OPT,
  KID_TK_ENC,
  KID_TK_SELECT,
  KID_TK_DECODE,
  KID_TK_DDENSE,
  KID_TK_DWD,
  KID_TK_DWE,
  KID_TK_DSAE,
  KID_TK_AUX,
  KID_EXCHANGE,        // data parallel: the gradient exchange (peer-exchange kernel or ncclAllReduce), on the stream it runs on
  KID_STATS_XCHG,      // data parallel: the batch statistics (push inside finalize_losses, or the statistics kernel + its exchange)
  KID_STEP_TOTAL,
  KID_COACT_PACK,      // feature co-activation (coact.h): the mask pack and the i8 update of sae_coact_files
  KID_COACT_UPDATE,
  KID_MANIP_SERIES,    // feature manipulation (manip.h): the series + operand rows, the standard decode, the apply rule
  KID_MANIP_DECODE,
  KID_MANIP_APPLY,
  KID_LABEL_PACK,      // feature labels (labels.h): the label pack + label counts and the rectangular i8 update of sae_label_files
  KID_LABEL_UPDATE,
  KID_HIST,            // activation histograms (hist.h): every kernel of sae_hist_files after the encoder
  KID_RECON_DECODE,    // reconstruction report (recon.h): the decode of the forward's latent, the residual sweep, the attribution
  KID_RECON_RESID,     //   (L1: the GEMM with EpiAttr; TopK: the dots and the column walk) with the fold
  KID_RECON_ATTR,
  KID_RECON_ATTR_STREAM,   // ... the same bracket when the attribution GEMM ran in the streaming form (gemm256s.h)
  KID_COLLECT,         // feature collection (collect.h): the row collect kernel of sae_collect_files after the encoder
  KID_TIMING,          // feature timing (timing.h): every kernel of sae_timing_files after the encoder
  KID_FRONTIER_SORT,   // sparsity frontier (frontier.h): the collect kernels into scratch, the walk alone, the dimension sums + the fold
  KID_FRONTIER_WALK,
  KID_FRONTIER_FOLD,
  KID_PURSUIT_GEMM,    // pursuit frontier (pursuit.h): the K selection GEMMs with EpiPursuit, the K step kernels, the finish + dimension sums + fold
  KID_PURSUIT_STEP,
  KID_PURSUIT_FOLD,
  KID_REFIT_SORT,      // refit frontier (refit.h): the collect kernels into scratch, the refit kernel alone, the finish + dimension sums + fold
  KID_REFIT_CHOL,
  KID_REFIT_FOLD,
  KID_CROSS_PACK,      // cross-activation (cross.h): the mask packs of sae_cross_mask_files (its update is context-free: no ring to record in)
  KID_COUNT
};
constexpr int EV_RING = 64;

struct EvRing {
  hipEvent_t beg[EV_RING], end[EV_RING];
  int n = 0;  // recorded since last read
};

// What the last forward-like call left in the context: a bf16 forward (latent rows, metrics), an fp32 evaluation (metrics and the
// per-feature maxima in e32_colmax, no bf16 latent rows), or a file pass (sae_search_files / sae_stats_files: nothing to read).
enum LastCall { LAST_FWD_BF16 = 0, LAST_FWD_E32, LAST_SEARCH, LAST_STATS, LAST_COACT, LAST_LABELS, LAST_HIST, LAST_RECON, LAST_COLLECT, LAST_TIMING, LAST_RESAMPLE, LAST_FRONTIER, LAST_PURSUIT, LAST_REFIT, LAST_CROSS };

// A file pass: the words of its entry point's messages, the flags it knows, the state it leaves (file_pass_end) and what the getters
// of the last forward call that state when they refuse (no_forward_left).  sae_manipulate_files leaves the state of sae_eval.
struct FilePassKind {
  const char *fn, *fp8_advice, *flags_noun;
  int flags_mask;
  LastCall leaves;
  const char* left_by;
};
static const FilePassKind kSearchPass = {"sae_search_files", "search in a bf16 context", "search", SAE_SEARCH_UNFUSED, LAST_SEARCH, "a feature search"};
static const FilePassKind kStatsPass = {"sae_stats_files", "run the statistics in a bf16 context", "stats", SAE_STATS_UNFUSED, LAST_STATS, "a feature statistics pass"};
static const FilePassKind kCoactPass = {"sae_coact_files", "count co-activations in a bf16 context", "co-activation", 0, LAST_COACT, "a feature co-activation pass"};
static const FilePassKind kLabelPass = {"sae_label_files", "count labels in a bf16 context", "label", 0, LAST_LABELS, "a feature label pass"};
static const FilePassKind kHistPass = {"sae_hist_files", "build the histograms in a bf16 context", "histogram", 0, LAST_HIST, "an activation histogram pass"};
static const FilePassKind kManipPass = {"sae_manipulate_files", "manipulate in a bf16 context", "manipulation", 0, LAST_FWD_BF16, nullptr};
static const FilePassKind kReconPass = {"sae_recon_files", "build the reconstruction report in a bf16 context", "reconstruction", SAE_RECON_UNFUSED, LAST_RECON, "a reconstruction report"};
static const FilePassKind kCollectPass = {"sae_collect_files", "collect the features in a bf16 context", "collect", SAE_COLLECT_IDX32, LAST_COLLECT, "a feature collection"};
static const FilePassKind kTimingPass = {"sae_timing_files", "time the features in a bf16 context", "timing", SAE_TIMING_ONE_CHUNK, LAST_TIMING, "a feature timing pass"};
static const FilePassKind kResamplePass = {"sae_resample_files", "resample in a bf16 context", "resample", 0, LAST_RESAMPLE, "a resampling pass"};
static const FilePassKind kFrontierPass = {"sae_frontier_files", "build the sparsity frontier in a bf16 context", "frontier", 0, LAST_FRONTIER, "a sparsity frontier pass"};
static const FilePassKind kPursuitPass = {"sae_pursuit_files", "run the pursuit in a bf16 context", "pursuit", 0, LAST_PURSUIT, "a pursuit frontier pass"};
static const FilePassKind kRefitPass = {"sae_refit_files", "run the refit in a bf16 context", "refit", 0, LAST_REFIT, "a refit frontier pass"};
static const FilePassKind kCrossPass = {"sae_cross_mask_files", "pack the masks in a bf16 context", "cross-activation", 0, LAST_CROSS, "a cross-activation pass"};
static const FilePassKind* const kFilePasses[] = {&kSearchPass, &kStatsPass, &kCoactPass, &kLabelPass, &kHistPass, &kReconPass, &kCollectPass,
                                                  &kTimingPass, &kResamplePass, &kFrontierPass, &kPursuitPass, &kRefitPass, &kCrossPass};

struct sae_ctx {
  // Every pointer field below that the context OWNS is allocated through `mem` (dev_mem.h; the last member, behind everything a step
  // touches) -- at creation with alloc, lazily with grow -- and released by its free_all in sae_destroy; nothing else frees.  What
  // is not owned says so: aliases and peer mappings.
  sae_config cfg;
  int d, n, d_p, n_p;
  int64_t max_rows_p;
  int64_t nW;       // d_p * n_p
  int64_t nparams;  // nW + n_p
  // flat parameter / state buffers: [W (d_p*n_p) | b (n_p)]
  float *P = nullptr, *Mom = nullptr, *Var = nullptr;
  float* G = nullptr;  // [grads (nparams) | metrics (8)]
  bf16_t *Wb = nullptr, *Wt = nullptr;
  // SAE_PREC_FP8: encoder / decoder GEMMs on e4m3 operands (l1_fp8.h); every padded dimension is a multiple of 256 then
  bool fp8 = false;
  bool fp8_bwd = false;         // SAE_PREC_FP8_BWD: the dpre GEMM of the backward on e4m3 operands too (dxh8 = e4m3(dx_hat s_g))
  unsigned char* dxh8 = nullptr;
  int row_pad = 128;            // M_p = round_up(M, row_pad)
  unsigned char *x8 = nullptr, *c8 = nullptr, *W8 = nullptr, *W8t = nullptr;
  float *scal8 = nullptr, *x8_part = nullptr;
  bool use_fused_fwd = false;
  int fwd_variant = 3;          // fused forward: 3 = fwd_split.h (fwd_fused2's products on encoder and decoder waves, two per SIMD),
                                // 2 = fwd_fused2.h (FREUD_FWD=2: A/B; the stamping diagnostic runs it), 1 = fwd_fused.h (FREUD_FWD=1: A/B, stamps)
  bf16_t *xb = nullptr, *c = nullptr, *dxh = nullptr, *dpre = nullptr;
  float *slab = nullptr, *db_part = nullptr, *l1_part = nullptr, *sq_part = nullptr, *scal = nullptr;
  double* gn_part = nullptr;
  float* cn_part = nullptr;
  bool cn_valid = false;       // cn_part holds the column-norm partials of the CURRENT weights (left by optimizer_l1_kernel)
  bool wb_valid = false;       // TopK: We_b / Wd_b are the bf16 copies of the CURRENT weights (left by optimizer_kernel)
  // L1, d_p <= 384 (optimizer_l1_cols_kernel): the update left the fp32 master UN-normalised (the reference's state after
  // optimizer.step()), the column denominators in cnorm and the bf16 copies Wb / Wt of the NORMALISED weights.
  //   wn_pending              that state holds;
  //   wn_fwd_seen             ... and one forward has used the copies since: the reference's W is normalised by now
  //                           (l1autoencoder.py:71-73), ours is so in effect -- the next update divides while loading, any other
  //                           reader of the master (settle_weights) has the division carried out first.
  float* cnorm = nullptr;
  bool wn_pending = false, wn_fwd_seen = false;
  sae_grad_ready_fn grad_ready = nullptr;   // data-parallel overlap hook (sae_set_grad_ready_callback)
  void* grad_ready_user = nullptr;
  int dw_chunk_rows = 0;       // generic L1 path: rows (of d_p) per weight-gradient GEMM launch when a hook is set
  int dw_chunk_splits = 1;     // its split-K factor
  int dw_col_chunks = 1;       // ... with the peer exchange: COLUMN chunks of dW instead (each reads only its own columns of the
  int dw_col_splits = 1;       //     latent / dpre streams, where a row chunk re-reads all of them), and their split-K factor
  float* cnt_part = nullptr;   // fused forward: per-workgroup masked-entry counts
  int gn_blocks = 0;
  bool step_fused_call = false; // set by sae_step: forward_backward and optimizer_step back to back
  bool gn_valid = false;       // gn_part holds the sum of squares of the UNSCALED local gradient
  bool metrics_fresh = false;  // the loss scalars were written by a forward and not yet averaged by an optimizer step
  const bf16_t* xb_cur = nullptr;   // bf16 GEMM copy of the current batch (== the caller's x when no copy is needed)
  unsigned int* masked = nullptr;
  int dw_splits = 1;
  // plain (single-launch) weight-gradient GEMM of the generic L1 path: whole tiles written straight into the gradient, the tiles
  // left over after whole rounds in K pieces through dw_tail (gemm_tail_plan); 0 = uniform split-K through the slabs
  int dw_tail_tiles = 0, dw_tail_pieces = 0;
  float* dw_tail = nullptr;
  int bwd_splits = 1;       // row ranges of the fused backward
  int bwd_range_splits = 1; // ... when it is launched in column-tile ranges (bwd_ranges > 1)
  bool use_fused_bwd = false;
  // ---- TopK variant (topkautoencoder.py): flat params [We (n_p*d_p) | be (n_p) | Wd (n_p*d_p) | bd (d_p)]
  bool topk = false;
  int k = 0, k_aux_cap = 0;
  int64_t rows_per_file = 0;          // T: x is [B][T][d] for x.mean(0); 0 = the whole batch is one file
  // decoder-norm constraint (sae_set_decoder_constraint; dec_norm.h): every optimizer step projects the gradient of W_dec off its
  // rows before the clip norm and renormalises the rows after the update (topkautoencoder.py:153-175)
  bool dec_constraint = false;
  double dead_threshold = 1e300;
  bf16_t *We_b = nullptr, *Wd_b = nullptr, *xs = nullptr, *pre = nullptr, *dense = nullptr, *aux_dense = nullptr;
  bf16_t *de_b = nullptr, *dh_b = nullptr;
  float *e = nullptr, *dh = nullptr, *e2_part = nullptr, *a2_part = nullptr, *dbd_part = nullptr, *ds_part = nullptr, *tkf = nullptr;
  int *top_idx = nullptr, *aux_idx = nullptr, *tk = nullptr;
  bf16_t *top_vals = nullptr, *aux_vals = nullptr, *multi_vals = nullptr;   // selected activations, compact [M_p][kcap]
  unsigned short* tile_max = nullptr;   // [M_p][n_p / 64] maxima of the pre-activation tiles (tile-driven select)
  unsigned char* sel_flag = nullptr;    // [M_p] rows the tile-driven select left to the general kernel
  bool dense_valid = false;     // the masked dense rows of the last forward were written (else: topk_densify on demand)
  bool multi_dense_valid = false;   // the same for the multi-TopK (4k) rows
  // AuxK on the compacted dead set (topk_aux.h)
  float* be_r = nullptr;            // encoder bias rounded to bf16 (as float), refreshed every step
  int slab_splits = 1;              // slabs allocated in c->slab (TopK)
  bool aux_compact = false;
  int *tkd = nullptr, *dead_cols = nullptr, *vec_rank = nullptr;
  unsigned char* vec_bits = nullptr;
  bf16_t* Wdd_b = nullptr;          // [n_p][d_p] rows of W_dec of the dead latents, compact
  float* aux_dbe_part = nullptr;    // [M_p / 128][n_p] column sums of the AuxK d pre-activations, compact columns
  int* dead_hint = nullptr;     // pinned host copy of tk[0] (number of dead latents), refreshed asynchronously every step
  double* tv_part = nullptr;
  long long* nfsf = nullptr;
  long long* dbe_fx = nullptr;  // [n_p] fixed-point d b_enc accumulator of the sparse d-activation kernel
  bool topk_sparse_da = false;  // sparse d pre-activations (topk_dacts_kernel) instead of the dense ddense GEMM + mask
  // CSC backward (topk_sparse.h): the selection sorted by latent, all three gradients as gathered weighted row sums
  bool topk_csc = false;
  unsigned short* csc_counts = nullptr;
  unsigned int *csc_block_off = nullptr, *csc_total = nullptr, *csc_start = nullptr, *csc_item_start = nullptr, *csc_item_latent = nullptr;
  unsigned int* csc_multi = nullptr;      // [0] = number of latents with no or several work items, [4 ...] = those latents (csc_items_kernel)
  CscEntry* csc_entries = nullptr;
  float *csc_part = nullptr, *csc_pbe = nullptr;
  int64_t csc_max_items = 0;
  // cfg.multi_topk (topkautoencoder.py:134-140): a second selection of 4k latents, its decode and its FVU / 8 in the loss
  bool multi = false;
  int k4 = 0;
  bf16_t *multi_dense = nullptr, *dm_b = nullptr;
  int* multi_idx = nullptr;
  float *em = nullptr, *m2_part = nullptr;
  unsigned char* dead = nullptr;
  // ---- data parallel (dp_kernels.h): batch statistics the losses normalise by, summed over the ranks
  double* stats = nullptr;      // [stats_cap] doubles
  int64_t stats_cap = 0, stats_n = 0;   // capacity / doubles the last sae_batch_stats wrote
  unsigned int* stats_part = nullptr;
  int dp_world = 0;             // > 0: forward_backward normalises by `stats` (which the host, or the engine's own RCCL
                                // communicator, has summed over dp_world ranks) instead of this rank's own batch
  // in-engine RCCL (sae_dist_init): statistics and gradient ranges are all-reduced on a communication stream
  bool dist = false;
  ncclComm_t comm = nullptr;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_x = nullptr, ev_stats = nullptr, ev_done = nullptr;
  hipEvent_t ev_range[16] = {};
  int ev_range_i = 0;
  int payload = SAE_DTYPE_F32;  // SAE_DTYPE_BF16: the fused d = 384 path all-reduces a bf16 copy of the gradient (sae_dist_set_payload)
  bf16_t* Gb = nullptr;         // that copy
  bool grads_in_bf16 = false;   // the current step's summed gradient lives in Gb (the optimizer step converts it back)
  int dist_error = 0;           // a collective of the current call failed to enqueue (message in dist_errmsg)
  char dist_errmsg[256] = "";
  // peer exchange over hipIpc mappings (p2p_exchange.h): the exchange of the in-engine protocol when sae_p2p_init was called
  bool p2p = false;
  int p2p_rank = 0;
  float* p2p_G[P2P_MAX_WORLD] = {};
  bf16_t* p2p_Gb[P2P_MAX_WORLD] = {};
  double* p2p_stats[P2P_MAX_WORLD] = {};
  unsigned long long* p2p_sig[P2P_MAX_WORLD] = {};
  void* p2p_opened[4 * P2P_MAX_WORLD] = {};      // peer mappings to close
  int p2p_nopened = 0;
  unsigned long long* sig = nullptr;             // this rank's flag block (uncached device memory)
  unsigned int* p2p_status = nullptr;            // device words: [0] sticky failure bits the exchange kernels set (P2P_ST_*), [1] self-test mismatches
  unsigned int* p2p_status_host = nullptr;       // host-mapped mirror of word 0 (hipHostMalloc): sae_dist_poll reads it without a sync
  unsigned int* p2p_status_hostdev = nullptr;    // its device address: an alias of p2p_status_host, not owned (never freed)
  int p2p_fault_kind = 0, p2p_fault_rank = -1;   // FREUD_P2P_FAULT=skip_phase2:<rank>[:<after exchanges>] (tests: the guards must catch it)
  unsigned long long p2p_fault_after = 0;
  float* col_stage = nullptr;                    // in-engine RCCL, d >= 1024: contiguous staging of the dW column chunks ([d_p x n_p] floats)
  float* audit_dst = nullptr;                    // sae_dist_audit: every gradient exchange first copies its segments here (the
                                                 // caller's buffer: an alias, not owned)
  bool finegrained = false;                      // FREUD_P2P_FINEGRAINED=1: G / Gb / stats in fine-grained device memory
  unsigned long long p2p_epoch[P2P_CHANNELS] = {};
  unsigned long long p2p_epoch_push = 0;         // epoch of the statistics push inside finalize_losses_kernel
  // 120 s of the 100 MHz clock (FREUD_P2P_TIMEOUT_MS): a LIVENESS bound, not a skew budget -- a rank may be late by a loader
  // stall, a validation pass or a checkpoint write; a failed context fails fast afterwards (sticky status, poisoned flags)
  unsigned long long p2p_timeout_ticks = 12000000000ull;
  bool gn_from_exchange = false;                 // gn_part holds the sum of squares of the EXCHANGED gradient
  int bal_m = 0;                // balanced fused backward (bwd_fused.h): quanta per workgroup (0 = uniform row ranges), workgroups,
  int bal_grid = 0;             //   and the blockIdx -> workgroup table (XCD-aware)
  short* bal_map = nullptr;
  int bwd_ranges = 1;           // fused d = 384 backward: column-tile ranges launched one after the other, each range reduced and
                                // exchanged on the communication stream under the next range's backward (sae_dist_set_overlap)
  // fp32 evaluation forward (eval_fp32.h; sae_set_eval_precision): buffers sized lazily for the largest evaluation batch seen
  bool stats_inline = true;     // fused d = 384 L1 path with the peer exchange: statistics pushed inside finalize_losses_kernel (see inline_stats)
  bool no_stream = false;       // this context's K = d GEMMs stay on the tile form (FREUD_GEMM_STREAM=0 / debug_flags 86 at ITS creation)
  int eval_prec = 0;            // 0 = the training kernels' arithmetic (bf16 operands, fp32 accumulate), 1 = fp32 end to end
  LastCall last_call = LAST_FWD_BF16;   // what the last forward-like call left behind (no_forward_left, the getters)
  // The one scratch of the file passes (passes.hip: pass_scratch), grow-only: a pass runs start to finish inside its entry point and
  // reads nothing of it afterwards, so each pass carves what it needs from the same bytes -- and finds another pass's leftovers there.
  char* pass_scratch = nullptr;
  // the fp32 evaluation's buffers: each grows to the largest evaluation batch seen; e32_colmax [n_p] is allocated once
  float *e32_x = nullptr, *e32_pre = nullptr, *e32_sel = nullptr, *e32_xhat = nullptr;
  double* e32_part = nullptr;
  int* e32_colmax = nullptr;
  int64_t step = 0;
  int64_t last_M = 0, last_M_p = 0;
  int last_dtype = 0;
  int profile = 0;
  int64_t prof_tick = 0;        // forward/backward calls since sae_profile (level 1 samples every prof_period-th)
  int prof_period = 8;
  EvRing ev[KID_COUNT];
  bool ev_init = false;
  DevMem mem;
};

#pragma GCC visibility push(hidden)
int use_device(const sae_ctx* c);
#pragma GCC visibility pop
#define USE_DEVICE(c)          \
  do {                         \
    int rc_ = use_device(c);   \
    if (rc_) return rc_;       \
  } while (0)

// c->field through the context's owner (op: alloc at creation, grow for a lazy buffer); a failure returns the owner's message
#define CTX_MEM(op, field, bytes, kind)                                                  \
  do {                                                                                   \
    if (!c->mem.op(c->field, (long long)(bytes), (kind), "c->" #field)) return fail(SAE_ERR_HIP, "%s", c->mem.err); \
  } while (0)
#define CTX_ALLOC(field, bytes) CTX_MEM(alloc, field, bytes, DM_DEVICE)

// the getters of the last forward refuse after a file pass (after_search = false: after a statistics pass only)
static int no_forward_left(const sae_ctx* c, bool after_search = true) {
  if (c->last_call == LAST_SEARCH && !after_search) return SAE_OK;
  for (const FilePassKind* k : kFilePasses)
    if (c->last_call == k->leaves)
      return fail(SAE_ERR_STATE, "the last call was %s: it leaves no forward to read (run sae_eval first)", k->left_by);
  return SAE_OK;
}

static void file_pass_end(const FilePassKind& kind, sae_ctx* c) { c->last_call = kind.leaves; }

// the tensors of a bf16 forward (latent rows, top-k indices, 4k buffers, dx_hat, the fp8 operands) are not what the fp32
// evaluation computed: it has its own buffers and leaves those of the last training step as they were
static int no_bf16_forward_left(const sae_ctx* c) {
  if (c->last_call == LAST_FWD_E32)
    return fail(SAE_ERR_STATE, "the last forward was an fp32 evaluation: it leaves no bf16 latent rows, indices or debug tensors (run a bf16 sae_eval first)");
  return SAE_OK;
}

static int dominant_kid(const sae_ctx* c) { return c->topk ? KID_TK_ENC : (c->use_fused_bwd ? KID_BWD_FUSED : KID_DW); }
// Level 1 brackets the dominant kernel and the whole step on every PROF_PERIOD-th step only: an event record is a packet of
// its own in the queue and costs ~6 us of idle GPU between two dependent kernels (kernel trace of the C2 step: 3 records
// per step were 3 % of it), so the timed region of bench.py samples instead of instrumenting every step (sae_profile_period).
static bool ev_on(const sae_ctx* c, int kid) {
  if (c->profile >= 2) return true;
  return c->profile == 1 && (kid == dominant_kid(c) || kid == KID_STEP_TOTAL) && (c->prof_tick % c->prof_period) == 0;
}
static void ev_begin(sae_ctx* c, int kid, hipStream_t s) {
  if (ev_on(c, kid)) {
    EvRing& r = c->ev[kid];
    (void)hipEventRecord(r.beg[r.n % EV_RING], s);   // a failure stays sticky and is reported by the hipGetLastError that ends the call
  }
}
static void ev_end(sae_ctx* c, int kid, hipStream_t s) {
  if (ev_on(c, kid)) {
    EvRing& r = c->ev[kid];
    (void)hipEventRecord(r.end[r.n % EV_RING], s);
    r.n++;
  }
}

// ------------------------------------------------------------------------------------------
// what passes.hip calls of engine.hip (defined there, next to the training paths that use them)
// ------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
void prep_weights_l1(sae_ctx* c, hipStream_t s);
void settle_weights(sae_ctx* c, hipStream_t s);
void refresh_decoder_operand(sae_ctx* c, hipStream_t s);
GemmArgs enc_gemm_args(const sae_ctx* c, const bf16_t* xb, int64_t Mp);
int dispatch_fwd_bwd(sae_ctx* c, const void* x, int64_t M, int x_dtype, void* stream, bool backward);
int decode_l1_latent(sae_ctx* c, const bf16_t* lat, int64_t nbm, int64_t M, float* x_hat, hipStream_t s);
// launch_prep_x<T> and launch_encoder<T> behind plain functions: templates over the activation type in engine.hip, where that fixes
// the place of their kernels in the code object
void launch_prep_x_dtype(sae_ctx* c, const void* x, int x_dtype, int64_t M, int64_t Mp, hipStream_t s);
int launch_encoder_l1(sae_ctx* c, const GemmArgs& g, int64_t M, hipStream_t s);
#pragma GCC visibility pop
