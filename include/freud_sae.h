/*
 * freud_sae.h -- C ABI of libfreud_sae.so, the MI355X (gfx950) SAE training engine.
 *
 * This is the drop-in boundary for the one hot path of ksadov/FREUD that this repository
 * replaces: the body of the training loop in src/scripts/train_sae.py:421-453
 * (forward under autocast -> backward -> clip_grad_norm_ -> optimizer.step) together with
 * the model arithmetic it calls (src/models/l1autoencoder.py:69-95, mse_loss :29-36;
 * src/models/topkautoencoder.py:72-151).  The reference has no FFI of its own (it is pure
 * PyTorch); the entry points below are what a ctypes/cffi binding added to the reference's
 * train() would call instead of `dist_model(activations)`, `loss.backward()`,
 * `clip_grad_norm_` and `optimizer.step()` -- see INTEGRATION.md for that stub.
 *
 * Conventions
 *   - plain C types only; every pointer marked "dev" is a device (HBM) pointer owned by the
 *     caller, every pointer marked "host" is ordinary host memory;
 *   - all calls return 0 on success, a negative code on failure; sae_last_error() then
 *     returns a description (thread-local).  No exceptions cross the boundary;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     enqueued on it; only the calls documented as synchronising wait for the device;
 *   - one host thread drives one context; a context is bound to one GPU;
 *   - parameter layouts are the reference's own (row-major fp32), so checkpoints written from
 *     sae_get_params are bit-layout compatible with the reference's state_dict:
 *       L1   : decoder.weight W[d][n], encoder_bias b[n]            (l1autoencoder.py:56-60)
 *       TopK : encoder.weight We[n][d], encoder.bias be[n], W_dec Wd[n][d], b_dec bd[d]
 *                                                                  (topkautoencoder.py:62-70)
 */
#ifndef FREUD_SAE_H
#define FREUD_SAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sae_ctx sae_ctx;

enum { SAE_VARIANT_L1 = 0, SAE_VARIANT_TOPK = 1 };          /* train_sae.py:352-361 autoencoder_variant */
enum { SAE_OPT_RADAM = 0, SAE_OPT_ADAM = 1 };               /* train_sae.py:374-381 optimizer           */
enum { SAE_DTYPE_F32 = 0, SAE_DTYPE_F16 = 1, SAE_DTYPE_BF16 = 2 }; /* dtype of the activation rows x     */

enum {
  SAE_OK = 0,
  SAE_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
  SAE_ERR_HIP = -2,       /* a HIP runtime call failed                */
  SAE_ERR_STATE = -3      /* call sequence error                      */
};

/* Mirrors the knobs of train() that reach the step (train_sae.py:297-320, 356-381) and the
 * autoencoder_config dataclasses (src/models/config.py:5-28). */
typedef struct sae_config {
  int32_t variant;        /* SAE_VARIANT_*                                               */
  int32_t d_model;        /* activation_size (feat_dim, train_sae.py:65)                 */
  int32_t n_dict;         /* get_n_dict_components(...) (src/utils/models.py:1-6)         */
  int32_t k;              /* TopK only: cfg.k                                            */
  int32_t optimizer;      /* SAE_OPT_*                                                   */
  int32_t device_id;      /* HIP device ordinal                                          */
  int64_t max_rows;       /* largest M = batch_size*T this context will be asked to step */
  /* hyper-parameters are doubles because the reference holds them as Python floats */
  double recon_alpha;     /* L1 only: cfg.recon_alpha                                    */
  double auxk_alpha;      /* TopK only: cfg.auxk_alpha                                   */
  double clip_thresh;     /* clip_grad_norm_ max_norm (train_sae.py:449)                 */
  double weight_decay;    /* RAdam only (train_sae.py:375-377)                           */
  double beta1, beta2;    /* 0.9 / 0.999 (torch defaults the reference relies on)        */
  double eps;             /* 1e-5 RAdam (train_sae.py:376), 1e-8 Adam (torch default)    */
  /* development / test switches (zero in production): */
  int32_t force_generic;  /* 1: generic GEMM path even where a fused d=384 kernel exists (tests cover both)          */
  int32_t debug_flags;    /* kernel timing experiments of bench.py --dbg (65, 66, 70: results become wrong) and A/B    */
                          /* paths that stay correct: 75 = no tile-driven TopK select, 76 = AuxK through the gather   */
                          /* kernels instead of the compacted dead-set GEMMs (tests compare both), 78 = the loss         */
                          /* finalisation as its own kernel between the fused forward and backward (round 2's order),   */
                          /* 79 = the flat optimizer kernel + a separate column-norm pass for L1 (round 2's order),      */
                          /* 80 = L1 with d <= 384: the tiled update + normalize_cast in the next forward instead of the */
                          /* update that also writes the next forward's weight copies (tests compare both to the bit),  */
                          /* 81 = uniform split-K through slabs for the plain weight-gradient GEMM of the generic L1     */
                          /* path (instead of whole tiles straight into the gradient + the tail tiles in K pieces)       */
  int32_t force_gemm128;  /* 1: 128x128 GEMM tiles even where the 256x256 kernel applies (A/B timing, tests)        */
  int32_t topk_dense_backward; /* TopK backward A/B (tests): 0 CSC sparse backward, 1 dense GEMMs + mask, 2 sparse d      */
                          /* pre-activations + dense weight-gradient GEMMs                                            */
  /* model / numerics options: */
  int32_t multi_topk;     /* TopK only: cfg.multi_topk (topkautoencoder.py:134-140, loss term train_sae.py:442)     */
  int32_t precision;      /* SAE_PREC_*: operand type of the L1 encoder / decoder GEMMs                             */
  int32_t reserved[2];    /* must be zero                                                                           */
} sae_config;

/* SAE_PREC_BF16: every GEMM on bf16 operands (the reference's CPU autocast precision; the parity configuration).
 * SAE_PREC_FP8 : BASELINE configs[4] -- encoder and decoder GEMMs on OCP e4m3 operands (x, W and the latent quantised
 *                with per-tensor power-of-two scales), fp32 MFMA accumulation, outputs rounded to bf16 like the bf16 path;
 *                the backward GEMMs and the fp32 master weights / optimizer are unchanged. */
/* SAE_PREC_FP8_BWD: SAE_PREC_FP8 plus the dpre GEMM of the backward (dc = dx_hat W: a third of the backward's FLOPs) on e4m3
 *                operands -- dx_hat quantised per tensor with a power-of-two scale from its own maximum, W as above; the
 *                weight-gradient GEMMs stay bf16.  Beyond BASELINE configs[4] ("fp8 enc/dec"); an option with a stated cost:
 *                raw gradients within 5e-2 (rel-Frobenius) of the bf16 arithmetic (tests/test_fp8_gpu.py). */
enum { SAE_PREC_BF16 = 0, SAE_PREC_FP8 = 1, SAE_PREC_FP8_BWD = 2,
       SAE_PREC_FP32 = 3 /* evaluation only: sae_set_eval_precision */ };

/* Metrics of the most recent sae_forward_backward / sae_eval (all fp32). */
enum {
  SAE_M_LOSS_RECON = 0,   /* L1: out.reconstruction_loss  (l1autoencoder.py:86)  | TopK: fvu            */
  SAE_M_LOSS_L1 = 1,      /* L1: out.l1_loss              (l1autoencoder.py:85)  | TopK: auxk_loss      */
  SAE_M_MSE = 2,          /* the return_mse value         (l1autoencoder.py:93-94, topk :149-150)       */
  SAE_M_GRAD_NORM = 3,    /* total_norm returned by clip_grad_norm_ (valid after sae_optimizer_step)    */
  SAE_M_COUNT = 4,        /* number of unmasked elements (x != -1) entering the masked MSE             */
  SAE_M_DEAD_PCT = 5,     /* TopK: fraction of dead latents (train/dead_pct, train_sae.py:481-485)                      */
  SAE_M_MULTI_TOPK_FVU = 6, /* TopK with cfg.multi_topk: out.multi_topk_fvu (topkautoencoder.py:134-140), else 0      */
  SAE_M_RESERVED7 = 7,
  SAE_NUM_METRICS = 8
};

const char* sae_last_error(void);
int sae_version(void);

/* Create / destroy.  Allocates every HBM buffer the context will ever need (no allocation
 * happens inside the step calls, so they can be captured into a hipGraph). */
int sae_create(const sae_config* cfg, sae_ctx** out);
void sae_destroy(sae_ctx* ctx);

/* Parameters, reference layouts (see top).  `is_device` selects host or device pointers.
 * For L1 pass (W, b, NULL, NULL); for TopK pass (We, be, Wd, bd).  Synchronising.
 * Replaces model.load_state_dict / model.state_dict (train_sae.py:232-251, 265-294).
 * sae_get_params returns what the reference's state_dict holds at the same point of the same call sequence: for L1 the
 * decoder weight is UN-normalised right after an update (train_sae.py:450) and normalised once a forward has run
 * (l1autoencoder.py:71-73 normalises in place on every forward) -- the engine may postpone that in-place division
 * internally, never its visible effect. */
int sae_set_params(sae_ctx* ctx, const float* p0, const float* p1, const float* p2, const float* p3, int is_device);
int sae_get_params(sae_ctx* ctx, float* p0, float* p1, float* p2, float* p3, int is_device);

/* Optimizer moments (exp_avg / exp_avg_sq per parameter, same order and layouts as the
 * parameters) and the step counter.  Replaces optimizer.state_dict()/load_state_dict().
 * Pointers may be NULL to skip a tensor.  Synchronising. */
int sae_set_opt_state(sae_ctx* ctx, int64_t step, const float* const exp_avg[4], const float* const exp_avg_sq[4], int is_device);
int sae_get_opt_state(sae_ctx* ctx, int64_t* step, float* const exp_avg[4], float* const exp_avg_sq[4], int is_device);

/* Forward + backward of one batch of M activation rows x[M][d_model] (dev pointer, row-major,
 * dtype SAE_DTYPE_*).  For L1 this is: renormalise decoder columns in place, encoder GEMM +
 * bias + ReLU, decoder GEMM, masked MSE + L1, and the full backward into the gradient buffer
 * (train_sae.py:429-448).  Asynchronous on `stream`. */
int sae_forward_backward(sae_ctx* ctx, const void* x_dev, int64_t M, int x_dtype, void* stream);

/* The flat fp32 gradient buffer the backward fills and the optimizer consumes:
 * [ grads of every parameter, padded | SAE_NUM_METRICS loss scalars ].  A data-parallel host
 * all-reduces (sum) exactly this buffer between sae_forward_backward and sae_optimizer_step and
 * passes grad_scale = 1/world_size.  Pointer is stable for the life of the context. */
int sae_grad_buffer(sae_ctx* ctx, void** dev_ptr, int64_t* n_floats);

/* Data-parallel overlap (the reference has no data parallelism; this is what a DDP-style wrapper around
 * "loss.backward()", train_sae.py:448, needs).  When a callback is set, sae_forward_backward calls it on the calling
 * thread each time a contiguous range [offset, offset + count) of the gradient buffer has become final in `stream`
 * order (the kernels that produce it have been enqueued), so that the host can start that range's all-reduce on a
 * communication stream while the remaining backward kernels run.  The ranges of one call are disjoint and cover the
 * whole buffer.  The weight-gradient GEMM of the generic L1 path is issued in row chunks for this (one chunk, i.e. no
 * change, without a callback).  fn == NULL removes the callback. */
typedef void (*sae_grad_ready_fn)(void* user, int64_t offset, int64_t count, void* stream);
int sae_set_grad_ready_callback(sae_ctx* ctx, sae_grad_ready_fn fn, void* user);

/* ---- data-parallel exactness and the engine's own communicator (the reference is single-process: train_sae.py never
 * leaves one device; this is the partitioning BASELINE.json's north_star asks for).
 *
 * R ranks x batch B must train like one rank x batch R B.  The gradients are linear in the per-row contributions but the
 * losses NORMALISE by whole-batch quantities -- the number of unmasked entries of the masked MSE and the row count of the
 * L1 mean (l1autoencoder.py:29-36,85); for TopK the total variance around x.mean(0) over ALL files (topkautoencoder.py:
 * 104-106) and the rows of mse -- so those statistics are summed over the ranks FIRST (they depend on the batch only, not
 * on the model) and every rank's backward normalises by the global values; the summed gradients then ARE the whole
 * batch's and no 1/R rescaling follows (grad_scale = 1).
 *
 *   sae_batch_stats   writes this rank's statistics of batch x into the context's statistics buffer (float64, device;
 *                     L1: [unmasked entries, rows]; TopK: [rows, files, sum_b x, sum_b x^2 per (t, feature)]); asynchronous.
 *   sae_stats_buffer  the buffer and the number of doubles the last sae_batch_stats wrote: a host-driven data-parallel
 *                     loop all-reduces (sum) exactly that range before sae_forward_backward.
 *   sae_set_dp_world  world > 0: sae_forward_backward normalises by the statistics buffer (and loss scalars become this
 *                     rank's SHARE of the global losses: they sum over the ranks; dead_pct is pre-divided by world);
 *                     0 (default): by the rank's own batch.
 *
 * sae_dist_unique_id / sae_dist_init give the context its own RCCL communicator (one process per GPU; the unique id made on
 * rank 0 travels to the others by any host channel).  Afterwards sae_forward_backward / sae_step do the whole protocol
 * inside the engine, with no host code in the step: statistics + their all-reduce on a communication stream while the
 * forward runs, every gradient range all-reduced on that stream as soon as its backward kernels are enqueued (i.e. under
 * the remaining backward GEMMs), the compute stream joining before the optimizer.  sae_optimizer_step takes grad_scale 1. */
int sae_batch_stats(sae_ctx* ctx, const void* x_dev, int64_t M, int x_dtype, void* stream);
int sae_stats_buffer(sae_ctx* ctx, void** dev_ptr, int64_t* n_doubles);
int sae_set_dp_world(sae_ctx* ctx, int world);
int sae_dist_unique_id(void* out_host, int64_t capacity_bytes);       /* 128 bytes (ncclUniqueId) */
int sae_dist_init(sae_ctx* ctx, const void* unique_id_host, int64_t id_bytes, int rank, int world);
int sae_dist_world(sae_ctx* ctx);                                      /* 0 without a communicator */
/* Gradient payload of the in-engine all-reduce: SAE_DTYPE_F32 (default: R ranks == one rank exactly, up to summation
 * order) or SAE_DTYPE_BF16 -- the fused d = 384 path then sums a bf16 copy of the parameter gradients (half the bytes of
 * a latency- and link-bound 4.7 MB exchange; the loss scalars stay fp32).  The reference's own CPU autocast rounds these
 * gradients to bf16 as well (the weight-gradient GEMMs' outputs), so this stays inside the parity tolerance; paths
 * other than the fused one keep fp32. */
int sae_dist_set_payload(sae_ctx* ctx, int dtype);

/* ---- peer exchange: the same in-engine protocol with the all-reduces done by the engine's own kernels over hipIpc peer
 * mappings instead of RCCL (on the full xGMI mesh a direct reduce-scatter + all-gather pulls 1/R of
 * the payload over EVERY link at once and needs three flag round trips, where a ring moves the payload over one link per hop
 * -- the 4.7 MB gradient of the d = 384 model is latency-bound).  Up to 8 ranks of one node, one process per GPU.  Like the
 * RCCL form it stands where a DDP wrapper would stand around loss.backward() (train_sae.py:448); results are bit-identical on
 * every rank (each range is summed once, in rank order, by its owner).
 *   sae_p2p_blob_bytes  size of the blob one rank publishes;
 *   sae_p2p_export      allocates the exchange state and writes this rank's blob (hipIpc handles of the gradient buffer, its
 *                       bf16 copy, the statistics buffer and the flag block) to host memory;
 *   sae_p2p_init        takes the blobs of ALL ranks (rank order, gathered over any host channel), maps the peers and runs a
 *                       self-test (collective: every rank must call it): four exchanges of every payload form -- fp32, bf16
 *                       payload, a strided 2-D block, fp64 statistics, the statistics push -- over the SAME addresses with a
 *                       different rank-dependent pattern each time, checked on the device, so that a stale cached peer line, a
 *                       flag overtaking its data or a wrong mapping shows as wrong sums BEFORE the first step; a peer that
 *                       cannot be reached makes it FAIL after min(FREUD_P2P_TIMEOUT_MS, 40 s) (default 120000: a liveness bound of the run's steps)
 *                       instead of hanging.  Afterwards sae_forward_backward / sae_step run the data-parallel protocol
 *                       through the peer exchange; sae_dist_world() == world.  FREUD_P2P_FINEGRAINED=1 (read by sae_create)
 *                       puts the three peer-read buffers in fine-grained memory (a peer never caches their lines non-coherently, so
 *                       correctness does not rest on cache maintenance; measured free for the LOCAL kernels on one GPU at C2 and C4,
 *                       profiles/r04_ab_finegrained_c{2,4}.txt; its cross-device cost is unmeasured).  Default of train() / bench.py
 *                       for WORLD_SIZE > 1.
 *   sae_dist_set_overlap  fused d = 384 path: launch the backward in `nranges` column-tile ranges; each range's gradient is
 *                       exchanged on the communication stream under the next range's backward (needs the peer exchange:
 *                       RCCL sums contiguous buffers only).  1 (default) = one launch, exchanged in line.
 *   sae_dist_check      synchronises and reports a failed exchange (a peer that never arrived: the exchange kernels give up
 *                       after the timeout, POISON the flags they owe their peers so that no rank sails on, and the failure is
 *                       sticky -- the replicas are out of step and the run must stop);
 *   sae_dist_poll       the same report without synchronising (host-mapped mirror of the failure word): free after every step;
 *   sae_dist_audit      snapshot_dev != NULL: from now on every gradient exchange first copies the segments it is about to sum
 *                       (this rank's own contribution) into snapshot_dev (device, same layout and size as sae_grad_buffer).
 *                       The host sums the snapshots over the ranks with an INDEPENDENT carrier (torch.distributed) and
 *                       compares with the exchanged gradient: a wrong-but-identical sum, which no replica comparison can
 *                       see, shows here (freud_amd/dp.py: audit_step).  NULL switches it off.
 *   sae_param_checksum  out_host[4] = order-independent 64-bit checksums of {parameters, first moments, second moments} and the
 *                       step count.  Replicas are bit-identical by construction, so ANY difference between ranks is an
 *                       exchange bug; train() compares them over the host channel at every logging step and before every
 *                       checkpoint (no reference counterpart: train_sae.py:448-450 is single-device).  Synchronises. */
int sae_p2p_blob_bytes(void);
int sae_p2p_export(sae_ctx* ctx, void* blob_out_host, int64_t capacity_bytes);
int sae_p2p_init(sae_ctx* ctx, const void* all_blobs_host, int64_t bytes_per_rank, int rank, int world);
int sae_p2p_leave(sae_ctx* ctx);     /* undo sae_p2p_init (a PEER's self-test failed: every rank falls back together); no-op otherwise */
int sae_dist_set_overlap(sae_ctx* ctx, int nranges);
int sae_dist_check(sae_ctx* ctx);
int sae_dist_poll(sae_ctx* ctx);
int sae_dist_audit(sae_ctx* ctx, float* snapshot_dev);
int sae_grad_layout(sae_ctx* ctx, int64_t out_host[3]);   /* floats of sae_grad_buffer: {parameter gradients, loss scalars, did_fire flags} */
int sae_param_checksum(sae_ctx* ctx, uint64_t out_host[4]);

/* clip_grad_norm_ + Adam/RAdam update with learning rate `lr` (train_sae.py:449-450).
 * grad_scale multiplies every gradient (and the loss scalars) first.  Asynchronous. */
int sae_optimizer_step(sae_ctx* ctx, double lr, double grad_scale, void* stream);

/* TopK only.  dead_feature_threshold: a latent is dead when num_frames_since_fired > threshold
 * (autoencoder_config["dead_feature_threshold"], train_sae.py:436-439).  rows_per_file: T of the
 * [B][T][d] batch -- the FVU denominator is sum (x - x.mean(0))^2 with the mean over the B files
 * (topkautoencoder.py:104); 0 = treat the batch as one file. */
int sae_set_topk_options(sae_ctx* ctx, double dead_feature_threshold, int64_t rows_per_file);

/* TopK, bf16 contexts only (anything else: SAE_ERR_STATE).  The decoder-norm constraint: what the reference model defines as
 * remove_gradient_parallel_to_decoder_directions() and set_decoder_norm_to_unit_norm() (topkautoencoder.py:153-175) and its train()
 * never calls.  Off by default: the rows of W_dec are unit at initialisation only and drift afterwards, as in the reference.
 * While it is on, every sae_optimizer_step (and so sae_step)
 *   1. projects the gradient of W_dec off its rows, g_j <- g_j - (g_j . w_j) w_j (no division by |w_j|^2), in the gradient buffer,
 *      after any data-parallel sum and before the clip norm, which is then formed from the projected buffer;
 *   2. clips and updates every parameter exactly as without the constraint (the Adam moments are neither projected nor rescaled);
 *   3. renormalises the rows, w_j <- w_j / (||w_j||_2 + eps) with eps = 2^-23, in the fp32 master; the bf16 copy the next forward
 *      multiplies by is taken from the renormalised rows.  A zero row, and the padding, stay exactly zero.
 * Switching it on (SAE_DEC_CONSTRAINT_ON), and sae_set_params while it is on, run step 3 once (synchronous), so that the rows are unit
 * before the first projection: loading weights that were trained without the constraint changes the model at step 0.  Step 3 is not
 * idempotent in fp32 (w / (||w|| + eps) of a row it produced moves most rows by an ulp again), so a run that resumes ITS OWN
 * checkpoint -- rows that step 3 already left -- loads the parameters first and then switches the constraint on with
 * SAE_DEC_CONSTRAINT_ON_KEEP_ROWS, which skips the renorm at the switch: the resumed run then continues bit for bit.  0 switches it
 * off; any other value: SAE_ERR_INVALID.  sae_get_decoder_constraint: 1 / 0. */
enum { SAE_DEC_CONSTRAINT_ON = 1, SAE_DEC_CONSTRAINT_ON_KEEP_ROWS = 2 };
int sae_set_decoder_constraint(sae_ctx* ctx, int on);
int sae_get_decoder_constraint(sae_ctx* ctx);

/* TopK bookkeeping state num_frames_since_fired[n_dict] (int64, train_sae.py:412-415,443-446).  The reference keeps
 * it only in the live process and restarts it from zero on resume (train_sae.py:396-415 never saves it); these two
 * calls let the host persist it next to the checkpoint.  Host buffers of n_dict int64.
 * Synchronous.  SAE_ERR_INVALID on an L1 context. */
int sae_get_topk_state(sae_ctx* ctx, int64_t* num_frames_since_fired_host, int64_t n);
int sae_set_topk_state(sae_ctx* ctx, const int64_t* num_frames_since_fired_host, int64_t n);

/* Convenience: sae_forward_backward + sae_optimizer_step(lr, 1). */
int sae_step(sae_ctx* ctx, const void* x_dev, int64_t M, int x_dtype, double lr, void* stream);

/* Forward only (no parameter update except the in-place column renormalisation the reference's
 * encode() also performs in eval).  Fills the metrics.  Asynchronous. */
int sae_eval(sae_ctx* ctx, const void* x_dev, int64_t M, int x_dtype, void* stream);

/* ---- inference (the SAE inside FlyActivationDataLoader.__iter__, dataset/activations.py:
 * 96-108, and manipulate_latent, utils/activations.py:243-268).  sae_eval is encode(): afterwards
 *   sae_latent_buffer  -> the latent of the last forward, bf16 [M][*row_stride] on the device (columns [0, n_dict)):
 *                         L1: c = relu(x W + b) (l1autoencoder.py:69-75); TopK: the top-k activations scattered into a
 *                         dense row, zeros elsewhere (topkautoencoder.py:79-85 + eager_decode's buffer, :15-18);
 *   sae_topk_indices   -> TopK only: int32 [M][k] top_indices of the last forward (tie order: lowest column first).
 * Pointers are owned by the context and overwritten by the next forward.
 * sae_decode: x_hat[M][d_model] (fp32, device, dense) = latent . W^T (L1 decode(), l1autoencoder.py:77-78, with the
 * CURRENT weights, no renormalisation) or latent_dense . W_dec + b_dec (TopK decode(), topkautoencoder.py:87-91).
 * latent: device, row-major, `ld` elements per row, SAE_DTYPE_F32 or SAE_DTYPE_BF16; bf16 MFMA arithmetic like the
 * train step.  M <= max_rows.  Asynchronous on `stream`. */
int sae_latent_buffer(sae_ctx* ctx, void** dev_ptr, int64_t* row_stride);
int sae_topk_indices(sae_ctx* ctx, void** dev_ptr, int* k);
int sae_decode(sae_ctx* ctx, const void* latent_dev, int latent_dtype, int64_t ld, int64_t M, float* x_hat_dev, void* stream);
/* TopK with cfg.multi_topk only: the second selection of the last forward -- the top 4k activations scattered into a
 * dense bf16 row [M][*row_stride] and their int32 indices [M][*k4].  TopKAutoEncoder.forward() returns THESE as
 * out.encoded / out.sae_out when multi_topk is set (topkautoencoder.py:134-147 re-binds the names); encode() keeps k. */
int sae_multi_topk_buffers(sae_ctx* ctx, void** dense_dev, int64_t* row_stride, void** idx_dev, int* k4);

/* validate() without per-file host round trips (train_sae.py:168-190 reads four .item()s per file): sae_eval of one file,
 * then its SAE_NUM_METRICS loss scalars go to metrics_out_dev[8] and -- unless colmax_out_dev is NULL -- its per-feature
 * maxima of |latent| (train_sae.py:176-178) to colmax_out_dev[n_dict]; both are CALLER-OWNED device rows (one pair per
 * file), so a whole validation folder is enqueued without a single synchronisation and read back once.  Asynchronous. */
int sae_eval_into(sae_ctx* ctx, const void* x_dev, int64_t M, int x_dtype, float* metrics_out_dev, float* colmax_out_dev, void* stream);

/* Arithmetic of sae_eval / sae_eval_into.  SAE_PREC_BF16 (default): the training kernels' -- bf16 operands, fp32 accumulation, i.e.
 * CPU autocast's.  SAE_PREC_FP32: fp32 end to end, which is what the reference's validate() computes on device='cpu'
 * (train_sae.py:162-166: nullcontext() instead of autocast; L1AutoEncoder.forward l1autoencoder.py:69-95, TopKAutoEncoder.forward
 * topkautoencoder.py:93-151 without a dead mask) and what its bestval.pth selection (train_sae.py:585-595) rests on: fp32 matrix
 * instructions, fp32 bias / ReLU / top-k (ties: lowest column first), loss sums in double.  The in-place column normalisation of
 * the L1 weights happens first, exactly as in every other forward.  Training steps are not affected.  Any SAE_PREC_* other than
 * these two: SAE_ERR_INVALID.
 * The fp32 forward obeys M <= max_rows like every other forward and works in buffers of its own: it leaves no bf16 latent rows.
 * While it is the last forward, sae_latent_buffer, sae_topk_indices, sae_multi_topk_buffers and sae_debug_read(0, 1, 3, 8, 9, 14)
 * return SAE_ERR_STATE (run a bf16 sae_eval to read those); sae_read_metrics and sae_latent_colmax answer for the fp32 forward,
 * and sae_debug_read(2) (the gradients of the last training forward), sae_get_params, sae_get_opt_state, sae_get_topk_state and
 * sae_decode stay valid. */
int sae_set_eval_precision(sae_ctx* ctx, int precision);

/* Copy the SAE_NUM_METRICS scalars to host.  Synchronises `stream`. */
int sae_read_metrics(sae_ctx* ctx, float out_host[SAE_NUM_METRICS], void* stream);

/* Per-dictionary-feature maximum of |latent| over the M rows of the last forward
 * (torch.max(torch.abs(latent), dim=0) in validate(), train_sae.py:176-178) -> out_host[n_dict].
 * Synchronises `stream`. */
int sae_latent_colmax(sae_ctx* ctx, float* out_host, int64_t capacity_floats, void* stream);

/* ---- Feature search: the reference's top_activations (utils/activations.py:61-132, served by gui_server.py:91-99) for EVERY
 * latent in one pass over the data, instead of one pass over a collected SAE-activation dataset per latent.
 *
 * A search is three steps per batch of files, all asynchronous on `stream`, all buffers CALLER-OWNED device memory:
 *   1. file keys: per (file, latent) one uint64 (freud_amd/csrc/search_keys.h): ord(value) << 32 | (0xFFFFFFFF - frame), the
 *      maximum of the file's trimmed series and its first frame -- trimmed_activation.max() / .argmax() (activations.py:104-124);
 *   2. sae_search_merge: the batch's keys merged into a running per-latent top-N table -- the reference's filter, append, stable
 *      sort by value and truncation to n_files (activations.py:118-129): order (value descending, file ascending);
 *   3. optionally sae_search_file_values: the per-file values of chosen latents (return_max_per_file, activations.py:111-117).
 * The host reads the table back once at the end (freud_amd/feature_search.py).
 *
 * A batch holds n_files files of rows_per_file (T) rows each, row-major [n_files][T][d].  lengths_dev (int32 [n_files], or NULL
 * = T): only the first min(length, T) frames of a file count (trim_activation, activations.py:19-29); a length below 1 is treated
 * as 1 (the Python layer rejects it: the reference fails on max() of an empty series).  Shape checks fail before anything is
 * enqueued. */
enum { SAE_SEARCH_ABS = 1, SAE_SEARCH_MIN = 2, SAE_SEARCH_MAX = 4, SAE_SEARCH_UNFUSED = 8 };
#define SAE_SEARCH_MAX_TOP 4096

/* File keys of the context's SAE latents, file_keys_dev[n_files][n_dict].  L1: c = relu(x W + b) of sae_eval (bf16 operands, the
 * in-place column renormalisation of encode() included), reduced in the encoder GEMM's epilogue -- the latent is never written
 * (SAE_SEARCH_UNFUSED: stored and reduced by a second kernel; also taken where the streaming GEMM does not apply -- it needs an even
 * number of 128-row blocks, so a max_rows with room for round_up(n_files * rows_per_file, 256) rows, and T <= 65535).  TopK: the eval
 * forward, then its top-k selection scattered into the keys; frames where a latent is not selected count as 0
 * (activation_tensor_from_indexed, activations.py:41-58), so a latent that never fires has value 0 at frame 0.  Both latents are
 * >= 0, so the abs mode of the merge equals the plain one for them.  n_files * rows_per_file <= max_rows; fp8 contexts:
 * SAE_ERR_INVALID.  Training state (parameters, moments, num_frames_since_fired) is untouched; afterwards sae_latent_buffer,
 * sae_topk_indices, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next
 * sae_eval / step (sae_decode reads the caller's latent and is unaffected). */
int sae_search_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                     int flags, uint64_t* file_keys_dev, void* stream);

/* Raw mode (no SAE: the README's single-neuron search): file keys of x itself, file_keys_dev[n_files][d], fp32 / fp16 / bf16 values
 * as they are.  absolute != 0 (activations.py:106-113): the keys rank |a| (first frame of max |a|), and aux_dev[n_files][d] holds
 * the signed value at that frame (high 32 bits, fp32) and the frame of the SIGNED maximum (low 32 bits) -- the time the reference
 * returns even in abs mode (activations.py:120-121).  Runs on the current device. */
int sae_search_raw_files(const void* x_dev, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths_dev,
                         int absolute, uint64_t* file_keys_dev, uint64_t* aux_dev, void* stream);

/* Merge the keys of files [file0, file0 + n_files) (file_keys_dev[n_files][ncols], aux_dev of a raw abs search or NULL) into the
 * top-N table top_keys_dev / top_frames_dev, both [n_top][ncols] (latent-minor).  Table entries are rank keys
 * ord(value) << 32 | (0xFFFFFFFF - file) (search_keys.h; 0 = empty: zero the table before the first batch) and frames.  flags:
 * SAE_SEARCH_ABS ranks |value| and filters the signed value, SAE_SEARCH_MIN / _MAX apply min_val <= value <= max_val (in double,
 * as the reference compares .item() floats).  1 <= n_top <= SAE_SEARCH_MAX_TOP; n_top may exceed the number of files.  One
 * thread per latent, files in order: deterministic.  Runs on the current device. */
int sae_search_merge(const uint64_t* file_keys_dev, const uint64_t* aux_dev, int64_t n_files, int64_t ncols, int64_t file0, int n_top,
                     int flags, double min_val, double max_val, uint64_t* top_keys_dev, int32_t* top_frames_dev, void* stream);

/* return_max_per_file: out_dev[l * out_stride + file0 + f] = the per-file value of latent latents_dev[l] (the signed value in abs
 * mode) for the files of this batch.  out_stride >= file0 + n_files.  Runs on the current device. */
int sae_search_file_values(const uint64_t* file_keys_dev, const uint64_t* aux_dev, int64_t n_files, int64_t ncols, int flags,
                           const int32_t* latents_dev, int64_t n_latents, int64_t file0, int64_t out_stride, float* out_dev, void* stream);

/* ---- File features: the reference's top_activations_for_audio (utils/activations.py:135-209, served as /top_features) for
 * every file of a batch at once -- which latents describe a file.  Input: the file keys file_keys_dev[n_files][ncols] exactly as
 * sae_search_files / sae_search_raw_files (absolute = 0) leave them.  Output per file, best first: top_latents_dev[n_files][n_top]
 * (int32, -1 = empty slot) and top_keys_dev[n_files][n_top] (the latents' file keys, 0 = empty slot: value and first frame of the
 * maximum, freud_amd/csrc/search_keys.h).
 *
 * Order: file key descending -- value descending, then the earlier first frame of the maximum, as the reference's stable sort over
 * the frames in order gives -- and for equal keys the lower latent index (the reference leaves that case to torch.topk's
 * unspecified order within a frame).  Zero rule: with SAE_FILE_TOP_POSITIVE only latents whose value is > 0 are reported (magnitude
 * bits: a -0.0 is not positive); the reference pads a short answer of an SAE with zero-valued latents that torch.topk picks among
 * ties.  Without the flag (raw mode) signed values are reported as they are, zero and negative included.  n_top may exceed ncols or
 * the number of reportable latents: the remaining slots are empty.
 *
 * 1 <= n_top <= SAE_FILE_TOP_MAX, n_files >= 1, 1 <= ncols <= 2^24, non-null pointers: otherwise SAE_ERR_INVALID before anything
 * is enqueued.  Caller-owned buffers, asynchronous on `stream`, runs on the current device, needs no context.  Exact and
 * deterministic: two runs give bitwise identical tables. */
enum { SAE_FILE_TOP_POSITIVE = 1 };      /* report only values > 0 (SAE latents) */
#define SAE_FILE_TOP_MAX 1024
int sae_file_top_features(const uint64_t* file_keys_dev, int64_t n_files, int64_t ncols, int n_top, int flags,
                          int32_t* top_latents_dev, uint64_t* top_keys_dev, void* stream);

/* ---- Feature statistics: how sparse the dictionary is on real data, in one pass over the data.  The SAE activations are never
 * collected or written.
 *
 * Semantics.  Files are the rows [f T, f T + T) of a batch (row-major [n_files][T][d]).  With lengths_dev (int32 [n_files]) only
 * the first min(length, T) frames of file f count (a length below 1 is treated as 1; the Python layer rejects it).  Without it
 * all T frames count.  Per frame and latent j, the latent a_j is exactly the value freud_amd.models encode() returns:
 *   L1:   the bf16 latent c = relu(x W + b) of the training kernels (the value sae_eval leaves in sae_latent_buffer);
 *   TopK: the scatter of the top-k selection (top_acts at top_indices), 0 elsewhere; a multi_topk context uses its k selection.
 * a_j is ACTIVE iff a_j > 0; a bf16 -0.0 is not active (the magnitude bits are compared).
 *
 * Output: a caller-owned device block of SAE_STATS_BYTES(n) bytes (8-byte aligned; n = n_dict) that holds running totals.  Zero it
 * before the first batch; every call adds one batch.  Byte offsets:
 *   SAE_STATS_N_FRAMES    int64                frames counted
 *   SAE_STATS_FIRE_COUNT  int64   [n]          frames where latent j is active
 *   SAE_STATS_ACT_SUM     float64 [n]          sum of a_j over the counted frames
 *   SAE_STATS_ACT_SQ_SUM  float64 [n]          sum of a_j^2
 *   SAE_STATS_L0_HIST     int64   [n + 1]      number of frames with exactly i active latents
 *   SAE_STATS_ACT_MAX     float32 [n]          max of a_j (0 if never active)
 * Invariants: sum(l0_hist) == n_frames, sum_i i * l0_hist[i] == sum(fire_count).
 *
 * Results are deterministic: two runs over the same batches give bitwise identical blocks.  Float sums are fp32 partials per
 * block of rows (plain stores), added in a fixed order into the fp64 totals; counts and maxima are integers. */
#define SAE_STATS_N_FRAMES(n) ((int64_t)0)
#define SAE_STATS_FIRE_COUNT(n) ((int64_t)8)
#define SAE_STATS_ACT_SUM(n) ((int64_t)8 + 8 * (int64_t)(n))
#define SAE_STATS_ACT_SQ_SUM(n) ((int64_t)8 + 16 * (int64_t)(n))
#define SAE_STATS_L0_HIST(n) ((int64_t)8 + 24 * (int64_t)(n))
#define SAE_STATS_ACT_MAX(n) ((int64_t)16 + 32 * (int64_t)(n))
#define SAE_STATS_BYTES(n) ((int64_t)16 + 36 * (int64_t)(n))
enum { SAE_STATS_UNFUSED = 1 };

/* Add the statistics of one batch (x_dev [n_files][rows_per_file][d], x_dtype) to stats_dev.  L1: the encoder GEMM reduces the
 * latent in its epilogue and never writes it; where the streaming GEMM does not apply (it needs an even number of 128-row blocks,
 * so a max_rows with room for round_up(n_files * rows_per_file, 256) rows), or with flags = SAE_STATS_UNFUSED, the latent is
 * stored and reduced by separate kernels.  TopK: the eval forward, then the statistics of its selection.  n_files * rows_per_file
 * <= max_rows; fp8 contexts: SAE_ERR_INVALID.  Shape and argument checks fail before anything is enqueued.  Asynchronous on
 * `stream`; the first call allocates the context's scratch (about 16 bytes per 128 rows and latent, plus one byte per row and 64
 * latents for L1).  Training state (parameters, moments, num_frames_since_fired) is untouched; afterwards sae_latent_buffer,
 * sae_topk_indices, sae_decode, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the
 * next sae_eval / step. */
int sae_stats_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                    int flags, void* stats_dev, void* stream);

/* ---- Feature co-activation: which latents fire together.  C[i][j] = the number of counted frames on which latents i and j are both
 * active, for every pair, in one pass over the data; then per latent the neighbours that share the most frames with it.
 *
 * Semantics.  Frames count exactly as in sae_stats_files (lengths_dev, the first min(length, T) frames of a file), and "active" is
 * its rule: the value encode() returns is > 0 (magnitude bits: a -0.0 is not active; a selected zero of a TopK row is not active).
 * C is symmetric, C[i][i] is the fire_count of the statistics.  Counts are int32: THE CALLER GUARANTEES that at most 2^31 - 1 frames
 * are counted into one table (freud_amd/coactivation.py refuses a pass whose files x T exceeds that).
 *
 * sae_coact_files adds one batch to counts_dev [n_dict][n_dict] (int32, row-major, caller-owned, zeroed before the first batch); after
 * every call the table is the full symmetric matrix.  The batch's activity mask is packed as int8 into context scratch (allocated by
 * the first call: n_dict rounded up to 128, times max_rows rounded up to 128, bytes) and the table is updated on the i8 MFMA, upper
 * triangle of tiles only, mirrored on the way out.  Sums are integers: two runs give bitwise identical tables.  flags must be 0.
 * n_files * rows_per_file <= max_rows; fp8 contexts: SAE_ERR_INVALID.  Shape and argument checks fail before anything is enqueued.
 * Asynchronous on `stream`.  Training state is untouched; afterwards sae_latent_buffer, sae_topk_indices, sae_decode,
 * sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next sae_eval / step. */
int sae_coact_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                    int flags, int32_t* counts_dev, void* stream);

/* Neighbour keys of the rows [row0, row0 + n_rows) of a count table counts_dev [n][n]: keys_dev[n_rows][n] =
 * ord(score) << 32 | C[i][j] (freud_amd/csrc/coact.h), 0 for j == i and for C[i][j] == 0.  score = one fp64 division converted once
 * to fp32: SAE_COACT_JACCARD C[i][j] / (C[i][i] + C[j][j] - C[i][j]); SAE_COACT_COND C[i][j] / C[i][i]; SAE_COACT_COUNT C[i][j].
 * sae_file_top_features(keys_dev, n_rows, n, n_top, SAE_FILE_TOP_POSITIVE, ...) then gives each latent's neighbours in the order
 * score descending, then the larger count, then the lower partner index; the latent itself and partners it never fires with are not
 * reported.  Null pointers, n outside [1, 2^24], an empty or out-of-range row block, an unknown measure: SAE_ERR_INVALID.  Needs no
 * context, runs on the current device, asynchronous on `stream`, deterministic. */
enum { SAE_COACT_JACCARD = 0, SAE_COACT_COND = 1, SAE_COACT_COUNT = 2 };
int sae_coact_neighbor_keys(const int32_t* counts_dev, int64_t n, int64_t row0, int64_t n_rows, int measure, uint64_t* keys_dev,
                            void* stream);

/* ---- Feature labels: which latents detect which labels of the data (an ESC-50 class, a speaker, the phoneme of a 20 ms frame), in
 * one pass over the files.  The reference has no counterpart: its README reaches such statements by listening.
 *
 * Semantics.  Frames count exactly as in sae_stats_files / sae_coact_files (lengths_dev: the first min(length, T) frames of a file;
 * without, all T), and "active" is their rule: the value encode() returns is > 0 (magnitude bits: a -0.0 and a selected zero of a
 * TopK row are not active; a multi_topk context uses its k selection).  Every frame carries up to n_slots class ids in
 * [0, n_classes) in labels_dev [n_files * rows_per_file][n_slots] (int32); -1 is an empty slot, the ids of one frame are distinct,
 * any other id outside the range is ignored.  1 <= n_slots <= SAE_LABEL_MAX_SLOTS, 1 <= n_classes <= SAE_LABEL_MAX_CLASSES.
 *
 * A[l][j] = counts_dev [n_classes + 1][n_dict] (int32, row-major) is the number of counted frames that carry label l and on which
 * latent j is active; row n_classes is the "any" row, the number of counted frames on which j is active (the fire_count of the
 * statistics, the diagonal of the co-activation table).  label_count_dev [n_classes + 1] (int64) is the number of counted frames
 * that carry l; entry n_classes is the number of counted frames.  Both are running totals, caller-owned, zeroed before the first
 * batch.  Counts are int32: THE CALLER GUARANTEES that at most 2^31 - 1 frames are counted into one table
 * (freud_amd/feature_labels.py refuses a pass whose files x T exceeds that).
 *
 * sae_label_files adds one batch.  The activity mask is packed exactly as by sae_coact_files, into the same context scratch; the
 * labels are packed as int8 into scratch of their own (allocated by the first call, grown when a later call brings more classes:
 * n_classes + 1 rounded up to 128, times max_rows rounded up to 128, bytes) and A += labels x mask runs on the i8 MFMA.  Sums are
 * integers: two runs give bitwise identical tables.  flags must be 0.  n_files * rows_per_file <= max_rows; fp8 contexts:
 * SAE_ERR_INVALID.  Null pointers, n_slots or n_classes out of range, unknown flags and bad shapes fail before anything is
 * enqueued.  Asynchronous on `stream`.  Training state is untouched; afterwards sae_latent_buffer, sae_topk_indices, sae_decode,
 * sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next sae_eval / step. */
#define SAE_LABEL_MAX_CLASSES 4096
#define SAE_LABEL_MAX_SLOTS 16
int sae_label_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                    const int32_t* labels_dev, int n_slots, int n_classes, int flags, int32_t* counts_dev, int64_t* label_count_dev,
                    void* stream);

/* Keys of a block of rows [row0, row0 + n_rows) of a label table (counts_dev, label_count_dev as sae_label_files leaves them; n =
 * n_dict).  by_latent = 0: the rows are labels, keys_dev [n_rows][n] -- a label's latents; by_latent = 1: the rows are latents,
 * keys_dev [n_rows][n_classes] -- a latent's labels (the "any" row is never a partner).  A key is ord(score) << 32 | A[l][j]
 * (freud_amd/csrc/labels.h), 0 where A[l][j] == 0.  score = ONE fp64 division converted once to fp32, with fire[j] =
 * A[n_classes][j]: SAE_LABEL_F1 2 A / (fire[j] + label_count[l]); SAE_LABEL_PRECISION A / fire[j]; SAE_LABEL_RECALL
 * A / label_count[l]; SAE_LABEL_COUNT A.  sae_file_top_features(keys_dev, n_rows, columns, n_top, SAE_FILE_TOP_POSITIVE, ...) then
 * gives each row's partners in the order score descending, then the larger count, then the lower index.  Null pointers, n_classes
 * or n out of range, an empty or out-of-range row block, an unknown measure or orientation: SAE_ERR_INVALID.  Needs no context,
 * runs on the current device, asynchronous on `stream`, deterministic. */
enum { SAE_LABEL_F1 = 0, SAE_LABEL_PRECISION = 1, SAE_LABEL_RECALL = 2, SAE_LABEL_COUNT = 3 };
int sae_label_keys(const int32_t* counts_dev, const int64_t* label_count_dev, int64_t n_classes, int64_t n, int measure, int by_latent,
                   int64_t row0, int64_t n_rows, uint64_t* keys_dev, void* stream);

/* ---- Cross-activation: how often latent i of dictionary A and latent j of dictionary B are active a fixed number of frames apart --
 * two dictionaries compared as functions of the data (other layers, other widths, L1 against TopK), and what follows what in time.
 *
 * Semantics (freud_amd/csrc/cross.h states the rule once).  A (n_a latents) and B (n_b latents) see the same files; file f has len_f
 * counted frames, exactly as in sae_stats_files; "active" is its rule.  For a lag l >= 0 the table X_l [(n_a + 1)][(n_b + 1)] (int32,
 * row-major, caller-owned, zeroed before the first batch) holds
 *     X_l[i][j]     = #{ (f, t) : t + l < len_f, A_i active at (f, t), B_j active at (f, t + l) }
 *     X_l[i][n_b]   = fire_a_l[i] = #{ (f, t) : t + l < len_f, A_i active at (f, t) }
 *     X_l[n_a][j]   = fire_b_l[j] = #{ (f, t) : t + l < len_f, B_j active at (f, t + l) }
 *     X_l[n_a][n_b] = n_pairs_l   = sum_f max(len_f - l, 0)
 * A pair of frames never crosses a file and an uncounted frame is on neither side.  A negative lag is the table of (B, A).  With
 * A = B and l = 0 the interior is the table of sae_coact_files.  Counts are int32: THE CALLER GUARANTEES that at most 2^31 - 1 frames
 * go into one table.
 *
 * A mask is int8 [n_dict + 1 rounded up to 128][rows rounded up to 128], latent-major, frames contiguous: sae_cross_mask_bytes bytes
 * (0 for n_dict outside [1, 2^21] or rows outside [1, 65535 * 128]).  Row n_dict is the margin row.  The SOURCE mask holds at
 * position (f, t) whether the latent is active on the counted frame (f, t), margin: (f, t) is counted.  The TARGET mask at lag l
 * holds whether the latent is active at (f, t + l) and t + l < len_f, margin: t + l < len_f.  Every padding byte is zero.
 *
 * sae_cross_mask_files encodes one batch once, as sae_coact_files does, and writes into masks_dev, one after the other, the source
 * mask (sides & SAE_CROSS_SOURCE) and the n_lags target masks in the order of lags_host (sides & SAE_CROSS_TARGET; a host array of
 * 1 to SAE_CROSS_MAX_LAGS distinct lags in [0, SAE_CROSS_MAX_LAG); without the bit n_lags must be 0).  masks_dev: caller-owned,
 * 16-byte aligned, masks_bytes >= the masks asked for, each of sae_cross_mask_bytes(n_dict, n_files * rows_per_file).
 * n_files * rows_per_file <= max_rows; fp8 contexts: SAE_ERR_INVALID.  Null pointers, bad sides, lags or shapes and a short buffer
 * fail before anything is enqueued.  Asynchronous on `stream`.  Training state is untouched; afterwards sae_latent_buffer,
 * sae_topk_indices, sae_decode, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next
 * sae_eval / step. */
#define SAE_CROSS_MAX_LAG 32768
#define SAE_CROSS_MAX_LAGS 8
enum { SAE_CROSS_SOURCE = 1, SAE_CROSS_TARGET = 2 };
int64_t sae_cross_mask_bytes(int64_t n_dict, int64_t rows);
int sae_cross_mask_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                         int sides, const int32_t* lags_host, int n_lags, void* masks_dev, int64_t masks_bytes, void* stream);

/* counts_dev [(n_a + 1)][(n_b + 1)] += mask_a x mask_b^T for two masks of the same `rows` (a source mask of A, a target mask of B):
 * one batch, one lag.  The i8 MFMA over the rectangle of 128 x 128 tiles, every tile computed; the K split of sae_coact_files
 * (integer atomic adds when split, plain read-modify-write otherwise): two runs give bitwise identical tables.  Null pointers,
 * dimensions outside those of sae_cross_mask_bytes, misaligned pointers (masks 16 bytes, table 4): SAE_ERR_INVALID.  Needs no
 * context, runs on the current device, asynchronous on `stream`. */
int sae_cross_update(const void* mask_a_dev, int64_t n_a, const void* mask_b_dev, int64_t n_b, int64_t rows, int32_t* counts_dev,
                     void* stream);

/* Keys of the rows [row0, row0 + n_rows) of a table X.  by_b = 0: the rows are latents of A, keys_dev [n_rows][n_b]; by_b = 1: the
 * rows are latents of B, keys_dev [n_rows][n_a].  A key is ord(score) << 32 | X[i][j] (freud_amd/csrc/cross.h), 0 where X[i][j] == 0
 * and, with exclude_diagonal = 1 (A and B are one dictionary and l = 0), where i == j.  score = one fixed fp64 expression converted
 * once to fp32, the margins read from the table: SAE_CROSS_JACCARD X / (fire_a + fire_b - X); SAE_CROSS_COND X / fire_a (by_b = 0:
 * P(B_j at t + l | A_i at t)) or X / fire_b (by_b = 1); SAE_CROSS_LIFT (X / fire_a) / (fire_b / n_pairs); SAE_CROSS_COUNT X.
 * sae_file_top_features(keys_dev, n_rows, columns, n_top, SAE_FILE_TOP_POSITIVE, ...) then gives each row's partners in the order
 * score descending, then the larger count, then the lower index.  Null pointers, n_a or n_b outside [1, 2^21], an empty or
 * out-of-range row block, an unknown measure, orientation or flag: SAE_ERR_INVALID.  Needs no context, runs on the current device,
 * asynchronous on `stream`, deterministic. */
enum { SAE_CROSS_JACCARD = 0, SAE_CROSS_COND = 1, SAE_CROSS_LIFT = 2, SAE_CROSS_COUNT = 3 };
int sae_cross_keys(const int32_t* counts_dev, int64_t n_a, int64_t n_b, int measure, int by_b, int exclude_diagonal, int64_t row0,
                   int64_t n_rows, uint64_t* keys_dev, void* stream);

/* ---- Activation histograms: how strongly every latent fires -- per latent the histogram of its value over the counted frames, the
 * histogram of every file's maximum (the reference GUI's "Histogram of Max Activation Values per File", for all latents at once)
 * and, for a few chosen latents, the frame histogram split by the frames' labels (the reference's plot_polysemantic.py).
 *
 * Semantics.  Frames count exactly as in sae_stats_files (lengths_dev: the first min(length, T) frames of a file; without, all T).
 * The value binned is the one encode() returns, on its bf16 bit pattern (freud_amd/csrc/hist_bins.h), mag = bits & 0x7FFF.  With
 * L = lo_exp (>= -126), O = octaves (>= 1, L + O <= 128), s = sub_bits (0..3), P = 2^s and O P <= 128, there are NB = O P + 3 bins:
 * bin 0: mag == 0 (inactive: a -0.0 and a selected zero of a TopK row as well; a multi_topk context uses its k selection); bin 1:
 * 0 < a < 2^L; bin 2 + i, 0 <= i < O P: i = (mag >> (7 - s)) - ((L + 127) << s), lower edge 2^(L + i / P) (1 + (i % P) / P); bin
 * NB - 1: a >= 2^(L + O), Inf and NaN patterns included.  Every edge is a bf16 value: the counts are exact.
 *
 * sae_hist_files adds one batch to frame_hist_dev [n_dict][NB] (per latent and bin, the counted frames), file_max_hist_dev
 * [n_dict][NB] (per latent, one count per file in the bin of the file's maximum over its counted frames; all inactive: bin 0) and
 * n_frames_dev [1].  With n_sel > 0 (at most SAE_HIST_MAX_SEL) it also adds to label_hist_dev [n_sel][n_classes + 1][NB] -- for
 * l < n_classes the counted frames that carry label l and on which latent sel_latents_dev[s] falls in the bin, row n_classes the
 * "any" row: frame_hist of that latent -- and to label_count_dev [n_classes + 1], both with the labels_dev layout and rules of
 * sae_label_files; a chosen latent outside [0, n_dict) counts nowhere.  n_sel = 0: the five label arguments are ignored.  All
 * arrays are int64 running totals, caller-owned, zeroed before the first batch and passed TOGETHER to every call of one pass (bin
 * 0 of a TopK context and the "any" rows are derived from the totals).  Sums are integers: two runs give bitwise identical arrays.
 *
 * An L1 context bins the stored latent of its ordinary encoder; a TopK context its selection, with scratch for the file maxima
 * (n_files x n_dict words, allocated by the first call and grown when a later one brings more files).  flags must be 0.  n_files *
 * rows_per_file <= max_rows; fp8 contexts: SAE_ERR_INVALID.  A bad spec, n_sel outside [0, SAE_HIST_MAX_SEL], label pointers
 * missing while n_sel > 0, n_slots or n_classes out of range, null or misaligned arrays, unknown flags and bad shapes fail before
 * anything is enqueued.  Asynchronous on `stream`.  Training state is untouched; afterwards sae_latent_buffer, sae_topk_indices,
 * sae_decode, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next sae_eval / step. */
#define SAE_HIST_MAX_BINS 131
#define SAE_HIST_MAX_SEL 64
int sae_hist_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                   int lo_exp, int octaves, int sub_bits, int flags, int64_t* frame_hist_dev, int64_t* file_max_hist_dev,
                   int64_t* n_frames_dev, const int32_t* labels_dev, int n_slots, int n_classes, const int32_t* sel_latents_dev, int n_sel,
                   int64_t* label_hist_dev, int64_t* label_count_dev, void* stream);

/* ---- Feature timing: for HOW LONG every latent fires -- per latent the histogram of its run durations, the histogram of the gaps
 * between consecutive runs of a file, and six totals.  A frame is one 20 ms step of Whisper's 30 s window; every other pass treats
 * the frames of a file as an unordered bag, this one carries state from frame t to frame t + 1.
 *
 * Semantics (freud_amd/csrc/timing_bins.h).  Frames count exactly as in sae_stats_files (lengths_dev: the first min(length, T)
 * frames of a file; without, all T); runs never cross a file boundary and never see an uncounted frame.  A frame is ACTIVE iff
 * mag > threshold_bits, mag = bits & 0x7FFF of the bf16 value encode() returns: threshold_bits = 0 is the rule of the statistics
 * (a -0.0 and a selected zero of a TopK row are inactive); a multi_topk context uses its k selection.  RUNS with a bridge g =
 * `bridge` (0 <= g <= SAE_TIMING_MAX_BRIDGE): with the active frames t1 < t2 < ... of a latent within one file's counted frames,
 * neighbours a < b belong to the same run iff b - a - 1 <= g.  A run's DURATION is last - first + 1, bridged frames included.  The
 * GAP between two consecutive runs of one file is b - a - 1 (> g); the silence before the first and after the last run of a file
 * is no gap.  A run is CENSORED iff it starts on frame 0 or ends on the last counted frame of its file: its duration is a lower
 * bound.  BINS, integers only: with s = sub_bits (0..3), P = 2^s and a duration or gap L >= 1, idx = L if L < 2P, else idx = sh P +
 * (L >> sh) with sh = floor(log2 L) - s; bin = idx - 1.  The lower edge of idx is idx if idx < 2P, else (P + idx % P) << (idx / P -
 * 1).  NB = idx(rows_per_file) bins; rows_per_file <= 65535 for this entry point, so NB <= SAE_TIMING_MAX_BINS.  s = 2: the
 * durations 1..7 have a bin each (20-140 ms), then four bins per octave; T = 1500: 37 bins.
 *
 * sae_timing_files adds one batch to run_hist_dev [n_dict][NB], gap_hist_dev [n_dict][NB], totals_dev [n_dict][SAE_TIMING_NTOTALS]
 * (SAE_TIMING_ACTIVE: active frames; _SPAN: the sum of the durations; _RUNS; _FILES: files with at least one run; _LONGEST: the
 * longest run, a running MAXIMUM; _CENSORED) and n_frames_dev [1].  All are int64 running totals, caller-owned, zeroed before the
 * first batch and passed together to every call of one pass.  Per latent: sum(run_hist) == RUNS, sum(gap_hist) == RUNS - FILES,
 * SPAN == ACTIVE at g = 0 and SPAN >= ACTIVE otherwise, LONGEST <= rows_per_file.  Every sum is an integer add and LONGEST an integer
 * max: two runs give bitwise identical arrays, whatever the batch and the launch geometry.
 *
 * An L1 context walks the stored latent of its ordinary encoder, a TopK context its selection (the indices of a row are distinct;
 * an index outside [0, n_dict) is ignored).  flags: 0, or SAE_TIMING_ONE_CHUNK -- an L1 context then walks all files of the call
 * in ONE chunk per column block instead of the chunks its launcher forms (a TopK context ignores it); the arrays do not depend on
 * it, which is what the tests use it for: it is slower.  n_files * rows_per_file <= max_rows; fp8 contexts: SAE_ERR_INVALID.
 * Null or misaligned arrays, sub_bits outside 0..3, bridge outside [0, SAE_TIMING_MAX_BRIDGE], threshold_bits > 0x7F80,
 * rows_per_file > 65535, unknown flags and bad shapes fail before anything is enqueued.  Asynchronous on `stream`.  Training state
 * is untouched; afterwards sae_latent_buffer, sae_topk_indices, sae_decode, sae_multi_topk_buffers, sae_latent_colmax and
 * sae_read_metrics return SAE_ERR_STATE until the next sae_eval / step. */
enum { SAE_TIMING_ACTIVE = 0, SAE_TIMING_SPAN = 1, SAE_TIMING_RUNS = 2, SAE_TIMING_FILES = 3, SAE_TIMING_LONGEST = 4, SAE_TIMING_CENSORED = 5,
       SAE_TIMING_NTOTALS = 6 };
#define SAE_TIMING_ONE_CHUNK 1
#define SAE_TIMING_MAX_BINS 111
#define SAE_TIMING_MAX_BRIDGE 15
int sae_timing_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                     int sub_bits, int bridge, uint32_t threshold_bits, int flags, int64_t* run_hist_dev, int64_t* gap_hist_dev,
                     int64_t* totals_dev, int64_t* n_frames_dev, void* stream);

/* ---- Dictionary comparison: what a dictionary IS against another one, or against itself -- which 32x latents an 8x latent split
 * into, whether two runs found the same features (mean max cosine similarity), which latents duplicate each other.  All of it is
 * the cosines between unit decoder directions and, per direction of A, its nearest directions of B.
 *
 * Semantics (freud_amd/csrc/dict_match.h).  A dictionary is n directions of length d in fp32: direction i, element e is
 * w_dev[i * dir_stride + e * elem_stride] (strides in elements, >= 1).  TopK: the rows of W_dec [n][d] (dir_stride d, elem_stride
 * 1); L1: the columns of the tied decoder.weight [d][n] (dir_stride 1, elem_stride n).  Both are read in place.
 *   Unit direction  u = w / ||w||.  ||w|| = the IEEE square root of an fp32 sum of squares taken in one fixed order (64 partial
 *                   sums, partial l adding the elements l, l + 64, ... in order with one fused multiply-add each, then the xor
 *                   butterfly 32, 16, 8, 4, 2, 1 over the partials); the division is the IEEE one.  The order does not depend on
 *                   the strides: the same dictionary in either layout gives the same bits.  A direction of norm 0 stays the zero
 *                   vector, its cosine with everything is 0.  Weights must be finite (freud_amd/dictionary_match.py refuses others).
 *   Cosine          S[i][j] = <ua_i, ub_j>, fp32 accumulation on the bf16 MFMA.  Each unit vector is split as hi = bf16(u),
 *                   lo = bf16(u - hi) and the product is hi.hi + hi.lo + lo.hi (the dropped lo.lo is at most 2^-18 relative):
 *                   concatenated along K, one bf16 GEMM with K = 3 d.
 *   Answer          per direction i of A its directions of B by cosine descending, then the lower index.  Signed values as they
 *                   are: no positivity filter, no clamp (1 + 1 ulp on a duplicate is reported as computed).
 *   Self mode       B is A: direction i is not its own neighbour (its duplicates are).
 *   Determinism     every output is written by one lane, there are no atomics: two runs give bitwise identical outputs, and the
 *                   keys of a row do not depend on the row block they were computed in.
 *
 * sae_dict_pack_bytes: the size of a packed operand for n directions of length d (0 when n or d is out of range).
 * sae_dict_pack: w_dev -> packed_dev (sae_dict_pack_bytes(n, d) bytes, 16-byte aligned, every byte written; the format is opaque:
 * n rounded up to 256 rows of three K segments of d rounded up to 64 bf16, SAE_DICT_LEFT packs [hi | hi | lo], SAE_DICT_RIGHT
 * [hi | lo | hi]) and norms_dev [n] (fp32).  A comparison packs A with SAE_DICT_LEFT and B with SAE_DICT_RIGHT; self mode packs
 * the same dictionary both ways.
 * sae_dict_sim_keys: keys_dev [n_rows][n_b] = ord(S[row0 + r][j]) << 32 (freud_amd/csrc/search_keys.h: order-preserving, -0.0 as
 * 0.0, never 0 for a finite value) for the rows [row0, row0 + n_rows) of A, and 0 at j == row0 + r in self mode.
 * sae_file_top_features(keys_dev, n_rows, n_b, n_neighbors, 0, ...) then gives the answer (a key of 0 is never reported).
 *
 * 1 <= n <= 2^24, 1 <= d <= SAE_DICT_MAX_D, side SAE_DICT_LEFT or SAE_DICT_RIGHT, self mode only with n_a == n_b, a non-empty row
 * block inside [0, n_a) of at most 2^30 256 x 256 tiles, non-null pointers: otherwise SAE_ERR_INVALID before anything is enqueued.
 * The calls need no context, run on the current device and are asynchronous on `stream`. */
#define SAE_DICT_MAX_D 8192
enum { SAE_DICT_LEFT = 0, SAE_DICT_RIGHT = 1 };
int64_t sae_dict_pack_bytes(int64_t n, int64_t d);
int sae_dict_pack(const float* w_dev, int64_t n, int64_t d, int64_t dir_stride, int64_t elem_stride, int side, void* packed_dev,
                  float* norms_dev, void* stream);
int sae_dict_sim_keys(const void* packed_a_dev, int64_t n_a, const void* packed_b_dev, int64_t n_b, int64_t d, int64_t row0,
                      int64_t n_rows, int self_mode, uint64_t* keys_dev, void* stream);

/* ---- Feature manipulation: the reference's manipulate_latent (utils/activations.py:243-272, served as /manipulate_feature) for
 * a batch of files, several edited latents and a sweep of edit values at once -- everything between the cached activations and
 * the tensors handed to whisper_subbed.forward: the standard reconstruction, the manipulated ones, and the per-frame series of
 * the edited latents.  A decode is linear in the latent, so one encode and one decode serve any number of edits and variants.
 *
 * Semantics (freud_amd/csrc/manip.h).  x_dev is [n_files][rows_per_file][d]; M = n_files * rows_per_file.  ALL M frames are
 * edited and decoded (the reference edits the padded frames too and trims only the series it returns, activations.py:283-289;
 * trimming belongs to the caller).  Per frame t and edit e, a = the value freud_amd.models encode() returns for latent
 * latents_host[e], widened exactly from bf16 to fp32: the stored L1 latent, or for TopK the selected activation and 0 where the
 * latent is not among the row's k (activation_tensor_from_indexed, activations.py:41-58; a multi_topk context uses its k
 * selection).  Variant v edits it with values_host[v * n_edits + e]:
 *   SAE_MANIP_SCALE  new = a * value (the reference's manipulation_factor, activations.py:247-249, 261), one fp32 rounding;
 *   SAE_MANIP_SET    new = value on every frame, selected or not (the latent clamped);
 * delta = new - a, one fp32 rounding.  Outputs, all fp32, dense, caller-owned device memory:
 *   series_dev      [n_edits][M]       a (the manipulated series is sm_new of it: the caller's arithmetic, one multiplication);
 *   standard_dev    [M][d]             L1: latent . W^T, the decoder GEMM of sae_decode on the forward's own bf16 latent and the
 *                                      bf16 copy of the current (normalised) W -- bit for bit sae_decode of sae_latent_buffer;
 *                                      TopK: b_dec + sum_i top_acts[t][i] * bf16(W_dec)[top_indices[t][i]], fp32 fmaf in stored
 *                                      list order (no dense row, no GEMM);
 *   manipulated_dev [n_variants][M][d] fmaf(delta_{v,E-1}, w_{E-1}[c], ... fmaf(delta_{v,0}, w_0[c], standard[t][c])): the edits
 *                                      in the order given, w_e = row latents_host[e] of the same bf16 decoder operand, widened.
 *                                      An edit whose delta is zero is skipped, so a frame on which nothing changes (and every
 *                                      frame of a SCALE by 1) is bit for bit standard.  This is the decode of the edited latent
 *                                      WITHOUT rounding the edited value back to a bf16 GEMM operand.
 *
 * SAE_ERR_INVALID before anything is enqueued: a null pointer, n_edits outside [1, SAE_MANIP_MAX_EDITS], n_variants outside
 * [1, SAE_MANIP_MAX_VARIANTS], a latent outside [0, n_dict), the same latent twice, an unknown op, a non-finite value, flags != 0,
 * an fp8 context, n_files * rows_per_file > max_rows.  Asynchronous on `stream`; the host arrays are read before the call returns.
 * Deterministic: two runs give bitwise identical outputs.  The first call allocates 64 x d bytes of context scratch (the operand
 * rows).  Training state (parameters, moments, num_frames_since_fired) is untouched; the forward is the bf16 one whatever
 * sae_set_eval_precision says, and afterwards the context is in the state sae_eval of the same batch leaves it in:
 * sae_latent_buffer, sae_topk_indices, sae_read_metrics, sae_latent_colmax and sae_decode answer for this batch. */
#define SAE_MANIP_MAX_EDITS 16
#define SAE_MANIP_MAX_VARIANTS 16
enum { SAE_MANIP_SCALE = 0, SAE_MANIP_SET = 1 };
int sae_manipulate_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype,
                         const int32_t* latents_host, const int32_t* ops_host, int n_edits,
                         const float* values_host /* [n_variants][n_edits] */, int n_variants, int flags,
                         float* standard_dev    /* [M][d]             */,
                         float* manipulated_dev /* [n_variants][M][d] */,
                         float* series_dev      /* [n_edits][M]       */, void* stream);

/* ---- Reconstruction report: how well the dictionary reconstructs the data, where it fails, and which latents carry the
 * reconstruction -- in one pass over the data.  Nothing of size frames x latents is stored.
 *
 * Both decoders are linear in the latent.  With r = x - x_hat the residual of a frame, a_j the value of latent j on it and w_j
 * its decoder direction, zeroing latent j changes the frame's squared error by 2 a_j (r . w_j) + a_j^2 |w_j|^2.  Summed over the
 * data, P_j = sum a_j (r . w_j) and Q_j = |w_j|^2 sum a_j^2 give
 *   ablation_j = 2 P_j + Q_j     the squared error latent j is worth,
 *   rescale_j  = 1 + P_j / Q_j   the least-squares gain of latent j with everything else held fixed (the shrinkage diagnostic of
 *                                an L1 dictionary: the L1 penalty pushes it above 1).
 *
 * Semantics (freud_amd/csrc/recon.h).
 *   Frames   count exactly as in sae_stats_files (lengths_dev: the first min(length, T) frames of a file; without, all T).
 *   a        is the value freud_amd.models encode() returns: the bf16 L1 latent, or the TopK k selection (a multi_topk context uses
 *            its k selection); a selected zero contributes nothing.
 *   x_hat    L1: sae_decode's GEMM on the forward's own latent, as sae_manipulate_files' standard_dev: the bf16 copy of the
 *            normalised W, the output rounded to bf16, no bias -- bit for bit models.decode(encode(x).latent).  TopK: the sparse
 *            fp32 decode of the compact selection with the bf16 W_dec, plus b_dec (standard_dev of sae_manipulate_files).
 *   r        = float(x) - x_hat, ONE fp32 subtraction on the delivered x (f32, or f16 / bf16 widened exactly), not on the engine's
 *            bf16 copy.  r = 0 on frames that do not count.
 * Per latent j < n, over the counted frames:
 *   attr_sum[j]    = P_j = sum a s, with s = r_b . w_j for L1 (r_b = bf16(r), round to nearest even; w_j the column of the bf16
 *                    normalised W; accumulated in fp32 by the MFMA and NOT rounded to bf16) and s = r . w_j in fp32 for TopK
 *                    (w_j = row j of the bf16 W_dec); a s is one fp32 product;
 *   act_sq_sum[j]  = sum a^2;
 *   dec_norm_sq[j] = |w_j|^2 of that decoder operand (written, not accumulated).
 * Per model dimension i < d: sum_x[i], sum_x_sq[i], sum_r_sq[i] over the counted frames.
 * Per file f of the batch: file_out[f] = {sum r^2, sum x^2} over the file's counted frames (written, not accumulated).
 * resid_dev (fp32 [M][d], may be null) receives r itself: the per-frame error.
 *
 * Output block: caller-owned, 8-byte aligned, SAE_RECON_BYTES(n, d) bytes of running totals; zero it before the first batch,
 * every call adds one batch.  Byte offsets:
 *   SAE_RECON_N_FRAMES    int64                frames counted
 *   SAE_RECON_ATTR_SUM    float64 [n]
 *   SAE_RECON_ACT_SQ_SUM  float64 [n]
 *   SAE_RECON_SUM_X       float64 [d]
 *   SAE_RECON_SUM_X_SQ    float64 [d]
 *   SAE_RECON_SUM_R_SQ    float64 [d]
 *   SAE_RECON_DEC_NORM_SQ float32 [n]
 *
 * Determinism: every float sum is a fixed-order fp32 partial written with plain stores -- per (row, 64 columns) for the file
 * sums, per (128-row block, column) for the model dimensions and the L1 latents, per (256-row block, latent) for TopK -- folded
 * in a fixed order into the fp64 totals.  No float atomics: two runs over the same batches give bitwise identical blocks.
 *
 * Out of scope: raw (no-SAE) activations; fp8 contexts; the ignored_index mask of the reference's mse_loss (an element of x equal
 * to -1 is data here); re-encoding after an ablation (the effect is first order in the decoder only); joint ablations. */
#define SAE_RECON_N_FRAMES(n, d) ((int64_t)0)
#define SAE_RECON_ATTR_SUM(n, d) ((int64_t)8)
#define SAE_RECON_ACT_SQ_SUM(n, d) ((int64_t)8 + 8 * (int64_t)(n))
#define SAE_RECON_SUM_X(n, d) ((int64_t)8 + 16 * (int64_t)(n))
#define SAE_RECON_SUM_X_SQ(n, d) ((int64_t)8 + 16 * (int64_t)(n) + 8 * (int64_t)(d))
#define SAE_RECON_SUM_R_SQ(n, d) ((int64_t)8 + 16 * (int64_t)(n) + 16 * (int64_t)(d))
#define SAE_RECON_DEC_NORM_SQ(n, d) ((int64_t)8 + 16 * (int64_t)(n) + 24 * (int64_t)(d))
#define SAE_RECON_BYTES(n, d) (((int64_t)8 + 20 * (int64_t)(n) + 24 * (int64_t)(d) + 7) / 8 * 8)
enum { SAE_RECON_UNFUSED = 1 };

/* Add the report of one batch (x_dev [n_files][rows_per_file][d], x_dtype) to block_dev and write file_out_dev / resid_dev.
 * L1: the encoder with the stored latent, the decoder GEMM, the residual sweep, then the attribution as the epilogue of the
 * backward's dpre-shaped GEMM (r_b x W) -- in the streaming GEMM where its conditions hold (as for sae_stats_files: an even number
 * of 128-row blocks, 2048 tiles of 256 x 256), in the tile GEMMs elsewhere; flags = SAE_RECON_UNFUSED keeps it off the streaming
 * kernel, so the two forms can be compared (they associate the fp32 sums of a 128-row block differently).  TopK: the eval forward, the sparse decode, the sweep, one dot
 * per selected slot and a column walk of the selection; d_model <= 1536.  n_files * rows_per_file <= max_rows; fp8 contexts:
 * SAE_ERR_INVALID.  Shape and argument checks fail before anything is enqueued.  Asynchronous on `stream`; the first call
 * allocates the context's scratch (4 d bytes per row, 8 bytes per 128 rows and latent, 4 k bytes per row for TopK).  Training
 * state (parameters, moments, num_frames_since_fired) is untouched; the stored latent is not valid afterwards, and
 * sae_latent_buffer, sae_topk_indices, sae_decode, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return
 * SAE_ERR_STATE until the next sae_eval / step. */
int sae_recon_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                    int flags, void* block_dev, double* file_out_dev /* [n_files][2] */, float* resid_dev /* or null */,
                    void* stream);

/* ---- Feature collection: the SAE features of a dataset in the reference's indexed form (collect_activations.py with sae_model
 * set: <layer>_activation_values.npy + <layer>_feature_indices.npy, read back as activation_type == "indexed"), written from the
 * cached layer activations -- one encode per row and a per-row select.
 *
 * Semantics.  Every frame (row) of every file is stored, all T of them: the reference collects untrimmed and trims at search time,
 * so there is no lengths argument.  Let a be the latent row exactly as freud_amd.models encode() returns it -- L1: the bf16
 * c = relu(x W + b) that sae_eval leaves in sae_latent_buffer; TopK: the scatter of the k selection, 0 elsewhere (a multi_topk
 * context uses its k selection).  The row's K slots are the first K entries of a stable descending sort of a: value descending,
 * equal values by the lower column -- numpy.argsort(-a, kind="stable")[:K].  So
 *   - slots are sorted: the first K' slots of a row are its top K', and a store can be truncated by prefix;
 *   - a row with fewer than K positive latents is padded with zero-valued latents in increasing column order, stored as +0.0 even
 *     where the latent holds a bf16 -0.0 (a latent is ACTIVE iff its magnitude bits are non-zero and its sign is clear, as in
 *     sae_stats_files);
 *   - the indices of a row are always distinct (the reference's activation_tensor_from_indexed raises on a repeated index);
 *   - for TopK this is the engine's own tie rule (lowest column first, selected zeros included): the store is the selection itself,
 *     canonically ordered.
 * Limits: L1 1 <= K <= min(n_dict, SAE_COLLECT_MAX_K); TopK 1 <= K <= k.
 *
 * values_dev [n_files * rows_per_file][K] fp32 (the bf16 value widened: exact) and indices_dev of the same shape, int64 or, with
 * SAE_COLLECT_IDX32, int32: caller-owned device memory, dense, in file order -- one file's block is one row of the .npy files.
 *
 * stats_dev: caller-owned int64[8], 8-byte aligned, running totals: zero it before the first batch, every call adds one batch.
 * Integer adds and integer maxima only, so it is order-free and deterministic.
 *   [0] rows collected                          [1] active latents stored
 *   [2] active latents dropped (active in the row but beyond slot K)
 *   [3] rows that dropped at least one          [4] largest number of active latents in a row
 *   [5] bf16 bit pattern of the largest dropped value (0 if none)        [6], [7] reserved, left 0
 * The store equals the latent iff [2] is 0.
 *
 * The call is the bf16 eval encoder followed by the collect kernels (freud_amd/csrc/collect.h), asynchronous on `stream`.  n_files
 * * rows_per_file <= max_rows; fp8 contexts: SAE_ERR_INVALID.  K out of range (TopK: K > k), unknown flag bits, null pointers, a
 * misaligned values_dev, indices_dev or stats_dev and bad shapes fail before anything is enqueued.  Training state (parameters,
 * moments, num_frames_since_fired) is untouched; afterwards sae_latent_buffer, sae_topk_indices, sae_decode,
 * sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return SAE_ERR_STATE until the next sae_eval / step, as after
 * sae_stats_files.  Exact and deterministic: two runs give the same bytes. */
enum { SAE_COLLECT_IDX32 = 1 };
#define SAE_COLLECT_MAX_K 1024
int sae_collect_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, int K, int flags,
                      float* values_dev, void* indices_dev, int64_t* stats_dev, void* stream);

/* ---- Sparsity frontier: the squared reconstruction error of a dataset at EVERY per-frame latent budget s = 0 .. K, and per frame
 * the budget that reaches a share of its energy -- the SAE's curve beside the PCA curve of sae_input_cov, and what a cut of the
 * feature store to K' slots costs (freud_amd/sparsity_frontier.py; kernels: freud_amd/csrc/frontier.h).
 *
 * Semantics.  Counted frames as in sae_recon_files: the first min(lengths[f], rows_per_file) frames of file f when lengths_dev is
 * given, all of them otherwise.  For a counted frame:
 *   (v_s, i_s), s < K   exactly the slots sae_collect_files defines for the row (the same entry word, predicate and tie rule: the
 *                       padding is +0.0 in column order, a multi_topk context uses its k selection), so the frontier's prefix at
 *                       K' IS the content of a store cut to K';
 *   w_j                 the bf16 decoder operand of the reconstruction report: the column of the normalised bf16 W for L1 (read
 *                       as a row of the transposed copy), row j of the bf16 W_dec for TopK;
 *   r_0     = float(x) - b, ONE fp32 subtraction on the delivered x; b = b_dec for TopK, 0 for L1;
 *   r_{s+1} = fmaf(-v_s, w_{i_s}, r_s) elementwise in fp32, in slot order (a padding slot changes nothing);
 *   e_s     = sum_i r_s[i]^2, s = 0 .. K, an fp32 sum in a fixed order that depends on the row alone (frontier.h: fr_lane_sq,
 *             fr_wave_sum) -- not on K, the batch, the grid or the row's neighbours.
 * An element of x equal to -1 is data, as in the reconstruction report.
 * The frame's BUDGET at a threshold tau is the smallest s in 0 .. K with e_s <= tau * e_0 (one fp32 product, one fp32 compare),
 * K + 1 if there is none; a frame with e_0 == 0 has budget 0.  Up to SAE_FRONTIER_MAX_TAU thresholds, a HOST array of floats, each
 * finite and inside (0, 1).
 *
 * Output block: caller-owned device memory, 8-byte aligned, SAE_FRONTIER_BYTES(n_tau, K, d) bytes of running totals; zero it before
 * the first batch, every call adds one batch (the same K and thresholds).  Byte offsets:
 *   SAE_FRONTIER_N_FRAMES    int64                  frames counted
 *   SAE_FRONTIER_ROWS_CUT    int64                  counted rows with more than K active latents   (sae_collect_files' stats [3])
 *   SAE_FRONTIER_ACTIVE_CUT  int64                  their active latents beyond slot K             (sae_collect_files' stats [2])
 *   SAE_FRONTIER_SSE         float64 [K + 1]        sum over the frames of e_s: the squared error with s latents per frame
 *   SAE_FRONTIER_SUM_X       float64 [d]            with SUM_X_SQ the denominator of the reconstruction report's FVU
 *   SAE_FRONTIER_SUM_X_SQ    float64 [d]
 *   SAE_FRONTIER_BUDGET      int64 [n_tau][K + 2]   per threshold the histogram of the frames' budgets
 *
 * Limits: 1 <= K <= SAE_FRONTIER_MAX_K; L1 K <= n_dict, TopK K <= k; d_model <= 1536 (padded); n_files * rows_per_file <=
 * max_rows; bf16 contexts only (fp8: SAE_ERR_INVALID).  Every shape and argument check -- K out of range, n_tau outside
 * [0, SAE_FRONTIER_MAX_TAU], a threshold outside (0, 1), unknown flag bits (none are defined), null pointers, a misaligned block --
 * fails before anything is enqueued.
 *
 * Determinism: every float sum is a fixed-order fp32 partial written with plain stores -- e_s per row, its sums per 32 consecutive
 * rows of the batch, sum_x / sum_x_sq per (128-row block, column) -- folded in a fixed order into the fp64 totals.  No float
 * atomics: two runs give the same bytes.  A frame's e_s depends on the frame alone, so the integer fields are the same for every
 * split of the files into batches, and the first K' + 1 entries of sse equal those of a run at K' over the same batches.
 *
 * The call is the bf16 eval encoder, the collect kernels into context scratch (8 K bytes per row, allocated by the first call) and
 * the walk, asynchronous on `stream`.  Training state (parameters, moments, num_frames_since_fired) is untouched; afterwards
 * sae_latent_buffer, sae_topk_indices, sae_decode, sae_multi_topk_buffers, sae_latent_colmax and sae_read_metrics return
 * SAE_ERR_STATE until the next sae_eval / step, as after sae_collect_files.
 *
 * Out of scope: K above a TopK context's k (no wider re-selection); re-encoding under a budget (the latent is encode()'s, only cut);
 * raw (no-SAE) activations; fp8 contexts; per-frame output arrays; NaN / Inf inputs. */
#define SAE_FRONTIER_MAX_K 256
#define SAE_FRONTIER_MAX_TAU 8
#define SAE_FRONTIER_N_FRAMES(n_tau, K, d) ((int64_t)0)
#define SAE_FRONTIER_ROWS_CUT(n_tau, K, d) ((int64_t)8)
#define SAE_FRONTIER_ACTIVE_CUT(n_tau, K, d) ((int64_t)16)
#define SAE_FRONTIER_SSE(n_tau, K, d) ((int64_t)24)
#define SAE_FRONTIER_SUM_X(n_tau, K, d) ((int64_t)32 + 8 * (int64_t)(K))
#define SAE_FRONTIER_SUM_X_SQ(n_tau, K, d) ((int64_t)32 + 8 * (int64_t)(K) + 8 * (int64_t)(d))
#define SAE_FRONTIER_BUDGET(n_tau, K, d) ((int64_t)32 + 8 * (int64_t)(K) + 16 * (int64_t)(d))
#define SAE_FRONTIER_BYTES(n_tau, K, d) ((int64_t)32 + 8 * (int64_t)(K) + 16 * (int64_t)(d) + 8 * (int64_t)(n_tau) * ((int64_t)(K) + 2))
int sae_frontier_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                       int K, const float* thresholds /* host, [n_tau] */, int n_tau, int flags, void* block_dev, void* stream);

/* ---- Pursuit frontier: the DECODER's best-case squared error at every per-frame latent budget s = 0 .. K -- every counted frame
 * coded greedily against the decoder directions, without the trained encoder (non-negative matching pursuit, "inference-time
 * optimisation").  The curve between sae_input_cov's PCA curve and sae_frontier_files' encoder curve: their difference at a budget
 * is the amortisation gap (freud_amd/pursuit.py; kernels: freud_amd/csrc/pursuit.h).
 *
 * Semantics.  Counted frames as in sae_frontier_files (lengths_dev, trimmed to min(length, rows_per_file)).  w_j, j < n_dict, is the
 * bf16 operand row the frontier uses: L1 -- row j of the transposed normalised copy, b = 0; TopK -- row j of the bf16 W_dec,
 * b = b_dec.  The per-direction constants are fp32, computed once per call in one fixed order (pursuit.h):
 *   q_j = sum_e w_j[e]^2,   z_j = 1 / sqrt(q_j);   a direction with q_j == 0 has z_j = 0 and is never chosen.
 * Per counted frame:
 *   r_0 = float(x) - b                          one fp32 subtraction on the delivered x
 *   step s = 0 .. K - 1, unless the row has stopped:
 *     rho   = bf16(r_s)                         round to nearest even, per element
 *     sc_j  = fp32_acc(rho . w_j) * z_j         the bf16 MFMA product; SELECTION ONLY
 *     j*    = argmax_j sc_j over j < n_dict     ties to the LOWER j; padding rows / columns are never eligible
 *     stop if sc_j* <= 0
 *     a     = fp32 dot(r_s, w_j*) / q_j*        from the fp32 residual, fixed order, IEEE division
 *     stop if not (a > 0)
 *     r_{s+1} = fmaf(-a, w_j*, r_s)
 *   e_s = |r_s|^2 (fp32, fixed order), s = 0 .. K; a stopped row keeps its e for the remaining s.
 * Non-negative matching pursuit, because SAE codes are non-negative.  A latent may be chosen again later -- the code then
 * accumulates -- so e_s is the error with AT MOST s distinct latents.  The bf16 product only chooses: every reported number comes
 * from the fp32 residual and the fp32 coefficient.  The frame's budget at a threshold is the frontier's (smallest s with
 * e_s <= tau e_0, K + 1 if none, e_0 == 0: budget 0).
 *
 * Output block: caller-owned device memory, 8-byte aligned, SAE_PURSUIT_BYTES(n_tau, K, d, n) bytes of running totals; zero it
 * before the first batch, every call adds one batch (the same K and thresholds).  Byte offsets:
 *   SAE_PURSUIT_N_FRAMES     int64                  frames counted
 *   SAE_PURSUIT_SSE          float64 [K + 1]        summed e_s
 *   SAE_PURSUIT_SUM_X        float64 [d]            the frontier's denominators
 *   SAE_PURSUIT_SUM_X_SQ     float64 [d]
 *   SAE_PURSUIT_BUDGET       int64 [n_tau][K + 2]   the frontier's budget histogram
 *   SAE_PURSUIT_STEPS        int64 [K + 1]          histogram of the number of picks a frame made before it stopped
 *   SAE_PURSUIT_PICKS        int64 [n]              how often latent j was chosen
 *   SAE_PURSUIT_IN_SUPPORT   int64 [K]              picks of step s that lie in the encoder's own active set for that frame (L1: the
 *                                                   stored bf16 latent of the eval encoder is > 0; TopK: the latent is among the
 *                                                   selected indices with a positive value)
 *
 * Optional trace, three device pointers, all or none (4-byte aligned), per row of THIS batch: trace_idx int32 [M][K] -- the pick, -1
 * after the stop and on uncounted frames; trace_val float32 [M][K] -- a, or +0.0; trace_err float32 [M][K + 1] -- e_s, 0 on
 * uncounted frames.  The trace is the pursuit code in pick order, not a feature store: indices may repeat.
 *
 * Limits: 1 <= K <= SAE_PURSUIT_MAX_K (whatever the context's k); n_tau <= SAE_PURSUIT_MAX_TAU, thresholds inside (0, 1);
 * d_model <= 1536 (padded); n_files * rows_per_file <= max_rows; bf16 contexts only; no flag bits are defined.  Every check fails
 * before anything is enqueued.
 *
 * Determinism: two runs give the same bytes.  The trace, STEPS, PICKS, IN_SUPPORT, BUDGET and N_FRAMES do not depend on the split
 * of the files into batches: a score's sum over K does not depend on the tile it is computed in, and everything after the pick is
 * per row.  Float sums are fixed-order fp32 partials folded in ascending order into fp64, as for sae_frontier_files; no float
 * atomics (integer adds and an unsigned 64-bit max only).
 *
 * The call is the bf16 eval encoder (for IN_SUPPORT), then K (GEMM, step) launch pairs on `stream` with no host synchronisation
 * between them, then the fold.  Context scratch: 6 d_p + 4 K + 48 bytes per row of max_rows, allocated by the first call.
 * Training state is untouched; the last-forward getters return SAE_ERR_STATE until the next sae_eval / step, as after
 * sae_frontier_files.
 *
 * Out of scope: orthogonal or gradient pursuit; signed codes; the pursuit code as a feature store (repeated picks would need
 * merging); an early exit of the GEMM for row blocks that have stopped; fp8 contexts. */
#define SAE_PURSUIT_MAX_K 256
#define SAE_PURSUIT_MAX_TAU 8
#define SAE_PURSUIT_N_FRAMES(n_tau, K, d, n) ((int64_t)0)
#define SAE_PURSUIT_SSE(n_tau, K, d, n) ((int64_t)8)
#define SAE_PURSUIT_SUM_X(n_tau, K, d, n) ((int64_t)16 + 8 * (int64_t)(K))
#define SAE_PURSUIT_SUM_X_SQ(n_tau, K, d, n) (SAE_PURSUIT_SUM_X(n_tau, K, d, n) + 8 * (int64_t)(d))
#define SAE_PURSUIT_BUDGET(n_tau, K, d, n) (SAE_PURSUIT_SUM_X(n_tau, K, d, n) + 16 * (int64_t)(d))
#define SAE_PURSUIT_STEPS(n_tau, K, d, n) (SAE_PURSUIT_BUDGET(n_tau, K, d, n) + 8 * (int64_t)(n_tau) * ((int64_t)(K) + 2))
#define SAE_PURSUIT_PICKS(n_tau, K, d, n) (SAE_PURSUIT_STEPS(n_tau, K, d, n) + 8 * ((int64_t)(K) + 1))
#define SAE_PURSUIT_IN_SUPPORT(n_tau, K, d, n) (SAE_PURSUIT_PICKS(n_tau, K, d, n) + 8 * (int64_t)(n))
#define SAE_PURSUIT_BYTES(n_tau, K, d, n) (SAE_PURSUIT_IN_SUPPORT(n_tau, K, d, n) + 8 * (int64_t)(K))
int sae_pursuit_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                      int K, const float* thresholds /* host, [n_tau] */, int n_tau, int flags, void* block_dev, int32_t* trace_idx_dev,
                      float* trace_val_dev, float* trace_err_dev, void* stream);

/* ---- Refit frontier: the squared error at every per-frame latent budget s = 0 .. K when the SUPPORT is the encoder's own (or one
 * the caller gives) and the COEFFICIENTS are the least-squares ones on every prefix of its slots.  It splits the amortisation gap of
 * the pursuit frontier: encoder - refit is the coefficient error (shrinkage, cross-talk), refit - pursuit the support error; on the
 * pursuit's own trace it is pursuit with a final orthogonal projection (freud_amd/refit.py; kernels: freud_amd/csrc/refit.h, the
 * rule in freud_amd/csrc/refit_chol.h).
 *
 * Semantics.  Counted frames, w_j, b and r_0 = float(x) - b are exactly those of sae_frontier_files.  The support of a frame:
 *   support_idx_dev == NULL   the K slots (v_s, i_s) of sae_collect_files (the same entry word, tie rule and padding); a slot is
 *                             ACTIVE iff v_s != 0;
 *   support_idx_dev != NULL   int32 [M][K], those indices; no encoder and no collect run.  -1 marks an empty slot; an index outside
 *                             [0, n_dict) is counted in BAD_INDEX, is never used as an address and leaves its slot empty; a repeated
 *                             index is legal (the rank rule below drops it).
 * Per frame, with the active slots in slot order:
 *   G[s][t] = sum_e w_{i_s}[e] w_{i_t}[e]   the products are exact, accumulated in fp32 by the bf16 MFMA in an order that depends on
 *             d_p alone (not on K, the row's neighbours or the batch).  G is specified by a bound, not by an order:
 *             |G - G64| <= gamma(d_p) sum |w w|, gamma(n) = n 2^-24 / (1 - n 2^-24).  A slot that is not active has G = 0.
 *   c[s]    = fp32 dot(r_0, w_{i_s}) in the lane and column order of the frontier (frontier.h: a lane's d_p / 64 columns in order
 *             from 0, the shares by fr_wave_sum); 0 on a slot that is not active
 *   e_0     = |r_0|^2 by the frontier's functions: bit-equal to the frontier's e_0.
 * From here every number has ONE defined order; the chains run over the KEPT slots u in ascending order:
 *   piv_s   = G[s][s], then fmaf(-L[s][u], L[s][u], .) over kept u < s
 *   the slot is DEPENDENT iff piv_s <= 2^-10 * G[s][s] (one fp32 product, one compare; G[s][s] == 0 is dependent);
 *   otherwise d_s = sqrt(piv_s) and the slot is kept
 *   L[s][t] = (G[s][t], then fmaf(-L[s][u], L[t][u], .) over kept u < t) / d_t, for kept t < s
 *   y_s     = (c[s], then fmaf(-L[s][u], y_u, .) over kept u < s) / d_s
 *   e_{s+1} = fmaxf(fmaf(-y_s, y_s, e_s), 0);   an empty, inactive or dependent slot has e_{s+1} = e_s
 * with correctly rounded square root and division.  e_s is the squared error of the least-squares fit on the first s slots; row s
 * of L depends on the slots <= s only, so the first K' + 1 entries equal those of a run at K'.  (2^-10: on unit bf16 directions,
 * random or strongly correlated, every kept slot has a pivot ratio >= 0.05 and every exact duplicate one <= 1e-6.)
 * Coefficients at the full budget: a_s = (y_s, then fmaf(-L[u][s], a_u, .) over kept u > s, DESCENDING) / d_s, a_s = +0.0 on every
 * other slot; r = r_0, then r = fmaf(-a_s, w_{i_s}, r) over the kept slots in slot order; e_final = |r|^2 by the frontier's norm --
 * the directly computed error at budget K, reported beside the curve, whose end comes from e_0 - sum y^2.  The coefficients are
 * signed; negative ones are counted.
 *
 * Output block: caller-owned device memory, 8-byte aligned, SAE_REFIT_BYTES(n_tau, K, d, n) bytes of running totals; zero it before
 * the first batch, every call adds one batch (the same K, thresholds and kind of support).  Byte offsets:
 *   SAE_REFIT_N_FRAMES    int64                  frames counted
 *   SAE_REFIT_SSE         float64 [K + 1]        summed e_s: the curve
 *   SAE_REFIT_SSE_FINAL   float64                summed e_final
 *   SAE_REFIT_SUM_X       float64 [d]            the frontier's denominators
 *   SAE_REFIT_SUM_X_SQ    float64 [d]
 *   SAE_REFIT_BUDGET      int64 [n_tau][K + 2]   the frontier's budget predicate on the refit curve
 *   SAE_REFIT_KEPT        int64 [K + 1]          histogram of the number of kept slots per frame
 *   SAE_REFIT_SLOTS       int64 [n]              frames that hold latent j in an active slot
 *   SAE_REFIT_NEG         int64 [n]              kept slots of latent j whose refit coefficient is below zero
 *   SAE_REFIT_DEP         int64 [n]              active slots of latent j that were dependent
 *   SAE_REFIT_RATIO       int64 [36]             histogram of a_s / v_s over the kept slots (ONE IEEE division, binned on the fp32
 *                                                bit pattern: negative | zero | below 2^-4 | the eight octaves [2^-4, 2^4) in four
 *                                                sub-bins each | at or above 2^4); the default support only
 *   SAE_REFIT_BAD_INDEX   int64                  out-of-range indices of a given support
 *
 * Optional trace, device pointers, each nullable and 4-byte aligned (trace_dep: bytes), for the rows of THIS batch:
 *   trace_coef float32 [M][K]          a_s
 *   trace_err  float32 [M][K + 1]      e_s, 0 on uncounted frames
 *   trace_dep  uint8   [M][K]          1 = the slot is active and dependent
 *   trace_gram float32 [M][K + 1][K]   rows 0 .. K - 1: G with both triangles filled; row K: c
 * The Gram trace lets a host replay everything after the MFMA to the bit (refit_chol.h: rf_row_serial).
 *
 * Limits: 1 <= K <= SAE_REFIT_MAX_K; for the default support K <= k (TopK) and K <= n_dict (L1); d_model <= 1536 (padded); bf16
 * contexts only; no flag bits are defined; n_tau and the thresholds as for sae_frontier_files.  Every check fails before anything
 * is enqueued.
 *
 * State and determinism: training state is untouched (an L1 context normalises its weights in place, as every forward does); the
 * last-forward getters return SAE_ERR_STATE until the next sae_eval / step.  No float atomics: two runs give the same bytes; the
 * integer fields and the trace do not depend on the split of the files into batches.
 *
 * Out of scope: non-negative or sparsity-regularised refits; orthogonal pursuit with a refit inside every step; per-latent float
 * sums; K above 128; fp8 contexts; writing refit codes as a feature store. */
#define SAE_REFIT_MAX_K 128
#define SAE_REFIT_MAX_TAU 8
#define SAE_REFIT_RATIO_BINS 36
#define SAE_REFIT_N_FRAMES(n_tau, K, d, n) ((int64_t)0)
#define SAE_REFIT_SSE(n_tau, K, d, n) ((int64_t)8)
#define SAE_REFIT_SSE_FINAL(n_tau, K, d, n) ((int64_t)16 + 8 * (int64_t)(K))
#define SAE_REFIT_SUM_X(n_tau, K, d, n) ((int64_t)24 + 8 * (int64_t)(K))
#define SAE_REFIT_SUM_X_SQ(n_tau, K, d, n) (SAE_REFIT_SUM_X(n_tau, K, d, n) + 8 * (int64_t)(d))
#define SAE_REFIT_BUDGET(n_tau, K, d, n) (SAE_REFIT_SUM_X(n_tau, K, d, n) + 16 * (int64_t)(d))
#define SAE_REFIT_KEPT(n_tau, K, d, n) (SAE_REFIT_BUDGET(n_tau, K, d, n) + 8 * (int64_t)(n_tau) * ((int64_t)(K) + 2))
#define SAE_REFIT_SLOTS(n_tau, K, d, n) (SAE_REFIT_KEPT(n_tau, K, d, n) + 8 * ((int64_t)(K) + 1))
#define SAE_REFIT_NEG(n_tau, K, d, n) (SAE_REFIT_SLOTS(n_tau, K, d, n) + 8 * (int64_t)(n))
#define SAE_REFIT_DEP(n_tau, K, d, n) (SAE_REFIT_SLOTS(n_tau, K, d, n) + 16 * (int64_t)(n))
#define SAE_REFIT_RATIO(n_tau, K, d, n) (SAE_REFIT_SLOTS(n_tau, K, d, n) + 24 * (int64_t)(n))
#define SAE_REFIT_BAD_INDEX(n_tau, K, d, n) (SAE_REFIT_RATIO(n_tau, K, d, n) + 8 * (int64_t)SAE_REFIT_RATIO_BINS)
#define SAE_REFIT_BYTES(n_tau, K, d, n) (SAE_REFIT_BAD_INDEX(n_tau, K, d, n) + 8)
int sae_refit_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                    int K, const float* thresholds /* host, [n_tau] */, int n_tau, int flags, const int32_t* support_idx_dev,
                    void* block_dev, float* trace_coef_dev, float* trace_err_dev, unsigned char* trace_dep_dev, float* trace_gram_dev,
                    void* stream);

/* ---- Feature index: the latent-major postings of an indexed feature store -- for every latent the (position, value) of the slots
 * that fire it, positions ascending (freud_amd/feature_index.py; kernels: freud_amd/csrc/findex.h).  The reference has no index:
 * it rebuilds one latent's series from the row-major store by scanning every slot of every file, per query
 * (src/utils/activations.py:41-58, activation_tensor_from_indexed, called per batch by top_activations, :95-101).  The index is
 * that scan made once for all latents: a stable counting sort of the store's slots by latent.
 *
 * Context-free (no sae_ctx, like sae_search_merge), asynchronous on `stream`, all pointers caller-owned DEVICE memory.  A batch is
 * values_dev [rows][K] fp32 and indices_dev [rows][K] int64 (int32 with SAE_FINDEX_IDX32): rows of whole files in file order,
 * 1 <= K <= SAE_COLLECT_MAX_K, 1 <= n_dict <= 2^30.  A slot is POSTED iff its value is not +-0.0 and its index lies in
 * [0, n_dict); an index outside is counted and never used as an address.  The position of row r of a batch is pos0 + r
 * (pos0 = file0 * T), below 2^32.
 *
 * sae_findex_count (sweep 1): totals_dev int64 [n_dict] += the batch's posted slots per latent; stats_dev int64
 *   [SAE_FINDEX_NSTATS] += [0] slots seen, [1] zero slots skipped, [2] non-zero slots with an index outside [0, n_dict),
 *   [3] slots posted; [4..7] reserved.  Integer adds only: order-free.  The caller zeroes both before the first batch.
 * sae_findex_fill (sweep 2), for a latent range [j0, j1): cursor_dev int64 [n_dict] holds every list's next free slot (absolute:
 *   it starts at the exclusive prefix sum of the totals).  Each posted slot of a latent j of the range is written to
 *   positions_out_dev / values_out_dev [cursor[j] - out_base + r], r = its rank among the batch's slots of latent j in row order,
 *   as (pos0 + row, the stored value bits); then cursor[j] advances by the batch's count.  out_base = the first slot of list j0,
 *   capacity = the slots the two buffers hold (< 2^32 - 1); a place at or beyond capacity is not written and counted in
 *   err_dev[1].  The place follows from the data alone (findex.h: Determinism); no float atomics, no returning global atomics.
 *   workspace_dev: sae_findex_workspace_bytes(rows, j1 - j0) bytes, 4-byte aligned, scratch (no state is kept in it between calls).
 * sae_findex_verify: over the finished lists of [j0, j1) (starts_dev int64 [n_dict + 1], absolute), err_dev[0] += the slots whose
 *   position is not strictly greater than the one before it in its list or is >= limit (= n_files * T).  Non-zero means that a
 *   row of the store repeats an index.  err_dev: int64 [2], zeroed by the caller.
 * sae_findex_workspace_bytes: bytes of workspace for batches of at most max_rows rows and a range of n_range latents; -1 for
 *   arguments out of range. */
enum { SAE_FINDEX_IDX32 = 1 };
#define SAE_FINDEX_NSTATS 8
int64_t sae_findex_workspace_bytes(int64_t max_rows, int64_t n_range);
int sae_findex_count(const float* values_dev, const void* indices_dev, int64_t rows, int K, int flags, int64_t n_dict, int64_t* totals_dev,
                     int64_t* stats_dev, void* stream);
int sae_findex_fill(const float* values_dev, const void* indices_dev, int64_t rows, int K, int flags, int64_t n_dict, int64_t j0, int64_t j1,
                    int64_t pos0, int64_t* cursor_dev, int64_t out_base, uint32_t* positions_out_dev, float* values_out_dev,
                    int64_t capacity, void* workspace_dev, int64_t workspace_bytes, int64_t* err_dev, void* stream);
int sae_findex_verify(const int64_t* starts_dev, int64_t n_dict, int64_t j0, int64_t j1, int64_t out_base, const uint32_t* positions_dev,
                      int64_t capacity, int64_t limit, int64_t* err_dev, void* stream);

/* ---- Dead-latent resampling for L1 training: revive latents that never fire from the inputs the dictionary reconstructs worst
 * (Bricken et al. 2023, "Towards Monosemanticity", neuron resampling; freud_amd/resample.py; kernels: freud_amd/csrc/resample.h, the
 * arithmetic: freud_amd/csrc/resample_draw.h).  L1 contexts in bf16 precision only: a TopK context is refused (it has AuxK,
 * auxk_alpha), an fp8 context is refused as by every file pass.
 *
 * The rule.  Over the rows i = file * T + frame of a set of files:
 *   dead set   latent j < n_dict is dead iff its firing count over the counted frames is 0 (firing as in sae_stats_files: the bf16
 *              latent's magnitude bits are non-zero); padding columns are never in the set;
 *   row loss   l_i = sum_k r_k^2, r = float(x) - x_hat with x_hat the decode of the forward's own latent, exactly as sae_recon_files
 *              defines it (an element equal to -1 is data): the fp32 sum, in ascending order, of the residual sweep's partials per 64
 *              columns; l_i = 0 on rows that do not count;
 *   weights    l_max = the maximum row loss (the losses are non-negative: the maximum of the bit patterns), e = its frexp exponent,
 *              q_i = floor(l_i 2^(16 - e)) in [0, 65535], w_i = q_i^2 (uint64): p proportional to the loss squared; c_i = the inclusive
 *              uint64 prefix, total = c_last (rows < 2^31: no overflow); total == 0: nothing is resampled;
 *   draw       dead latents in ascending order r = 0 .. |D| - 1: h = rs_hash(seed, round, r) (three splitmix64 finalisers), t =
 *              mulhi64(h, total), row = the first i with c_i > t.  Nothing depends on how the rows were batched or on a rank;
 *   distinct   of the latents that drew one row the lowest r owns it; the others stay dead this round (skipped_duplicate);
 *   column     x = the drawn shard row widened to fp32: s = fmaf-accumulated sum x_k^2 (k ascending), nrm = sqrt(s), W[:, j] = x / nrm,
 *              b_j = -((1 - alpha) nrm), each one correctly rounded fp32 operation: the seed frame then activates at alpha |x|.
 *              s == 0 or not finite: the pair is skipped (skipped_degenerate);
 *   optimizer  exp_avg and exp_avg_sq of column j of W and of b_j are set to 0; the step count is untouched.
 *
 * sae_resample_files: one batch (x_dev [n_files][rows_per_file][d], x_dtype; lengths_dev or null) -- the encoder with the stored
 *   latent, the count reduction of sae_stats_files' stored-latent path, the decoder GEMM and the residual sweep of sae_recon_files,
 *   and NOT its attribution GEMM.  Writes the batch's row losses to row_loss_dev [n_files * rows_per_file] (the caller passes its
 *   array + the batch's first row) and adds the firing counts to fire_count_dev int64 [n_dict] (zeroed by the caller before the
 *   first batch).  Argument rules, limits, scratch, the state it leaves and what it does not touch: as sae_recon_files.  Two runs
 *   give the same bytes.
 * sae_resample_select: context-free, like sae_search_merge; all pointers caller-owned device memory.  From row_loss_dev [rows]
 *   (1 <= rows < 2^31) and fire_count_dev [n] (1 <= n <= 2^24): the applying pairs in ascending latent order in latents_out_dev
 *   int32 [n] / rows_out_dev int64 [n] (the first counts[SAE_RESAMPLE_PAIRS] entries), and counts_out_dev int64
 *   [SAE_RESAMPLE_NCOUNTS]: DEAD, PAIRS, SKIPPED_DUPLICATE, TOTAL (the uint64 total), LMAX_BITS (the fp32 bits of l_max).
 *   workspace_dev: sae_resample_workspace_bytes(rows, n) bytes (-1: arguments out of range), 8-byte aligned scratch.  Integer
 *   arithmetic only; the atomics are an integer maximum and an integer minimum whose results do not depend on order.
 * sae_resample_apply: rewrites column latents_dev[i] (int32 [n_latents], device) of W, b and both moments from x_rows_dev
 *   [n_latents][d] fp32, inside the engine: the fp32 master is settled first (d_model <= 384: a training step may have left it
 *   un-normalised), every derived copy is rebuilt by the next forward exactly as after sae_set_params, and nothing else of the
 *   training state changes.  A latent outside [0, n_dict), a repeated latent, a TopK or fp8 context, alpha outside [0, 1]:
 *   SAE_ERR_INVALID before anything is written (the latents are read back first: the call synchronises `stream`).  out_stats_dev
 *   int64 [2 + n_latents], written: [0] revived, [1] skipped_degenerate, [2 + i] = 1 iff pair i was applied. */
enum { SAE_RESAMPLE_DEAD = 0, SAE_RESAMPLE_PAIRS = 1, SAE_RESAMPLE_SKIPPED_DUPLICATE = 2, SAE_RESAMPLE_TOTAL = 3, SAE_RESAMPLE_LMAX_BITS = 4,
       SAE_RESAMPLE_NCOUNTS = 8 };
int sae_resample_files(sae_ctx* ctx, const void* x_dev, int64_t n_files, int64_t rows_per_file, int x_dtype, const int32_t* lengths_dev,
                       float* row_loss_dev, int64_t* fire_count_dev, void* stream);
int64_t sae_resample_workspace_bytes(int64_t rows, int64_t n);
int sae_resample_select(const float* row_loss_dev, int64_t rows, const int64_t* fire_count_dev, int64_t n, uint64_t seed, uint64_t round,
                        int32_t* latents_out_dev, int64_t* rows_out_dev, int64_t* counts_out_dev, void* workspace_dev, int64_t workspace_bytes,
                        void* stream);
int sae_resample_apply(sae_ctx* ctx, const int32_t* latents_dev, int64_t n_latents, const float* x_rows_dev, double alpha,
                       int64_t* out_stats_dev, void* stream);

/* ---- Input statistics: the moments and the geometric median of a sample of activation rows, before any dictionary exists
 * (freud_amd/input_stats.py; kernels: freud_amd/csrc/input_stats.h).  Context-free like sae_search_raw_files: no SAE, the current
 * device, all pointers caller-owned device memory.  The sample is resident as x_dev [n_files][rows_per_file][d] (x_dtype); lengths_dev
 * as for the file passes (int32 [n_files] or NULL = T; only the first min(length, T) frames of a file count, a length below 1 counts
 * as 1).  N = the counted frames.  1 <= d <= SAE_INPUT_MAX_D, n_files and rows_per_file within the file passes' limits.
 *
 * sae_input_stats_workspace_bytes: the scratch both calls need (-1: arguments out of range); 8-byte aligned.
 * sae_input_moments: two sweeps.  out_dev, double [4 d + 2]: mean [d] | the centred sum of squares sum_i (x_i - mean)^2 [d] (a second
 *   sweep with the fp64 mean, not E[x^2] - mean^2) | min [d] | max [d] (exact) | sum_i |x_i|^2 | N.  All sums are fp64.
 * sae_input_median: Weiszfeld's iteration with a fixed count, from start_dev (double [d]; the mean, for the documented rule):
 *   dist_i = |x_i - m_k|, w_i = 1 / max(dist_i, floor), m_{k+1} = sum w_i x_i / sum w_i, J_k = sum dist_i / N.  x_i - m_k is formed from
 *   the fp64 estimate with one rounding to fp32; the squared distance, its root and w are fp32 (a fixed summation order); the three
 *   sums are fp64.  path_dev, double [iterations + 1][d]: m_0 (= start) .. m_I; objective_dev, double [iterations + 1]: J_0 .. J_I
 *   (iterations + 1 sweeps: the last one evaluates J at m_I).  FLT_MIN <= floor <= FLT_MAX, 1 <= iterations <=
 *   SAE_INPUT_MAX_ITERATIONS.  No convergence test and no host synchronisation between the iterations: asynchronous on `stream`.
 *
 * Every partial sum belongs to a fixed unit (a file and a block of 256 of its frames) and the units are added in ascending order on
 * the device: the results are a function of (x, lengths, iterations) alone, not of the grid or the device's size; no atomics; two
 * calls give the same bytes.  Null pointers, a shape, d, dtype, floor or iteration count out of range, a short or misaligned
 * workspace: SAE_ERR_INVALID before anything is enqueued. */
#define SAE_INPUT_MAX_D 2048
#define SAE_INPUT_MAX_ITERATIONS 1024
int64_t sae_input_stats_workspace_bytes(int64_t n_files, int64_t rows_per_file, int64_t d);
int sae_input_moments(const void* x_dev, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths_dev,
                      double* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);
int sae_input_median(const void* x_dev, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths_dev,
                     const double* start_dev, double floor, int iterations, double* path_dev, double* objective_dev, void* workspace_dev,
                     int64_t workspace_bytes, void* stream);

/* ---- Input covariance: the centred scatter of the same sample, the matrix whose diagonal sae_input_moments gives
 * (freud_amd/input_pca.py; kernels: freud_amd/csrc/input_cov.h, the decomposition: freud_amd/csrc/input_cov_plan.h).  Context-free;
 * x_dev, lengths_dev, the counted frames, N and the limits are those of sae_input_moments.
 *
 * The rule.  The operand of a counted frame k, column i is a_ki = double(x_ki) - c_i with c = center_dev (double [d]; NULL = zeros: the
 * raw second moment): the conversion is exact and the subtraction rounds once.  A frame that is not counted contributes a zero
 * operand, not 0 - c_i.  out_dev, double [d][d]: S_ij = sum_k a_ki a_kj, accumulated in fp64 (every product fused into its add),
 * NOT divided by N; the whole matrix is written and the lower triangle is the bit-for-bit mirror of the upper.
 *
 * The work splits into the output tiles on or above the diagonal and into segments, fixed runs of consecutive 256-frame units; a
 * workgroup adds its segment's frames in ascending order and a second kernel adds a tile's segments in ascending order.  So S is a
 * function of (x, lengths, c) alone, not of the grid, the device's size, the stream or what the workspace held; no atomics; two calls
 * give the same bytes.
 * sae_input_cov_workspace_bytes: the segments' partials (-1: arguments out of range), at most 64 MiB; 8-byte aligned.
 * sae_input_cov_plan: out[4] = the tile edge | the tiles computed | the segments | the units per segment: functions of
 *   (n_files, rows_per_file, d) alone.
 * sae_input_cov: asynchronous on `stream`, no host synchronisation.  Null x / out / workspace, a shape, d or dtype out of range, a
 *   short or misaligned workspace: SAE_ERR_INVALID before anything is enqueued. */
int64_t sae_input_cov_workspace_bytes(int64_t n_files, int64_t rows_per_file, int64_t d);
int sae_input_cov_plan(int64_t n_files, int64_t rows_per_file, int64_t d, int64_t out[4]);
int sae_input_cov(const void* x_dev, int64_t n_files, int64_t rows_per_file, int64_t d, int x_dtype, const int32_t* lengths_dev,
                  const double* center_dev, double* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* ---- The HBM-resident activation store (freud_amd/resident.py): a shard directory uploaded once as one device array
 * store [n_files][row_bytes], and every batch drawn from it on the device instead of over the host link.
 *
 * sae_store_convert: dst_dev[i] = bf16(src_dev[i]) for i < n_elems, by the rule of the loader's host conversion
 *   (freud_amd/csrc/bf16_guard.h; freud_amd/csrc/host_convert.c): round to nearest even; a NaN stays a quiet NaN
 *   ((u >> 16) | 0x40); a value that is not -1.0 but would round to 0xBF80 goes to 0xBF81 or 0xBF7F, because exactly -1.0 is the
 *   reference's mask value.  src 4-byte and dst 2-byte aligned; both 16-byte aligned take the vector form.  n_elems >= 0.
 * sae_store_gather: out_dev[j] = store_dev[idx_dev[j]] for j < nb, rows of row_bytes bytes, row j of the destination at
 *   out_dev + j * out_stride_bytes (out_stride_bytes >= row_bytes; the bytes between rows are left as they are).  A byte copy: it
 *   serves stores of any element type.  The store, the destination, row_bytes and out_stride_bytes must be multiples of 2 bytes;
 *   multiples of 16 take the 16-byte form, of 4 the 4-byte form.  One workgroup copies one piece of sae_store_piece_bytes() bytes
 *   of one row; nb * ceil(row_bytes / piece) <= 2^31 - 1.  An index outside [0, n_files) is clamped into it -- nothing outside the
 *   store is ever read -- and *err_dev (uint32, never cleared by the call) is incremented once per such batch row: the caller
 *   validates its index lists on the host and reads the word as the second line.
 * Both need no context, run on the current device, are asynchronous on `stream` and return SAE_ERR_INVALID for an argument outside
 * the above before anything is enqueued. */
int64_t sae_store_piece_bytes(void);
int sae_store_convert(const float* src_dev, void* dst_dev, int64_t n_elems, void* stream);
int sae_store_gather(const void* store_dev, int64_t n_files, int64_t row_bytes, const int32_t* idx_dev, int64_t nb, void* out_dev,
                     int64_t out_stride_bytes, uint32_t* err_dev, void* stream);

/* ---- Frame batches (freud_amd/resident.py, ResidentFrameDataLoader; freud_amd/csrc/frame_perm.h, frame_gather.h): a batch of
 * FRAMES of the resident store, drawn through a permutation that is evaluated in the kernel, not stored.
 *
 * The store is store_dev [n_files][rows_per_file][frame_bytes].  Its COUNTED frames are numbered g = 0 .. n_frames - 1 in file
 * order: all rows_per_file frames of every file (prefix_dev NULL; n_frames = n_files * rows_per_file), or the first len[f] frames
 * of file f (prefix_dev = int64 [n_files + 1], the exclusive prefix sum of the lengths, 1 <= len[f] <= rows_per_file,
 * prefix_dev[n_files] = n_frames; device memory, 8-byte aligned).  An epoch is fp_permute(key, n_frames, .) of frame_perm.h, an
 * exact bijection of [0, n_frames) for every key.
 *
 * sae_store_gather_frames: for j < rows, row j of the destination (out_dev + j * out_stride_bytes, out_stride_bytes >=
 *   frame_bytes, the bytes between rows left as they are) = the frame_bytes of counted frame fp_permute(key, n_frames, pos0 +
 *   j * pos_stride).  A byte copy: it serves stores of any element type.  ordinals_out_dev (NULL, or int64 [rows], 8-byte
 *   aligned) receives the frame's row in the store's [n_files * rows_per_file, frame_bytes] view, file * rows_per_file + t -- the
 *   counted ordinal itself when prefix_dev is NULL.  The store, the destination, frame_bytes and out_stride_bytes must be
 *   multiples of 2 bytes; multiples of 16 take the 16-byte form, of 4 the 4-byte form.  SAE_ERR_INVALID before anything is enqueued
 *   for: a null store, destination or error word; n_files, rows_per_file or frame_bytes outside [1, 2^31 - 1]; n_frames < 1 or
 *   > n_files * rows_per_file; rows < 0; with rows > 0, pos0 outside [0, n_frames), pos_stride < 1 or pos0 + (rows - 1) *
 *   pos_stride >= n_frames; out_stride_bytes < frame_bytes; addresses and sizes that admit no copy width.  rows == 0 succeeds and
 *   launches nothing.  The prefix is read on the device and cannot be checked here: a frame that a malformed prefix places
 *   outside the store is clamped into it -- nothing outside the store is ever read -- and *err_dev (uint32, never cleared by the
 *   call) is incremented once per such row.  Needs no context, runs on the current device, asynchronous on `stream`. */
int sae_store_gather_frames(const void* store_dev, int64_t n_files, int64_t rows_per_file, int64_t frame_bytes, const int64_t* prefix_dev,
                            int64_t n_frames, uint64_t key, int64_t pos0, int64_t pos_stride, int64_t rows, void* out_dev,
                            int64_t out_stride_bytes, int64_t* ordinals_out_dev, uint32_t* err_dev, void* stream);

/* Test / inspection hook: copy an internal tensor of the last step to host as fp32, un-padded.
 * which: 0 = latent c [M][n]; 1 = x_hat-derived dx_hat [M][d]; 2 = raw gradients in reference
 * layouts, concatenated in parameter order; 14 = the multi-TopK pass's d (decoder output) [M][d] of the last training forward, as
 * the sparse backward reads it (bf16 values; SAE_ERR_INVALID unless the context is TopK with multi_topk, SAE_ERR_STATE after an fp32
 * evaluation, like 1); 15 = the L1 weights as the kernels read them, bf16 Wt[n_p][d_p] widened to [n][d] (SAE_ERR_INVALID for a
 * TopK context).  Synchronising.  Not part of the hot path. */
int sae_debug_read(sae_ctx* ctx, int which, float* out_host, int64_t capacity_floats);

/* Test / inspection hook: the launch plan of the L1 weight gradient for a batch of M rows (1 <= M <= max_rows), nothing is launched.
 * out_host = {form (0 = fused d = 384, 1 = fused in column ranges, 2 .. 6 = the GEMM forms), splits (row ranges / split-K slabs),
 * balanced (0 / 1), bal_m (quanta per workgroup), bal_q (32-row steps per quantum), grid (workgroups of the fused backward, 0 for the
 * GEMM forms), M_p / 32, n_p / 128}; bal_m and bal_q are 0 unless balanced.  SAE_ERR_INVALID for TopK and fp8 contexts. */
int sae_l1_backward_plan(sae_ctx* ctx, int64_t M, int32_t out_host[8]);

/* Timing hooks for bench.py / profiling.  level 0 = off, 1 = bracket only the dominant kernel of
 * every step with HIP events on the launch stream, 2 = bracket every kernel (diagnostic).
 * sae_kernel_times synchronises, adds up the events recorded since the last call (at most the last
 * 64 launches per kernel are kept) and returns per-kernel total milliseconds and launch counts for
 * kernel ids 0..n-1 (ids: sae_kernel_name).  Level 1 samples every 8th step: an event record costs ~6 us of idle GPU
 * between two dependent kernels, which at three records per 0.6 ms step was 3 % of the thing being measured. */
int sae_profile(sae_ctx* ctx, int level);
int sae_profile_period(sae_ctx* ctx, int period);   /* level 1 samples every `period`-th step (default 8; short runs use less) */
int sae_kernel_times(sae_ctx* ctx, float* ms_sum, int32_t* launches, int n);
const char* sae_kernel_name(int id);        /* NULL past the last id */
int sae_dominant_kernel(sae_ctx* ctx);      /* id bracketed at level 1 */

#ifdef __cplusplus
}
#endif
#endif /* FREUD_SAE_H */
