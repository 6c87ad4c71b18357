"""GPU: dead-latent resampling (freud_amd/resample.py over include/freud_sae.h's sae_resample_*; freud_amd/csrc/resample.h).

Shapes: 10 files of T = 100 frames with ragged lengths, batches of 3 files (four batches, the last one ragged; 1000 rows: four scan
blocks of 256), n = 200 latents (n_p = 256: padding columns exist), d = 384 (the folded d <= 384 update: wn_pending) and d = 512 (the
generic path).  Every fourth latent is planted dead with b_j = -1e4.  The d = 384 data are small frames with three files of zero
frames (a zero frame has a loss where biases are positive: degenerate rows get drawn); the d = 512 data carry one frame 300 times
larger than the rest (nearly all the loss: the dead latents collide on it).

L1 weights: columns of exactly unit norm (tests/test_reconstruction_gpu.py's family), so the in-place renormalisation every L1
forward starts with is a bit-exact fixed point and every pass over the untrained dictionary sees the same weights.

1. row loss against the float64 sum of sae_recon_files' residual within d 2^-23 sum r^2, exactly 0 on uncounted rows, bitwise equal
   across two runs; fire counts equal to sae_stats_files';
2. the selection against the host reference (tests/resample_reference.py) from the device's own row losses and counts;
3. apply after one training step: untouched columns and moments, revived columns / biases / zeroed moments against the host
   reference to the bit; the next step() equal to that of a fresh engine loaded with the same state; two engines bit-identical;
4. the effect: every revived latent fires afterwards; 5. train() with the key: fewer dead, finite losses, resume bitwise; 6. refusals."""
import json
import os

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd.feature_stats import feature_stats
from freud_amd.loader import write_shards
from freud_amd.resample import resample_dead_latents
from tests import resample_reference as REF

pytestmark = pytest.mark.gpu

N, F, T, BATCH, LR = 200, 10, 100, 3, 1e-3
LENGTHS = np.array([100, 37, 100, 64, 1, 100, 99, 73, 100, 50], dtype=np.int32)
PLANTED = np.arange(1, N, 4)                       # 50 latents with b = -1e4
BIG = (7, 33)                                      # d = 512: the frame that holds nearly all the loss (inside file 7's 73 frames)
SEED, ROUND = 5, 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def weights(d, seed):
    g = np.random.default_rng(seed)
    W = np.zeros((d, N), np.float32)
    for j in range(N):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    b = g.normal(0, 0.3, N).astype(np.float32)
    b[PLANTED] = -1e4
    return W, b


def data(d):
    g = np.random.default_rng(100 + d)
    if d == 384:
        x = (0.05 * g.normal(0, 1, (F, T, d))).astype(np.float32)
        x[2:5] = 0
    else:
        x = g.normal(0, 1, (F, T, d)).astype(np.float32)
        x[BIG] *= 300
    return x


def fresh(d, W, b):
    eng = E.SaeEngine("l1", d, N, BATCH * T, optimizer="radam", recon_alpha=100.0)
    eng.set_params({"decoder.weight": W, "encoder_bias": b})
    return eng


def snapshot(eng):
    step, m1, m2 = eng.get_opt_state()
    return {"step": step, "params": eng.get_params(), "m1": m1, "m2": m2}


def assert_bitwise(a, b):
    assert a["step"] == b["step"]
    for grp in ("params", "m1", "m2"):
        for k in a[grp]:
            assert np.array_equal(bits(a[grp][k]), bits(b[grp][k])), (grp, k)


def batches(x):
    lens = torch.from_numpy(LENGTHS).cuda()
    for f0 in range(0, F, BATCH):
        f1 = min(f0 + BATCH, F)
        yield f0, f1, torch.from_numpy(x[f0:f1]).cuda(), lens[f0:f1]


def walk_resample(eng, x, fire=None):
    row_loss = torch.full((F * T,), float("nan"), device="cuda")
    fire = torch.zeros(N, dtype=torch.int64, device="cuda") if fire is None else fire
    for f0, _f1, xb, lb in batches(x):
        eng.resample_files(xb, row_loss, f0 * T, fire, lb)
    torch.cuda.synchronize()
    return row_loss, fire


class Case:
    pass


@pytest.fixture(scope="module", params=[384, 512])
def case(request, tmp_path_factory):
    """Everything the device computes for one d, once: the passes, the selection, the apply, the step after it."""
    d = request.param
    c = Case()
    c.d, c.x = d, data(d)
    c.W, c.b = weights(d, d)
    c.counted = (np.arange(T)[None, :] < LENGTHS[:, None]).reshape(-1)
    c.folder = str(tmp_path_factory.mktemp(f"shards{d}"))
    write_shards(c.folder, "enc", c.x.reshape(F, T * d), [T, d])

    # -- the passes over the untrained dictionary
    eng = fresh(d, c.W, c.b)
    rl, fire = walk_resample(eng, c.x)
    rl2, fire2 = walk_resample(eng, c.x)
    c.row_loss, c.row_loss_again, c.fire, c.fire_again = rl.cpu().numpy(), rl2.cpu().numpy(), fire.cpu().numpy(), fire2.cpu().numpy()
    resid = torch.zeros(F, T, d, device="cuda")
    block = torch.zeros(E.recon_layout(N, d)["bytes"], dtype=torch.uint8, device="cuda")
    file_out = torch.zeros(F, 2, dtype=torch.float64, device="cuda")
    sblock = torch.zeros(E.stats_layout(N)["bytes"], dtype=torch.uint8, device="cuda")
    for f0, f1, xb, lb in batches(c.x):
        eng.recon_files(xb, block, file_out[f0:f1], lb, resid=resid[f0:f1])
        eng.stats_files(xb, sblock, lb)
    torch.cuda.synchronize()
    c.resid = resid.cpu().numpy().reshape(F * T, d)
    c.stats_fire = E.unpack_block(sblock.cpu().numpy(), E.stats_layout(N))["fire_count"]
    c.after_pass_error = None
    try:
        eng.metrics()
    except E.EngineError as e:
        c.after_pass_error = str(e)
    c.fire_twice = walk_resample(eng, c.x, fire2)[1].cpu().numpy()    # (the counts add up; the last call is the resampling pass again)
    try:
        eng.metrics()
        c.last_call_error = None
    except E.EngineError as e:
        c.last_call_error = str(e)
    c.params_after_passes = eng.get_params()

    # -- the selection on the device
    lat = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    rows = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(E.RESAMPLE_NCOUNTS, dtype=torch.int64, device="cuda")
    ws = torch.empty(E.resample_workspace_bytes(F * T, N), dtype=torch.uint8, device="cuda")
    E.resample_select(rl, F * T, fire, N, SEED, ROUND, lat, rows, counts, ws)
    rows2 = rows.clone()
    E.resample_select(rl, F * T, fire, N, SEED, ROUND + 1, lat.clone(), rows2, counts.clone(), ws)
    torch.cuda.synchronize()
    c.counts = counts.cpu().numpy()
    pairs = int(c.counts[E.RESAMPLE_PAIRS])
    c.sel_lat, c.sel_rows, c.sel_tail = lat.cpu().numpy()[:pairs], rows.cpu().numpy()[:pairs], lat.cpu().numpy()[pairs:]
    c.sel_rows_next_round = rows2.cpu().numpy()
    eng.close()

    # -- apply after ONE training step (d = 384: the folded update has left the master un-normalised, wn_pending holds)
    xb = torch.from_numpy(c.x[0:3]).cuda()
    ref_eng = fresh(d, c.W, c.b)
    ref_eng.step(xb, LR)
    c.before = snapshot(ref_eng)                                       # (the getters settle this engine: it is not used again)
    ref_eng.close()
    eng = fresh(d, c.W, c.b)
    eng.step(xb, LR)
    dead = np.flatnonzero(c.fire == 0)
    extra = int([j for j in dead if j not in set(c.sel_lat.tolist())][0])          # one more dead latent, given a zero frame
    c.ap_lat = np.concatenate([c.sel_lat, [extra]]).astype(np.int32)
    c.ap_rows = np.concatenate([c.x.reshape(F * T, d)[c.sel_rows], np.zeros((1, d), np.float32)]).astype(np.float32)
    c.alpha = 0.2
    out_stats = torch.full((2 + len(c.ap_lat),), -7, dtype=torch.int64, device="cuda")
    eng.resample_apply(torch.from_numpy(c.ap_lat).cuda(), torch.from_numpy(c.ap_rows).cuda(), c.alpha, out_stats)
    torch.cuda.synchronize()
    c.out_stats = out_stats.cpu().numpy()
    c.after = snapshot(eng)
    # -- the next step against a fresh engine loaded with the same state
    x2 = torch.from_numpy(c.x[5:8]).cuda()
    eng.step(x2, LR)
    c.next_metrics = eng.metrics()
    c.next = snapshot(eng)
    eng.close()
    loaded = fresh(d, c.W, c.b)
    loaded.set_params(c.after["params"])
    loaded.set_opt_state(c.after["step"], c.after["m1"], c.after["m2"])
    loaded.step(x2, LR)
    c.loaded_metrics = loaded.metrics()
    c.loaded_next = snapshot(loaded)
    loaded.close()
    return c


# ---- 1. the pass ---------------------------------------------------------------------------------------------------------------
def test_row_loss_against_the_residual_of_the_reconstruction_pass(case):
    want = (case.resid.astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(case.row_loss.astype(np.float64) - want)
    bound = case.d * 2.0 ** -23 * want
    worst = int(np.argmax(err - bound))
    print(f"d={case.d}: largest |l - sum r^2| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3e} at row {worst}")
    assert np.isfinite(case.row_loss).all() and (err <= bound).all()
    assert (want[case.counted] > 0).all() and not bits(case.row_loss)[~case.counted].any()        # exactly +0 where a row does not count


def test_row_loss_and_counts_are_bitwise_reproducible(case):
    assert np.array_equal(bits(case.row_loss), bits(case.row_loss_again))
    np.testing.assert_array_equal(case.fire_again, case.fire)
    np.testing.assert_array_equal(case.fire_twice, 2 * case.fire)                                  # (the counts add up over the calls)


def test_fire_counts_equal_the_statistics_pass(case):
    np.testing.assert_array_equal(case.fire, case.stats_fire)
    assert not case.fire[PLANTED].any() and (case.fire > 0).sum() >= N // 2


def test_the_pass_leaves_a_file_pass_state_and_the_parameters(case):
    assert case.after_pass_error and "run sae_eval first" in case.after_pass_error
    assert case.last_call_error and "a resampling pass" in case.last_call_error
    assert np.array_equal(bits(case.params_after_passes["decoder.weight"]), bits(case.W))
    assert np.array_equal(bits(case.params_after_passes["encoder_bias"]), bits(case.b))


# ---- 2. the selection ----------------------------------------------------------------------------------------------------------
def test_selection_equals_the_host_reference(case):
    lat, rows, counts = REF.select(case.row_loss, case.fire, SEED, ROUND)
    np.testing.assert_array_equal(case.counts, counts)
    np.testing.assert_array_equal(case.sel_lat, lat)
    np.testing.assert_array_equal(case.sel_rows, rows)
    assert (case.sel_tail == -1).all()                                       # nothing is written past the pairs
    assert case.counts[E.RESAMPLE_DEAD] == (case.fire == 0).sum() >= len(PLANTED)
    assert (case.sel_lat < N).all() and case.counted[case.sel_rows].all() and len(set(case.sel_rows.tolist())) == len(case.sel_rows)
    assert case.counts[E.RESAMPLE_LMAX_BITS] == int(bits(case.row_loss).max())
    if case.d == 384:                                                        # another round draws other rows
        assert len(case.sel_rows) > 4 and not np.array_equal(case.sel_rows_next_round[:len(case.sel_rows)], case.sel_rows)
    zero_rows = ~case.x.reshape(F * T, case.d)[case.sel_rows].any(axis=1)
    if case.d == 512:
        # the planted collision: the lowest dead latent owns the big frame, (nearly) everybody else drew it too
        assert case.sel_rows[0] == BIG[0] * T + BIG[1] and case.sel_lat[0] == np.flatnonzero(case.fire == 0)[0]
        assert case.counts[E.RESAMPLE_SKIPPED_DUPLICATE] >= case.counts[E.RESAMPLE_DEAD] - 3
    else:
        assert zero_rows.any()                                               # planted zero frames were drawn


# ---- 3. apply ------------------------------------------------------------------------------------------------------------------
def test_apply_rewrites_exactly_the_chosen_columns(case):
    b, a = case.before, case.after
    (W, bias, m1W, m1b, m2W, m2b), applied = REF.apply_columns(
        b["params"]["decoder.weight"], b["params"]["encoder_bias"], b["m1"]["decoder.weight"], b["m1"]["encoder_bias"],
        b["m2"]["decoder.weight"], b["m2"]["encoder_bias"], case.ap_lat, case.ap_rows, case.alpha)
    assert not applied[-1] and applied.any()                                 # the zero frame is degenerate
    assert case.out_stats[0] == applied.sum() and case.out_stats[1] == (~applied).sum()
    np.testing.assert_array_equal(case.out_stats[2:] != 0, applied)
    assert a["step"] == b["step"] == 1
    for got, want, name in [(a["params"]["decoder.weight"], W, "W"), (a["params"]["encoder_bias"], bias, "b"),
                            (a["m1"]["decoder.weight"], m1W, "exp_avg W"), (a["m1"]["encoder_bias"], m1b, "exp_avg b"),
                            (a["m2"]["decoder.weight"], m2W, "exp_avg_sq W"), (a["m2"]["encoder_bias"], m2b, "exp_avg_sq b")]:
        assert np.array_equal(bits(got), bits(want)), name
    done = case.ap_lat[applied]
    keep = np.ones(N, bool)
    keep[done] = False
    # untouched: bit-equal to the state before; revived: unit columns, the bias of the rule, zero moments
    assert np.array_equal(bits(a["params"]["decoder.weight"][:, keep]), bits(b["params"]["decoder.weight"][:, keep]))
    assert np.array_equal(bits(a["m2"]["decoder.weight"][:, keep]), bits(b["m2"]["decoder.weight"][:, keep]))
    assert b["m2"]["decoder.weight"][:, keep].any() and not a["m2"]["decoder.weight"][:, done].any() and not a["m1"]["encoder_bias"][done].any()
    np.testing.assert_allclose(np.linalg.norm(a["params"]["decoder.weight"][:, done].astype(np.float64), axis=0), 1.0, atol=1e-6)
    assert (a["params"]["encoder_bias"][done] < 0).all() and (a["params"]["encoder_bias"][done] > -1e4).all()          # not the planted -1e4


def test_next_step_equals_a_fresh_engine_with_the_same_state(case):
    """Every cached copy of the weights (the bf16 operands, the column norms and their partials, the pending normalisation) was
    invalidated: the engine that was rewritten in place and one that was loaded with its state take the same step, to the bit."""
    assert_bitwise(case.next, case.loaded_next)
    assert np.array_equal(bits(case.next_metrics), bits(case.loaded_metrics))
    assert case.next["step"] == 2 and np.isfinite(case.next["params"]["decoder.weight"]).all()


# ---- 3b / 4. two engines, the report, the effect ----------------------------------------------------------------------------------
def test_two_engines_end_bit_identical_and_revived_latents_fire(case):
    d = case.d
    xb = torch.from_numpy(case.x[0:3]).cuda()
    engs, reports = [], []
    for _ in range(2):
        eng = fresh(d, case.W, case.b)
        eng.step(xb, LR)
        state = torch.get_rng_state()
        reports.append(resample_dead_latents(eng, case.folder, "enc", files=F, seed=SEED, round=ROUND, lengths=LENGTHS, batch_files=BATCH))
        assert torch.equal(state, torch.get_rng_state())
        engs.append(eng)
    a, b = reports
    assert a.summary() == b.summary()
    for k in ("latents", "files", "frames"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert engs[0].param_checksum() == engs[1].param_checksum()            # what the replica guard of train() compares
    assert_bitwise(snapshot(engs[0]), snapshot(engs[1]))
    print(f"d={d}: {a.summary()}")
    assert a.dead >= len(PLANTED) and a.revived >= 1 and a.n_frames == int(LENGTHS.sum())
    assert a.revived + a.skipped_duplicate + a.skipped_degenerate == a.dead
    assert (a.latents < N).all() and (np.diff(a.latents) > 0).all() and (a.frames < LENGTHS[a.files]).all()
    assert case.x[a.files, a.frames].any(axis=1).all()                       # no revived latent was seeded from a zero frame
    assert a.l_max > 0 and 0 < a.mean_row_loss <= a.l_max
    if d == 384:
        assert a.skipped_degenerate >= 1
    # the effect: every revived latent fires on at least one frame of the same files
    st = feature_stats(engs[0], case.folder, "enc", lengths=LENGTHS, subset_size=F, batch_files=BATCH)
    assert (st.fire_count[a.latents] > 0).all()
    for eng in engs:
        eng.close()


# ---- 5. train() ---------------------------------------------------------------------------------------------------------------
def _train_cfg(tmp_path, run, **over):
    d, T_, n_files = 384, 64, 16
    g = torch.Generator().manual_seed(3)
    rows = ((torch.relu(torch.randn(n_files * T_, 16, generator=g)) * 0.2) @ torch.randn(16, d, generator=g)).reshape(n_files, T_ * d)
    folder = os.path.join(str(tmp_path), "train")
    if not os.path.isdir(folder):
        write_shards(folder, "enc", rows.numpy(), [T_, d])
    cfg = {"whisper_config": {"model": "tiny", "layer_name": "enc"}, "seed": 0, "train_folder": folder, "val_folder": folder,
           "device": "cuda", "lr": 1e-3, "weight_decay": 0.0, "steps": 40, "clip_thresh": 1.0, "dl_max_workers": 0, "log_tb_every": 5,
           "save_every": 20, "val_every": 1000, "scheduler_params": {}, "start_checkpoint": None, "from_disk": True, "batch_size": 2,
           "run_dir": os.path.join(str(tmp_path), run), "autoencoder_variant": "l1", "optimizer": "radam", "scheduler": "cosine",
           "autoencoder_config": {"n_dict_components": 512, "recon_alpha": 100.0}, "resample": {"every": 10}}
    cfg.update(over)
    return cfg


def _planted_checkpoint(tmp_path, cfg):
    """A step-0 checkpoint whose model has every fourth latent planted dead (b = -1e4): what train() starts from."""
    from freud_amd.train_sae import save_checkpoint
    d, n = 384, 512
    g = torch.Generator().manual_seed(11)
    W = torch.empty(d, n)
    torch.nn.init.orthogonal_(W, generator=g)
    b = np.zeros(n, np.float32)
    b[::4] = -1e4
    eng = E.SaeEngine("l1", d, n, 128, optimizer="radam", recon_alpha=100.0)
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": b})
    order = ["encoder_bias", "decoder.weight"]
    state = {"engine": eng, "param_order": order, "state_dict_order": order, "optimizer": "radam", "scheduler": "cosine", "lr": cfg["lr"],
             "weight_decay": 0.0, "steps": cfg["steps"], "scheduler_params": {}, "step": 0, "best_val_loss": float("inf"),
             "hparams": {"autoencoder_variant": "l1", "autoencoder_config": cfg["autoencoder_config"], "activation_size": d},
             "world_size": 1, "epoch_rng_state": torch.get_rng_state(), "epoch_batches_done": 0}
    ck_dir = os.path.join(str(tmp_path), "init", "checkpoints")
    os.makedirs(ck_dir, exist_ok=True)
    path = os.path.join(ck_dir, "step0.pth")
    save_checkpoint(state, path)
    os.remove(os.path.join(str(tmp_path), "init", "resume", "step0.pth"))    # (the data order starts from the seed, as for a reference checkpoint)
    eng.close()
    return path, int((b < -1).sum())


def test_train_with_the_key_revives_and_resumes_bitwise(tmp_path):
    from freud_amd.train_sae import train
    cfg = _train_cfg(tmp_path, "whole")
    init, planted = _planted_checkpoint(tmp_path, cfg)
    whole = train(**dict(cfg, start_checkpoint=init))
    tags = [json.loads(l) for l in open(os.path.join(cfg["run_dir"], "metrics.jsonl"))]
    losses = [t["value"] for t in tags if t["tag"] == "train/loss"]
    dead = {t["step"]: t["value"] for t in tags if t["tag"] == "resample/dead"}
    revived = {t["step"]: t["value"] for t in tags if t["tag"] == "resample/revived"}
    print(f"planted {planted}; resample/dead {dead}; resample/revived {revived}; train/loss {losses}")
    assert sorted(dead) == [10, 20, 30, 40] and dead[10] >= planted and revived[10] >= 1
    assert len(losses) == 8 and np.isfinite(losses).all()
    st = feature_stats(whole["engine"], cfg["train_folder"], "enc", batch_files=2)
    print(f"dead at the end: {int(st.dead().sum())}")
    assert int(st.dead().sum()) < planted
    # interrupted at step 20 (the checkpoint holds the state AFTER that step's round) and resumed
    ck20 = os.path.join(cfg["run_dir"], "checkpoints", "step20.pth")
    resumed_cfg = _train_cfg(tmp_path, "resumed", start_checkpoint=ck20)
    train(**resumed_cfg)
    a = torch.load(os.path.join(cfg["run_dir"], "checkpoints", "step40.pth"), map_location="cpu", weights_only=True)
    b = torch.load(os.path.join(resumed_cfg["run_dir"], "checkpoints", "step40.pth"), map_location="cpu", weights_only=True)
    assert a["step"] == b["step"] == 40
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k
    for i in a["optimizer"]["state"]:
        for mk in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["optimizer"]["state"][i][mk], b["optimizer"]["state"][i][mk]), (i, mk)
    tags_b = [json.loads(l) for l in open(os.path.join(resumed_cfg["run_dir"], "metrics.jsonl"))]
    assert {t["step"]: t["value"] for t in tags_b if t["tag"] == "resample/revived"} == {s: v for s, v in revived.items() if s > 20}


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    d = 256
    x = torch.randn(2, 50, d).cuda()
    rl = torch.zeros(100, device="cuda")
    # a TopK context: pointed to AuxK
    tk = E.SaeEngine("topk", d, 512, 128, optimizer="adam", k=8, auxk_alpha=0.03125)
    fire = torch.zeros(512, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="auxk_alpha"):
        tk.resample_files(x, rl, 0, fire)
    st = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="auxk_alpha"):
        tk.resample_apply(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, d, device="cuda"), 0.2, st)
    tk.close()
    # an fp8 context: refused as by every file pass
    f8 = E.SaeEngine("l1", d, 512, 512, precision="fp8")
    with pytest.raises(E.EngineError, match="fp8"):
        f8.resample_files(x, rl, 0, fire)
    with pytest.raises(E.EngineError, match="fp8"):
        f8.resample_apply(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.ones(1, d, device="cuda"), 0.2, st)
    f8.close()
    torch.cuda.synchronize()
    assert not bool(rl.any()) and not bool(fire.any()) and not bool(st.any())
    # apply: a latent >= n (a padding column of n_p = 256 included), a repeated latent -- nothing is written
    W, b = weights(384, 1)
    eng = fresh(384, W, b)
    rows2 = torch.ones(2, 384, device="cuda")
    st2 = torch.zeros(4, dtype=torch.int64, device="cuda")
    for bad, msg in [([3, N], "outside"), ([3, 255], "outside"), ([-1, 3], "outside"), ([7, 7], "repeats")]:
        with pytest.raises(E.EngineError, match=msg):
            eng.resample_apply(torch.tensor(bad, dtype=torch.int32, device="cuda"), rows2, 0.2, st2)
    with pytest.raises(E.EngineError, match="alpha"):
        eng.resample_apply(torch.tensor([3, 4], dtype=torch.int32, device="cuda"), rows2, 1.5, st2)
    with pytest.raises(E.EngineError, match="x_rows"):
        eng.resample_apply(torch.tensor([3, 4], dtype=torch.int32, device="cuda"), torch.ones(2, 383, device="cuda"), 0.2, st2)
    torch.cuda.synchronize()
    p = eng.get_params()
    assert np.array_equal(bits(p["decoder.weight"]), bits(W)) and np.array_equal(bits(p["encoder_bias"]), bits(b)) and not bool(st2.any())
    # the selection's argument rules
    with pytest.raises(E.EngineError, match="workspace"):
        E.resample_select(rl, 100, fire[:200].contiguous(), 200, 0, 0, torch.zeros(200, dtype=torch.int32, device="cuda"),
                          torch.zeros(200, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda"),
                          torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(E.EngineError):
        E.resample_workspace_bytes(0, 10)
    # the Python front door
    with pytest.raises(ValueError, match="auxk_alpha"):
        tk2 = E.SaeEngine("topk", 384, 512, 300, optimizer="adam", k=8, auxk_alpha=0.03125)
        try:
            resample_dead_latents(tk2, "no/such/folder", "enc", seed=0)      # (never read: the variant is refused first)
        finally:
            tk2.close()
    eng.close()
