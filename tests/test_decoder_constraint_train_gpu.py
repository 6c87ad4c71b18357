"""GPU: train() with "decoder_constraint": true (freud_amd/train_sae.py -> sae_set_decoder_constraint) on a synthetic shard directory
(8 files, d = 128, n = 256): the checkpoint holds unit decoder rows, hparams records the key (and only when it is set), a run
stopped at step 3 and resumed ends in the same bits, and two ranks on one GPU (in-engine data parallel, mode auto) train like one
process on the doubled batch with their replicas bit-equal on every step."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import tests.test_dp_gpu as DP
from tests import decoder_constraint_reference as D

pytestmark = pytest.mark.gpu
DM, N, T, FILES = 128, 256, 32, 8


def _cfg(tmp_path, steps, run, **over):
    from freud_amd.loader import write_shards
    g = torch.Generator().manual_seed(5)
    rows = ((torch.relu(torch.randn(FILES * T, 16, generator=g)) * 0.2) @ torch.randn(16, DM, generator=g)).reshape(FILES, T * DM)
    folder = os.path.join(str(tmp_path), "train")
    if not os.path.isdir(folder):
        write_shards(folder, "enc", rows.numpy(), [T, DM])
    cfg = {
        "whisper_config": {"model": "tiny", "layer_name": "enc"}, "seed": 0, "train_folder": folder, "val_folder": folder,
        "device": "cuda", "lr": 1e-3, "weight_decay": 0.0, "steps": steps, "clip_thresh": 1.0, "dl_max_workers": 0,
        "log_tb_every": 1, "save_every": 3, "val_every": 1000, "scheduler_params": {}, "start_checkpoint": None, "from_disk": True,
        "batch_size": 2, "run_dir": os.path.join(str(tmp_path), run), "autoencoder_variant": "topk", "optimizer": "adam",
        "scheduler": "cosine",
        "autoencoder_config": {"n_dict_components": N, "k": 8, "auxk_alpha": 0.03125, "normalize_decoder": True, "multi_topk": False,
                               "dead_feature_threshold": 300.0},
    }
    cfg.update(over)
    return cfg


def _run(tmp_path, cfg, name):
    from freud_amd.train_sae import main
    path = os.path.join(str(tmp_path), name)
    json.dump(cfg, open(path, "w"))
    main(["--config", path])


def _load(run_dir, step):
    return torch.load(os.path.join(run_dir, "checkpoints", f"step{step}.pth"), map_location="cpu", weights_only=True)


def _row_norm_limit():
    """Adam moves an element by a few lr per step at most, a row of d = 128 by under 0.04 at lr = 1e-3: the norm before the last renorm
    is above 0.9, and decoder_constraint_reference.row_norm_bound for such a row is EPS / (0.9 + EPS) + (d_p / 2 + 3) U SLACK."""
    return float(D.row_norm_bound(np.full((1, DM), 0.9 / np.sqrt(DM)), DM)[0])


def test_checkpoint_has_unit_rows_records_the_key_and_resumes_bitwise(tmp_path):
    steps = 6
    whole = _cfg(tmp_path, steps, "whole", decoder_constraint=True)
    _run(tmp_path, whole, "whole.json")
    a = _load(whole["run_dir"], steps)
    assert a["hparams"]["decoder_constraint"] is True and a["step"] == steps
    nrm = np.sqrt((a["model"]["W_dec"].numpy().astype(np.float64) ** 2).sum(1))
    assert nrm.shape == (N,) and (np.abs(nrm - 1.0) <= _row_norm_limit()).all(), np.abs(nrm - 1.0).max()
    # the same config without the key: hparams without it, and rows that drifted
    plain = _cfg(tmp_path, steps, "plain")
    _run(tmp_path, plain, "plain.json")
    b = _load(plain["run_dir"], steps)
    assert "decoder_constraint" not in b["hparams"]
    nrm_b = np.sqrt((b["model"]["W_dec"].numpy().astype(np.float64) ** 2).sum(1))
    assert (np.abs(nrm_b - 1.0) > _row_norm_limit()).any(), "without the constraint the rows leave the bound: the check above can fail"
    # stopped at 3, resumed to 6
    ck3 = os.path.join(whole["run_dir"], "checkpoints", "step3.pth")
    assert _load(whole["run_dir"], 3)["hparams"]["decoder_constraint"] is True
    resumed = _cfg(tmp_path, steps, "resumed", decoder_constraint=True, start_checkpoint=ck3)
    _run(tmp_path, resumed, "resumed.json")
    r = _load(resumed["run_dir"], steps)
    assert r["step"] == steps and r["hparams"]["decoder_constraint"] is True
    for k in a["model"]:
        assert torch.equal(a["model"][k], r["model"][k]), k
    for i in a["optimizer"]["state"]:
        for mk in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["optimizer"]["state"][i][mk], r["optimizer"]["state"][i][mk]), (i, mk)
        assert float(a["optimizer"]["state"][i]["step"]) == float(r["optimizer"]["state"][i]["step"]) == steps


def test_two_ranks_on_one_gpu_train_like_one_process(tmp_path):
    steps, B, world = 3, 2, 2
    base = _cfg(tmp_path, steps, "unused", decoder_constraint=True, save_every=1)
    script = os.path.join(str(tmp_path), "child.py")
    open(script, "w").write(DP._TRAIN_CHILD)
    cfg2 = dict(copy.deepcopy(base), batch_size=B, run_dir=os.path.join(str(tmp_path), "dp2"))
    cfg1 = dict(copy.deepcopy(base), batch_size=world * B, run_dir=os.path.join(str(tmp_path), "dp1"))
    for name, cfg in (("cfg2.json", cfg2), ("cfg1.json", cfg1)):
        json.dump(cfg, open(os.path.join(str(tmp_path), name), "w"))
    outs = DP._run_children(script, os.path.join(str(tmp_path), "cfg2.json"), world, {"FREUD_P2P_TIMEOUT_MS": "20000"})     # FREUD_DP: auto
    assert "data parallel: 2 ranks, exchange = " in outs[0][0] and "exchange = host" not in outs[0][0], outs[0][0][-1000:]
    # every step logs and saves: before each, train()'s guard compared the replicas' checksums (parameters, both moments, step) and
    # the auditor compared the exchanged gradient with a gloo all-reduce of the ranks' own
    for so, _ in outs:
        assert f"AUDITS_PASSED {steps}" in so, so[-500:]
    DP._run_children(script, os.path.join(str(tmp_path), "cfg1.json"), 1, {})
    a, b = _load(cfg2["run_dir"], steps), _load(cfg1["run_dir"], steps)
    assert a["hparams"]["decoder_constraint"] is True
    for k in a["model"]:
        assert DP._rel(a["model"][k].numpy(), b["model"][k].numpy()) < (1e-4 if a["model"][k].dim() == 2 else 1e-3), k
    nrm = np.sqrt((a["model"]["W_dec"].numpy().astype(np.float64) ** 2).sum(1))
    assert (np.abs(nrm - 1.0) <= _row_norm_limit()).all()
    sc = lambda run: {(json.loads(l)["tag"], json.loads(l)["step"]): json.loads(l)["value"] for l in open(os.path.join(run, "metrics.jsonl"))}
    s2, s1 = sc(cfg2["run_dir"]), sc(cfg1["run_dir"])
    for step in range(1, steps + 1):
        for tag in ("train/fvu", "train/auxk_loss", "train/grad_norm"):
            assert s2[(tag, step)] == pytest.approx(s1[(tag, step)], rel=1e-4, abs=1e-7), (tag, step)
