"""GPU: train() with the optional key "init_b_dec" (freud_amd/train_sae.py -> freud_amd/input_stats.py) on tiny TopK shards (6 files,
T = 37, d = 24, n = 64, k = 4) with a planted offset: b_dec starts at the geometric median (or the mean) of the training files, to
the bit what input_statistics returns; the other initial parameters are those of the run without the key; the key is recorded in the
checkpoint's hparams; a resume leaves the checkpoint's b_dec alone; and the first step's FVU is below the one of the run without
the key.  The initial parameters are captured around the real engine through train()'s engine_factory hook."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DM, N, K, T, FILES = 24, 64, 4, 37, 6


def _cfg(tmp_path, run, steps=2, **over):
    from freud_amd.loader import write_shards
    folder = os.path.join(str(tmp_path), "train")
    if not os.path.isdir(folder):
        rng = np.random.default_rng(3)
        rows = (np.maximum(rng.standard_normal((FILES * T, 8)), 0) * 0.5) @ rng.standard_normal((8, DM))
        rows += 0.05 * rng.standard_normal(rows.shape)
        rows[:, 1] += 40.0                                   # the planted offset: a constant no latent should pay for
        rows[:, 5] -= 15.0
        write_shards(folder, "enc", rows.astype(np.float32).reshape(FILES, T * DM), [T, DM])
    cfg = {
        "whisper_config": {"model": "tiny", "layer_name": "enc"}, "seed": 0, "train_folder": folder, "val_folder": folder,
        "device": "cuda", "lr": 1e-3, "weight_decay": 0.0, "steps": steps, "clip_thresh": 1.0, "dl_max_workers": 0,
        "log_tb_every": 1, "save_every": 1, "val_every": 1000, "scheduler_params": {}, "start_checkpoint": None, "from_disk": True,
        "batch_size": 2, "run_dir": os.path.join(str(tmp_path), run), "autoencoder_variant": "topk", "optimizer": "adam",
        "scheduler": "cosine",
        "autoencoder_config": {"n_dict_components": N, "k": K, "auxk_alpha": 0.03125, "normalize_decoder": True, "multi_topk": False,
                               "dead_feature_threshold": 300.0},
    }
    cfg.update(over)
    return cfg


def _train(cfg):
    """train() on the real engine; returns every set_params() call's parameters, in order."""
    from freud_amd.engine import SaeEngine
    from freud_amd.train_sae import train
    calls = []

    def factory(**kw):
        eng = SaeEngine(**kw)
        inner = eng.set_params

        def set_params(params):
            calls.append({k: np.array(v, copy=True) for k, v in params.items()})
            return inner(params)

        eng.set_params = set_params
        return eng

    train(**cfg, engine_factory=factory)
    return calls


def _load(run_dir, step):
    return torch.load(os.path.join(run_dir, "checkpoints", f"step{step}.pth"), map_location="cpu", weights_only=True)


def _scalars(run_dir):
    rows = [json.loads(l) for l in open(os.path.join(run_dir, "metrics.jsonl"))]
    return {(r["tag"], r["step"]): r["value"] for r in rows}


def test_b_dec_starts_at_the_statistic_and_nothing_else_moves(tmp_path):
    from freud_amd.input_stats import input_statistics
    plain = _cfg(tmp_path, "plain")
    keyed = _cfg(tmp_path, "keyed", init_b_dec="geometric_median")
    torch.manual_seed(99)
    a = _train(plain)[0]
    torch.manual_seed(99)
    b = _train(keyed)[0]
    st = input_statistics(keyed["train_folder"], "enc", files=256, iterations=32)
    assert st.n_files == FILES and st.n_frames == FILES * T
    assert np.array_equal(a["b_dec"], np.zeros(DM, np.float32))
    assert b["b_dec"].dtype == np.float32 and b["b_dec"].tobytes() == st.geometric_median.tobytes()
    assert abs(float(b["b_dec"][1]) - 40.0) < 1.0 and abs(float(b["b_dec"][5]) + 15.0) < 1.0
    for k in ("encoder.weight", "encoder.bias", "W_dec"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # recorded in hparams, and only where it is set; logged once
    assert _load(keyed["run_dir"], 1)["hparams"]["init_b_dec"] == "geometric_median"
    assert "init_b_dec" not in _load(plain["run_dir"], 1)["hparams"]
    s_keyed, s_plain = _scalars(keyed["run_dir"]), _scalars(plain["run_dir"])
    assert s_keyed[("init/b_dec_norm", 0)] == pytest.approx(float(np.linalg.norm(st.geometric_median.astype(np.float64))), rel=1e-6)
    assert s_keyed[("init/mean_energy_fraction", 0)] == pytest.approx(st.mean_energy_fraction, rel=1e-6)
    assert s_keyed[("init/median_shift", 0)] == pytest.approx(st.shift, rel=1e-6, abs=1e-300)
    assert not any(tag.startswith("init/") for tag, _ in s_plain)
    # the loader's shuffles are those of the run without the key: the steps saw the same batches, so the parameters the key does
    # not touch at step 0 received gradients of the same files -- and the direction of the effect: the first step's FVU is lower
    for step in (1, 2):
        assert np.isfinite(s_keyed[("train/fvu", step)]) and np.isfinite(s_plain[("train/fvu", step)])
    assert s_keyed[("train/fvu", 1)] < s_plain[("train/fvu", 1)]
    # a resume records the key and leaves the checkpoint's b_dec alone
    ck1 = os.path.join(plain["run_dir"], "checkpoints", "step1.pth")
    resumed = _cfg(tmp_path, "resumed", init_b_dec={"method": "geometric_median", "files": 4}, start_checkpoint=ck1)
    calls = _train(resumed)
    ck_b = _load(plain["run_dir"], 1)["model"]["b_dec"].numpy()
    assert np.array_equal(calls[0]["b_dec"], np.zeros(DM, np.float32))                  # not applied
    assert calls[-1]["b_dec"].tobytes() == ck_b.tobytes() and len(calls) == 2          # the checkpoint's stands
    r2 = _load(resumed["run_dir"], 2)
    assert r2["hparams"]["init_b_dec"] == {"method": "geometric_median", "files": 4}
    p2 = _load(plain["run_dir"], 2)
    for k in p2["model"]:
        assert torch.equal(p2["model"][k], r2["model"][k]), k


def test_mean_and_the_object_form(tmp_path):
    from freud_amd.input_stats import input_statistics
    cfg = _cfg(tmp_path, "mean", steps=1, init_b_dec={"method": "mean", "files": 4, "iterations": 2})
    b = _train(cfg)[0]
    st = input_statistics(cfg["train_folder"], "enc", files=4, iterations=2)
    assert st.n_files == 4
    assert b["b_dec"].tobytes() == st.mean.astype(np.float32).tobytes()
    assert _load(cfg["run_dir"], 1)["hparams"]["init_b_dec"] == {"method": "mean", "files": 4, "iterations": 2}
