"""Checkpoints written by the HIP engine on an MI355X (tests/golden/engine_ckpt/, produced by tools/make_engine_checkpoints.py)
are what the reference consumes.  What the REAL reference produced from them (src.dataset.activations.init_sae_from_checkpoint,
src.scripts.train_sae.load_checkpoint and one more step) is stored in tests/golden/engine_ckpt/reference_outputs.npz, written by
tools/reference_consumes_checkpoint.py; this test checks the checkpoints against it without the reference: the state_dict layouts
the reference's modules and optimizers load, the reference's fp32 forward recomputed from the checkpoint's weights, and the
engine's own evaluation of the same weights against that forward."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import sae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CK = os.path.join(ROOT, "tests", "golden", "engine_ckpt")


def _load(name, step):
    return torch.load(os.path.join(CK, f"{name}_step{step}.pth"), map_location="cpu", weights_only=True)


def _forward(name, P, hp, x, autocast):
    """The reference module's forward on checkpoint weights P: [loss a, loss b, mse] and the dense latent [rows, n]."""
    if name == "l1":                             # encode() renormalises the decoder columns first
        out = O.l1_forward(x.reshape(-1, x.shape[-1]), O.normalize_columns(P["decoder.weight"]), P["encoder_bias"],
                           hp["autoencoder_config"]["recon_alpha"], autocast=autocast)
        return [out["reconstruction_loss"].item(), out["l1_loss"].item(), out["mse"].item()], out["c"].float().numpy()
    k = hp["autoencoder_config"]["k"]
    out = O.topk_forward(x, P["encoder.weight"], P["encoder.bias"], P["W_dec"], P["b_dec"], k, autocast=autocast)
    acts, idx = out["top_acts"].float().reshape(-1, k).numpy(), out["top_indices"].reshape(-1, k).numpy()
    lat = np.zeros((acts.shape[0], P["encoder.bias"].shape[0]), np.float32)
    np.put_along_axis(lat, idx, acts, 1)
    return [out["fvu"].item(), out["auxk_loss"].item(), out["mse"].item()], lat


def test_reference_loads_engine_written_checkpoints():
    for name in ("l1", "topk"):
        _check(name)


def _check(name):
    ref = np.load(os.path.join(CK, "reference_outputs.npz"))
    meta = json.loads(str(ref["meta"]))[name]
    summary = json.load(open(os.path.join(CK, "summary.json")))[name]
    x = torch.tensor(np.load(os.path.join(CK, "x_eval.npy")))

    # init_sae_from_checkpoint: the reference module's load_state_dict (strict) takes exactly these keys and shapes
    ck = _load(name, 6)
    assert {k: list(v.shape) for k, v in ck["model"].items()} == meta["model_state"]
    hp = ck["hparams"]
    assert hp["autoencoder_variant"] == name and hp["activation_size"] == x.shape[-1]
    P = {k: v.float() for k, v in ck["model"].items()}

    # the reference's fp32 forward, recomputed from the checkpoint's weights, is the one the reference produced
    got, lat = _forward(name, P, hp, x, autocast=False)
    assert got == pytest.approx(meta["fp32_forward"], rel=1e-5, abs=1e-7)
    lat_ref = ref[f"{name}_latent"]
    assert np.linalg.norm(lat - lat_ref) <= 1e-5 * np.linalg.norm(lat_ref)

    # the engine's (bf16) evaluation of the same weights against the reference's fp32 forward (TopK: boundary ties pick other latents)
    m = summary["eval_metrics"][:3]
    for a, b in zip(meta["fp32_forward"], m):
        assert (a == 0 and b == 0) or abs(a - b) / max(abs(b), 1e-12) < (2e-2 if name == "l1" else 6e-2), (meta["fp32_forward"], m)
    lat_eng = np.load(os.path.join(CK, f"latent_{name}.npy"))
    assert np.linalg.norm(lat_ref - lat_eng) / np.linalg.norm(lat_ref) < (2e-2 if name == "l1" else 0.3)

    # load_checkpoint: torch's own load_state_dict of the reference's optimizer and scheduler takes the step-3 state, and one
    # more step leaves the reference's step counter and learning rate; the loss of that step is the reference's bf16-autocast
    # forward on the step-3 weights
    ck3 = _load(name, 3)
    assert ck3["step"] == meta["resumed_step"] == 3 and ck3["hparams"]["autoencoder_variant"] == name
    params = [torch.nn.Parameter(torch.zeros(s)) for s in meta["param_shapes"]]
    hp3 = ck3["hparams"]
    if name == "l1":
        opt = torch.optim.RAdam(params, eps=1e-5, lr=hp3["lr"], weight_decay=hp3["weight_decay"])
        sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=hp3["steps"], eta_min=0)
    else:
        warm = hp3["scheduler_params"]["num_warmup_steps"]
        opt = torch.optim.Adam(params, lr=hp3["lr"])
        sch = torch.optim.lr_scheduler.LambdaLR(   # transformers' get_linear_schedule_with_warmup
            opt, lambda s: s / max(1, warm) if s < warm else max(0.0, (hp3["steps"] - s) / max(1, hp3["steps"] - warm)))
    opt.load_state_dict(ck3["optimizer"])
    sch.load_state_dict(dict(ck3["scheduler"]))
    assert sorted(k for k in opt.state_dict()["param_groups"][0] if k != "params") == meta["param_group_keys"]
    assert sorted(ck3["scheduler"].keys()) == meta["scheduler_keys"]
    assert all(opt.state[p]["exp_avg"].shape == p.shape for p in params)
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    sch.step()
    assert int(next(iter(opt.state.values()))["step"]) == meta["optimizer_step_after"] == 4
    assert sch.get_last_lr()[0] == pytest.approx(meta["lr_after"], rel=1e-9)
    loss = sum(_forward(name, {k: v.float() for k, v in ck3["model"].items()}, hp3, x, autocast=True)[0][:2])
    assert loss == pytest.approx(meta["loss_after_resume"], rel=1e-3)
