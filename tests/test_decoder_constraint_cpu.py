"""CPU: the rule and the bounds of tests/decoder_constraint_reference.py (the decoder-norm constraint of TopK training,
sae_set_decoder_constraint) -- the yardstick tests/test_decoder_constraint_gpu.py holds the kernels to.

1. Golden from the real reference (tests/golden/decoder_constraint.npz, written by tests/golden/make_decoder_constraint_golden.py from the
   reference model's own remove_gradient_parallel_to_decoder_directions / set_decoder_norm_to_unit_norm inside three torch training steps):
   the float64 rule reproduces every stage from that stage's stored input within the derived bound.
2. An fp32 emulation of both kernels (lane partial, then the butterfly) lies inside the bounds at d_p = 128, 384 and 1280.
3. Fifteen mutations of the rule fall outside a bound on inputs the test constructs.
4. train()'s argument errors for the "decoder_constraint" key, against the fake engine.

No tolerance here is a measured number."""
import copy
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from tests import decoder_constraint_reference as D
from tests import optimizer_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_constraint.npz")
NAMES = ("W_dec", "b_dec", "encoder.weight", "encoder.bias")


def topk_shapes(d, n):
    return {"encoder.weight": (n, d), "encoder.bias": (n,), "W_dec": (n, d), "b_dec": (d,)}


# ---- 1. the golden of the real reference ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("s", range(3))
def test_float64_rule_reproduces_every_stage_of_the_reference(golden, s):
    z = golden
    d = z["s0_W_before"].shape[1]
    W, G = z[f"s{s}_W_before"], z[f"s{s}_grad_W_dec"]
    assert np.array_equal(W, z[f"s{s}_p_W_dec"])
    if s:
        assert np.array_equal(W, z[f"s{s - 1}_W_renormed"])
    assert (np.abs(G).sum(1) > 0).mean() > 0.5 and np.abs((G * W).sum(1)).max() > 1e-4, "the gradient has a parallel part to remove"
    # project: torch sums the d products of a row in an order of its own -- the bound is for any order (N = d: no padding here)
    got = z[f"s{s}_grad_W_dec_projected"]
    bad = D.violations(got, D.project(G, W), D.project_bound(G, W, d))
    print(f"step {s}: projection |error| / bound {D.worst_ratio(got, D.project(G, W), D.project_bound(G, W, d)):.3f}")
    assert not bad.any(), int(bad.sum())
    assert D.violations(G, D.project(G, W), D.project_bound(G, W, d)).mean() > 0.5, "the unprojected gradient is far outside"
    # update: clip_grad_norm_ of the projected gradients, then Adam -- tests/optimizer_reference.py with torch's own norm error
    c = R.Case("adam", s + 1, (0.9, 0.999), 0.0, 1.0, 1.0, False, lr=1e-2)
    p = {k: z[f"s{s}_p_{k}"] for k in NAMES}
    g = {k: z[f"s{s}_grad_{k}"] for k in NAMES}
    g["W_dec"] = got
    m = {k: z[f"s{s}_m_{k}"] for k in NAMES}
    v = {k: z[f"s{s}_v_{k}"] for k in NAMES}
    total = R.clip_of(g, c)[0]
    off_u = abs(float(z[f"s{s}_total_norm"]) / total - 1.0) / R.U
    assert off_u <= sum(a.size for a in p.values()) + 3
    ref = R.reference_step(p, g, m, v, c, norm_extra_u=off_u)
    bad = R.violations({"W_dec": z[f"s{s}_W_updated"]}, {"p": {"W_dec": ref["p"]["W_dec"]}, "tol_p": {"W_dec": ref["tol_p"]["W_dec"]}}, "p")
    assert not bad["W_dec"].any(), int(bad["W_dec"].sum())
    unprojected = R.reference_step(p, dict(g, W_dec=G), m, v, c, norm_extra_u=off_u)
    assert (np.abs(z[f"s{s}_W_updated"] - unprojected["p"]["W_dec"]) > unprojected["tol_p"]["W_dec"]).any(), "the projection shows in the update"
    # renorm
    Wu, Wr = z[f"s{s}_W_updated"], z[f"s{s}_W_renormed"]
    bad = D.violations(Wr, D.renorm(Wu), D.renorm_bound(Wu, d))
    print(f"step {s}: renorm |error| / bound {D.worst_ratio(Wr, D.renorm(Wu), D.renorm_bound(Wu, d)):.3f}")
    assert not bad.any(), int(bad.sum())
    nrm = np.sqrt((Wr.astype(np.float64) ** 2).sum(1))
    assert (np.abs(nrm - 1.0) <= D.row_norm_bound(Wu, d)).all()
    nu = np.sqrt((Wu.astype(np.float64) ** 2).sum(1))
    assert (np.abs(nu - 1.0) > D.row_norm_bound(Wu, d)).mean() > 0.5, "the update moved the norms: the renorm shows"


# ---- 2. the fp32 emulation ----------------------------------------------------------------------------------------------------------
def constructed(d, n, case=R.KERNEL_CASES[0], seed=7):
    """The family of the GPU test at (d, n): p, g, m, v with the planted rows."""
    p, g, m, v = R.make_inputs(topk_shapes(d, n), case, seed)
    return D.plant_rows(p, g, m, v)


def wide_rows(d, n, seed=9):
    """Rows whose norms are 2^e, e spread over [-40, 40]; row ZERO_ROW all zero."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((n, d))
    W = W / np.sqrt((W * W).sum(1, keepdims=True)) * 2.0 ** np.linspace(-40, 40, n)[:, None]
    W = R.f32(W)
    W[D.ZERO_ROW] = 0.0
    return W


@pytest.mark.parametrize("d,d_p", [(128, 128), (100, 128), (384, 384), (1280, 1280)])
def test_fp32_emulation_of_both_kernels_is_inside_the_bounds(d, d_p):
    n = 64
    p, g, _, _ = constructed(d, n)
    W, G = p["W_dec"], g["W_dec"]
    got = D.emulate_project(G, W, d_p)
    ref, tol = D.project(G, W), D.project_bound(G, W, d_p)
    print(f"d_p {d_p}: emulated projection |error| / bound {D.worst_ratio(got, ref, tol):.4f}")
    assert not D.violations(got, ref, tol).any()
    assert not got[D.ZERO_ROW].any() and not got[D.ZERO_GRAD_ROW].any()
    assert np.abs(got[D.PARALLEL_ROW]).max() <= 3 * 2e-3 * 1.01 * np.abs(W[D.PARALLEL_ROW]).max() + tol[D.PARALLEL_ROW].max()
    for rows in (W, wide_rows(d, n)):
        out, outb = D.emulate_renorm(rows, d_p)
        ref, tol = D.renorm(rows), D.renorm_bound(rows, d_p)
        print(f"d_p {d_p}: emulated renorm |error| / bound {D.worst_ratio(out, ref, tol):.4f}")
        assert not D.violations(out, ref, tol).any()
        assert not out[D.ZERO_ROW].any() and not np.signbit(out[D.ZERO_ROW]).any()
        assert np.array_equal(outb, D.bf16_round(out))
    out, _ = D.emulate_renorm(W, d_p)
    live = np.arange(n) != D.ZERO_ROW
    nrm = np.sqrt((out.astype(np.float64) ** 2).sum(1))
    assert (np.abs(nrm - 1.0) <= D.row_norm_bound(W, d_p))[live].all()


# ---- 3. mutations -------------------------------------------------------------------------------------------------------------------
def chain(p, g, m, v, c, d_p, d, mut=None):
    """One constrained step in float64 on padded rows [n][d_p] of W_dec (d of them real) -> its stage outputs.  `mut` names one mutation
    of the rule."""
    W, G = np.asarray(p["W_dec"], np.float64), np.asarray(g["W_dec"], np.float64)
    d = d if mut == "dot_over_d" else d_p
    dot = (G[:, :d] * W[:, :d]).sum(1, keepdims=True)
    if mut == "divide_by_w2":
        with np.errstate(invalid="ignore", divide="ignore"):
            dot = np.where((W * W).sum(1, keepdims=True) > 0, dot / (W * W).sum(1, keepdims=True), 0.0)
    gproj = G + dot * W if mut == "sign_flipped" else G - dot * W
    if mut == "project_columns":
        gproj = G - (G * W).sum(0, keepdims=True) * W
    if mut == "project_after_clip_norm":          # the clip norm is formed from the unprojected buffer
        total = R.clip_of(g, c)[0]
        coef = min(1.0, c.thresh / (total + 1e-6))
        true_total = R.clip_of(dict(g, W_dec=gproj), c)[0]
        scale_fix = coef / min(1.0, c.thresh / (true_total + 1e-6))
    else:
        total, scale_fix = R.clip_of(dict(g, W_dec=gproj), c)[0], 1.0
    Wstart = D.renorm(W) if mut == "renorm_before_update" else W
    ref = R.reference_step(dict(p, W_dec=Wstart), {k: np.asarray(a, np.float64) * scale_fix for k, a in dict(g, W_dec=gproj).items()}, m, v, c)
    W_upd, m1, v1 = ref["p"]["W_dec"], ref["m"]["W_dec"], ref["v"]["W_dec"]
    if mut == "project_with_updated_row":
        gproj = G - (G * W_upd).sum(1, keepdims=True) * W_upd
    if mut == "moments_projected":
        m1 = D.project(m1, W)
    nrm = np.sqrt((W_upd * W_upd).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        if mut == "renorm_before_update":
            W_out = W_upd
        elif mut == "eps_dropped":
            W_out = np.where(nrm > 0, W_upd / np.where(nrm > 0, nrm, 1.0), 0.0)
        elif mut == "eps_inside_sqrt":
            W_out = W_upd / np.sqrt(nrm * nrm + D.EPS)
        elif mut == "eps_of_float64":
            W_out = W_upd / (nrm + 2.0 ** -52)
        elif mut == "padding_divided_to_nan":
            W_out = W_upd / (nrm + D.EPS * (nrm > 0))
        elif mut == "renorm_columns":
            W_out = W_upd / (np.sqrt((W_upd * W_upd).sum(0, keepdims=True)) + D.EPS)
        else:
            W_out = W_upd / (nrm + D.EPS)
    if mut == "moments_rescaled":
        m1 = m1 / (nrm + D.EPS)
    Wb = D.bf16_round(R.f32(W_upd if mut == "bf16_copy_before_renorm" else W_out)).astype(np.float64)
    return {"gproj": gproj, "total": total, "m": m1, "v": v1, "W_upd": W_upd, "W_out": W_out, "Wb": Wb, "ref": ref}


def outside(mutant, good, p, g, d_p):
    """Does the mutant leave a bound of the rule anywhere?  Stage by stage, each against the good chain's value and bound."""
    W, G = p["W_dec"], g["W_dec"]
    ref = good["ref"]
    tol_out = D.renorm_bound(good["W_upd"], d_p)
    # the bf16 copy: half a bf16 ulp (at most 2^-8 relative) around the renormalised value, which itself is known to its bound
    tol_b = 2.0 ** -8 * np.abs(good["W_out"]) + tol_out * (1 + 2.0 ** -8) + 2.0 ** -134
    return bool(D.violations(mutant["gproj"], good["gproj"], D.project_bound(G, W, d_p)).any()
                or abs(mutant["total"] - good["total"]) > ref["tol_total"]
                or D.violations(mutant["m"], good["m"], ref["tol_m"]["W_dec"]).any()
                or D.violations(mutant["v"], good["v"], ref["tol_v"]["W_dec"]).any()
                or D.violations(mutant["W_out"], good["W_out"], tol_out).any()
                or D.violations(mutant["Wb"], good["W_out"], tol_b).any())


def padded_inputs(d, n, d_p, plant_padding, wide):
    p, g, m, v = constructed(d, n)
    if wide:
        p["W_dec"] = wide_rows(d, n)
        g["W_dec"][:] = 0.0                        # (and no gradient for them: this input is for the renorm alone)

    def pad(a):
        out = np.zeros((n, d_p), a.dtype)
        out[:, :d] = a
        return out
    for t in (p, g, m, v):
        t["W_dec"] = pad(t["W_dec"])
    if plant_padding:                              # what the engine never has: non-zero padding columns, in both operands of the dot
        p["W_dec"][:, d:] = np.float32(0.01)
        g["W_dec"][:, d:] = np.float32(0.01)
    return p, g, m, v


MUTATIONS = {           # name -> (padding planted, wide row norms)
    "divide_by_w2": (False, False),
    "eps_dropped": (False, True),
    "eps_inside_sqrt": (False, True),
    "eps_of_float64": (False, True),
    "project_after_clip_norm": (False, False),
    "project_with_updated_row": (False, False),
    "renorm_before_update": (False, False),
    "moments_projected": (False, False),
    "moments_rescaled": (False, False),
    "bf16_copy_before_renorm": (False, False),
    "padding_divided_to_nan": (False, False),
    "dot_over_d": (True, False),
    "sign_flipped": (False, False),
    "project_columns": (False, False),
    "renorm_columns": (False, False),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_every_mutation_of_the_rule_falls_outside_a_bound(mutation):
    d, n, d_p = 100, 64, 128
    planted, wide = MUTATIONS[mutation]
    c = R.KERNEL_CASES[0]                           # Adam, clipped: the clip coefficient carries the norm into every element
    if wide:                                        # (lr = 0: the renorm sees the wide rows themselves, not rows an update of 1e-3 refilled)
        c = dataclasses.replace(c, lr=0.0)
    p, g, m, v = padded_inputs(d, n, d_p, planted, wide)
    args = (p, g, m, v, c, d_p, d)
    good = chain(*args)
    assert not outside(good, good, p, g, d_p)
    # ... and the bound is not so tight that fp32 itself leaves it: the emulated kernels on the same inputs
    assert not D.violations(D.emulate_project(g["W_dec"], p["W_dec"], d_p), good["gproj"], D.project_bound(g["W_dec"], p["W_dec"], d_p)).any()
    out, outb = D.emulate_renorm(R.f32(good["W_upd"]), d_p)
    tol = D.renorm_bound(R.f32(good["W_upd"]), d_p)
    assert not D.violations(out, D.renorm(R.f32(good["W_upd"])), tol).any()
    mutant = chain(*args, mut=mutation)
    assert outside(mutant, good, p, g, d_p), f"{mutation} passes every bound"


def test_there_are_at_least_ten_mutations_and_the_issue_s_are_among_them():
    want = {"divide_by_w2", "eps_dropped", "eps_inside_sqrt", "project_after_clip_norm", "project_with_updated_row", "renorm_before_update",
            "moments_projected", "bf16_copy_before_renorm", "padding_divided_to_nan", "dot_over_d"}
    assert want <= set(MUTATIONS) and len(MUTATIONS) >= 10


def test_the_renorm_is_not_idempotent_in_fp32():
    """Why a run that resumes its own checkpoint switches the constraint on with keep_rows: a second renorm of rows the first one left
    moves most of them again (the fixed point of n -> n / (n + EPS) is 1 - EPS, and fl(n + EPS) is 1 only by luck)."""
    W = constructed(128, 64)[0]["W_dec"]
    a, _ = D.emulate_renorm(W, 128)
    b, _ = D.emulate_renorm(a, 128)
    assert (a != b).any(1).mean() > 0.25
    assert not D.violations(b, a.astype(np.float64), 4 * D.U * np.abs(a.astype(np.float64)) + 1e-300).any()      # by an ulp or two, no more


# ---- 4. train()'s argument errors ---------------------------------------------------------------------------------------------------
from freud_amd.loader import write_shards       # noqa: E402
from freud_amd.train_sae import train           # noqa: E402
from tests.fake_engine import OracleEngine      # noqa: E402


def _train_cfg(tmp_path, golden_dir, which, **over):
    z = np.load(os.path.join(golden_dir, f"trainloop_{which}.npz"))
    meta = json.loads(str(z["meta"]))
    folder = os.path.join(str(tmp_path), "train_" + which)
    if not os.path.exists(folder):
        write_shards(folder, meta["layer"], z["shard"], [meta["T"], meta["d"]], [f"/data/audio/file_{i:04d}.flac" for i in range(meta["n_files"])])
    cfg = copy.deepcopy(meta["config"])
    cfg.update(train_folder=folder, val_folder=folder, run_dir=os.path.join(str(tmp_path), "run_" + which), device="cpu", steps=2, val_every=1000)
    cfg.update(over)
    return cfg


def test_train_refuses_the_key_for_l1(tmp_path, golden_dir):
    with pytest.raises(ValueError, match="TopK"):
        train(**_train_cfg(tmp_path, golden_dir, "l1", decoder_constraint=True), engine_factory=OracleEngine)


def test_train_refuses_the_key_without_normalize_decoder(tmp_path, golden_dir):
    cfg = _train_cfg(tmp_path, golden_dir, "topk", decoder_constraint=True)
    cfg["autoencoder_config"]["normalize_decoder"] = False
    with pytest.raises(ValueError, match="normalize_decoder"):
        train(**cfg, engine_factory=OracleEngine)


def test_train_refuses_the_key_on_an_engine_without_the_constraint(tmp_path, golden_dir):
    assert not hasattr(OracleEngine, "set_decoder_constraint")
    with pytest.raises(RuntimeError, match="sae_set_decoder_constraint"):
        train(**_train_cfg(tmp_path, golden_dir, "topk", decoder_constraint=True), engine_factory=OracleEngine)


def test_train_without_the_key_is_a_reference_run(tmp_path, golden_dir):
    st = train(**_train_cfg(tmp_path, golden_dir, "topk"), engine_factory=OracleEngine)
    assert "decoder_constraint" not in st["hparams"]
    st = train(**_train_cfg(tmp_path, golden_dir, "topk", decoder_constraint=False, run_dir=os.path.join(str(tmp_path), "off")), engine_factory=OracleEngine)
    assert "decoder_constraint" not in st["hparams"]
    with pytest.raises(ValueError, match="true or false"):
        train(**_train_cfg(tmp_path, golden_dir, "topk", decoder_constraint="yes"), engine_factory=OracleEngine)
