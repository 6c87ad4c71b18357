"""CPU: the host side of the reconstruction report (freud_amd/reconstruction.py) and the check of tests/reconstruction_reference.py.

* the attribution bound can fail: a float32 emulation of the kernels violates it on no latent, each deliberately wrong answer on at
  least 90 % of the firing latents -- what keeps the GPU test, which allows none, from passing vacuously;
* the derived quantities against a dense float64 computation on a small synthetic report, the npz round trip;
* the boundary: header, EXPORTED_SYMBOLS, the built library, recon_layout against the offset macros;
* argument errors raised before any GPU work."""
import os
import re

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import reconstruction as RC
from freud_amd.loader import write_shards
from tests import reconstruction_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 0.90


# ---- the bound can fail
@pytest.fixture(scope="module")
def l1_case():
    """d=256, n=1024, 6 files of 100 frames with trimmed lengths; unit-norm columns of +-1/16, bias N(-1, 0.3).  The forward in numpy
    as the engine runs it: c = bf16(relu(bf16(x_b W_b) + b)), x_hat = bf16(c W_b^T), r = x - x_hat, r_b = bf16(r)."""
    d, n, F, T = 256, 1024, 6, 100
    g = np.random.default_rng(7)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    b = g.normal(-1, 0.3, n).astype(np.float32)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = T
    Wb = R.bf16(W)
    x2 = x.reshape(F * T, d)
    c = R.bf16(np.maximum(R.bf16(R.bf16(x2) @ Wb) + b, 0))
    x_hat = R.bf16(c @ Wb.T)
    counted = (np.arange(T)[None, :] < L[:, None]).reshape(-1)
    r = (x2 - x_hat).astype(np.float32)
    r[~counted] = 0
    w_op = np.ascontiguousarray(Wb.T)
    lat = torch.from_numpy(c.reshape(F, T, n))
    ref = R.reference(x, r.reshape(F, T, d), lambda f: lat[f], w_op, L, "l1")
    assert ref.fired.mean() >= 0.9 and counted.sum() < F * T
    return {"a": c, "r_b": R.bf16(r), "w_op": w_op, "counted": counted, "ref": ref, "T": T, "L": L, "x2": x2, "x_hat": x_hat}


def share(attr, c):
    bad = R.violations(attr, c["ref"], "attr_sum")[c["ref"].fired]
    print(f"violating share of the firing latents {bad.mean():.4f}")
    return bad.mean()


def test_emulation_has_no_violation(l1_case):
    c = l1_case
    got = R.emulate_attr_l1(c["a"], c["r_b"], c["w_op"], c["counted"])
    print(R.describe(got, c["ref"], "attr_sum"))
    assert not R.violations(got, c["ref"], "attr_sum").any()


def test_dropped_last_k_tile(l1_case):
    c = l1_case
    assert share(R.emulate_attr_l1(c["a"], c["r_b"], c["w_op"], c["counted"], drop_last_k_tile=True), c) >= FLOOR


def test_lengths_ignored(l1_case):
    c = l1_case
    r_all = R.bf16((c["x2"] - c["x_hat"]).astype(np.float32))
    assert share(R.emulate_attr_l1(c["a"], r_all, c["w_op"], np.ones_like(c["counted"])), c) >= FLOOR


def test_latent_from_next_column(l1_case):
    c = l1_case
    assert share(R.emulate_attr_l1(np.roll(c["a"], -1, axis=1), c["r_b"], c["w_op"], c["counted"]), c) >= FLOOR


def test_latent_from_next_row(l1_case):
    c = l1_case
    assert share(R.emulate_attr_l1(np.roll(c["a"], -1, axis=0), c["r_b"], c["w_op"], c["counted"]), c) >= FLOOR


def test_non_finite_is_a_violation(l1_case):
    c = l1_case
    got = R.emulate_attr_l1(c["a"], c["r_b"], c["w_op"], c["counted"])
    got[3] = np.nan
    bad = R.violations(got, c["ref"], "attr_sum")
    assert bad[3] and bad.sum() == 1


# ---- derived quantities
def synthetic_report():
    """A dense toy problem in float64: 3 files x 7 frames, d = 5, n = 4 (latent 2 never fires), x_hat = a W, everything counted."""
    g = np.random.default_rng(1)
    F, T, d, n = 3, 7, 5, 4
    W = g.normal(size=(n, d))
    a = np.maximum(g.normal(size=(F * T, n)), 0)
    a[:, 2] = 0
    x = a @ W + 0.3 * g.normal(size=(F * T, d)) + 1.0
    r = x - a @ W
    rep = RC.ReconstructionReport(
        n_frames=F * T, attr_sum=(a * (r @ W.T)).sum(0), act_sq_sum=(a * a).sum(0), dec_norm_sq=(W * W).sum(1).astype(np.float32),
        sum_x=x.sum(0), sum_x_sq=(x * x).sum(0), sum_r_sq=(r * r).sum(0), file_sse=(r * r).reshape(F, -1).sum(1),
        file_energy=(x * x).reshape(F, -1).sum(1), filenames=["a.wav", "b.wav", "c.wav"])
    return rep, x, a, W, r


def test_derived_quantities():
    rep, x, a, W, r = synthetic_report()
    sse = (r * r).sum()
    assert rep.sse() == pytest.approx(sse, rel=1e-12)
    tv = ((x - x.mean(0)) ** 2).sum()
    assert rep.total_variance() == pytest.approx(tv, rel=1e-10)
    assert rep.fvu() == pytest.approx(sse / tv, rel=1e-10)
    np.testing.assert_allclose(rep.fvu_by_dim(), (r * r).sum(0) / ((x - x.mean(0)) ** 2).sum(0), rtol=1e-10)
    np.testing.assert_allclose(rep.file_nmse(), rep.file_sse / rep.file_energy, rtol=1e-12)
    worst = rep.worst_files(2)
    order = np.argsort(-rep.file_nmse())
    assert [w[0] for w in worst] == [int(order[0]), int(order[1])] and worst[0][1] == rep.filenames[order[0]]
    # the ablation IS the change of the summed squared error when the latent is zeroed (exact: the decoder is linear)
    for j in range(4):
        a0 = a.copy()
        a0[:, j] = 0
        want = ((x - a0 @ W) ** 2).sum() - sse
        assert rep.ablation()[j] == pytest.approx(want, rel=1e-5, abs=1e-9), j      # (dec_norm_sq is float32)
    np.testing.assert_allclose(rep.ablation_share(), rep.ablation() / sse, rtol=1e-12)
    # the rescale IS the least-squares gain of the latent with everything else fixed
    resc = rep.rescale()
    assert np.isnan(resc[2]) and rep.ablation()[2] == 0
    for j in (0, 1, 3):
        contrib = a[:, j:j + 1] * W[j][None, :]
        target = r + contrib
        gain = (target * contrib).sum() / (contrib * contrib).sum()
        assert resc[j] == pytest.approx(gain, rel=1e-5), j
    top = rep.top_latents(4)
    assert [t[0] for t in top] == [int(i) for i in np.argsort(-rep.ablation(), kind="stable")]
    assert rep.top_latents(4, by="rescale")[-1][0] == 2, "NaN comes last"
    with pytest.raises(ValueError):
        rep.top_latents(2, by="size")
    s = rep.summary()
    assert s["n_frames"] == 21 and s["n_latents"] == 4 and s["n_files"] == 3
    assert s["fvu"] == pytest.approx(rep.fvu()) and s["top_latent"] == top[0][0]


def test_npz_round_trip(tmp_path):
    rep = synthetic_report()[0]
    p = str(tmp_path / "r.npz")
    rep.to_npz(p)
    back = RC.ReconstructionReport.from_npz(p)
    assert back.n_frames == rep.n_frames and isinstance(back.n_frames, int) and back.filenames == rep.filenames
    for k in R.FLOAT_FIELDS:
        a, b = getattr(back, k), getattr(rep, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


# ---- the boundary
def test_block_layout_matches_header():
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    n, d = 37, 11
    lay = E.recon_layout(n, d)

    def macro(name):
        m = re.search(rf"#define SAE_RECON_{name}\(n, d\) (.+)", text)
        assert m, name
        return eval(m.group(1).replace("(int64_t)", "").replace("/", "//"), {"n": n, "d": d})
    for name, mac in [("n_frames", "N_FRAMES"), ("attr_sum", "ATTR_SUM"), ("act_sq_sum", "ACT_SQ_SUM"), ("sum_x", "SUM_X"),
                      ("sum_x_sq", "SUM_X_SQ"), ("sum_r_sq", "SUM_R_SQ"), ("dec_norm_sq", "DEC_NORM_SQ")]:
        assert macro(mac) == lay[name][0], name
    assert macro("BYTES") == lay["bytes"] and lay["bytes"] % 8 == 0
    fields = [v for k, v in lay.items() if k != "bytes"]
    spans = sorted((off, off + np.dtype(dt).itemsize * cnt) for off, dt, cnt in fields)
    assert spans[0][0] == 0 and 0 <= lay["bytes"] - spans[-1][1] < 8
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(off % np.dtype(dt).itemsize == 0 for off, dt, _ in fields)


def test_from_block_reads_the_layout():
    n, d = 5, 3
    lay = E.recon_layout(n, d)
    blk = np.zeros(lay["bytes"], np.uint8)
    vals = {"n_frames": np.array([42]), "attr_sum": np.linspace(-1, 1, n), "act_sq_sum": np.linspace(2, 3, n), "sum_x": np.arange(d) - 1.0,
            "sum_x_sq": np.arange(d) + 5.0, "sum_r_sq": np.arange(d) + 0.5, "dec_norm_sq": np.linspace(4, 5, n)}
    for k, v in vals.items():
        off, dt, cnt = lay[k]
        blk[off:off + np.dtype(dt).itemsize * cnt] = np.asarray(v, dt).view(np.uint8)
    files = np.array([[1.0, 2.0], [3.0, 4.0]])
    rep = RC.ReconstructionReport.from_block(blk, n, d, files, ["a", "b"])
    assert rep.n_frames == 42 and rep.filenames == ["a", "b"]
    for k in ("attr_sum", "act_sq_sum", "sum_x", "sum_x_sq", "sum_r_sq"):
        np.testing.assert_array_equal(getattr(rep, k), vals[k])
    np.testing.assert_array_equal(rep.dec_norm_sq, vals["dec_norm_sq"].astype(np.float32))
    np.testing.assert_array_equal(rep.file_sse, [1.0, 3.0])
    np.testing.assert_array_equal(rep.file_energy, [2.0, 4.0])


def test_recon_symbol_exported_and_declared():
    E.build()
    lib = E.load()
    assert hasattr(lib, "sae_recon_files")
    assert "sae_recon_files" in E.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert re.search(r"\bint sae_recon_files\(", text)
    assert "SAE_RECON_UNFUSED = 1" in text and E.RECON_UNFUSED == 1
    names = [lib.sae_kernel_name(i) for i in range(64)]
    for k in (b"recon_decode", b"recon_resid", b"recon_attr"):
        assert k in names


# ---- argument errors that need no device
def _shards(tmp_path, F=4, T=10, d=16):
    x = np.random.default_rng(0).normal(size=(F, T * d)).astype(np.float32)
    write_shards(str(tmp_path), "enc", x, [T, d])
    return str(tmp_path)


def _fake_engine(d, n, precision):
    eng = E.SaeEngine.__new__(E.SaeEngine)
    eng.variant, eng.d, eng.n, eng.max_rows, eng.device_id, eng.precision = "l1", d, n, 1500, 0, precision
    eng._ctx = None
    return eng


def test_argument_errors(tmp_path):
    path = _shards(tmp_path)
    eng = _fake_engine(16, 64, "bf16")
    with pytest.raises(ValueError, match="batch_files"):
        RC.reconstruction_report(eng, path, "enc", batch_files=0)
    with pytest.raises(ValueError, match="one entry per file"):
        RC.reconstruction_report(eng, path, "enc", lengths=np.array([3, 4]))
    with pytest.raises(ValueError, match=">= 1"):
        RC.reconstruction_report(eng, path, "enc", lengths=np.array([3, 0, 4, 5]))
    with pytest.raises(ValueError, match="bf16"):
        RC.reconstruction_report(_fake_engine(16, 64, "fp8"), path, "enc")
    with pytest.raises(ValueError, match="d_model=32"):
        RC.reconstruction_report(_fake_engine(32, 64, "bf16"), path, "enc")
    with pytest.raises(ValueError, match="needs an SAE"):
        RC.reconstruction_report(None, path, "enc")
    with pytest.raises(ValueError, match="needs an SAE"):
        RC.reconstruction_report("none", path, "enc")
    with pytest.raises(TypeError):
        RC.reconstruction_report(object(), path, "enc")
