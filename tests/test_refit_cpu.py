"""CPU: the refit frontier without a device.

* freud_amd/csrc/refit_chol.h compiled for the host (g++ -Wall -Werror -ffp-contract=off, tests/refit_reference.py: SERIAL_SRC):
  rf_row_serial / rf_frame_serial against the float64 rule within the derived bounds on random and on correlated supports; a planted
  exact duplicate and a zero row are dependent and the curve repeats there; the prefix property to the bit; e non-increasing and
  non-negative; an orthogonal support; the ratio bin at every edge;
* the pivot ratios of the test dictionaries: every kept slot >= 0.05, every duplicate <= 1e-6 (the 2^-10 threshold sits decades from
  both), and no frame undecided -- from the reference alone;
* a float32 numpy emulation of the rule passes the checks and eight mutations of it each FAIL them;
* the module: RefitFrontier's arithmetic on a hand-made block, decompose, save / load, the argument rules;
* the boundary: refit_layout against the header's macros, the symbol in the header, EXPORTED_SYMBOLS and the built library."""
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from freud_amd import engine as E
from freud_amd import pursuit as P
from freud_amd import refit as RF
from freud_amd import sparsity_frontier as SF
from tests import refit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return R.build_serial(tmp_path_factory.mktemp("rf"), ROOT)


def unit_bf16(w):
    return R.bf16((w / np.linalg.norm(w, axis=-1, keepdims=True)).astype(np.float32))


def supports(kind, rows, K, d, seed, dup=True):
    """w [rows, K, d] unit bf16 directions (random, or strongly correlated: a shared direction plus noise, pairwise cosine ~0.5), with
    one exact duplicate planted per frame -> (w, active, the duplicate's slot per frame)."""
    g = np.random.default_rng(seed)
    w = g.normal(size=(rows, K, d))
    if kind == "correlated":
        w = w / np.sqrt(d) + g.normal(size=(rows, 1, d)) / np.sqrt(d)
    w = unit_bf16(w)
    where = np.full(rows, -1)
    if dup and K > 1:
        for r in range(rows):
            s = int(g.integers(1, K))
            w[r, s] = w[r, int(g.integers(0, s))]
            where[r] = s
    return w, np.ones((rows, K), np.uint8), where


def frames_x(w, seed, b):
    """Frames near the span of their support: a few rows with decaying amplitudes plus noise, plus b."""
    g = np.random.default_rng(seed)
    rows, K, d = w.shape
    a = g.normal(size=(rows, K)) * 2.0 ** -np.arange(K)[None, :].clip(max=6)
    x = np.einsum("rk,rkd->rd", a, w.astype(np.float64)) + 0.05 * g.normal(size=(rows, d))
    return (x + (0 if b is None else b)).astype(np.float32)


CASES = [("random", 12, 16, 128, 1), ("random", 6, 64, 256, 2), ("random", 4, 33, 768, 3), ("correlated", 12, 32, 128, 4)]


@pytest.mark.parametrize("kind,rows,K,d,seed", CASES)
def test_serial_against_the_float64_rule(prog, tmp_path, kind, rows, K, d, seed):
    w, act, where = supports(kind, rows, K, d, seed)
    b = R.bf16(0.3 * np.random.default_rng(seed + 50).normal(size=d).astype(np.float32))
    x = frames_x(w, seed + 100, b)
    r0 = R.r0_fp32(x, b)
    fs = R.frames(w, act, r0)
    # the reference alone: ratios far from the threshold on both sides, nothing undecided
    ratios = np.array([f.ratio for f in fs])
    dupmask = np.arange(K)[None, :] == where[:, None]
    print(f"{kind} d={d} K={K}: kept ratios >= {ratios[~dupmask].min():.3g}, duplicates <= {ratios[dupmask].max():.3g}")
    assert (ratios[~dupmask] >= 0.05).all() and (ratios[dupmask] <= 1e-6).all()
    assert R.assert_decided(fs).all()
    o = R.serial_frames(prog, tmp_path, w, act, x, b)
    d_p = R.round_up(d, 128)
    worst = 0.0
    for r, f in enumerate(fs):
        assert np.abs(f.e - R.lstsq_prefix_errors(w[r], f.kept, r0[r])).max() <= 1e-9 * f.e0          # the rule IS lstsq on every prefix
        G64 = w[r].astype(np.float64) @ w[r].astype(np.float64).T
        assert (np.abs(o["G"][r, :K] - G64) <= R.gram_bound(w[r], d_p)).all()
        assert (np.abs(o["G"][r, K] - w[r].astype(np.float64) @ r0[r].astype(np.float64)) <= R.c_bound(w[r], r0[r], d_p)).all()
        err = np.abs(o["e"][r] - f.e)
        worst = max(worst, float((err / f.e0).max()))
        assert (err <= f.curve_bound(d_p)).all()
        assert abs(float(o["e_final"][r, 0]) - float(o["e"][r, K])) <= f.final_bound(d_p)
        assert ((o["d"][r] > 0) == f.kept).all() and int(o["kept"][r, 0]) == int(f.kept.sum())
        assert np.abs(o["a"][r] - f.coef).max() <= 1e-3 * max(1.0, np.abs(f.coef).max())
        # the duplicate: dependent, coefficient +0.0, the curve repeats
        s = where[r]
        assert o["dep"][r, s] == 1 and o["dep"][r].sum() == 1 and o["a"][r, s].tobytes() == np.float32(0).tobytes()
        assert o["e"][r, s + 1].tobytes() == o["e"][r, s].tobytes()
        assert (np.diff(o["e"][r]) <= 0).all() and (o["e"][r] >= 0).all()
    print(f"{kind} d={d} K={K}: worst |e - e64| / e_0 = {worst:.3e}")


def test_zero_row_inactive_slot_and_prefix_property(prog, tmp_path):
    w, act, _ = supports("random", 6, 24, 128, 9, dup=False)
    w[:, 5] = 0                                 # a zero row: G[s][s] == 0 is dependent
    act[:, 11] = 0                              # an inactive slot
    x = frames_x(w, 10, None)
    o = R.serial_frames(prog, tmp_path, w, act, x, None)
    assert (o["dep"][:, 5] == 1).all() and (o["dep"][:, 11] == 0).all() and (o["d"][:, 11] == 0).all() and (o["a"][:, [5, 11]] == 0).all()
    assert (o["e"][:, 6] == o["e"][:, 5]).all() and (o["e"][:, 12] == o["e"][:, 11]).all() and (o["kept"][:, 0] == 22).all()
    # a run at K' is the bitwise prefix of the run at K
    for Kp in (1, 7, 12, 23):
        p = R.serial_frames(prog, tmp_path, w[:, :Kp], act[:, :Kp], x, None)
        for name, cnt in (("e", Kp + 1), ("y", Kp), ("d", Kp), ("dep", Kp)):
            assert p[name].tobytes() == np.ascontiguousarray(o[name][:, :cnt]).tobytes(), (Kp, name)
        assert p["G"][:, :Kp].tobytes() == np.ascontiguousarray(o["G"][:, :Kp, :Kp]).tobytes()


def test_orthogonal_support(prog, tmp_path):
    """Rows 2 e_j: G = 4 I, so d = 2, y = c / 2 and a = c / 4 -- the dot product to the bit of one division; the curve is
    e_0 - sum y^2 in slot order."""
    K, d = 8, 128
    w = np.zeros((3, K, d), np.float32)
    for r in range(3):
        w[r, np.arange(K), 7 * np.arange(K) + r] = 2.0
    x = np.random.default_rng(1).normal(size=(3, d)).astype(np.float32)
    o = R.serial_frames(prog, tmp_path, w, np.ones((3, K), np.uint8), x, None)
    c = o["G"][:, K]
    assert (c == 2 * x[np.arange(3)[:, None], 7 * np.arange(K)[None, :] + np.arange(3)[:, None]]).all()
    assert (o["a"].view(np.uint32) == (c / np.float32(4)).view(np.uint32)).all() and (o["d"] == 2).all() and not o["dep"].any()
    assert (o["y"].view(np.uint32) == (c / np.float32(2)).view(np.uint32)).all()


def test_ratio_bin_edges(prog, tmp_path):
    edges = RF.ratio_edges().astype(np.float32)
    assert edges[0] == 2.0 ** -4 and edges[-1] == 16 and edges[4] == 2.0 ** -3 and edges[1] == np.float32(2.0 ** -4 * 1.25)
    below = np.nextafter(edges, np.float32(0))
    got_at, got_below = R.serial_bins(prog, tmp_path, edges), R.serial_bins(prog, tmp_path, below)
    assert got_at.tolist() == [3 + i for i in range(32)] + [35] and got_below.tolist() == [2] + [3 + i for i in range(32)]
    special = np.array([0.0, -0.0, -1e-30, -1.0, -np.inf, 1e-40, 1e-30, np.inf, np.nan, 1.0, 3.99], np.float32)
    assert R.serial_bins(prog, tmp_path, special).tolist() == [1, 1, 0, 0, 0, 2, 2, 35, 35, 3 + 16, 3 + 23]      # (3.99: octave [2, 4), top sub-bin)
    assert E.REFIT_RATIO_BINS == RF.RATIO_BINS == 36


# ---- a float32 emulation of the rule, with the mistakes the checks must catch ------------------------------------------------
f32 = np.float32


def fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def emulate(w, act, x, b, mut=None):
    """One frame by the rule in float32 -> (e [K + 1], a [K], e_final, kept [K]).  mut: one of MUTATIONS."""
    K, d = w.shape
    w = w.astype(f32)
    r0 = x.astype(f32) if (b is None or mut == "b_dropped") else (x.astype(f32) - b.astype(f32)).astype(f32)
    csrc = x.astype(f32) if mut == "c_from_x" else r0
    G = (w.astype(np.float64) @ w.astype(np.float64).T).astype(f32)
    c = (w.astype(np.float64) @ csrc.astype(np.float64)).astype(f32)
    L = np.zeros((K, K), f32)
    dd, y, kept = np.zeros(K, f32), np.zeros(K, f32), np.zeros(K, bool)
    chain = np.zeros(K, bool)                   # the slots later chains run over
    e = [f32((r0.astype(np.float64) ** 2).sum())]
    thr = f32(0) if mut == "threshold_0" else f32(2.0 ** -10)
    for s in range(K):
        e.append(e[-1])
        if not act[s]:
            continue
        for t in range(s):
            if not chain[t]:
                continue
            v = G[s, t]
            for u in range(t):
                if chain[u]:
                    v = fma(-L[s, u], L[u, t] if mut == "L_transposed" else L[t, u], v)
            L[s, t] = f32(v / dd[t])
        piv = G[s, s]
        for u in range(s):
            if chain[u]:
                piv = fma(-L[s, u], L[s, u], piv)
        if piv <= f32(thr * G[s, s]):
            if mut == "dependent_not_skipped":  # the slot is reported dependent but stays in the later chains, root and y included
                chain[s] = True
                with np.errstate(invalid="ignore", divide="ignore"):
                    dd[s] = f32(np.sqrt(piv))
                    v = c[s]
                    for u in range(s):
                        if chain[u]:
                            v = fma(-L[s, u], y[u], v)
                    y[s] = f32(v / dd[s])
            if mut == "stale_y_in_walk":        # the y it would have had, left behind for the walk
                y[s] = f32(c[s] / np.sqrt(G[s, s])) if G[s, s] > 0 else f32(0)
            continue
        dd[s] = f32(np.sqrt(piv))
        kept[s] = chain[s] = True
        v = c[s]
        for u in range(s):
            if chain[u]:
                v = fma(-L[s, u], y[u], v)
        y[s] = f32(v / dd[s])
        nxt = fma(-y[s], y[s], e[-2])
        e[-1] = nxt if mut == "no_clamp" else max(nxt, f32(0))
    a = np.zeros(K, f32)
    order = range(K) if mut == "ascending_back_substitution" else range(K - 1, -1, -1)
    for s in order:
        if not kept[s]:
            continue
        v = y[s]
        others = range(s) if mut == "ascending_back_substitution" else range(K - 1, s, -1)
        for u in others:
            if kept[u]:
                v = fma(-(L[s, u] if mut == "ascending_back_substitution" else L[u, s]), a[u], v)
        a[s] = f32(v / dd[s])
    r = r0.copy()
    for s in range(K):
        coef = a[s] if kept[s] else (y[s] if mut == "stale_y_in_walk" and act[s] else f32(0))
        r = (r - coef * w[s]).astype(f32)
    return np.array(e, f32), a, f32((r.astype(np.float64) ** 2).sum()), kept


MUTATIONS = ["threshold_0", "dependent_not_skipped", "ascending_back_substitution", "b_dropped", "no_clamp", "L_transposed", "c_from_x",
             "stale_y_in_walk"]


def emulation_cases():
    """Frames for the checks: correlated supports with a duplicate each, a bias, and frames that lie IN the span of their support
    (the fit is exact: e reaches 0 from above and below in float32 -- the frames that need the clamp)."""
    w, act, where = supports("correlated", 40, 12, 128, 21)
    b = R.bf16(0.5 * np.random.default_rng(22).normal(size=128).astype(np.float32))
    x = frames_x(w, 23, b)
    g = np.random.default_rng(24)
    for r in range(20, 40):                     # exactly representable combinations of the first three rows
        x[r] = (b.astype(np.float64) + w[r, :3].astype(np.float64).T @ g.integers(1, 4, 3)).astype(np.float32)
    return w, act, x, b


def violations(w, act, x, b, mut):
    """The checks of the tests on the emulation's output: the curve and e_final within their bounds, the kept set, e >= 0."""
    r0 = R.r0_fp32(x, b)
    bad = 0
    for r in range(len(w)):
        f = R.Frame(w[r], act[r], r0[r])
        e, a, ef, kept = emulate(w[r], act[r], x[r], b, mut)
        # (a frame inside its support's span has r_0 with rounded entries: the bound's e_0 term covers it)
        ok = (np.abs(e.astype(np.float64) - f.e) <= f.curve_bound(128)).all() and abs(float(ef) - float(e[-1])) <= f.final_bound(128)
        ok = ok and (kept == f.kept).all() and (e >= 0).all() and (np.diff(e) <= 0).all()
        bad += not ok
    return bad


def test_the_emulation_passes_and_eight_mutations_fail():
    w, act, x, b = emulation_cases()
    assert violations(w, act, x, b, None) == 0
    for mut in MUTATIONS:
        n = violations(w, act, x, b, mut)
        print(f"{mut}: {n} of {len(w)} frames fail")
        assert n > 0, mut


# ---- the module ----------------------------------------------------------------------------------------------------------------
def hand_block():
    K, d, n, n_tau = 3, 2, 5, 2
    lay = E.refit_layout(n_tau, K, d, n)
    blk = np.zeros(lay["bytes"], np.uint8)

    def put(name, vals):
        off, dt, cnt = lay[name]
        blk[off:off + cnt * np.dtype(dt).itemsize] = np.asarray(vals, dt).reshape(cnt).view(np.uint8)
    put("n_frames", [10]); put("sse", [100, 30, 8, 4]); put("sse_final", [4.5]); put("sum_x", [10, 20]); put("sum_x_sq", [110, 140])
    put("budget", [0, 7, 2, 1, 0, 0, 0, 4, 5, 1]); put("kept", [0, 1, 3, 6]); put("slots", [9, 0, 8, 0, 7]); put("neg", [3, 0, 0, 0, 1])
    put("dep", [0, 0, 2, 0, 1]); put("bad_index", [0])
    ratio = np.zeros(36, np.int64)
    ratio[[0, 1, 3 + 16, 3 + 17, 35]] = [2, 1, 10, 6, 1]
    put("ratio", ratio)
    return blk, lay


def test_module_arithmetic(tmp_path):
    K, d, n = 3, 2, 5
    blk, lay = hand_block()
    assert lay["bytes"] == lay["bad_index"][0] + 8 and len({v[0] for k, v in lay.items() if k != "bytes"}) == 12
    rf = RF.RefitFrontier.from_block(blk, K, SF.check_thresholds((0.5, 0.1)), d, n)
    tv = (110 - 100 / 10) + (140 - 400 / 10)
    assert rf.n_frames == 10 and rf.d == d and rf.n == n and rf.total_variance() == tv
    assert np.allclose(rf.fvu_curve(), np.array([100, 30, 8, 4]) / tv) and rf.fvu(3) == 4 / tv and rf.final_fvu() == 4.5 / tv
    assert rf.marginal().tolist() == [70, 22, 4] and rf.budget_for_fvu(0.05) == 2
    assert rf.frame_budget_hist(0.5).tolist() == [0, 7, 2, 1, 0] and rf.frame_budget_quantile(0.1, 0.5) == 3
    assert rf.kept_hist().tolist() == [0, 1, 3, 6]
    per, tot = rf.dependent_fraction()
    assert np.allclose(per[[0, 2, 4]], [0, 2 / 8, 1 / 7]) and np.isnan(per[1]) and tot == 3 / 24
    per, tot = rf.negative_fraction()
    assert np.allclose(per[[0, 2, 4]], [3 / 9, 0, 1 / 7]) and tot == 4 / 24
    assert rf.shrinkage_hist().sum() == 20 and rf.shrinkage_quantile(0.5) == 1.0 and rf.shrinkage_quantile(0.05) == float("-inf")
    assert rf.shrinkage_quantile(0.9) == 1.25 and rf.shrinkage_quantile(1.0) == 16.0 and rf.shrinkage_quantile(0.15) == 0.0
    fr = SF.SparsityFrontier(K=3, thresholds=rf.thresholds, n_frames=10, rows_cut=0, active_cut=0, sse=np.array([100.0, 50.0, 30.0, 20.0]),
                             sum_x=rf.sum_x, sum_x_sq=rf.sum_x_sq, budget=np.zeros((2, 5), np.int64))
    pu = P.PursuitFrontier(K=2, thresholds=rf.thresholds, n_frames=10, sse=np.array([100.0, 25.0, 6.0]), sum_x=rf.sum_x, sum_x_sq=rf.sum_x_sq,
                           budget=np.zeros((2, 4), np.int64), steps=np.zeros(3, np.int64), picks=np.zeros(n, np.int64),
                           in_support=np.zeros(2, np.int64))
    c = rf.compare(fr)
    assert c.shape == (4, 2) and np.allclose(c[:, 0] - c[:, 1], np.array([0, 20, 22, 16]) / tv)
    dec = rf.decompose(fr, pu)
    assert np.allclose(dec["coefficient_gap"], np.array([0, 20, 22]) / tv) and np.allclose(dec["support_gap"], np.array([0, 5, 2]) / tv)
    assert np.allclose(dec["coefficient_gap"] + dec["support_gap"], pu.amortisation_gap(fr))
    with pytest.raises(ValueError, match="frames"):
        rf.decompose(dataclasses.replace(fr, n_frames=9), pu)
    with pytest.raises(ValueError, match="d="):
        rf.compare(dataclasses.replace(fr, sum_x=np.zeros(3), sum_x_sq=np.zeros(3)))
    rf.save(str(tmp_path / "r.npz"))
    back = RF.RefitFrontier.load(str(tmp_path / "r.npz"))
    assert all(np.array_equal(getattr(back, k), getattr(rf, k)) for k in ("sse", "budget", "kept", "slots", "neg", "dep", "ratio", "thresholds"))
    assert back.K == K and back.sse_final == 4.5 and back.summary() == rf.summary() and rf.summary()["mean_kept"] == 2.5


def test_argument_rules():
    assert RF.check_K(None, "topk", 1024, 32) == 32 and RF.check_K(None, "l1", 1024, 0) == 64 and RF.check_K(None, "topk", 4096, 512) == 128
    assert RF.check_K(128, "l1", 1024, 0) == 128 and RF.check_K(100, "topk", 64, 8, given=True) == 100
    for bad in ((0, "l1", 64, 0), (129, "l1", 1024, 0), (9, "topk", 64, 8), (65, "l1", 64, 0)):
        with pytest.raises(ValueError):
            RF.check_K(*bad)
    with pytest.raises(ValueError, match="needs an SAE"):
        RF.refit_frontier(None, "/nonexistent", "enc")
    with pytest.raises(ValueError):
        RF.refit_frontier("none", "/nonexistent", "enc", thresholds=(2.0,))


def test_boundary():
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert re.search(r"\bint sae_refit_files\(", hdr) and "sae_refit_files" in E.EXPORTED_SYMBOLS
    assert hasattr(E.load(), "sae_refit_files")
    assert f"#define SAE_REFIT_MAX_K {E.REFIT_MAX_K}" in hdr and f"#define SAE_REFIT_MAX_TAU {E.REFIT_MAX_TAU}" in hdr
    assert (RF.MAX_K, RF.MAX_TAU) == (E.REFIT_MAX_K, E.REFIT_MAX_TAU)
    names = ["N_FRAMES", "SSE", "SSE_FINAL", "SUM_X", "SUM_X_SQ", "BUDGET", "KEPT", "SLOTS", "NEG", "DEP", "RATIO", "BAD_INDEX", "BYTES"]
    src = '#include <stdio.h>\n#include <stdint.h>\n#include "freud_sae.h"\nint main(){' + "".join(
        f'printf("%lld\\n", (long long)SAE_REFIT_{nm}(3, 17, 200, 1000));' for nm in names) + "return 0;}"
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "m.c"), "w").write(src)
        subprocess.run(["gcc", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(td, "m.c"), "-o", os.path.join(td, "m")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "m")], check=True, capture_output=True, text=True).stdout.split()]
    lay = E.refit_layout(3, 17, 200, 1000)
    assert got == [lay[k.lower()][0] for k in names[:-1]] + [lay["bytes"]]
    # refit.h defines kernels: it belongs to exactly one translation unit
    mk = open(os.path.join(ROOT, "freud_amd", "csrc", "Makefile")).read()
    assert "refit.h" in re.search(r"^HDRS_passes := (.*)$", mk, re.M).group(1) and "refit.h" not in re.search(r"^HDRS_engine := (.*)$", mk, re.M).group(1)
    units = [f for f in ("engine.hip", "passes.hip") if '#include "refit.h"' in open(os.path.join(ROOT, "freud_amd", "csrc", f)).read()]
    assert units == ["passes.hip"]
