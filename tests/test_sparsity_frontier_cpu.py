"""CPU: the sparsity frontier without a device.

* the host half of freud_amd/csrc/frontier.h (fr_row_serial: the walk, the norms in the kernel's own order, the budget predicate)
  compiled with g++ -Wall -Werror into a stand-alone program and replayed against the float64 rule of tests/frontier_reference.py
  on built rows: K = 1, K = 37 (no power of two, across the slot chunk of 32), K = 256, a row of only padding slots, e_0 == 0 (the
  threshold met at s = 0), a threshold met at s = K and one never met, a non-monotone e_s, d no multiple of 128;
* the bounds can fail: six deliberately wrong answers are each caught;
* the module: the derived quantities on hand-made arrays, the npz round trip, compare_pca and its d mismatch;
* the boundary: frontier_layout against the header's macros, the symbol in the header, EXPORTED_SYMBOLS and the built library,
  the one unit that builds frontier.h, the constants;
* the argument rules that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

from freud_amd import engine as E
from freud_amd import sparsity_frontier as SF
from freud_amd.input_pca import InputCovariance
from freud_amd.loader import write_shards
from tests import build_units
from tests import frontier_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frontier.h"

// argv: data file -- int32 rows, K, d_p, n_tau, has_b; float taus[n_tau]; per row float vals[K], w[K][d_p], x[d_p], b[d_p] (if has_b)
// -> per row one line of the K + 1 norms' bits and one of the n_tau budgets
int main(int argc, char** argv) {
  FILE* fp = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int32_t h[5];
  if (!fp || fread(h, 4, 5, fp) != 5) return 2;
  const int rows = h[0], K = h[1], d_p = h[2], n_tau = h[3], has_b = h[4];
  if (K < 1 || K > FR_MAX_K || d_p % 128 || d_p > FR_MAX_D || n_tau > FR_MAX_TAU) return 2;
  std::vector<float> taus(n_tau ? n_tau : 1), vals(K), w((size_t)K * d_p), x(d_p), b(d_p), e(K + 1);
  std::vector<int> bud(n_tau ? n_tau : 1);
  if (n_tau && fread(taus.data(), 4, n_tau, fp) != (size_t)n_tau) return 2;
  for (int r = 0; r < rows; ++r) {
    if (fread(vals.data(), 4, K, fp) != (size_t)K || fread(w.data(), 4, w.size(), fp) != w.size() || fread(x.data(), 4, d_p, fp) != (size_t)d_p) return 2;
    if (has_b && fread(b.data(), 4, d_p, fp) != (size_t)d_p) return 2;
    fr_row_serial(K, vals.data(), w.data(), x.data(), has_b ? b.data() : NULL, d_p, taus.data(), n_tau, e.data(), bud.data());
    for (int s = 0; s <= K; ++s) { uint32_t u; memcpy(&u, &e[s], 4); printf("%08x ", u); }
    printf("\n");
    for (int t = 0; t < n_tau; ++t) printf("%d ", bud[t]);
    printf("\n");
  }
  fclose(fp);
  // the predicate on its own: <=, against e[0], K + 1 when never met
  const float e3[4] = {8.f, 4.f, 4.f, 1.f};
  if (fr_budget(e3, 3, 0.5f) != 1 || fr_budget(e3, 3, 0.125f) != 3 || fr_budget(e3, 3, 0.1f) != 4 || fr_budget(e3, 2, 0.4f) != 3) return 3;
  const float z[2] = {0.f, 0.f};
  if (fr_budget(z, 1, 0.5f) != 0) return 3;
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("fr")
    src = d / "fr.cpp"
    src.write_text(_SRC)
    exe = d / "fr"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def serial(prog, tmp_path, vals, wrows, x, b, taus):
    """fr_row_serial on rows: vals [R, K], wrows [R, K, d_p], x [R, d_p], b [d_p] or None -> (e float32 [R, K + 1], budgets [R, n_tau])."""
    vals, wrows, x = (np.ascontiguousarray(a, np.float32) for a in (vals, wrows, x))
    Rn, K = vals.shape
    d_p = x.shape[1]
    taus = np.asarray(taus, np.float32)
    blob = [np.array([Rn, K, d_p, len(taus), int(b is not None)], np.int32).tobytes(), taus.tobytes()]
    for r in range(Rn):
        blob += [vals[r].tobytes(), wrows[r].tobytes(), x[r].tobytes()]
        if b is not None:
            blob.append(np.ascontiguousarray(b, np.float32).tobytes())
    data = tmp_path / "rows.bin"
    data.write_bytes(b"".join(blob))
    out = subprocess.run([prog, str(data)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 2 * Rn
    e = np.array([[int(v, 16) for v in out[2 * r].split()] for r in range(Rn)], np.uint32).view(np.float32).reshape(Rn, K + 1)
    bud = np.array([[int(v) for v in out[2 * r + 1].split()] for r in range(Rn)], np.int64).reshape(Rn, len(taus))
    return e, bud


def pad(a, d_p):
    out = np.zeros(a.shape[:-1] + (d_p,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def built_rows(K, d, seed, with_b=True):
    """Rows of K slots on d dimensions: a dictionary of bf16-valued unit-ish rows, sorted positive values, and per row an x that
    makes one case.  -> (vals [R, K], idx [R, K], w_op [n, d], x [R, d], b or None, names)."""
    g = np.random.default_rng(seed)
    n = max(2 * K, 8)
    w_op = R.bf16(g.normal(0, 1, (n, d)).astype(np.float32) / np.sqrt(d))
    b = R.bf16(0.3 * g.normal(size=d).astype(np.float32)).astype(np.float32) if with_b else None
    bb = b if with_b else np.zeros(d, np.float32)

    def slots(nnz):
        v = np.zeros(K, np.float32)
        v[:nnz] = -np.sort(-R.bf16(g.uniform(0.5, 3.0, nnz).astype(np.float32)))
        return v, g.permutation(n)[:K]
    rows, names = [], []
    # 1. the row is its own reconstruction plus a little: the error falls to nearly nothing
    v, i = slots(K)
    rows.append((v, i, bb + v @ w_op[i] + 0.01 * g.normal(size=d)))
    names.append("reconstructed")
    # 2. only padding slots
    v, i = slots(0)
    rows.append((v, i, bb + g.normal(size=d)))
    names.append("padding only")
    # 3. e_0 == 0: x is b to the bit (the threshold is met at s = 0), the slots then raise the error
    v, i = slots(min(K, 3))
    rows.append((v, i, bb.copy()))
    names.append("e_0 == 0")
    # 4. met at s = K only: one-hot operand rows (appended to the dictionary) of length 1/16, the LAST of length 4, every value 1 (one
    # long tie), and a residue of 0.5 on a dimension no slot touches: e_s = 16 + (K - 1 - s) / 256 + 0.25 until the last slot takes
    # the 16 away -- tau = 0.5 and 0.1 are met at s = K, tau = 0.001 never
    if K >= 2 and d >= K + 1:
        alpha = np.full(K, 0.0625, np.float32)
        alpha[K - 1] = 4.0
        w_op = np.concatenate([w_op, alpha[:, None] * np.eye(K, d, dtype=np.float32)])
        xr = bb + pad(alpha, d)
        xr[K] += 0.5
        rows.append((np.ones(K, np.float32), n + np.arange(K), xr))
        names.append("met at K")
    # 5. never met: the slots miss most of x
    v, i = slots(K)
    rows.append((v, i, bb + 0.05 * (v @ w_op[i]) + 3.0 * g.normal(size=d)))
    names.append("never met")
    # 6. not monotone: the first slot's direction enters x with the opposite sign, so taking it RAISES the error
    v, i = slots(K)
    rows.append((v, i, bb - 2.0 * v[0] * w_op[i[0]] + (v[1:] @ w_op[i[1:]] if K > 1 else 0) + 0.01 * g.normal(size=d)))
    names.append("not monotone")
    vals = np.stack([r[0] for r in rows])
    idx = np.stack([r[1] for r in rows])
    x = np.stack([np.asarray(r[2], np.float32) for r in rows])
    return vals, idx, w_op, x, b, names


TAUS = np.array([0.5, 0.1, 0.001], np.float32)


@pytest.mark.parametrize("K,d,with_b", [(1, 128, True), (37, 256, True), (256, 384, False), (37, 200, True), (5, 72, False)])
def test_host_half_against_the_float64_rule(prog, tmp_path, K, d, with_b):
    vals, idx, w_op, x, b, names = built_rows(K, d, seed=K * 1000 + d, with_b=with_b)
    d_p = R.round_up(d, 128)
    ref = R.reference(vals, idx, w_op, x, b, d_p=d_p)
    e, bud = serial(prog, tmp_path, vals, pad(w_op[idx], d_p), pad(x, d_p), None if b is None else pad(b, d_p), TAUS)
    bad = R.e_violations(e, ref)
    rel = np.abs(e - ref.E) / np.maximum(ref.B, 1e-300)
    print(f"K={K} d={d}: worst |e - E| / bound = {rel.max():.3e}; rows {names}")
    assert not bad.any()
    for t, tau in enumerate(TAUS):
        dec = ref.decided(tau)
        assert dec.all(), (float(tau), [names[r] for r in np.flatnonzero(~dec)])          # the built rows are all decided
        assert not R.budget_violations(bud[:, t], ref, tau).any(), (float(tau), bud[:, t].tolist(), ref.budgets(tau)[0].tolist())
    by = dict(zip(names, range(len(names))))
    assert (e[by["padding only"]] == e[by["padding only"], 0]).all() and (bud[by["padding only"]] == K + 1).all()
    assert e[by["e_0 == 0"], 0] == 0 and (bud[by["e_0 == 0"]] == 0).all() and e[by["e_0 == 0"], 1] > 0
    assert (bud[by["never met"]] == K + 1).all()
    assert e[by["not monotone"], 1] > e[by["not monotone"], 0]
    if "met at K" in by:
        assert bud[by["met at K"], 1] == K and bud[by["met at K"], 2] == K + 1 and bud[by["met at K"], 0] == K


def test_padding_slot_repeats_the_norm_to_the_bit(prog, tmp_path):
    g = np.random.default_rng(3)
    K, d = 9, 128
    w = R.bf16(g.normal(size=(1, K, d)).astype(np.float32))
    vals = np.array([[2.0, 1.0, 0.5, 0, 0, 0, 0, 0, 0]], np.float32)
    e, _ = serial(prog, tmp_path, vals, w, g.normal(size=(1, d)).astype(np.float32), None, TAUS)
    assert (e[0, 3:].view(np.uint32) == e[0, 3].view(np.uint32)).all() and len(set(e[0, :4].tolist())) == 4


# ---- the bounds can fail
@pytest.fixture(scope="module")
def case():
    """185 rows of K = 32 slots at d = 256 with a bias: planted frames (six dictionary rows with falling amplitudes), the slots the
    six planted latents in value order and 26 more."""
    g = np.random.default_rng(5)
    Rn, K, d, n = 185, 32, 256, 512
    w_op = R.bf16(g.normal(0, 1, (n, d)).astype(np.float32) / np.sqrt(d))
    b = (0.3 * g.normal(size=d)).astype(np.float32)
    vals, idx = np.empty((Rn, K), np.float32), np.empty((Rn, K), np.int64)
    x = np.empty((Rn, d), np.float32)
    for r in range(Rn):
        idx[r] = g.permutation(n)[:K]
        v = np.concatenate([8 * 0.6 ** np.arange(6) * (1 + 0.1 * g.uniform(-1, 1, 6)), g.uniform(0.01, 0.2, K - 6)])
        vals[r] = -np.sort(-R.bf16(v.astype(np.float32)))
        x[r] = b + vals[r] @ w_op[idx[r]] + 0.05 * g.normal(size=d)
    x[0] = b                                                     # a frame with e_0 == 0: budget 0, which `<` misses
    ref = R.reference(vals, idx, w_op, x, b)
    taus = np.array([0.5, 0.2, 0.1, 0.05], np.float32)
    R.assert_decidable(ref, taus, "mutations")
    return dict(vals=vals, idx=idx, w_op=w_op, x=x, b=b, ref=ref, taus=taus)


def flagged(case, **mut):
    e, bud = R.emulate(case["vals"], case["idx"], case["w_op"], case["x"], case["b"], case["taus"], **mut)
    ref = case["ref"]
    e_bad = R.e_violations(e, ref).any(1).mean()
    b_bad = max(R.budget_violations(bud[:, t], ref, tau).mean() for t, tau in enumerate(case["taus"]))
    print(f"{mut}: rows with a norm outside its bound {e_bad:.3f}, rows with a wrong budget {b_bad:.3f}")
    return e_bad, b_bad


def test_emulation_has_no_violation(case):
    assert flagged(case) == (0.0, 0.0)


def test_unsorted_slot_order_is_caught(case):
    assert flagged(case, order=np.arange(31, -1, -1))[0] >= 0.9


def test_plus_v_is_caught(case):
    assert flagged(case, sign=1.0)[0] >= 0.9


def test_b_left_out_is_caught(case):
    assert flagged(case, use_b=False)[0] >= 0.9


def test_norms_one_slot_off_are_caught(case):
    e_bad, b_bad = flagged(case, shift=1)
    assert e_bad >= 0.9 and b_bad >= 0.25


def test_strict_compare_is_caught(case):
    e_bad, b_bad = flagged(case, strict=True)
    assert e_bad == 0.0 and b_bad > 0.0                          # the norms are right; the frame with e_0 == 0 lands in K + 1


def test_threshold_against_x_is_caught(case):
    e_bad, b_bad = flagged(case, against_x=True)
    assert e_bad == 0.0 and b_bad >= 0.05


def test_non_finite_is_a_violation(case):
    e, _ = R.emulate(case["vals"], case["idx"], case["w_op"], case["x"], case["b"], case["taus"])
    e[3, 7] = np.nan
    bad = R.e_violations(e, case["ref"])
    assert bad[3, 7] and bad.sum() == 1


# ---- the module
def hand_made():
    K, d = 4, 3
    sse = np.array([100.0, 40.0, 10.0, 12.0, 2.0])
    sum_x = np.array([10.0, 0.0, -10.0])
    sum_x_sq = np.array([60.0, 50.0, 40.0])                       # n_frames = 10: variance by dim 50, 50, 30 -> 130
    budget = np.array([[1, 5, 3, 0, 0, 1], [0, 0, 2, 2, 2, 4]], np.int64)
    return SF.SparsityFrontier(K=K, thresholds=np.array([0.5, 0.1], np.float32), n_frames=10, rows_cut=3, active_cut=7, sse=sse, sum_x=sum_x,
                               sum_x_sq=sum_x_sq, budget=budget)


def test_derived_quantities():
    fr = hand_made()
    assert fr.d == 3 and fr.total_variance() == pytest.approx(130.0)
    np.testing.assert_allclose(fr.fvu_curve(), fr.sse / 130.0)
    assert fr.sse_curve() is fr.sse and fr.fvu(2) == pytest.approx(10 / 130)
    np.testing.assert_array_equal(fr.marginal(), [60.0, 30.0, -2.0, 10.0])
    assert fr.budget_for_fvu(0.5) == 1 and fr.budget_for_fvu(0.08) == 2 and fr.budget_for_fvu(0.02) == 4 and fr.budget_for_fvu(0.01) is None
    assert fr.budget_for_fvu(1.0) == 0
    np.testing.assert_array_equal(fr.frame_budget_hist(0.5), [1, 5, 3, 0, 0, 1])
    assert fr.frame_budget_quantile(0.5, 0.5) == 1 and fr.frame_budget_quantile(0.5, 0.1) == 0 and fr.frame_budget_quantile(0.5, 0.9) == 2
    assert fr.frame_budget_quantile(0.5, 1.0) == 5 and fr.frame_budget_quantile(0.1, 0.7) == 5      # K + 1: not within K
    assert fr.frame_budget_quantile(0.1, 0.5) == 4 and fr.cut_fraction() == pytest.approx(0.3)
    with pytest.raises(ValueError, match="not one of the thresholds"):
        fr.frame_budget_hist(0.3)
    with pytest.raises(ValueError):
        fr.fvu(5)
    with pytest.raises(ValueError):
        fr.frame_budget_quantile(0.5, 1.5)
    s = fr.summary()
    assert s["K"] == 4 and s["n_frames"] == 10 and s["fvu"]["4"] == pytest.approx(2 / 130) and s["median_budget"]["0.5"] == 1
    assert list(s["median_budget"]) == ["0.5", "0.1"]                 # the user's decimals, not float32's digits
    import json
    json.dumps(s)


def test_compare_pca_and_the_d_mismatch():
    fr = hand_made()
    S = np.diag([6.0, 3.0, 1.0])
    cov = InputCovariance(n_files=1, n_frames=10, d=3, center=np.zeros(3), mean=np.zeros(3), scatter=S)
    got = fr.compare_pca(cov)
    assert got.shape == (5, 2) and got.dtype == np.float64
    np.testing.assert_allclose(got[:, 0], fr.fvu_curve())
    np.testing.assert_allclose(got[:, 1], [1.0, 0.4, 0.1, 0.0, 0.0], atol=1e-12)       # ranks above d stay at the last entry
    bad = InputCovariance(n_files=1, n_frames=10, d=2, center=np.zeros(2), mean=np.zeros(2), scatter=np.eye(2))
    with pytest.raises(ValueError, match="d=2"):
        fr.compare_pca(bad)


def test_npz_round_trip(tmp_path):
    fr = hand_made()
    p = str(tmp_path / "f.npz")
    fr.to_npz(p)
    back = SF.SparsityFrontier.from_npz(p)
    for k in ("K", "n_frames", "rows_cut", "active_cut"):
        assert getattr(back, k) == getattr(fr, k) and isinstance(getattr(back, k), int)
    for k in ("thresholds", "sse", "sum_x", "sum_x_sq", "budget"):
        a, b = getattr(back, k), getattr(fr, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_from_block_reads_the_layout():
    n_tau, K, d = 2, 4, 3
    fr = hand_made()
    lay = E.frontier_layout(n_tau, K, d)
    blk = np.zeros(lay["bytes"], np.uint8)
    for k, v in {"n_frames": [10], "rows_cut": [3], "active_cut": [7], "sse": fr.sse, "sum_x": fr.sum_x, "sum_x_sq": fr.sum_x_sq,
                 "budget": fr.budget.reshape(-1)}.items():
        off, dt, cnt = lay[k]
        blk[off:off + np.dtype(dt).itemsize * cnt] = np.asarray(v, dt).view(np.uint8)
    back = SF.SparsityFrontier.from_block(blk, K, fr.thresholds, d)
    assert (back.n_frames, back.rows_cut, back.active_cut) == (10, 3, 7)
    for k in ("sse", "sum_x", "sum_x_sq", "budget"):
        np.testing.assert_array_equal(getattr(back, k), getattr(fr, k))


# ---- the boundary
def test_block_layout_matches_header():
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for n_tau, K, d in [(4, 64, 768), (0, 1, 5), (8, 256, 1536), (3, 37, 200)]:
        lay = E.frontier_layout(n_tau, K, d)

        def macro(name):
            m = re.search(rf"#define SAE_FRONTIER_{name}\(n_tau, K, d\) (.+)", text)
            assert m, name
            return eval(m.group(1).replace("(int64_t)", "").replace("/", "//"), {"n_tau": n_tau, "K": K, "d": d})
        for name in ("n_frames", "rows_cut", "active_cut", "sse", "sum_x", "sum_x_sq", "budget"):
            assert macro(name.upper()) == lay[name][0], name
        assert macro("BYTES") == lay["bytes"] and lay["bytes"] % 8 == 0
        fields = [v for k, v in lay.items() if k != "bytes"]
        spans = sorted((off, off + np.dtype(dt).itemsize * cnt) for off, dt, cnt in fields)
        assert spans[0][0] == 0 and spans[-1][1] == lay["bytes"]
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert lay["sse"][2] == K + 1 and lay["budget"][2] == n_tau * (K + 2)


def test_symbol_header_library_and_constants():
    raw = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+sae_frontier_files\s*\(", text)
    assert "sae_frontier_files" in E.EXPORTED_SYMBOLS
    E.build()
    lib = E.load()
    assert hasattr(lib, "sae_frontier_files")
    assert int(re.search(r"#define\s+SAE_FRONTIER_MAX_K\s+(\d+)", text).group(1)) == E.FRONTIER_MAX_K == SF.MAX_K == 256
    assert int(re.search(r"#define\s+SAE_FRONTIER_MAX_TAU\s+(\d+)", text).group(1)) == E.FRONTIER_MAX_TAU == SF.MAX_TAU == 8
    src = open(os.path.join(ROOT, "freud_amd", "csrc", "frontier.h")).read()
    assert int(re.search(r"#define\s+FR_MAX_K\s+(\d+)", src).group(1)) == 256
    assert int(re.search(r"#define\s+FR_CHUNK\s+(\d+)", src).group(1)) == R.FR_CHUNK
    assert int(re.search(r"#define\s+FR_UNIT\s+(\d+)", src).group(1)) == R.FR_UNIT
    assert build_units.assert_one_unit_builds("frontier.h") == "passes.hip"
    assert callable(E.SaeEngine.frontier_files)
    names = [lib.sae_kernel_name(i) for i in range(64)]
    for k in (b"frontier_sort", b"frontier_walk", b"frontier_fold"):
        assert k in names
    for out in ("K above a TopK context's k", "re-encoding under a budget", "raw (no-SAE) activations", "fp8 contexts", "per-frame output arrays",
                "NaN / Inf inputs"):
        assert out in raw, out


# ---- argument rules that need no device
class _OracleModel:
    """tests/fake_engine.py's OracleEngine, as it is, behind the two attributes and the one method file_pass asks a model for: the
    rules below read its public variant / d / n / k only and are all decided before a device is looked for."""

    def __init__(self, variant, d, n, k=0):
        from tests.fake_engine import OracleEngine
        self.eng = OracleEngine(variant, d, n, 1500, k=k)
        self.variant, self.n, self.k = self.eng.variant, self.eng.n, self.eng.k
        self.activation_size, self.n_dict_components = self.eng.d, self.eng.n

    def _ensure(self, rows):
        raise AssertionError("an argument rule let the pass reach the engine")


def _bare_engine(precision):
    """An SaeEngine without a context: the one rule that reads SaeEngine.precision (bf16 contexts only)."""
    eng = E.SaeEngine.__new__(E.SaeEngine)
    eng.variant, eng.d, eng.n, eng.max_rows, eng.device_id, eng.precision, eng.k = "l1", 16, 64, 1500, 0, precision, 0
    eng._ctx = None
    return eng


def test_argument_errors(tmp_path):
    from tests.fake_engine import OracleEngine
    x = np.random.default_rng(0).normal(size=(4, 10 * 16)).astype(np.float32)
    write_shards(str(tmp_path), "enc", x, [10, 16])
    path = str(tmp_path)
    sae = _OracleModel("l1", 16, 64)
    with pytest.raises(ValueError, match="needs an SAE"):
        SF.sparsity_frontier(None, path, "enc")
    with pytest.raises(ValueError, match="needs an SAE"):
        SF.sparsity_frontier("none", path, "enc")
    with pytest.raises(TypeError):                                   # the bare oracle stand-in is neither a model nor an engine
        SF.sparsity_frontier(OracleEngine("l1", 16, 64, 64), path, "enc", K=4)
    for bad in ((0.5,) * 9, (0.0,), (1.0,), (0.5, float("nan")), (-0.1,), (1e-60,)):
        with pytest.raises(ValueError, match="thresholds"):
            SF.sparsity_frontier(sae, path, "enc", thresholds=bad)
    for K in (0, -3, 257):
        with pytest.raises(ValueError, match="K="):
            SF.sparsity_frontier(sae, path, "enc", K=K)
    with pytest.raises(ValueError, match="K=65"):
        SF.sparsity_frontier(sae, path, "enc", K=65)                 # above n_dict
    with pytest.raises(ValueError, match="K=9"):
        SF.sparsity_frontier(_OracleModel("topk", 16, 64, k=8), path, "enc", K=9)
    with pytest.raises(ValueError, match="batch_files"):
        SF.sparsity_frontier(sae, path, "enc", batch_files=0)
    with pytest.raises(ValueError, match="one entry per file"):
        SF.sparsity_frontier(sae, path, "enc", lengths=np.array([3, 4]))
    with pytest.raises(ValueError, match=">= 1"):
        SF.sparsity_frontier(sae, path, "enc", lengths=np.array([3, 0, 4, 5]))
    with pytest.raises(ValueError, match="d_model=32"):
        SF.sparsity_frontier(_OracleModel("l1", 32, 64), path, "enc")
    with pytest.raises(ValueError, match="bf16"):
        SF.sparsity_frontier(_bare_engine("fp8"), path, "enc")
    assert SF.check_K(None, "l1", 512, 0) == 64 and SF.check_K(None, "l1", 40, 0) == 40 and SF.check_K(None, "topk", 4096, 32) == 32
    assert SF.check_K(None, "topk", 4096, 512) == 256 and SF.check_thresholds(()).size == 0
