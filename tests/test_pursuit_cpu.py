"""CPU: the pursuit frontier without a device.

* the host half of freud_amd/csrc/pursuit.h compiled with g++ -Wall -Werror into a stand-alone program: the pick key (signed scores,
  -0.0 as +0.0, the lower column wins a tie, key 0 is never eligible), the stop predicates, and the serial reference pu_row_serial
  replayed against tests/pursuit_reference.py on small random and planted rows;
* the bounds of tests/pursuit_reference.py hold for an fp32 / bf16 numpy emulation of the kernel's arithmetic, and eight mutations of
  the rule each FAIL the checks;
* the module: PursuitFrontier's arithmetic on a hand-made block, compare's refusals, save / load, check_K, the threshold checks;
* the boundary: pursuit_layout against the header's macros, the symbol in the header, EXPORTED_SYMBOLS and the built library, the one
  unit that builds pursuit.h."""
import os
import re
import subprocess

import numpy as np
import pytest

from freud_amd import engine as E
from freud_amd import pursuit as P
from freud_amd import sparsity_frontier as SF
from tests import pursuit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pursuit.h"

static int keys() {
  // signed scores order; -0.0 is +0.0; the lower column wins a tie; 0 is below every real key
  if (!(pu_key(2.f, 7) > pu_key(1.f, 3))) return 1;
  if (!(pu_key(1.f, 3) > pu_key(-1.f, 0))) return 2;
  if (!(pu_key(-1.f, 9) > pu_key(-2.f, 0))) return 3;
  if (pu_key(-0.f, 5) != pu_key(0.f, 5)) return 4;
  if (!(pu_key(1.f, 3) > pu_key(1.f, 4))) return 5;
  if (!(pu_key(-3.e38f, 0xFFFFFFu) > 0ull)) return 6;
  if (pu_key_col(pu_key(1.f, 123456)) != 123456u || pu_key_score(pu_key(-2.5f, 1)) != -2.5f) return 7;
  // eligibility: a padding column and a direction of norm 0 give the key 0
  if (pu_col_key(5.f, 1.f, 10, 10) != 0ull || pu_col_key(5.f, 0.f, 3, 10) != 0ull || pu_col_key(5.f, 0.5f, 3, 10) != pu_key(2.5f, 3)) return 8;
  // the stop predicates: no eligible key, a score <= 0, a coefficient that is not > 0 (NaN included)
  if (!pu_stops_on_key(0ull) || !pu_stops_on_key(pu_key(0.f, 1)) || !pu_stops_on_key(pu_key(-1.f, 1)) || pu_stops_on_key(pu_key(1e-30f, 1))) return 9;
  if (!pu_stops_on_coef(0.f) || !pu_stops_on_coef(-1.f) || !pu_stops_on_coef(NAN) || pu_stops_on_coef(1e-30f)) return 10;
  if (pu_z_of(0.f) != 0.f || pu_z_of(4.f) != 0.5f) return 11;
  return 0;
}

// argv: data file -- int32 rows, K, n, d_p, n_tau, has_b; float taus[n_tau]; W[n][d_p]; b[d_p] (if has_b); per row x[d_p]
// -> per row: idx[K] | val bits[K] | e bits[K + 1] | budgets[n_tau] | steps, one line each
int main(int argc, char** argv) {
  if (int rc = keys()) { fprintf(stderr, "key check %d\n", rc); return 3; }
  FILE* fp = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int32_t h[6];
  if (!fp || fread(h, 4, 6, fp) != 6) return 2;
  const int rows = h[0], K = h[1], n = h[2], d_p = h[3], n_tau = h[4], has_b = h[5];
  if (K < 1 || K > PU_MAX_K || d_p % 128 || d_p > FR_MAX_D || n_tau > PU_MAX_TAU) return 2;
  std::vector<float> taus(n_tau ? n_tau : 1), W((size_t)n * d_p), b(d_p), x(d_p), qz(2 * (size_t)n), val(K), e(K + 1);
  std::vector<int> idx(K), bud(n_tau ? n_tau : 1);
  if (n_tau && fread(taus.data(), 4, n_tau, fp) != (size_t)n_tau) return 2;
  if (fread(W.data(), 4, W.size(), fp) != W.size()) return 2;
  if (has_b && fread(b.data(), 4, d_p, fp) != (size_t)d_p) return 2;
  pu_consts_serial(W.data(), n, d_p, qz.data());
  for (int r = 0; r < rows; ++r) {
    if (fread(x.data(), 4, d_p, fp) != (size_t)d_p) return 2;
    const int steps = pu_row_serial(K, W.data(), n, qz.data(), x.data(), has_b ? b.data() : NULL, d_p, taus.data(), n_tau, idx.data(), val.data(),
                                    e.data(), bud.data());
    for (int s = 0; s < K; ++s) printf("%d ", idx[s]);
    printf("\n");
    for (int s = 0; s < K; ++s) { uint32_t u; memcpy(&u, &val[s], 4); printf("%08x ", u); }
    printf("\n");
    for (int s = 0; s <= K; ++s) { uint32_t u; memcpy(&u, &e[s], 4); printf("%08x ", u); }
    printf("\n");
    for (int t = 0; t < n_tau; ++t) printf("%d ", bud[t]);
    printf("\n%d\n", steps);
  }
  fclose(fp);
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("pu")
    src = d / "pu.cpp"
    src.write_text(_SRC)
    exe = d / "pu"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def pad(a, d_p):
    out = np.zeros(a.shape[:-1] + (d_p,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def serial(prog, tmp_path, w_op, x, b, K, taus):
    """pu_row_serial on rows -> (idx [R, K], val float32 [R, K], e float32 [R, K + 1], budgets [R, n_tau], steps [R])."""
    n, d = w_op.shape
    d_p = R.round_up(d, 128)
    taus = np.asarray(taus, np.float32)
    Rn = x.shape[0]
    blob = [np.array([Rn, K, n, d_p, len(taus), int(b is not None)], np.int32).tobytes(), taus.tobytes(), pad(np.asarray(w_op, np.float32), d_p).tobytes()]
    if b is not None:
        blob.append(pad(np.asarray(b, np.float32), d_p).tobytes())
    blob.append(pad(np.asarray(x, np.float32), d_p).tobytes())
    data = tmp_path / "rows.bin"
    data.write_bytes(b"".join(blob))
    out = subprocess.run([prog, str(data)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(out) >= 5 * Rn
    ints = lambda ln: [int(v) for v in ln.split()]
    hexs = lambda ln: [int(v, 16) for v in ln.split()]
    idx = np.array([ints(out[5 * r]) for r in range(Rn)], np.int64).reshape(Rn, K)
    val = np.array([hexs(out[5 * r + 1]) for r in range(Rn)], np.uint32).view(np.float32).reshape(Rn, K)
    e = np.array([hexs(out[5 * r + 2]) for r in range(Rn)], np.uint32).view(np.float32).reshape(Rn, K + 1)
    bud = np.array([ints(out[5 * r + 3]) for r in range(Rn)], np.int64).reshape(Rn, len(taus))
    steps = np.array([int(out[5 * r + 4]) for r in range(Rn)], np.int64)
    return idx, val, e, bud, steps


def dictionary(d, n, seed, unequal=False):
    """bf16-valued rows, roughly unit (unequal: norms between 0.25 and 4), and a bf16-valued bias."""
    g = np.random.default_rng(seed)
    w = g.normal(0, 1, (n, d)) / np.sqrt(d)
    if unequal:
        w *= 2.0 ** g.integers(-2, 3, n)[:, None]
    return R.bf16(w.astype(np.float32)), R.bf16(0.3 * g.normal(size=d).astype(np.float32))


def frames(w_op, b, seed, rows, nplant, sigma=0.044):
    g = np.random.default_rng(seed)
    n, d = w_op.shape
    x = np.tile(b, (rows, 1)) + sigma * g.normal(size=(rows, d))
    for r in range(rows):
        js = g.permutation(n)[:nplant]
        a = 8 * 0.6 ** np.arange(nplant) * (1 + 0.1 * g.uniform(-1, 1, nplant)) / np.linalg.norm(w_op[js], axis=1)
        x[r] += a @ w_op[js]
    return x.astype(np.float32)


def exact_case():
    """Scaled one-hot rows with bf16-exact entries (row 9 a copy of row 5), frames of 4 rows with amplitudes 8, 4, 2, 1, a zero frame
    and the frame b - w_0: -> (w_op, b, x, idx [R, K], val [R, K]) with K = 6."""
    n, d, K = 24, 128, 6
    g = np.random.default_rng(3)
    W = np.zeros((n, d), np.float32)
    W[np.arange(n), 3 * np.arange(n) + 1] = np.where(g.random(n) < 0.5, np.float32(1.0), np.float32(1.5))
    W[9] = W[5]
    b = (g.integers(-8, 9, d) / 4).astype(np.float32)
    amps = np.array([8, 4, 2, 1], np.float32)
    pool = np.array([j for j in range(n) if j not in (5, 9)])
    rows = 12
    js = np.stack([g.permutation(pool)[:4] for _ in range(rows)])
    js[0, 0], js[1, 2], js[2, 3] = 5, 5, 5
    x = b + (amps[None, :, None] * W[js]).sum(1)
    x[3] = b + (amps[:, None] * W[[9, 1, 2, 3]]).sum(0)        # planted through the copy: picked as row 5
    js[3] = [5, 1, 2, 3]
    idx = np.concatenate([js, np.full((rows, K - 4), -1)], axis=1)
    val = np.concatenate([np.tile(amps, (rows, 1)), np.zeros((rows, K - 4), np.float32)], axis=1)
    x = np.concatenate([x, b[None], (b - W[0])[None]]).astype(np.float32)
    idx = np.concatenate([idx, np.full((2, K), -1)])
    val = np.concatenate([val, np.zeros((2, K), np.float32)])
    return W, b, x, idx, val, K


def coef_stop_case():
    """One direction w_0 = e_0 + 1.5 e_1 and x = (1.504, -1.0039): bf16(x) = (1.5078125, -1.0), so the bf16 product is +0.0078 (a
    positive score) while the fp32 product is 1.504 - 1.50585 < 0: the row must stop on the coefficient at step 0."""
    W = np.zeros((1, 128), np.float32)
    W[0, 0], W[0, 1] = 1.0, 1.5
    x = np.zeros((1, 128), np.float32)
    x[0, 0], x[0, 1] = 1.504, -1.0039
    assert float((R.bf16(x[0]) * W[0]).sum()) > 0 and float((x[0].astype(np.float64) * W[0]).sum()) < 0
    return W, x


def violations(idx, val, err, w_op, x, b):
    """Every check of the replay on a trace -> the names of the ones that fail."""
    rp = R.Replay(idx, val, w_op, x, b)
    out = []
    for name, v in (("shape", rp.shape_violations()), ("choice", rp.choice_violations()), ("stop", rp.stop_violations()),
                    ("value", rp.value_violations()), ("err", rp.err_violations(err))):
        if v.any():
            out.append(name)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def test_serial_reference_against_the_float64_rule(prog, tmp_path):
    """pu_row_serial (which also runs the key and predicate checks) on random rows at d = 96 (padded) and 256, with and without a bias:
    every check of the replay holds, the decided rows make the float64 rule's picks, budgets / steps follow from its own e."""
    for d, n, K, seed, with_b in ((96, 40, 4, 1, True), (256, 64, 6, 2, False), (128, 16, 37, 3, True)):
        w_op, b = dictionary(d, n, seed, unequal=True)
        b = b if with_b else None
        x = frames(w_op, b if with_b else np.zeros(d, np.float32), seed + 10, 24, min(K, 6))
        taus = (0.5, 0.1, 0.01)
        idx, val, e, bud, steps = serial(prog, tmp_path, w_op, x, b, K, taus)
        assert violations(idx, val, e, w_op, x, b) == []
        i64, v64, _, _, _ = R.greedy64(w_op, x, b, K)
        dec = R.Replay(i64, v64, w_op, x, b).decided()
        assert np.array_equal(idx[dec], i64[dec]) and (K > 6 or dec.mean() >= 0.9)
        assert np.array_equal(steps, (idx >= 0).sum(1))
        budget, st, _ = R.derived(idx, e, np.asarray(taus, np.float32), n, K)
        assert np.array_equal(st, np.bincount(steps, minlength=K + 1))
        for t in range(len(taus)):
            assert np.array_equal(np.bincount(bud[:, t], minlength=K + 2), budget[t])


def test_serial_reference_on_planted_cases(prog, tmp_path):
    W, b, x, idx_want, val_want, K = exact_case()
    idx, val, e, _, steps = serial(prog, tmp_path, W, x, b, K, (0.5,))
    assert np.array_equal(idx, idx_want) and val.tobytes() == val_want.tobytes()
    assert (e[:12, 4:].view(np.uint32) == 0).all() and (e[:12, :4] > 0).all()             # e_4 == 0 to the bit, and held
    assert steps.tolist() == [4] * 12 + [0, 0] and e[12, 0] == 0 and (e[13] == e[13, 0]).all() and e[13, 0] > 0
    Wc, xc = coef_stop_case()
    idx, val, e, _, steps = serial(prog, tmp_path, Wc, xc, None, 3, (0.5,))
    assert (idx == -1).all() and (val.view(np.uint32) == 0).all() and steps[0] == 0 and (e == e[0, 0]).all()


def test_bounds_hold_for_the_emulation():
    for d, n, K, seed in ((256, 512, 6, 23), (96, 320, 4, 24), (384, 128, 12, 25)):
        w_op, b = dictionary(d, n, seed, unequal=True)
        x = frames(w_op, b, seed + 100, 40, min(K, 6))
        idx, val, err = R.emulate(w_op, n, x, b, K)
        assert violations(idx, val, err, w_op, x, b) == [], (d, n, K)
    W, b, x, idx_want, val_want, K = exact_case()
    idx, val, err = R.emulate(W, W.shape[0], x, b, K)
    assert np.array_equal(idx, idx_want) and val.tobytes() == val_want.tobytes() and violations(idx, val, err, W, x, b) == []


MUTATIONS = {
    # name -> (the emulation's switch, the case, the checks of which at least one must fail)
    "tie to the higher column": ("tie_high", "exact", {"planted"}),
    "|score| instead of the signed score": ("abs_score", "negative", {"choice", "stop", "shape"}),
    "no z_j with directions of unequal norm": ("no_z", "random", {"choice"}),
    "a without / q": ("no_q", "random", {"value"}),
    "no stop on a <= 0": ("no_coef_stop", "coef", {"shape"}),
    "a formed from the bf16 residual": ("coef_from_bf16", "random", {"value"}),
    "e not held after the stop": ("no_hold", "exact", {"err"}),
    "a padding column eligible": ("pad_eligible", "padding", {"shape"}),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_are_caught(name):
    switch, case, expect = MUTATIONS[name]
    if case == "exact":
        W, b, x, idx_want, val_want, K = exact_case()
        n = W.shape[0]
    elif case == "coef":
        (W, x), b, K = coef_stop_case(), None, 3
        n = 1
    elif case == "negative":
        # frames that are MINUS a direction plus a weak positive one: the largest |score| is negative
        W, b = dictionary(128, 32, 40)
        n, K = 32, 3
        x = (b - 6 * W[np.arange(10) % n] + 1.5 * W[(np.arange(10) + 7) % n]).astype(np.float32)
    elif case == "padding":
        # 24 eligible directions, and behind them 8 padding rows that hold (what must never be read as a direction) the strongest ones
        W, b = dictionary(128, 32, 41)
        n, K = 24, 4
        x = (b + 5 * W[24 + np.arange(10) % 8] + 2 * W[np.arange(10)]).astype(np.float32)
    else:
        W, b = dictionary(256, 256, 42, unequal=True)
        n, K = 256, 6
        x = frames(W, b, 142, 40, 6)
    w_elig = W[:n]

    def failed(**kw):
        idx, val, err = R.emulate(W, n, x, b, K, **kw)
        out = set(violations(idx, val, err, w_elig, x, b)) if (idx < n).all() else {"shape"}
        if case == "exact" and not (np.array_equal(idx, idx_want) and val.tobytes() == val_want.tobytes()):
            out.add("planted")
        return out

    assert failed() == set(), "the unmutated rule must pass on the same case"
    got = failed(**{switch: True})
    assert got & expect, (name, got)


# ---------------------------------------------------------------------------------------------------------------------------
def hand_block(K=3, d=2, n=5, taus=(0.5, 0.1)):
    lay = E.pursuit_layout(len(taus), K, d, n)
    blk = np.zeros(lay["bytes"], np.uint8)

    def put(name, values):
        off, dt, cnt = lay[name]
        blk[off:off + cnt * np.dtype(dt).itemsize] = np.asarray(values, dt).reshape(-1).view(np.uint8)
    put("n_frames", [10])
    put("sse", [100.0, 40.0, 10.0, 5.0])
    put("sum_x", [10.0, -20.0])
    put("sum_x_sq", [110.0, 140.0])
    put("budget", [[0, 6, 3, 1, 0], [0, 0, 2, 3, 5]])
    put("steps", [1, 2, 3, 4])
    put("picks", [9, 0, 7, 0, 4])
    put("in_support", [6, 3, 1])
    return blk, lay


def test_module_arithmetic(tmp_path):
    K, d, n = 3, 2, 5
    blk, lay = hand_block()
    assert lay["bytes"] == lay["in_support"][0] + 8 * K and len({v[0] for k, v in lay.items() if k != "bytes"}) == 8
    pf = P.PursuitFrontier.from_block(blk, K, SF.check_thresholds((0.5, 0.1)), d, n)
    tv = (110 - 100 / 10) + (140 - 400 / 10)
    assert pf.n_frames == 10 and pf.d == d and pf.n == n and pf.total_variance() == tv
    assert np.allclose(pf.fvu_curve(), np.array([100, 40, 10, 5]) / tv) and pf.fvu(2) == 10 / tv
    assert pf.marginal().tolist() == [60, 30, 5] and pf.budget_for_fvu(0.06) == 2 and pf.budget_for_fvu(0.01) is None
    assert pf.frame_budget_hist(0.5).tolist() == [0, 6, 3, 1, 0] and pf.frame_budget_quantile(0.1, 0.5) == 3
    assert pf.steps_hist.tolist() == [1, 2, 3, 4] and pf.picks_at_step().tolist() == [9, 7, 4]
    assert np.allclose(pf.usage(), np.array([9, 0, 7, 0, 4]) / 10) and pf.never_picked().tolist() == [1, 3]
    assert np.allclose(pf.support_agreement(), [6 / 9, 3 / 7, 1 / 4])
    with pytest.raises(ValueError):
        pf.fvu(K + 1)
    with pytest.raises(ValueError):
        pf.frame_budget_hist(0.3)
    # compare: the encoder's curve over THIS denominator; a frontier of other frames or another d is refused
    fr = SF.SparsityFrontier(K=2, thresholds=pf.thresholds, n_frames=10, rows_cut=0, active_cut=0, sse=np.array([100.0, 50.0, 30.0]),
                             sum_x=pf.sum_x, sum_x_sq=pf.sum_x_sq, budget=np.zeros((2, 4), np.int64))
    c = pf.compare(fr)
    assert c.shape == (3, 2) and np.allclose(c[:, 0], np.array([100, 50, 30]) / tv) and np.allclose(c[:, 1], np.array([100, 40, 10]) / tv)
    assert np.allclose(pf.amortisation_gap(fr), np.array([0, 10, 20]) / tv)
    import dataclasses
    with pytest.raises(ValueError, match="frames"):
        pf.compare(dataclasses.replace(fr, n_frames=9))
    with pytest.raises(ValueError, match="d="):
        pf.compare(dataclasses.replace(fr, sum_x=np.zeros(3), sum_x_sq=np.zeros(3)))

    class Cov:
        d = 2

        def fvu_curve(self):
            return np.array([1.0, 0.3, 0.0])
    assert np.allclose(pf.compare_pca(Cov())[:, 1], [1.0, 0.3, 0.0, 0.0])
    Cov.d = 3
    with pytest.raises(ValueError):
        pf.compare_pca(Cov())
    pf.save(str(tmp_path / "p.npz"))
    back = P.PursuitFrontier.load(str(tmp_path / "p.npz"))
    assert all(np.array_equal(getattr(back, k), getattr(pf, k)) for k in ("sse", "budget", "steps", "picks", "in_support", "thresholds"))
    assert back.K == K and back.n_frames == 10 and back.summary() == pf.summary() and pf.summary()["never_picked"] == 2


def test_argument_rules():
    assert P.check_K(None, "topk", 1024, 32) == 32 and P.check_K(None, "l1", 1024, 0) == 64 and P.check_K(None, "l1", 40, 0) == 40
    assert P.check_K(None, "topk", 4096, 512) == 256 and P.check_K(256, "topk", 64, 8) == 256 and P.check_K(1, "l1", 64, 0) == 1
    for bad in (0, -1, 257):
        with pytest.raises(ValueError):
            P.check_K(bad, "topk", 64, 8)
    for bad in ((0.0,), (1.0,), (float("nan"),), (0.5, -0.1), (0.1,) * 9):
        with pytest.raises(ValueError):
            SF.check_thresholds(bad)
    with pytest.raises(ValueError, match="needs an SAE"):
        P.pursuit_frontier(None, "/nonexistent", "enc")
    with pytest.raises(ValueError):
        P.pursuit_frontier("none", "/nonexistent", "enc", thresholds=(2.0,))


def test_boundary():
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert re.search(r"\bint sae_pursuit_files\(", hdr) and "sae_pursuit_files" in E.EXPORTED_SYMBOLS
    assert hasattr(E.load(), "sae_pursuit_files")
    assert f"#define SAE_PURSUIT_MAX_K {E.PURSUIT_MAX_K}" in hdr and f"#define SAE_PURSUIT_MAX_TAU {E.PURSUIT_MAX_TAU}" in hdr
    assert (P.MAX_K, P.MAX_TAU) == (E.PURSUIT_MAX_K, E.PURSUIT_MAX_TAU)
    # the layout against the header's macros, evaluated by the C compiler
    names = ["N_FRAMES", "SSE", "SUM_X", "SUM_X_SQ", "BUDGET", "STEPS", "PICKS", "IN_SUPPORT", "BYTES"]
    src = '#include <stdio.h>\n#include <stdint.h>\n#include "freud_sae.h"\nint main(){' + "".join(
        f'printf("%lld\\n", (long long)SAE_PURSUIT_{nm}(3, 17, 200, 1000));' for nm in names) + "return 0;}"
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "m.c"), "w").write(src)
        subprocess.run(["gcc", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(td, "m.c"), "-o", os.path.join(td, "m")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "m")], check=True, capture_output=True, text=True).stdout.split()]
    lay = E.pursuit_layout(3, 17, 200, 1000)
    assert got == [lay[k][0] for k in ("n_frames", "sse", "sum_x", "sum_x_sq", "budget", "steps", "picks", "in_support")] + [lay["bytes"]]
    # pursuit.h defines kernels: it belongs to exactly one translation unit
    mk = open(os.path.join(ROOT, "freud_amd", "csrc", "Makefile")).read()
    assert "pursuit.h" in re.search(r"^HDRS_passes := (.*)$", mk, re.M).group(1) and "pursuit.h" not in re.search(r"^HDRS_engine := (.*)$", mk, re.M).group(1)
    units = [f for f in ("engine.hip", "passes.hip") if '#include "pursuit.h"' in open(os.path.join(ROOT, "freud_amd", "csrc", f)).read()]
    assert units == ["passes.hip"]
