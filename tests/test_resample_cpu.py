"""CPU: dead-latent resampling without a device.

* freud_amd/csrc/resample_draw.h compiled for the HOST (g++ -ffp-contract=off -Wall -Werror) against the numpy restatement of
  tests/resample_reference.py: the weight word on every exponent edge, the prefix search at its edges, the hash and the draws, the
  selection (owner rule against np.unique, batch independence, total == 0), the column arithmetic to the bit, a degenerate row;
* a chi-square check of the draw frequencies against w_i / total, and twelve mutations of the draw that must fall outside;
* the scheduling of a round in train() with a recording subclass of tests/fake_engine.OracleEngine;
* the symbols in the header and in EXPORTED_SYMBOLS, ResampleReport's npz round trip, the argument rules that need no device."""
import copy
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import resample_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "resample_draw.h"

static bool rd(FILE* fp, void* p, size_t bytes) { return fread(p, 1, bytes, fp) == bytes; }

// weights FILE   (int64 rows, float loss[rows])                         -> lmax bits, e, then q_i and w_i per row
// search FILE    (int64 rows, nt, uint64 c[rows], uint64 t[nt])         -> rs_search per t
// draws FILE     (int64 rows, n_draws, seed, round, float loss[rows])   -> total, then the row of every draw
// select FILE    (int64 rows, n, seed, round, batch_rows, float loss[rows], uint64 fire[n]) -> counts, then the pairs
// column FILE    (int64 d, float alpha, float x[d])                     -> degenerate, bits of s, nrm, b, then of u_k
// hash S R r     -> rs_hash
int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "hash")) {
    printf("%llu\n", (unsigned long long)rs_hash(strtoull(argv[2], 0, 0), strtoull(argv[3], 0, 0), strtoull(argv[4], 0, 0)));
    return 0;
  }
  if (argc != 3) return 1;
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  if (!strcmp(argv[1], "weights")) {
    int64_t rows;
    if (!rd(fp, &rows, 8)) return 2;
    std::vector<float> l((size_t)rows);
    if (!rd(fp, l.data(), (size_t)rows * 4)) return 2;
    const uint32_t m = rs_max_bits(l.data(), rows);
    const int e = rs_frexp_exp(m);
    printf("%u\n%d\n", m, e);
    for (int64_t i = 0; i < rows; ++i) {
      uint32_t b;
      memcpy(&b, &l[(size_t)i], 4);
      printf("%u %llu\n", rs_weight_q(rs_loss_bits(b), e), (unsigned long long)rs_weight(b, e));
    }
    return 0;
  }
  if (!strcmp(argv[1], "search")) {
    int64_t h[2];
    if (!rd(fp, h, 16)) return 2;
    std::vector<uint64_t> c((size_t)h[0]), t((size_t)h[1]);
    if (!rd(fp, c.data(), c.size() * 8) || !rd(fp, t.data(), t.size() * 8)) return 2;
    for (uint64_t v : t) printf("%lld\n", (long long)rs_search(c.data(), h[0], v));
    return 0;
  }
  if (!strcmp(argv[1], "draws")) {
    int64_t h[4];
    if (!rd(fp, h, 32)) return 2;
    std::vector<float> l((size_t)h[0]);
    if (!rd(fp, l.data(), l.size() * 4)) return 2;
    std::vector<uint64_t> c(l.size());
    const uint64_t total = rs_prefix_batch(l.data(), h[0], rs_frexp_exp(rs_max_bits(l.data(), h[0])), 0, c.data());
    printf("%llu\n", (unsigned long long)total);
    for (int64_t r = 0; r < h[1]; ++r) printf("%lld\n", (long long)rs_draw(c.data(), h[0], total, (uint64_t)h[2], (uint64_t)h[3], (uint64_t)r));
    return 0;
  }
  if (!strcmp(argv[1], "select")) {
    int64_t h[5];
    if (!rd(fp, h, 40)) return 2;
    std::vector<float> l((size_t)h[0]);
    std::vector<uint64_t> fire((size_t)h[1]);
    if (!rd(fp, l.data(), l.size() * 4) || !rd(fp, fire.data(), fire.size() * 8)) return 2;
    std::vector<int32_t> lat((size_t)h[1]);
    std::vector<int64_t> rows((size_t)h[1]);
    int64_t counts[RS_NCOUNTS];
    const int64_t np = rs_select_ref(l.data(), h[0], fire.data(), (int)h[1], (uint64_t)h[2], (uint64_t)h[3], lat.data(), rows.data(), counts, h[4]);
    for (int i = 0; i < RS_NCOUNTS; ++i) printf("%lld\n", (long long)counts[i]);
    for (int64_t i = 0; i < np; ++i) printf("%d %lld\n", lat[(size_t)i], (long long)rows[(size_t)i]);
    return 0;
  }
  if (!strcmp(argv[1], "column")) {
    int64_t d;
    float alpha;
    if (!rd(fp, &d, 8) || !rd(fp, &alpha, 4)) return 2;
    std::vector<float> x((size_t)d);
    if (!rd(fp, x.data(), x.size() * 4)) return 2;
    const float s = rs_norm_sq(x.data(), (int)d);
    const float nrm = rs_norm(s), b = rs_bias(alpha, nrm);
    uint32_t w[3];
    memcpy(&w[0], &s, 4); memcpy(&w[1], &nrm, 4); memcpy(&w[2], &b, 4);
    printf("%d\n%u\n%u\n%u\n", (int)rs_degenerate(s), w[0], w[1], w[2]);
    for (int64_t k = 0; k < d; ++k) {
      const float u = rs_unit(x[(size_t)k], nrm);
      uint32_t ub;
      memcpy(&ub, &u, 4);
      printf("%u\n", ub);
    }
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("rs")
    src = d / "rs.cpp"
    src.write_text(_SRC)
    exe = d / "rs"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)],
                   check=True)
    return str(exe), d


def _run(prog, mode, payload: bytes, name="in.bin"):
    exe, d = prog
    path = d / name
    path.write_bytes(payload)
    out = subprocess.run([exe, mode, str(path)], check=True, capture_output=True, text=True).stdout
    return out.split("\n")[:-1]


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _weights(prog, loss):
    loss = np.ascontiguousarray(loss, dtype=np.float32)
    out = _run(prog, "weights", struct.pack("<q", loss.size) + loss.tobytes())
    qw = np.array([l.split() for l in out[2:]], dtype=np.uint64).reshape(-1, 2)
    return int(out[0]), int(out[1]), qw[:, 0], qw[:, 1]


# ---- the weight word ------------------------------------------------------------------------------------------------------
EDGE_FAMILIES = {
    "power_of_two_max": _f32([0x40000000, 0x3FFFFFFF, 0x3F800000, 0x3F7FFFFF, 0x38000000, 0x37FFFFFF, 0x00000001, 0]),      # l_max = 2.0
    "just_below_power": _f32([0x3FFFFFFF, 0x3F800000, 0x3F000000, 0x2F800001, 0x00800000, 0x007FFFFF, 0]),
    "subnormal_losses": _f32([0x3F800000, 0x00400000, 0x00000001, 0x007FFFFF, 0x00800000, 0x01000000]),
    "subnormal_max": _f32([0x00000001, 0]),
    "subnormal_max_wide": _f32([0x007FFFFF, 0x00400000, 0x00000100, 0x000000FF, 0x00000001, 0]),
    "subnormal_max_power": _f32([0x00004000, 0x00003FFF, 0x00002000, 0x00000001]),
    "smallest_normal_max": _f32([0x00800000, 0x007FFFFF, 0x00400000, 0x00000080, 0x0000007F]),
    "largest_finite_max": _f32([0x7F7FFFFF, 0x7F000000, 0x3F800000, 0x00000001]),
    "all_zero": np.zeros(5, np.float32),
}


@pytest.mark.parametrize("name", sorted(EDGE_FAMILIES))
def test_weight_word_on_exponent_edges(prog, name):
    loss = EDGE_FAMILIES[name]
    lmax, e, q, w = _weights(prog, loss)
    assert lmax == REF.l_max_bits(loss) and e == REF.frexp_exp(lmax)
    np.testing.assert_array_equal(q, REF.weight_q(loss, e))
    np.testing.assert_array_equal(w, REF.weights(loss))
    assert (q <= 65535).all()
    if lmax:
        # the maximum lands in the top octave of the word: 2^15 <= q_max < 2^16, so the weights keep 15 to 16 bits of l / l_max
        assert 32768 <= int(q.max()) <= 65535 and int(q[np.argmax(REF.loss_bits(loss))]) == int(q.max())
        # and by the definition, in exact rational arithmetic
        from fractions import Fraction
        for li, qi in zip(loss, q):
            assert int(qi) == int(Fraction(float(li)) * Fraction(2) ** (16 - e) // 1)
    else:
        assert e == 0 and not q.any()


def test_weight_word_on_random_losses(prog):
    rng = np.random.default_rng(0)
    loss = np.concatenate([rng.lognormal(0, 3, 4000), np.zeros(50), rng.uniform(0, 1e-40, 50)]).astype(np.float32)
    lmax, e, q, w = _weights(prog, loss)
    np.testing.assert_array_equal(q, REF.weight_q(loss, e))
    np.testing.assert_array_equal(w, q * q)


# ---- the prefix search --------------------------------------------------------------------------------------------------------
def test_prefix_search_edges(prog):
    w = np.array([5, 0, 0, 7, 1, 0, 9, 0], dtype=np.uint64)
    c = REF.prefix(w)
    total = int(c[-1])
    t = [0, total - 1]
    for ci in c:
        t += [int(ci) - 1, int(ci)]
    t = np.array([v for v in t if 0 <= v < total], dtype=np.uint64)
    out = _run(prog, "search", struct.pack("<qq", c.size, t.size) + c.tobytes() + t.tobytes())
    got = np.array(out, dtype=np.int64)
    np.testing.assert_array_equal(got, np.searchsorted(c, t, side="right"))
    assert got[0] == 0 and got[1] == 6                     # t = 0: the first row with weight; t = total - 1: the last one
    assert (w[got] > 0).all()                              # a row of weight 0 is never drawn
    for ti, gi in zip(t, got):                             # c_{i-1} <= t < c_i
        assert int(c[gi]) > int(ti) and (gi == 0 or int(c[gi - 1]) <= int(ti))


def test_hash_matches_restatement(prog):
    exe, _ = prog
    for seed, rnd, r in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2 ** 64 - 1, 2 ** 63, 12345), (42, 3, 2 ** 40 + 7)]:
        got = int(subprocess.run([exe, "hash", str(seed), str(rnd), str(r)], check=True, capture_output=True, text=True).stdout)
        assert got == REF.rs_hash_int(seed, rnd, r) == int(REF.rs_hash(seed, rnd, np.array([r], dtype=np.uint64))[0])
    a = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 0x9E3779B97F4A7C15], dtype=np.uint64)
    for b in (1, 2 ** 32 + 1, 2 ** 64 - 1, 0xDEADBEEFCAFEF00D):
        np.testing.assert_array_equal(REF.mulhi64(a, b), np.array([(int(x) * b) >> 64 for x in a], dtype=np.uint64))


# ---- the draw frequencies -------------------------------------------------------------------------------------------------------
N_ROWS, N_DRAWS, DRAW_SEED, DRAW_ROUND = 64, 200_000, 2023, 1
# 63 degrees of freedom: the reference must stay below the 1 % point, a mutation above the 1e-9 point (fixed table values; with scipy
# the p-values are computed)
CHI2_63_P01, CHI2_63_P1EM9 = 92.010, 155.0


def _draw_losses():
    return np.random.default_rng(7).lognormal(0.0, 0.6, N_ROWS).astype(np.float32)


def _p_value(stat, dof):
    try:
        from scipy import stats
    except ImportError:
        return None
    return float(stats.chi2.sf(stat, dof))


@pytest.fixture(scope="module")
def header_draws(prog):
    loss = _draw_losses()
    out = _run(prog, "draws", struct.pack("<qqqq", N_ROWS, N_DRAWS, DRAW_SEED, DRAW_ROUND) + loss.tobytes())
    return loss, int(out[0]), np.array(out[1:], dtype=np.int64)


def test_draws_match_restatement_and_their_frequencies_follow_the_weights(header_draws):
    loss, total, rows = header_draws
    w = REF.weights(loss)
    assert total == int(w.sum()) and (w > 0).all()
    np.testing.assert_array_equal(rows, REF.draw_rows(loss, N_DRAWS, DRAW_SEED, DRAW_ROUND))
    stat, dof = REF.chi_square(rows, w)
    p = _p_value(stat, dof)
    print(f"chi-square {stat:.2f} on {dof} degrees of freedom, p = {p}")
    assert dof == 63
    assert stat < CHI2_63_P01
    if p is not None:
        assert p > 0.01


@pytest.mark.parametrize("mutation", REF.MUTATIONS)
def test_every_mutation_of_the_draw_falls_outside(mutation):
    loss = _draw_losses()
    rows = REF.draw_rows(loss, N_DRAWS, DRAW_SEED, DRAW_ROUND, mutation=mutation)
    stat, dof = REF.chi_square(rows, REF.weights(loss))
    p = _p_value(stat, dof)
    print(f"{mutation}: chi-square {stat:.2f}, p = {p}")
    assert stat > CHI2_63_P1EM9
    if p is not None:
        assert p < 1e-9


# ---- the selection ----------------------------------------------------------------------------------------------------------------
def _select(prog, loss, fire, seed, rnd, batch_rows=0):
    loss, fire = np.ascontiguousarray(loss, np.float32), np.ascontiguousarray(fire, np.uint64)
    out = _run(prog, "select", struct.pack("<qqqqq", loss.size, fire.size, seed, rnd, batch_rows) + loss.tobytes() + fire.tobytes())
    counts = np.array(out[:REF.NCOUNTS], dtype=np.int64)
    pairs = np.array([l.split() for l in out[REF.NCOUNTS:]], dtype=np.int64).reshape(-1, 2)
    return pairs[:, 0], pairs[:, 1], counts


def _case(rows=1000, n=200, dead_every=3, seed=0):
    rng = np.random.default_rng(seed)
    loss = rng.lognormal(0, 1.0, rows).astype(np.float32)
    fire = rng.integers(1, 100, n)
    fire[::dead_every] = 0
    return loss, fire


def test_selection_matches_restatement_and_np_unique(prog):
    loss, fire = _case()
    lat, rows, counts = _select(prog, loss, fire, 11, 2)
    rl, rr, rc = REF.select(loss, fire, 11, 2)
    np.testing.assert_array_equal(lat, rl)
    np.testing.assert_array_equal(rows, rr)
    np.testing.assert_array_equal(counts, rc)
    assert counts[REF.DEAD] == (fire == 0).sum() and counts[REF.PAIRS] + counts[REF.SKIPPED_DUPLICATE] == counts[REF.DEAD]
    assert len(set(rows.tolist())) == rows.size and (np.diff(lat) > 0).all() and (fire[lat] == 0).all()
    # another round or seed draws other rows
    assert not np.array_equal(rows, _select(prog, loss, fire, 11, 3)[1]) and not np.array_equal(rows, _select(prog, loss, fire, 12, 2)[1])


def test_collision_goes_to_the_lowest_rank(prog):
    loss, fire = _case(rows=300, n=64, dead_every=2)
    loss[137] = 1e6                                        # nearly all the weight on one row: (almost) every dead latent draws it
    lat, rows, counts = _select(prog, loss, fire, 5, 0)
    dead = np.flatnonzero(fire == 0)
    assert rows[0] == 137 and lat[0] == dead[0]
    assert counts[REF.SKIPPED_DUPLICATE] >= dead.size - 3 and counts[REF.PAIRS] == rows.size
    np.testing.assert_array_equal(rows, REF.select(loss, fire, 5, 0)[1])


@pytest.mark.parametrize("batch_rows", [1, 7, 256, 300, 999])
def test_draws_do_not_depend_on_the_batching(prog, batch_rows):
    loss, fire = _case()
    whole = _select(prog, loss, fire, 3, 1)
    split = _select(prog, loss, fire, 3, 1, batch_rows)
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_total_zero_resamples_nothing(prog):
    _loss, fire = _case()
    lat, rows, counts = _select(prog, np.zeros(1000, np.float32), fire, 3, 1)
    assert lat.size == 0 and counts[REF.TOTAL] == 0 and counts[REF.PAIRS] == 0 and counts[REF.SKIPPED_DUPLICATE] == 0
    assert counts[REF.DEAD] == (fire == 0).sum()
    np.testing.assert_array_equal(counts, REF.select(np.zeros(1000, np.float32), fire, 3, 1)[2])


def test_no_dead_latent(prog):
    loss, _fire = _case()
    lat, _rows, counts = _select(prog, loss, np.ones(200), 3, 1)
    assert lat.size == 0 and counts[REF.DEAD] == 0 and counts[REF.TOTAL] > 0


# ---- the column -------------------------------------------------------------------------------------------------------------------
def _column(prog, x, alpha):
    x = np.ascontiguousarray(x, np.float32)
    out = _run(prog, "column", struct.pack("<qf", x.size, alpha) + x.tobytes())
    v = np.array(out, dtype=np.uint64).astype(np.uint32)
    return bool(v[0]), v[1:4].view(np.float32), v[4:].view(np.float32)


@pytest.mark.parametrize("d,alpha,scale", [(384, 0.2, 1.0), (512, 0.2, 30.0), (77, 0.5, 1e-3), (5, 0.0, 1e18), (9, 1.0, 1e-15), (3, 1.0, 1e-21)])
def test_column_arithmetic_is_bit_equal_to_float32_numpy(prog, d, alpha, scale):
    x = (np.random.default_rng(d).standard_normal(d) * scale).astype(np.float32)
    deg, (s, nrm, b), u = _column(prog, x, alpha)
    rdeg, ru, rb = REF.column(x, alpha)
    assert not deg and not rdeg
    assert s.view(np.uint32) == REF.norm_sq(x).view(np.uint32)
    assert nrm.view(np.uint32) == np.sqrt(REF.norm_sq(x), dtype=np.float32).view(np.uint32)
    np.testing.assert_array_equal(u.view(np.uint32), ru.view(np.uint32))
    assert b.view(np.uint32) == rb.view(np.uint32)
    # what the column is for: the seed frame's pre-activation is about alpha |x| (u and b carry one fp32 rounding per element,
    # nrm those of the d-term sum: (d + 8) 2^-23 |x| covers them)
    # -- while s is a normal number: a subnormal s (the last case) has lost bits before the root is taken
    if float(s) >= 2.0 ** -126:
        assert float(np.dot(x.astype(np.float64), u.astype(np.float64)) + b) == pytest.approx(alpha * float(nrm), abs=(d + 8) * 2.0 ** -23 * float(nrm))
    else:
        assert scale == 1e-21


def test_degenerate_rows(prog):
    assert _column(prog, np.zeros(16, np.float32), 0.2)[0] and REF.column(np.zeros(16, np.float32), 0.2)[0]
    big = np.full(16, 3e38, np.float32)                     # the sum of squares overflows
    assert _column(prog, big, 0.2)[0] and REF.column(big, 0.2)[0]
    nan = np.array([1, np.nan, 2], np.float32)
    assert _column(prog, nan, 0.2)[0] and REF.column(nan, 0.2)[0]
    tiny = np.array([1e-30, 0], np.float32)                 # s underflows to 0: degenerate, although x is not zero
    assert _column(prog, tiny, 0.2)[0] and REF.column(tiny, 0.2)[0]


def test_fma32_is_a_single_rounding():
    # 1 + 2^-12 squared = 1 + 2^-11 + 2^-24: the product rounds to 1 + 2^-11 first and the tie is lost; the fma keeps it
    a = np.float32(1 + 2.0 ** -12)
    assert REF.fma32(a, a, np.float32(2.0 ** -24)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(a * a) + np.float32(2.0 ** -24) == np.float32(1 + 2.0 ** -11)


# ---- the report and the argument rules ----------------------------------------------------------------------------------------------
def _report(revived=2):
    from freud_amd.resample import ResampleReport
    return ResampleReport(dead=5, revived=revived, skipped_duplicate=2, skipped_degenerate=1, l_max=3.5, mean_row_loss=0.25, n_frames=777,
                          latents=np.array([3, 9], np.int32)[:revived], files=np.array([0, 4], np.int64)[:revived],
                          frames=np.array([17, 99], np.int64)[:revived])


def test_report_npz_round_trip(tmp_path):
    from freud_amd.resample import ResampleReport
    r = _report()
    r.to_npz(str(tmp_path / "r.npz"))
    back = ResampleReport.from_npz(str(tmp_path / "r.npz"))
    assert back.summary() == r.summary() == {"dead": 5, "revived": 2, "skipped_duplicate": 2, "skipped_degenerate": 1, "l_max": 3.5,
                                             "mean_row_loss": 0.25, "n_frames": 777}
    for k in ("latents", "files", "frames"):
        np.testing.assert_array_equal(getattr(back, k), getattr(r, k))
        assert getattr(back, k).dtype == getattr(r, k).dtype


def test_checkpoint_rewrite_resets_only_the_revived_moments():
    from freud_amd.resample import resample_checkpoint
    d, n = 4, 12
    ck = {"model": {"encoder_bias": torch.ones(n), "decoder.weight": torch.ones(d, n)}, "step": 7, "hparams": {"a": 1},
          "optimizer": {"param_groups": [{"lr": 1.0}],
                        "state": {0: {"step": torch.tensor(7.0), "exp_avg": torch.ones(n), "exp_avg_sq": torch.ones(n)},
                                  1: {"step": torch.tensor(7.0), "exp_avg": torch.ones(d, n), "exp_avg_sq": torch.ones(d, n)}}}}
    params = {"encoder_bias": np.full(n, 2, np.float32), "decoder.weight": np.full((d, n), 3, np.float32)}
    out = resample_checkpoint(ck, _report(), params)
    assert out["step"] == 7 and out["hparams"] == {"a": 1} and out["optimizer"]["param_groups"] == [{"lr": 1.0}]
    assert (out["model"]["encoder_bias"] == 2).all() and (out["model"]["decoder.weight"] == 3).all()
    keep = np.ones(n, bool)
    keep[[3, 9]] = False
    for mk in ("exp_avg", "exp_avg_sq"):
        assert (out["optimizer"]["state"][0][mk].numpy() == keep).all() and (out["optimizer"]["state"][1][mk].numpy() == keep[None, :]).all()
        assert (ck["optimizer"]["state"][0][mk] == 1).all()                   # the input is not written
    assert float(out["optimizer"]["state"][1]["step"]) == 7.0


def test_argument_rules_without_a_device():
    from freud_amd.resample import check_resample_args, resample_dead_latents
    check_resample_args(1, 0.0)
    check_resample_args(512, 1.0)
    for files, a in [(0, 0.2), (-3, 0.2), (8, -0.1), (8, 1.5), (8, float("nan"))]:
        with pytest.raises(ValueError):
            check_resample_args(files, a)
    for sae in (None, "none", "some/checkpoint.pth"):
        with pytest.raises(ValueError, match="live SAE"):
            resample_dead_latents(sae, "x", "l", seed=0)


def test_symbols_in_header_and_binding():
    from freud_amd import engine
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for name in ("sae_resample_files", "sae_resample_select", "sae_resample_apply", "sae_resample_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in engine.EXPORTED_SYMBOLS and name in engine._SIGNATURES
    m = re.search(r"SAE_RESAMPLE_DEAD = (\d), SAE_RESAMPLE_PAIRS = (\d), SAE_RESAMPLE_SKIPPED_DUPLICATE = (\d), SAE_RESAMPLE_TOTAL = (\d), "
                  r"SAE_RESAMPLE_LMAX_BITS = (\d),\s*SAE_RESAMPLE_NCOUNTS = (\d)", text)
    assert m and tuple(int(v) for v in m.groups()) == (engine.RESAMPLE_DEAD, engine.RESAMPLE_PAIRS, engine.RESAMPLE_SKIPPED_DUPLICATE,
                                                        engine.RESAMPLE_TOTAL, engine.RESAMPLE_LMAX_BITS, engine.RESAMPLE_NCOUNTS)
    assert (REF.DEAD, REF.PAIRS, REF.SKIPPED_DUPLICATE, REF.TOTAL, REF.LMAX_BITS, REF.NCOUNTS) == tuple(int(v) for v in m.groups())
    from tests.build_units import assert_one_unit_builds
    assert assert_one_unit_builds("resample.h") == "passes.hip"


# ---- the scheduling of a round in train() ---------------------------------------------------------------------------------------
from freud_amd.loader import write_shards       # noqa: E402
from freud_amd.train_sae import train           # noqa: E402
from tests.fake_engine import OracleEngine      # noqa: E402


class RecordingEngine(OracleEngine):
    """OracleEngine that records, with the optimizer step they happen at, the calls whose order train() promises: metrics() (the
    logging block), resample_dead_latents() (the round) and get_params() (save_checkpoint)."""
    draws_rng = False
    log = None

    def metrics(self, stream=None):
        type(self).log.append(("metrics", self.st.step))
        return super().metrics(stream)

    def get_params(self):
        type(self).log.append(("get_params", self.st.step))
        return super().get_params()

    def resample_dead_latents(self, data_path, layer_name, **kw):
        type(self).log.append(("resample", self.st.step, data_path, layer_name, dict(kw), torch.get_rng_state().clone()))
        if self.draws_rng:
            torch.rand(1000)
            torch.randperm(17)
        return _report()


def _recorder(draws_rng=False):
    return type("Rec", (RecordingEngine,), {"draws_rng": draws_rng, "log": []})


def _train_cfg(tmp_path, golden_dir, run="run", **over):
    z = np.load(os.path.join(golden_dir, "trainloop_l1.npz"))
    meta = json.loads(str(z["meta"]))
    folder = os.path.join(str(tmp_path), "train")
    if not os.path.exists(folder):
        write_shards(folder, meta["layer"], z["shard"], [meta["T"], meta["d"]], [f"/data/audio/file_{i:04d}.flac" for i in range(meta["n_files"])])
    cfg = copy.deepcopy(meta["config"])
    cfg.update(train_folder=folder, val_folder=folder, run_dir=os.path.join(str(tmp_path), run), device="cpu")
    cfg.update(over)
    return cfg


def test_rounds_fire_at_the_right_steps_between_logging_and_checkpoint(tmp_path, golden_dir):
    cfg = _train_cfg(tmp_path, golden_dir, steps=7, log_tb_every=2, save_every=2, val_every=1000,
                     resample={"every": 2, "until": 5, "files": 3, "activation_scale": 0.3})
    Rec = _recorder()
    st = train(**cfg, engine_factory=Rec)
    rounds = [e for e in Rec.log if e[0] == "resample"]
    assert [e[1] for e in rounds] == [2, 4]                                # s % 2 == 0 and s <= 5: not 6
    for e in rounds:
        assert e[2] == cfg["train_folder"] and e[3] == cfg["whisper_config"]["layer_name"]
        assert e[4] == {"files": 3, "seed": cfg["seed"], "round": e[1] // 2, "activation_scale": 0.3}
    for s in (2, 4):                                                       # logging, then the round, then the checkpoint
        names = [e[0] for e in Rec.log if e[1] == s]
        assert names[:3] == ["metrics", "resample", "get_params"], names
    assert [e[0] for e in Rec.log if e[1] == 6][:2] == ["metrics", "get_params"]
    assert st["hparams"]["resample"] == {"every": 2, "until": 5, "files": 3, "activation_scale": 0.3}
    tags = [json.loads(l) for l in open(os.path.join(cfg["run_dir"], "metrics.jsonl"))]
    assert [(t["step"], t["value"]) for t in tags if t["tag"] == "resample/dead"] == [(2, 5.0), (4, 5.0)]
    assert [(t["step"], t["value"]) for t in tags if t["tag"] == "resample/revived"] == [(2, 2.0), (4, 2.0)]
    ck = torch.load(os.path.join(cfg["run_dir"], "checkpoints", "step4.pth"), map_location="cpu", weights_only=True)
    assert ck["hparams"]["resample"]["every"] == 2


def test_defaults_until_is_steps_files_512_scale_02(tmp_path, golden_dir):
    cfg = _train_cfg(tmp_path, golden_dir, steps=6, val_every=1000, resample={"every": 3})
    Rec = _recorder()
    train(**cfg, engine_factory=Rec)
    rounds = [e for e in Rec.log if e[0] == "resample"]
    assert [e[1] for e in rounds] == [3, 6]
    assert rounds[0][4] == {"files": 512, "seed": cfg["seed"], "round": 1, "activation_scale": 0.2} and rounds[1][4]["round"] == 2


def test_global_rng_is_unchanged_across_a_round(tmp_path, golden_dir):
    """A round that draws from the global torch RNG must not move the run: the same batches, the same final state as with a round
    that draws nothing (the epoch permutations after a round come from that RNG)."""
    over = dict(steps=7, val_every=1000, resample={"every": 2})
    quiet, noisy = _recorder(False), _recorder(True)
    a = train(**_train_cfg(tmp_path, golden_dir, "quiet", **over), engine_factory=quiet)
    b = train(**_train_cfg(tmp_path, golden_dir, "noisy", **over), engine_factory=noisy)
    ra, rb = ([e for e in R.log if e[0] == "resample"] for R in (quiet, noisy))
    assert len(ra) == len(rb) == 3
    for ea, eb in zip(ra, rb):
        assert torch.equal(ea[5], eb[5])                                   # the RNG state every round starts from
    pa, pb = a["engine"].P, b["engine"].P
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert torch.equal(a["epoch_rng_state"], b["epoch_rng_state"])


def test_topk_with_the_key_raises_and_bad_keys_are_refused(tmp_path, golden_dir):
    cfg = _train_cfg(tmp_path, golden_dir, resample={"every": 2})
    topk = dict(cfg, autoencoder_variant="topk")
    with pytest.raises(ValueError, match="auxk_alpha"):
        train(**topk, engine_factory=_recorder())
    for bad in ({}, {"every": 0}, {"every": 2, "window": 3}, {"every": 2, "files": 0}, {"every": 2, "activation_scale": 2.0}):
        with pytest.raises(ValueError):
            train(**dict(cfg, resample=bad), engine_factory=_recorder())


def test_a_config_without_the_key_makes_no_resample_call(tmp_path, golden_dir):
    cfg = _train_cfg(tmp_path, golden_dir, val_every=1000)
    Rec = _recorder()
    st = train(**cfg, engine_factory=Rec)
    assert not [e for e in Rec.log if e[0] == "resample"]
    assert "resample" not in st["hparams"]
    assert not any(json.loads(l)["tag"].startswith("resample/") for l in open(os.path.join(cfg["run_dir"], "metrics.jsonl")))
