"""CPU: the feature timing without a device.

* the bin arithmetic of freud_amd/csrc/timing_bins.h compiled for the HOST with g++: timing_index of every L in 1..65535 for every
  sub_bits against np.searchsorted over closed-form edges, bins contiguous and monotone, lower_edge(index(L)) <= L <
  lower_edge(index(L) + 1), nbins, bad specs refused by the header and by Python alike;
* the header's serial reference against the numpy reference (tests/feature_timing_reference.py: np.diff of the padded mask) on
  random and on planted masks, bridges 0, 1, 3, with and without lengths;
* FeatureTiming on hand-made arrays: quantile brackets, top_latents ties, the npz round trip;
* the argument rules that need no device; the symbol in the header and in EXPORTED_SYMBOLS."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import feature_timing_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "timing_bins.h"

// bins S          -> timing_index(L, S) of every L in 1 .. 65535, then timing_lower_edge(idx, S) of idx = 1 .. NB(65535) + 1
// ok S G THR T    -> timing_spec_ok, then timing_nbins when it is
// rows FILE       -> (int32 s g thr nf T ld n has_len, int32 lengths[nf], uint16 lat[nf T][ld]) -> n_frames, run_hist, gap_hist, totals
int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "bins")) {
    const int s = atoi(argv[2]);
    for (uint32_t L = 1; L <= 65535; ++L) printf("%d\n", timing_index(L, s));
    for (int i = 1; i <= timing_nbins(s, 65535) + 1; ++i) printf("%u\n", timing_lower_edge(i, s));
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "ok")) {
    const int s = atoi(argv[2]), g = atoi(argv[3]);
    const uint32_t thr = (uint32_t)strtoul(argv[4], nullptr, 0);
    const long long T = atoll(argv[5]);
    const bool ok = timing_spec_ok(s, g, thr, T);
    printf("%d %d\n", (int)ok, ok ? timing_nbins(s, T) : 0);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "rows")) {
    FILE* fp = fopen(argv[2], "rb");
    int h[8];
    if (!fp || fread(h, 4, 8, fp) != 8) return 2;
    const int s = h[0], g = h[1], nf = h[3], T = h[4], ld = h[5], n = h[6], has_len = h[7];
    const uint32_t thr = (uint32_t)h[2];
    std::vector<int> L(nf);
    std::vector<uint16_t> lat((size_t)nf * T * ld);
    if (fread(L.data(), 4, nf, fp) != (size_t)nf || fread(lat.data(), 2, lat.size(), fp) != lat.size()) return 2;
    fclose(fp);
    const int nb = timing_nbins(s, T);
    std::vector<int64_t> rh((size_t)n * nb, 0), gh((size_t)n * nb, 0), tot((size_t)n * TB_NTOTALS, 0);
    int64_t frames = 0;
    timing_rows_ref(lat.data(), ld, n, nf, T, has_len ? L.data() : nullptr, s, g, thr, rh.data(), gh.data(), tot.data(), &frames);
    printf("%lld\n", (long long)frames);
    for (int64_t v : rh) printf("%lld\n", (long long)v);
    for (int64_t v : gh) printf("%lld\n", (long long)v);
    for (int64_t v : tot) printf("%lld\n", (long long)v);
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb")
    src = d / "tb.cpp"
    src.write_text(_SRC)
    exe = d / "tb"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_timing_index_of_every_length_and_edges(prog, s):
    from freud_amd import engine
    from freud_amd.feature_timing import lower_edges
    out = np.array(subprocess.run([prog, "bins", str(s)], check=True, capture_output=True, text=True).stdout.split(), np.int64)
    idx, edge = out[:65535], out[65535:]
    L = np.arange(1, 65536)
    P = 1 << s
    np.testing.assert_array_equal(idx - 1, REF.bins_of(L, s, 65535))                      # by value, over the closed-form edges
    assert idx[0] == 1 and (np.diff(idx) >= 0).all() and (np.diff(idx) <= 1).all()        # monotone and contiguous: no empty bin
    assert (idx[:2 * P - 1] == L[:2 * P - 1]).all()                                       # exact on the small integers
    nb = int(idx[-1])
    assert nb == {0: 16, 1: 31, 2: 59, 3: 111}[s] and edge.shape[0] == nb + 1
    lower = np.concatenate([[0], edge])                                                   # lower[i] = lower edge of idx i
    assert (lower[idx] <= L).all() and (L < lower[idx + 1]).all()
    assert (np.diff(edge) > 0).all()
    np.testing.assert_array_equal(edge, REF.closed_form_edges(s, 65535)[: nb + 1])
    np.testing.assert_array_equal(lower_edges(s, nb), edge)                               # the Python layer restates the edges
    for T in (1, 2, 7, 8, 70, 1500, 65535):
        assert engine.timing_nbins(s, T) == idx[T - 1] == REF.n_bins(s, T)
        assert engine.timing_index(T, s) == idx[T - 1]


def test_documented_bin_counts():
    from freud_amd import engine
    assert engine.timing_nbins(2, 1500) == 37 and engine.timing_nbins(3, 65535) == engine.TIMING_MAX_BINS == 111
    from freud_amd.feature_timing import lower_edges
    e = lower_edges(2, 37)
    assert e[:8].tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and e[8:12].tolist() == [10, 12, 14, 16] and e[36] == 1280 and e[37] == 1536


@pytest.mark.parametrize("bad", [(-1, 0, 0, 100), (4, 0, 0, 100), (2, -1, 0, 100), (2, 16, 0, 100), (2, 0, 0x7F81, 100), (2, 0, 0, 0),
                                 (2, 0, 0, 65536)])
def test_bad_specs_are_refused_by_header_and_python(prog, bad):
    from freud_amd import engine
    from freud_amd import feature_timing as FT
    out = subprocess.run([prog, "ok", *map(str, bad)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "0"
    s, g, thr, T = bad

    def python_accepts(s, g, thr, T):
        try:
            FT._check_args("ckpt", s, g, float("nan") if thr > 0x7F80 else 0.0)      # (a pattern above +Inf is no finite threshold)
            engine.timing_nbins(s, T)
            return True
        except ValueError:
            return False

    assert not python_accepts(s, g, thr, T)
    good = subprocess.run([prog, "ok", "2", "15", str(0x7F80), "65535"], check=True, capture_output=True, text=True).stdout.split()
    assert good == ["1", "59"] and python_accepts(2, 15, 0, 65535)


# ---------------------------------------------------------------------------------------------------------------------------
def run_rows(prog, tmp_path, lat, L, s, g, thr, with_lengths, n):
    nf, T, ld = lat.shape
    path = tmp_path / f"rows_{s}_{g}_{thr}_{int(with_lengths)}.bin"
    with open(path, "wb") as f:
        f.write(np.array([s, g, thr, nf, T, ld, n, int(with_lengths)], np.int32).tobytes())
        f.write(np.asarray(L, np.int32).tobytes())
        f.write(np.ascontiguousarray(lat, np.uint16).tobytes())
    out = np.array(subprocess.run([prog, "rows", str(path)], check=True, capture_output=True, text=True).stdout.split(), np.int64)
    nb = REF.n_bins(s, T)
    a, b = 1 + n * nb, 1 + 2 * n * nb
    return out[0], out[1:a].reshape(n, nb), out[a:b].reshape(n, nb), out[b:].reshape(n, 6)


def check_against_numpy(prog, tmp_path, lat, L, s, g, thr, with_lengths, n):
    nf, T, _ = lat.shape
    lens = np.minimum(np.maximum(L, 1), T) if with_lengths else np.full(nf, T)
    masks = [((lat[f, :lens[f], :n] & 0x7FFF) > thr) for f in range(nf)]
    want_r, want_g, want_t, frames, seen = REF.timing_reference(masks, s, g, T)
    got_f, got_r, got_g, got_t = run_rows(prog, tmp_path, lat, L, s, g, thr, with_lengths, n)
    assert got_f == frames == lens.sum()
    np.testing.assert_array_equal(got_r, want_r)
    np.testing.assert_array_equal(got_g, want_g)
    np.testing.assert_array_equal(got_t, want_t)
    # the invariants of include/freud_sae.h
    assert (got_r.sum(1) == got_t[:, REF.RUNS]).all() and (got_g.sum(1) == got_t[:, REF.RUNS] - got_t[:, REF.FILES]).all()
    assert (got_t[:, REF.SPAN] == got_t[:, REF.ACTIVE]).all() if g == 0 else (got_t[:, REF.SPAN] >= got_t[:, REF.ACTIVE]).all()
    assert (got_t[:, REF.LONGEST] <= T).all()
    return want_r, want_g, want_t, seen


@pytest.mark.parametrize("with_lengths", [False, True])
@pytest.mark.parametrize("g", [0, 1, 3])
def test_serial_reference_against_numpy_on_random_masks(prog, tmp_path, g, with_lengths):
    rng = np.random.default_rng(7 + g)
    nf, T, ld, n = 6, 61, 24, 19
    # columns of different densities, each a thresholded slow walk: runs of every length
    walk = np.cumsum(rng.normal(0, 1, (nf, T, ld)), axis=1) + rng.normal(0, 2, (1, 1, ld))
    lat = np.where(walk > 0, 0x3F80, 0).astype(np.uint16)
    lat[:, :, 3] = np.where(rng.random((nf, T)) < 0.5, 0x3F80, 0)        # a flickering column
    lat[:, :, 4] = 0                                                     # a dead column
    lat[0, 5, 2] = 0x8000                                                # -0.0: inactive
    lat[0, 6, 2] = 0x0001                                                # the smallest subnormal: active at threshold 0
    L = np.array([T, 1, 20, T + 5, 9, 2], np.int32)
    for s in (0, 2, 3):
        _, want_g, want_t, seen = check_against_numpy(prog, tmp_path, lat, L, s, g, 0, with_lengths, n)
        assert seen["dur1"] > 0 and seen["octave"] > 0 and seen["gaps"] > 0 and 0 < want_t[:, REF.CENSORED].sum() < want_t[:, REF.RUNS].sum()
        assert want_t[4].sum() == 0
        if g:
            assert seen["raw_gaps_le_g"] > 0
    # a threshold between the two values of a column
    lat[:, :, 7] = np.where(lat[:, :, 7] > 0, np.where(rng.random((nf, T)) < 0.5, 0x3F80, 0x4000), 0)
    _, _, t_lo, _ = check_against_numpy(prog, tmp_path, lat, L, 2, g, 0, with_lengths, n)
    _, _, t_hi, _ = check_against_numpy(prog, tmp_path, lat, L, 2, g, 0x3F80, with_lengths, n)
    assert 0 < t_hi[7, REF.ACTIVE] < t_lo[7, REF.ACTIVE] and t_hi[3].sum() == 0


@pytest.mark.parametrize("g", [0, 1, 3])
def test_serial_reference_on_planted_masks(prog, tmp_path, g):
    """Column 0: always on; 1: period 2; 2: only frame 0; 3: only the last counted frame; 4: two single frames a gap of exactly g
    apart; 5: a gap of g + 1; 6: never on.  File 1 has a single counted frame."""
    nf, T, ld, n = 3, 24, 8, 7
    L = np.array([T, 1, 17], np.int32)
    lat = np.zeros((nf, T, ld), np.uint16)
    on = 0x3F80
    lat[:, :, 0] = on
    lat[:, ::2, 1] = on
    lat[:, 0, 2] = on
    for f in range(nf):
        lat[f, L[f] - 1, 3] = on
    lat[:, 4, 4] = lat[:, 4 + g + 1, 4] = on
    lat[:, 4, 5] = lat[:, 4 + g + 2, 5] = on
    r, gp, t, seen = check_against_numpy(prog, tmp_path, lat, L, 2, g, 0, True, n)
    A, S, R, F, LG, C = (t[:, i] for i in range(6))
    # always on: one censored run per file, as long as the file
    assert R[0] == F[0] == C[0] == 3 and LG[0] == T and S[0] == L.sum() and gp[0].sum() == 0 and seen["whole_file_by_latent"][0] == 3
    # period 2: every active frame a run of its own at g = 0, one run per file once bridged
    per_file = [(l + 1) // 2 for l in L]
    if g == 0:
        assert R[1] == sum(per_file) and LG[1] == 1 and gp[1, 0] == R[1] - F[1]
    else:
        assert R[1] == 3 and gp[1].sum() == 0 and S[1] == sum(2 * p - 1 for p in per_file)
    assert R[2] == C[2] == 3 and LG[2] == 1                     # only frame 0: censored
    assert R[3] == C[3] == 3 and LG[3] == 1                     # only the last counted frame: censored (file 1: both at once)
    assert R[4] == 2 and LG[4] == g + 2                         # a gap of exactly g: bridged (g = 0: adjacent frames); the one
    assert gp[4].sum() == 0 and C[4] == 0                       # counted frame of file 1 holds nothing of columns 4 and 5
    assert R[5] == 2 * 2 and gp[5].sum() == 2 and gp[5, REF.bins_of([g + 1], 2, T)[0]] == 2 and LG[5] == 1
    assert t[6].sum() == 0 and r[6].sum() == 0
    # without lengths every file has T frames
    check_against_numpy(prog, tmp_path, lat, L, 2, g, 0, False, n)


# ---------------------------------------------------------------------------------------------------------------------------
def hand_made(s=2, g=0, T=200, n=5, n_files=30, seed=3):
    """Known lists of durations per latent -> masks -> the reference's arrays, as a FeatureTiming."""
    from freud_amd.feature_timing import FeatureTiming
    rng = np.random.default_rng(seed)
    masks, durs = [], [[] for _ in range(n)]
    for _ in range(n_files):
        m = np.zeros((T, n), bool)
        for j in range(1, n):                                    # latent 0 stays dead
            t = 1 + int(rng.integers(0, 5))
            while True:
                d = int(min(rng.geometric(1.0 / (1 + 6 * j)), 60))
                if t + d >= T - 1:
                    break
                m[t:t + d, j] = True
                durs[j].append(d)
                t += d + 1 + g + int(rng.integers(0, 12))
        masks.append(m)
    rh, gh, tot, frames, _ = REF.timing_reference(masks, s, g, T)
    return FeatureTiming(frames, n_files, T, (s, g, 0), rh, gh, tot), durs


@pytest.mark.parametrize("s", [0, 2])
def test_quantile_brackets_hold_the_order_statistic(s):
    ft, durs = hand_made(s=s)
    ft.check()
    assert ft.totals[:, REF.CENSORED].sum() == 0                 # every planted run lies strictly inside its file
    for q in (0.0, 0.1, 0.5, 0.9, 0.99, 1.0):
        lo, hi = ft.quantile(q)
        assert np.isnan(lo[0]) and np.isnan(hi[0])               # the dead latent: nothing to rank
        for j in range(1, ft.n_latents):
            srt = np.sort(durs[j])
            assert len(srt) == ft.n_runs[j]
            stat = srt[max(1, int(np.ceil(q * srt.size))) - 1]
            assert stat == np.quantile(srt, q, method="inverted_cdf")
            assert lo[j] <= stat < hi[j], (q, j)
            if stat < (2 << s):
                assert lo[j] == stat and hi[j] == stat + 1       # an exact bin
    glo, ghi = ft.quantile(0.5, which="gap")
    assert np.isnan(glo[0]) and (glo[1:] >= 1).all() and (ghi[1:] > glo[1:]).all()
    with pytest.raises(ValueError):
        ft.quantile(1.5)
    with pytest.raises(ValueError):
        ft.quantile(0.5, which="frame")


def test_accessors_and_top_latents_ties_break_by_the_lower_index():
    from freud_amd.feature_timing import FeatureTiming
    nb = 37
    tot = np.array([[12, 12, 4, 2, 5, 1],       # mean 3
                    [0, 0, 0, 0, 0, 0],         # dead
                    [30, 30, 10, 3, 5, 0],      # mean 3: ties with latent 0 on mean_duration and on longest
                    [8, 8, 8, 4, 1, 2],         # flicker: mean 1, persistence 0
                    [50, 50, 1, 1, 50, 1]], np.int64)
    rh = np.zeros((5, nb), np.int64)
    gh = np.zeros((5, nb), np.int64)
    rh[0, [0, 2, 4]] = [1, 2, 1]; rh[2, [0, 2, 4]] = [3, 4, 3]; rh[3, 0] = 8; rh[4, 24] = 1      # noqa: E702
    gh[0, 3] = 2; gh[2, 1] = 7; gh[3, 0] = 4                                                      # noqa: E702
    ft = FeatureTiming(100, 4, 50, (2, 0, 0), rh, gh, tot)
    ft.check()
    np.testing.assert_array_equal(ft.n_runs, [4, 0, 10, 8, 1])
    md = ft.mean_duration()
    assert md[0] == md[2] == 3.0 and np.isnan(md[1]) and md[3] == 1.0 and md[4] == 50.0
    np.testing.assert_allclose(ft.duty(), [0.12, 0, 0.3, 0.08, 0.5])
    pers = ft.persistence()
    assert pers[3] == 0.0 and pers[4] == 1 - 1 / 50 and np.isnan(pers[1])
    cf = ft.censored_fraction()
    assert cf[0] == 0.25 and cf[4] == 1.0 and np.isnan(cf[1])
    assert ft.top_latents("mean_duration", 3).tolist() == [4, 0, 2]          # 0 before 2: the tie goes to the lower index
    assert ft.top_latents("longest", 5).tolist() == [4, 0, 2, 3]             # the dead latent has no run
    assert ft.top_latents("runs", 2).tolist() == [2, 3]
    assert ft.top_latents("persistence", 2).tolist() == [4, 0]               # 1 - 4/12 = 1 - 10/30: 0 before 2
    assert ft.top_latents("mean_duration", 5, min_runs=5).tolist() == [2, 3]
    with pytest.raises(ValueError):
        ft.top_latents("area")
    assert FeatureTiming.seconds(50) == 1.0 and FeatureTiming.seconds([1, 5], frame_ms=10).tolist() == [0.01, 0.05]
    lo, hi = ft.bin_bounds()
    assert lo[:7].tolist() == [1, 2, 3, 4, 5, 6, 7] and hi[:7].tolist() == [2, 3, 4, 5, 6, 7, 8] and lo[8] == 10 and hi[8] == 12
    s = ft.summary()
    assert json.loads(json.dumps(s)) == s and s["runs"] == 23 and s["dead"] == 1 and s["longest_run"] == 50 and s["whole_file_latents"] == 1
    bridged = FeatureTiming(100, 4, 50, (2, 1, 0), rh, gh, tot)
    with pytest.raises(ValueError, match="bridge"):
        bridged.persistence()
    # check() names a broken invariant
    broken = tot.copy()
    broken[0, REF.RUNS] += 1
    with pytest.raises(RuntimeError, match="run_hist"):
        FeatureTiming(100, 4, 50, (2, 0, 0), rh, gh, broken).check()
    broken = tot.copy()
    broken[4, REF.LONGEST] = 51
    with pytest.raises(RuntimeError, match="LONGEST"):
        FeatureTiming(100, 4, 50, (2, 0, 0), rh, gh, broken).check()


def test_npz_round_trip_is_bitwise(tmp_path):
    from freud_amd.feature_timing import FeatureTiming
    ft, _ = hand_made(g=1)
    p = str(tmp_path / "t.npz")
    ft.to_npz(p)
    back = FeatureTiming.from_npz(p)
    assert (back.n_frames, back.n_files, back.T, back.spec) == (ft.n_frames, ft.n_files, ft.T, ft.spec)
    for k in ("run_hist", "gap_hist", "totals"):
        a, b = getattr(ft, k), getattr(back, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_rules_need_no_device(tmp_path, monkeypatch):
    import torch
    from freud_amd import file_pass
    from freud_amd import feature_timing as FT
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((3, 4 * 8), np.float32), [4, 8])

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the argument checks")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(file_pass, "resolve_sae", no_device)
    path = str(tmp_path)
    ft = FT.feature_timing
    with pytest.raises(ValueError, match="not a bf16 value"):
        ft("ckpt", path, "enc", threshold=0.1)
    with pytest.raises(ValueError, match="not a bf16 value"):
        ft("ckpt", path, "enc", threshold=1.0 + 2.0 ** -8)                  # a float32, one bit beyond bf16
    with pytest.raises(ValueError, match="non-negative"):
        ft("ckpt", path, "enc", threshold=-0.5)
    for v in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite"):
            ft("ckpt", path, "enc", threshold=v)
    with pytest.raises(ValueError, match="bridge"):
        ft("ckpt", path, "enc", bridge=16)
    with pytest.raises(ValueError, match="bridge"):
        ft("ckpt", path, "enc", bridge=-1)
    with pytest.raises(ValueError, match="sub_bits"):
        ft("ckpt", path, "enc", sub_bits=4)
    with pytest.raises(ValueError, match="needs an SAE"):
        ft(None, path, "enc")
    with pytest.raises(ValueError, match="needs an SAE"):
        ft("none", path, "enc")
    with pytest.raises(ValueError, match="batch_files"):
        ft("ckpt", path, "enc", batch_files=0)
    with pytest.raises(ValueError, match="lengths"):
        ft("ckpt", path, "enc", lengths=np.array([1, 2]))
    assert FT.threshold_bits(0.0) == 0 and FT.threshold_bits(0.5) == 0x3F00 and FT.threshold_bits(1.5) == 0x3FC0
    assert FT.threshold_bits(2.0 ** -133) == 1                                # the smallest subnormal bf16


def test_header_library_and_symbol_list():
    from freud_amd import engine
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sae_timing_files\s*\(", code)
    assert "sae_timing_files" in engine.EXPORTED_SYMBOLS
    engine.build()
    assert hasattr(engine.load(), "sae_timing_files")
    for name, val in (("MAX_BINS", engine.TIMING_MAX_BINS), ("MAX_BRIDGE", engine.TIMING_MAX_BRIDGE)):
        m = re.search(rf"#define\s+SAE_TIMING_{name}\s+(\d+)", code)
        assert m and int(m.group(1)) == val
    slots = dict(re.findall(r"SAE_TIMING_(ACTIVE|SPAN|RUNS|FILES|LONGEST|CENSORED|NTOTALS)\s*=\s*(\d+)", code))
    assert {k: int(v) for k, v in slots.items()} == {"ACTIVE": engine.TIMING_ACTIVE, "SPAN": engine.TIMING_SPAN, "RUNS": engine.TIMING_RUNS,
                                                    "FILES": engine.TIMING_FILES, "LONGEST": engine.TIMING_LONGEST,
                                                    "CENSORED": engine.TIMING_CENSORED, "NTOTALS": engine.TIMING_NTOTALS}
    assert (REF.ACTIVE, REF.SPAN, REF.RUNS, REF.FILES, REF.LONGEST, REF.CENSORED) == (0, 1, 2, 3, 4, 5)
