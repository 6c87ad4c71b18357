"""CPU: the host part of the cross-activation (freud_amd/csrc/cross.h) compiled with g++ -- the serial reference of the whole rule
against the numpy restatement (tests/cross_activation_reference.py) on ragged files at lags 0, 1, 3, T - 1, T and T + 2; scores and
keys against numpy bit for bit for all four measures in both orientations; the key order through file_top.h's ft_select_serial
against numpy.lexsort on tables with tied scores -- and seven mutations of the header, each of which must fail one of those
checks.  Plus the argument errors that need no device, the refusal of directories that do not hold the same files, and the npz
round trip."""
import os
import subprocess

import numpy as np
import pytest

from tests import build_units
from tests import cross_activation_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "freud_amd", "csrc")

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "cross.h"
#include "file_top.h"

// tables FILE: int32 F T n_a n_b has_len n_lags, int32 lengths[F], int32 lags[n_lags], uint8 za[F T n_a], uint8 zb[F T n_b]
//   -> per lag the (n_a + 1)(n_b + 1) counts, one per line.  (The arrays are padded with zero rows: a mutated rule may read on.)
// keys FILE measure by_b exclude_diagonal n_top: int32 n_a n_b, int32 table[(n_a + 1)(n_b + 1)]
//   -> per row of the orientation one line "key-hex score-bits" per column, then n_top lines "partner count score-bits"
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  if (!strcmp(argv[1], "tables")) {
    int h[6];
    if (fread(h, 4, 6, fp) != 6) return 2;
    const int F = h[0], T = h[1], n_a = h[2], n_b = h[3], n_lags = h[5];
    std::vector<int> len(F), lags(n_lags);
    if (fread(len.data(), 4, F, fp) != (size_t)F || fread(lags.data(), 4, n_lags, fp) != (size_t)n_lags) return 2;
    int pad = 1;
    for (int l : lags) pad = l + 1 > pad ? l + 1 : pad;
    std::vector<uint8_t> za((size_t)(F * T + pad) * n_a, 0), zb((size_t)(F * T + pad) * n_b, 0);
    if (fread(za.data(), 1, (size_t)F * T * n_a, fp) != (size_t)F * T * n_a || fread(zb.data(), 1, (size_t)F * T * n_b, fp) != (size_t)F * T * n_b) return 2;
    for (int l : lags) {
      std::vector<int32_t> table((size_t)(n_a + 1) * (n_b + 1), 0);
      cx_reference(za.data(), n_a, zb.data(), n_b, F, T, h[4] ? len.data() : nullptr, l, table.data());
      for (int32_t v : table) printf("%d\n", v);
    }
    return 0;
  }
  int n_a, n_b;
  if (fread(&n_a, 4, 1, fp) != 1 || fread(&n_b, 4, 1, fp) != 1) return 2;
  const int W = n_b + 1;
  std::vector<int32_t> X((size_t)(n_a + 1) * W);
  if (fread(X.data(), 4, X.size(), fp) != X.size()) return 2;
  const int measure = atoi(argv[3]), by_b = atoi(argv[4]), excl = atoi(argv[5]), n_top = atoi(argv[6]);
  const int rows = by_b ? n_b : n_a, cols = by_b ? n_a : n_b;
  std::vector<uint64_t> keys(cols), out(n_top);
  std::vector<int32_t> lat(n_top);
  for (int r = 0; r < rows; ++r) {
    for (int c = 0; c < cols; ++c) {
      const int i = by_b ? c : r, j = by_b ? r : c;
      const int32_t x = X[(size_t)i * W + j], fa = X[(size_t)i * W + n_b], fb = X[(size_t)n_a * W + j], np = X[(size_t)n_a * W + n_b];
      keys[c] = cx_key(measure, by_b, excl, i, j, x, fa, fb, np);
      printf("%016llx %08x\n", (unsigned long long)keys[c], sk_bits(cx_score(measure, by_b, x, fa, fb, np)));
    }
    ft_select_serial(keys.data(), cols, n_top, FT_POSITIVE, lat.data(), out.data());
    for (int t = 0; t < n_top; ++t) printf("%d %d %08x\n", lat[t], co_key_count(out[t]), sk_bits(co_key_score(out[t])));
  }
  return 0;
}
"""


def compile_prog(folder, header_text=None):
    """The program over freud_amd/csrc -- or over a changed cross.h placed in front of it."""
    src = folder / "cx.cpp"
    src.write_text(_SRC)
    inc = [f"-I{CSRC}"]
    if header_text is not None:
        (folder / "cross.h").write_text(header_text)
        inc.insert(0, f"-I{folder}")
    exe = folder / "cx"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *inc, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_prog(tmp_path_factory.mktemp("cx"))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
T_ = 9
LAGS = (0, 1, 3, T_ - 1, T_, T_ + 2)


def random_masks(F, T, n_a, n_b, seed):
    """Dense enough that every window holds pairs: a few dead, dense and duplicated latents on either side; ragged lengths with a
    full file followed by another file."""
    g = np.random.default_rng(seed)
    za = (g.random((F, T, n_a)) < g.choice([0.0, 0.2, 0.5, 0.9], n_a)[None, None, :]).astype(np.uint8)
    zb = (g.random((F, T, n_b)) < g.choice([0.0, 0.2, 0.5, 0.9], n_b)[None, None, :]).astype(np.uint8)
    za[:, :, 0], zb[:, :, 0] = 0, 0                      # a dead latent on either side
    za[:, :, 1], zb[:, :, 1] = 1, 1                      # one latent on every frame: the margins show in the interior
    za[:, :, 3], zb[:, :, 3] = g.random((F, T)) < 0.5, g.random((F, T)) < 0.5
    za[:, :, 2], zb[:, :, 2] = za[:, :, 3], zb[:, :, 3]  # twins on either side: tied scores in both orientations
    L = g.integers(1, T + 1, F).astype(np.int32)
    L[0], L[1] = T, 2
    return za, zb, L


CASES = {"ragged": lambda: random_masks(5, T_, 7, 5, 1), "full": lambda: random_masks(3, T_, 4, 6, 2)[:2] + (None,)}


def run_tables(prog, tmp_path, za, zb, L, lags):
    F, T, n_a = za.shape
    n_b = zb.shape[2]
    data = tmp_path / "m.bin"
    lens = np.zeros(F, np.int32) if L is None else L.astype(np.int32)
    data.write_bytes(np.array([F, T, n_a, n_b, int(L is not None), len(lags)], np.int32).tobytes() + lens.tobytes()
                     + np.array(lags, np.int32).tobytes() + za.tobytes() + zb.tobytes())
    out = subprocess.run([prog, "tables", str(data)], check=True, capture_output=True, text=True).stdout.split()
    return np.array(out, np.int64).reshape(len(lags), n_a + 1, n_b + 1)


def check_tables(prog, tmp_path):
    """The serial reference against numpy on every case and lag; the cases' own preconditions."""
    for name, make in CASES.items():
        za, zb, L = make()
        got = run_tables(prog, tmp_path, za, zb, L, LAGS)
        want = np.stack([REF.cross_table(za, zb, L, l) for l in LAGS])
        if name == "ragged":
            # the inputs tell the rules apart: file boundaries, lengths and the side of the lag all matter, some window is partly empty
            assert any((REF.cross_table(za, zb, L, l, ignore_files=True) != want[a]).any() for a, l in enumerate(LAGS))
            assert any((REF.cross_table(za, zb, None, l) != want[a]).any() for a, l in enumerate(LAGS))
            assert (REF.cross_table(zb, za, L, 1).T != want[1]).any()
            assert (want[1][:-1, :-1] == 0).any() and (want[1][:-1, :-1] > 0).any()
        assert (want[LAGS.index(T_)] == 0).all() and (want[LAGS.index(T_ + 2)] == 0).all()
        X, fa, fb, n_pairs = REF.split(want[0])
        assert n_pairs == (za.shape[0] * T_ if L is None else int(L.sum())) and (X[1] == fb).all() and (X[:, 1] == fa).all()
        np.testing.assert_array_equal(got, want, err_msg=name)


def key_table(square, seed):
    """A table with zeros, a live diagonal (square) and tied scores: from masks with duplicated latents."""
    n = 6 if square else 8
    za, zb, L = random_masks(6, T_, 6, n, seed)
    if square:
        zb = za.copy()
        zb[:, :, 4] = za[:, :, 5]
    return REF.cross_table(za, zb, L, 1 if square else 0).astype(np.int32)


def check_keys(prog, tmp_path, measures=tuple(REF.MEASURES), orientations=(0, 1)):
    """Scores, keys and the selection order against numpy, on a rectangular table and on a square one with and without its diagonal."""
    for square, excl, n_top in ((False, 0, 3), (True, 0, 7), (True, 1, 2)):
        table = key_table(square, 5)
        n_a, n_b = table.shape[0] - 1, table.shape[1] - 1
        live = REF.reported(table, excl)
        assert live.any() and (~live).any()
        if square:
            assert (np.diag(table[:-1, :-1]) > 0).any()
        data = tmp_path / "t.bin"
        data.write_bytes(np.array([n_a, n_b], np.int32).tobytes() + table.tobytes())
        assert any(REF.has_tied_scores(table, m, b, excl) for m in measures for b in orientations), "no tied scores"
        for measure in measures:
            for by_b in orientations:
                lines = subprocess.run([prog, "keys", str(data), str(REF.MEASURES[measure]), str(by_b), str(excl), str(n_top)], check=True,
                                       capture_output=True, text=True).stdout.split("\n")
                S, K = REF.scores(table, measure, by_b), REF.keys(table, measure, by_b, excl)
                lv = live
                if by_b:
                    S, K, lv = S.T, K.T, live.T
                nb, cn, sc = REF.partners(table, measure, n_top, by_b, excl)
                p = 0
                for r in range(K.shape[0]):
                    for c in range(K.shape[1]):
                        key, bits = lines[p].split()
                        p += 1
                        assert int(key, 16) == int(K[r, c]), (measure, by_b, r, c)
                        assert (int(key, 16) == 0) == (not lv[r, c])
                        if lv[r, c]:
                            assert int(bits, 16) == int(S[r, c].view(np.uint32)), (measure, by_b, r, c)
                    for t in range(n_top):
                        part, cnt, bits = lines[p].split()
                        p += 1
                        assert int(part) == nb[r, t] and int(cnt) == cn[r, t], (measure, by_b, r, t)
                        if nb[r, t] >= 0:
                            assert int(bits, 16) == int(sc[r, t].view(np.uint32)), (measure, by_b, r, t)


def test_serial_reference_equals_numpy(prog, tmp_path):
    check_tables(prog, tmp_path)


@pytest.mark.parametrize("measure", sorted(REF.MEASURES))
@pytest.mark.parametrize("by_b", [0, 1])
def test_scores_keys_and_order_against_numpy(prog, tmp_path, measure, by_b):
    check_keys(prog, tmp_path, (measure,), (by_b,))


MUTATIONS = {
    "file_boundary_ignored": ("const bool open = cx_window(t, lag, len);", "const bool open = f * T + t + lag < F * T;"),
    "window_from_T": ("const bool open = cx_window(t, lag, len);", "const bool open = cx_window(t, lag, T);"),
    "lag_on_the_wrong_side": ("const uint8_t* a = za + (f * T + t) * n_a;\n      const uint8_t* b = zb + (f * T + t + lag) * n_b;",
                              "const uint8_t* a = za + (f * T + t + lag) * n_a;\n      const uint8_t* b = zb + (f * T + t) * n_b;"),
    "margin_not_windowed": ("const bool on = j < n_b ? (open && b[j]) : open;", "const bool on = j < n_b ? (open && b[j]) : true;"),
    "diagonal_dropped_between_two_dictionaries": ("(exclude_diagonal && i == j)", "(i == j)"),
    "cond_by_the_other_margin": ("(by_b ? FB : FA)", "(by_b ? FA : FB)"),
    "window_one_frame_long": ("return t + lag < len;", "return t + lag <= len;"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_of_the_header_are_caught(name, tmp_path):
    old, new = MUTATIONS[name]
    text = open(os.path.join(CSRC, "cross.h")).read()
    assert text.count(old) == 1, f"the header no longer holds {old!r}"
    mutant = compile_prog(tmp_path, text.replace(old, new))
    failed = []
    for check in (check_tables, check_keys):
        try:
            check(mutant, tmp_path)
        except AssertionError:
            failed.append(check.__name__)
    assert failed, f"{name} passes every check"


def test_boundary_has_the_entry_points():
    import re
    from freud_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for sym in ("sae_cross_mask_bytes", "sae_cross_mask_files", "sae_cross_update", "sae_cross_keys"):
        assert sym in E.EXPORTED_SYMBOLS
        assert re.search(r"\b(int|int64_t)\s+" + sym + r"\s*\(", hdr), sym
    for name, code in REF.MEASURES.items():
        assert int(re.search(r"SAE_CROSS_" + name.upper() + r"\s*=\s*(\d+)", hdr).group(1)) == code == E.CROSS_MEASURES[name]
    assert int(re.search(r"#define\s+SAE_CROSS_MAX_LAG\s+(\d+)", hdr).group(1)) == E.CROSS_MAX_LAG == 32768
    assert int(re.search(r"#define\s+SAE_CROSS_MAX_LAGS\s+(\d+)", hdr).group(1)) == E.CROSS_MAX_LAGS == 8
    assert build_units.assert_one_unit_builds("cross.h") == "passes.hip"


# ---- the Python surface without a device --------------------------------------------------------------------------------------
@pytest.fixture
def no_device(tmp_path, monkeypatch):
    """3 files of T = 4 frames, d = 2; any look at the device fails the test."""
    import torch
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path / "a"), "enc", np.zeros((3, 8), np.float32), [4, 2])

    def touched():
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    return tmp_path


def test_arguments_are_checked_without_a_device(no_device):
    from freud_amd import cross_activation as CX
    from freud_amd.engine import FILE_TOP_MAX
    path = str(no_device / "a")

    def run(sae="ckpt.pth", **kw):
        return CX.cross_activation(sae, path, "enc", **kw)

    for raw in (None, "none"):
        with pytest.raises(ValueError, match="needs an SAE"):
            run(raw)
    with pytest.raises(ValueError, match="needs an SAE"):
        run(sae_b="none")
    for bad in (0, FILE_TOP_MAX + 1):
        with pytest.raises(ValueError, match="n_neighbors"):
            run(n_neighbors=bad)
    with pytest.raises(ValueError, match="measure"):
        run(measure="f1")
    for bad in ((), tuple(range(9))):
        with pytest.raises(ValueError, match="1 to 8"):
            run(lags=bad)
    for bad in ((-1,), (32768,), (0, 40000)):
        with pytest.raises(ValueError, match="outside"):
            run(lags=bad)
    with pytest.raises(ValueError, match="duplicate"):
        run(lags=(0, 2, 2))
    for bad in ((0.5,), ("x",), 3):
        with pytest.raises(ValueError, match="integers"):
            run(lags=bad)
    with pytest.raises(ValueError, match="go together"):
        run(sae_b="b.pth", data_path_b=path)
    with pytest.raises(ValueError, match="need sae_b"):
        run(data_path_b=path, layer_name_b="enc")


def test_directories_that_do_not_hold_the_same_files_are_refused_without_a_device(no_device):
    from freud_amd import cross_activation as CX
    from freud_amd.loader import write_shards
    names = [f"file_{i:06d}.flac" for i in range(3)]
    a = str(no_device / "a")
    write_shards(str(no_device / "renamed"), "mid", np.zeros((3, 12), np.float16), [4, 3], names[:2] + ["other.flac"])
    write_shards(str(no_device / "fewer"), "mid", np.zeros((2, 12), np.float16), [4, 3], names[:2])
    write_shards(str(no_device / "longer"), "mid", np.zeros((3, 15), np.float16), [5, 3], names)
    write_shards(str(no_device / "same"), "mid", np.zeros((3, 12), np.float16), [4, 3], names)
    for folder, match in (("renamed", "other.flac"), ("fewer", "3 and 2 files"), ("longer", "T=4 and T=5")):
        with pytest.raises(ValueError, match=match):
            CX.cross_activation("a.pth", a, "enc", sae_b="b.pth", data_path_b=str(no_device / folder), layer_name_b="mid")
    CX.check_same_files(a, "enc", str(no_device / "same"), "mid", None)
    CX.check_same_files(a, "enc", str(no_device / "fewer"), "mid", 2)           # (the first two files of either)


def test_too_many_frames_are_refused_without_a_device(no_device, monkeypatch):
    from freud_amd import cross_activation as CX
    monkeypatch.setattr(CX, "MAX_FRAMES", 11)          # 3 files x 4 frames
    with pytest.raises(ValueError, match="exceed the 11 frames"):
        CX.cross_activation("ckpt.pth", str(no_device / "a"), "enc", lags=(0, 1))


def test_npz_round_trip_and_the_readers(tmp_path):
    from freud_amd import cross_activation as CX
    za, zb, L = random_masks(6, T_, 6, 8, 5)
    lags, K = (0, 2), 3
    tabs = [REF.cross_table(za, zb, L, l) for l in lags]
    sides = [[np.stack(q) for q in zip(*(REF.partners(t, "lift", K, by_b, 0) for t in tabs))] for by_b in (0, 1)]
    cx = CX.CrossActivation(np.array(lags, np.int64), np.array([t[-1, -1] for t in tabs]), np.stack([t[:-1, -1] for t in tabs]),
                            np.stack([t[-1, :-1] for t in tabs]), *sides[0], *sides[1],
                            np.stack([t[:-1, :-1] for t in tabs]).astype(np.int32), "lift", False)
    i = int(np.argmax((sides[0][0][1] >= 0).sum(1)))
    want = [(int(p), int(c), float(s)) for p, c, s in zip(sides[0][0][1, i], sides[0][1][1, i], sides[0][2][1, i]) if p >= 0]
    assert want and cx.top(i, lag=2) == want
    with pytest.raises(KeyError):
        cx.top(0, lag=1)
    with pytest.raises(ValueError):
        cx.top(0, side="c")
    pa, pb = sides[0][0][0], sides[1][0][0]
    mutual = [(i, int(pa[i, 0])) for i in range(6) if pa[i, 0] >= 0 and pb[pa[i, 0], 0] == i]
    assert [m[:2] for m in cx.mutual_best(0)] == mutual
    for side, (fire, best) in {"a": (cx.fire_a[0], sides[0][2][0, :, 0]), "b": (cx.fire_b[0], sides[1][2][0, :, 0])}.items():
        thr = float(np.nanmedian(best))
        firing = fire > 0
        assert 0 < firing.sum() < fire.size          # a dead latent has no partner and is not counted
        assert cx.coverage(0, thr, side) == float((np.nan_to_num(best, nan=-1.0)[firing] >= np.float32(thr)).sum() / firing.sum())
    s = cx.summary()
    assert s["n_a"] == 6 and s["n_b"] == 8 and s["measure"] == "lift" and [e["lag"] for e in s["lags"]] == [0, 2]
    assert s["lags"][0]["n_pairs"] == int(L.sum())
    for with_tables in (True, False):
        if not with_tables:
            cx.tables = None
        path = str(tmp_path / f"cx{int(with_tables)}.npz")
        cx.to_npz(path)
        back = CX.CrossActivation.from_npz(path)
        assert back.measure == "lift" and back.same_dictionary is False
        for k in CX._FIELDS:
            assert getattr(back, k).tobytes() == getattr(cx, k).tobytes() and getattr(back, k).dtype == getattr(cx, k).dtype, k
        assert (back.tables is None) == (not with_tables)
        if with_tables:
            np.testing.assert_array_equal(back.tables, cx.tables)
