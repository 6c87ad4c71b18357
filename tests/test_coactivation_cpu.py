"""CPU: the score and key arithmetic of the feature co-activation (freud_amd/csrc/coact.h, its host part) compiled with g++ and
checked against numpy for all three measures -- score = (num.astype(f8) / den.astype(f8)).astype(f4), key =
ord(score) << 32 | count, 0 for the latent itself and for pairs that never co-fire -- and the keys fed through file_top.h's
ft_select_serial against numpy.lexsort in the stated order (score descending, then the larger count, then the lower partner).  The
count matrices are small and random, with many zero entries and many tied scores.  Plus the boundary (header, symbol list) and the
argument errors that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import build_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURES = {"jaccard": 0, "cond": 1, "count": 2}

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "coact.h"
#include "file_top.h"

// argv: data file (int32 n, int32 C[n][n]) measure n_top -> per row i: n lines "key-hex score-bits", then n_top lines
// "partner count score-bits" of ft_select_serial with FT_POSITIVE
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[1], "rb");
  int n;
  if (fread(&n, 4, 1, fp) != 1) return 2;
  std::vector<int32_t> C((size_t)n * n);
  if (fread(C.data(), 4, C.size(), fp) != C.size()) return 2;
  fclose(fp);
  const int measure = atoi(argv[2]), n_top = atoi(argv[3]);
  std::vector<uint64_t> keys(n), out(n_top);
  std::vector<int32_t> lat(n_top);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      keys[j] = co_key(measure, i, j, C[(size_t)i * n + j], C[(size_t)i * n + i], C[(size_t)j * n + j]);
      printf("%016llx %08x\n", (unsigned long long)keys[j], sk_bits(co_score(measure, C[(size_t)i * n + j], C[(size_t)i * n + i], C[(size_t)j * n + j])));
    }
    ft_select_serial(keys.data(), n, n_top, FT_POSITIVE, lat.data(), out.data());
    for (int t = 0; t < n_top; ++t) printf("%d %d %08x\n", lat[t], co_key_count(out[t]), sk_bits(co_key_score(out[t])));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("co")
    src = d / "co.cpp"
    src.write_text(_SRC)
    exe = d / "co"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def count_matrix(n, frames, seed):
    """C = Z^T Z of a random 0/1 matrix with a few dead, a few duplicated and a few dense latents: zeros and tied scores."""
    g = np.random.default_rng(seed)
    prob = g.choice([0.0, 0.05, 0.2, 0.9], n)
    prob[5] = 0.5                                    # alive, and duplicated twice below: every row that meets it has ties
    Z = (g.random((frames, n)) < prob[None, :]).astype(np.int64)
    Z[:, 3] = Z[:, 5]
    Z[:, 7] = Z[:, 5]
    return (Z.T @ Z).astype(np.int32)


def np_scores(C, measure):
    n = C.shape[0]
    num = np.broadcast_to(C.astype(np.int64), (n, n))
    dii = np.diag(C).astype(np.int64)
    if measure == "jaccard":
        den = dii[:, None] + dii[None, :] - C
    elif measure == "cond":
        den = np.broadcast_to(dii[:, None], (n, n))
    else:
        den = np.ones((n, n), np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (num.astype("f8") / den.astype("f8")).astype("f4")


def ordf(s):
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def np_neighbors(C, measure, K):
    """The numpy restatement of the neighbour tables: lexsort by (score desc, count desc, partner asc)."""
    n = C.shape[0]
    S = np_scores(C, measure)
    nb = np.full((n, K), -1, np.int64)
    cn = np.zeros((n, K), np.int64)
    sc = np.full((n, K), np.nan, np.float32)
    for i in range(n):
        ok = (C[i] > 0) & (np.arange(n) != i)
        j = np.flatnonzero(ok)
        order = j[np.lexsort((j, -C[i, j].astype(np.int64), -S[i, j].astype(np.float64)))][:K]
        m = len(order)
        nb[i, :m], cn[i, :m], sc[i, :m] = order, C[i, order], S[i, order]
    return nb, cn, sc


@pytest.mark.parametrize("measure", sorted(MEASURES))
@pytest.mark.parametrize("n,frames,n_top", [(24, 40, 5), (37, 12, 40), (9, 8, 1)])
def test_scores_keys_and_order_against_numpy(prog, tmp_path, measure, n, frames, n_top):
    C = count_matrix(n, frames, seed=n + frames)
    off = C[~np.eye(n, dtype=bool)]
    assert (off == 0).any() and (off > 0).any()
    S = np_scores(C, measure)
    live = (C > 0) & ~np.eye(n, dtype=bool)
    assert any(len(np.unique(S[i][live[i]])) < live[i].sum() for i in range(n)), "no tied scores"
    data = tmp_path / "c.bin"
    data.write_bytes(np.array([n], np.int32).tobytes() + C.tobytes())
    lines = subprocess.run([prog, str(data), str(MEASURES[measure]), str(n_top)], check=True, capture_output=True, text=True).stdout.split("\n")
    want_keys = np.where(live, (ordf(S) << np.uint64(32)) | C.astype(np.uint64), np.uint64(0))
    nb, cn, sc = np_neighbors(C, measure, n_top)
    p = 0
    for i in range(n):
        for j in range(n):
            key, bits = lines[p].split()
            p += 1
            assert int(key, 16) == int(want_keys[i, j]), (i, j)
            if live[i, j]:
                assert int(bits, 16) == int(S[i, j].view(np.uint32)), (i, j)
        for t in range(n_top):
            part, cnt, bits = lines[p].split()
            p += 1
            assert int(part) == nb[i, t] and int(cnt) == cn[i, t], (i, t)
            if nb[i, t] >= 0:
                assert int(bits, 16) == int(sc[i, t].view(np.uint32)), (i, t)


def test_decode_matches_the_keys():
    from freud_amd import coactivation as CO
    C = count_matrix(16, 30, seed=1)
    S = np_scores(C, "jaccard")
    keys = ((ordf(S[2, [5, 9]]) << np.uint64(32)) | C[2, [5, 9]].astype(np.uint64)).astype(np.uint64)
    tk = np.array([[keys[0], keys[1], 0]], np.uint64).view(np.int64)
    nb, cn, sc = CO.decode_neighbor_table(np.array([[5, 9, -1]], np.int32), tk)
    assert nb.dtype == np.int64 and cn.dtype == np.int64 and sc.dtype == np.float32
    assert nb.tolist() == [[5, 9, -1]] and cn.tolist() == [[int(C[2, 5]), int(C[2, 9]), 0]]
    assert sc[0, 0] == S[2, 5] and sc[0, 1] == S[2, 9] and np.isnan(sc[0, 2])


def test_boundary_has_the_entry_points():
    from freud_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for sym in ("sae_coact_files", "sae_coact_neighbor_keys"):
        assert sym in E.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr), sym
    for name, code in MEASURES.items():
        assert int(re.search(r"SAE_COACT_" + name.upper() + r"\s*=\s*(\d+)", hdr).group(1)) == code == E.COACT_MEASURES[name]
    assert "2^31 - 1" in hdr
    assert build_units.assert_one_unit_builds("coact.h") == "passes.hip"
    assert callable(E.coact_neighbor_keys) and callable(E.SaeEngine.coact_files)


def test_arguments_are_checked_without_a_device(tmp_path):
    from freud_amd import coactivation as CO
    from freud_amd.engine import FILE_TOP_MAX
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((3, 8), np.float32), [4, 2])
    for raw in (None, "none"):
        with pytest.raises(ValueError, match="needs an SAE"):
            CO.feature_coactivation(raw, str(tmp_path), "enc")
    for bad in (0, -1, FILE_TOP_MAX + 1):
        with pytest.raises(ValueError, match="n_neighbors"):
            CO.feature_coactivation("ckpt.pth", str(tmp_path), "enc", n_neighbors=bad)
    with pytest.raises(ValueError, match="measure"):
        CO.feature_coactivation("ckpt.pth", str(tmp_path), "enc", measure="cosine")


def test_too_many_frames_are_refused_without_a_device(tmp_path, monkeypatch):
    from freud_amd import coactivation as CO
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((3, 8), np.float32), [4, 2])
    monkeypatch.setattr(CO, "MAX_FRAMES", 11)          # 3 files x 4 frames
    with pytest.raises(ValueError, match="exceed the 11 frames"):
        CO.feature_coactivation("ckpt.pth", str(tmp_path), "enc")


def test_npz_round_trip(tmp_path):
    from freud_amd import coactivation as CO
    C = count_matrix(12, 30, seed=2)
    nb, cn, sc = np_neighbors(C, "cond", 4)
    co = CO.CoActivation(30, np.diag(C).astype(np.int64), nb, cn, sc, C, "cond")
    assert co.top(5) == [(int(p), int(c), float(s)) for p, c, s in zip(nb[5], cn[5], sc[5]) if p >= 0]
    for with_matrix in (True, False):
        if not with_matrix:
            co.matrix = None
        path = str(tmp_path / f"co{int(with_matrix)}.npz")
        co.to_npz(path)
        back = CO.CoActivation.from_npz(path)
        assert back.n_frames == 30 and back.measure == "cond"
        for k in ("fire_count", "neighbors", "counts", "scores"):
            assert getattr(back, k).tobytes() == getattr(co, k).tobytes() and getattr(back, k).dtype == getattr(co, k).dtype
        assert (back.matrix is None) == (not with_matrix)
        if with_matrix:
            np.testing.assert_array_equal(back.matrix, C)
