"""CPU: the score and key arithmetic of the feature labels (freud_amd/csrc/labels.h, its host part) compiled with g++ and checked
against numpy for all four measures -- score = np.float32(np.float64(num) / np.float64(den)), key = ord(score) << 32 | count, 0
iff the count is 0 -- and the keys of both orientations fed through file_top.h's ft_select_serial against numpy.lexsort in the
stated order (score descending, then the larger count, then the lower index).  The tables are small: random ones with zero
entries and tied scores, and one of edge counts (A = 1, A = fire = label_count, counts next to 2^31 - 1).  Plus every argument
error that needs no device, the npz round trip and the look-up by class name."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import build_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURES = {"f1": 0, "precision": 1, "recall": 2, "count": 3}
I31 = 2 ** 31 - 1

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "labels.h"
#include "file_top.h"

// argv: data file (int32 C, int32 n, int32 A[C + 1][n], int64 label_count[C + 1]) measure n_top by_latent -> per row of the chosen
// orientation: one line "key-hex score-bits" per column, then n_top lines "partner count score-bits" of ft_select_serial
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[1], "rb");
  int C, n;
  if (fread(&C, 4, 1, fp) != 1 || fread(&n, 4, 1, fp) != 1) return 2;
  std::vector<int32_t> A((size_t)(C + 1) * n);
  std::vector<int64_t> lc(C + 1);
  if (fread(A.data(), 4, A.size(), fp) != A.size() || fread(lc.data(), 8, lc.size(), fp) != lc.size()) return 2;
  fclose(fp);
  const int measure = atoi(argv[2]), n_top = atoi(argv[3]), by_latent = atoi(argv[4]);
  const int rows = by_latent ? n : C, cols = by_latent ? C : n;
  std::vector<uint64_t> keys(cols), out(n_top);
  std::vector<int32_t> lat(n_top);
  for (int r = 0; r < rows; ++r) {
    for (int c = 0; c < cols; ++c) {
      const int l = by_latent ? c : r, j = by_latent ? r : c;
      const int32_t a = A[(size_t)l * n + j], fire = A[(size_t)C * n + j];
      keys[c] = lb_key(measure, a, fire, lc[l]);
      printf("%016llx %08x\n", (unsigned long long)keys[c], sk_bits(lb_score(measure, a, fire, lc[l])));
    }
    ft_select_serial(keys.data(), cols, n_top, FT_POSITIVE, lat.data(), out.data());
    for (int t = 0; t < n_top; ++t) printf("%d %d %08x\n", lat[t], co_key_count(out[t]), sk_bits(co_key_score(out[t])));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("lb")
    src = d / "lb.cpp"
    src.write_text(_SRC)
    exe = d / "lb"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def random_table(C, n, frames, seed):
    """A [C + 1][n] and label_count [C + 1] of random 0/1 activity (a few dead, duplicated and dense latents) against one label per
    frame, some frames unlabelled and one class never seen: zeros and tied scores."""
    g = np.random.default_rng(seed)
    prob = g.choice([0.0, 0.05, 0.2, 0.9], n)
    prob[2] = 0.5
    Z = (g.random((frames, n)) < prob[None, :]).astype(np.int64)
    Z[:, 1] = Z[:, 2]
    Z[:, n - 1] = Z[:, 2]
    lab = g.integers(-1, max(C - 1, 1), frames)                 # (class C - 1 is never seen when C > 1)
    onehot = np.zeros((frames, C + 1), np.int64)
    onehot[np.arange(frames)[lab >= 0], lab[lab >= 0]] = 1
    onehot[:, C] = 1
    return (onehot.T @ Z).astype(np.int32), onehot.sum(0).astype(np.int64)


def edge_table():
    """Hand-made counts (every A <= fire and <= label_count): A = 1 against large totals, A = fire = label_count, and counts next to
    2^31 - 1."""
    fire = np.array([1, I31, I31, I31 - 1, 7, 3], np.int32)
    A = np.array([[1, 1, I31, I31 - 2, 7, 0],
                  [1, I31, I31 - 1, 1, 0, 3],
                  [0, 1, 1, I31 - 1, 7, 3]], np.int32)
    lc = np.array([I31, I31, I31 - 1, I31], np.int64)
    lc[1] = 2 * I31                                             # (a label may ride on more frames than one latent fires on)
    return np.vstack([A, fire[None, :]]), lc


def np_scores(A, lc, measure):
    """[C][n] fp32: ONE fp64 division, converted once."""
    C = A.shape[0] - 1
    a = A[:C].astype(np.int64)
    fire = np.broadcast_to(A[C].astype(np.int64)[None, :], a.shape)
    lcb = np.broadcast_to(lc[:C].astype(np.int64)[:, None], a.shape)
    num, den = {"f1": (2 * a, fire + lcb), "precision": (a, fire), "recall": (a, lcb), "count": (a, np.ones_like(a))}[measure]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)


def ordf(s):
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def np_top(A, lc, measure, K, by_latent):
    """The numpy restatement of a table: lexsort by (score desc, count desc, index asc); -1 / 0 / NaN in empty slots."""
    C = A.shape[0] - 1
    cnt = A[:C].astype(np.int64)
    S = np_scores(A, lc, measure)
    if by_latent:
        cnt, S = cnt.T, S.T
    rows = cnt.shape[0]
    nb = np.full((rows, K), -1, np.int64)
    cn = np.zeros((rows, K), np.int64)
    sc = np.full((rows, K), np.nan, np.float32)
    for i in range(rows):
        j = np.flatnonzero(cnt[i] > 0)
        order = j[np.lexsort((j, -cnt[i, j], -S[i, j].astype(np.float64)))][:K]
        m = len(order)
        nb[i, :m], cn[i, :m], sc[i, :m] = order, cnt[i, order], S[i, order]
    return nb, cn, sc


TABLES = {"random_c6": lambda: random_table(6, 24, 40, 3), "random_c1": lambda: random_table(1, 9, 12, 4),
          "random_c37": lambda: random_table(37, 11, 60, 5), "edges": edge_table}


@pytest.mark.parametrize("measure", sorted(MEASURES))
@pytest.mark.parametrize("by_latent", [0, 1])
@pytest.mark.parametrize("table,n_top", [("random_c6", 5), ("random_c1", 1), ("random_c37", 40), ("edges", 4)])
def test_scores_keys_and_order_against_numpy(prog, tmp_path, measure, by_latent, table, n_top):
    A, lc = TABLES[table]()
    C, n = A.shape[0] - 1, A.shape[1]
    assert (A[:C] <= A[C][None, :]).all() and (A[:C] <= lc[:C, None]).all()
    S = np_scores(A, lc, measure)
    live = A[:C] > 0
    if table == "random_c6":
        assert (~live).any() and live.any()
        assert any(len(np.unique(S[l][live[l]])) < live[l].sum() for l in range(C)), "no tied scores"
    if table == "edges":
        assert (A[:C] == 1).any() and ((A[:C] == A[C][None, :]) & (A[:C] == lc[:C, None])).any() and (A[:C] >= I31 - 2).any()
    data = tmp_path / "a.bin"
    data.write_bytes(np.array([C, n], np.int32).tobytes() + A.tobytes() + lc.tobytes())
    lines = subprocess.run([prog, str(data), str(MEASURES[measure]), str(n_top), str(by_latent)], check=True, capture_output=True,
                           text=True).stdout.split("\n")
    want_keys = np.where(live, (ordf(S) << np.uint64(32)) | A[:C].astype(np.uint64), np.uint64(0))
    assert ((want_keys == 0) == (A[:C] == 0)).all()                       # a key is 0 iff the count is 0
    if by_latent:
        want_keys, S, live = want_keys.T, S.T, live.T
    nb, cn, sc = np_top(A, lc, measure, n_top, by_latent)
    p = 0
    for r in range(want_keys.shape[0]):
        for c in range(want_keys.shape[1]):
            key, bits = lines[p].split()
            p += 1
            assert int(key, 16) == int(want_keys[r, c]), (r, c)
            assert (int(key, 16) == 0) == (not live[r, c])
            if live[r, c]:
                assert int(bits, 16) == int(S[r, c].view(np.uint32)), (r, c)
        for t in range(n_top):
            part, cnt, bits = lines[p].split()
            p += 1
            assert int(part) == nb[r, t] and int(cnt) == cn[r, t], (r, t)
            if nb[r, t] >= 0:
                assert int(bits, 16) == int(sc[r, t].view(np.uint32)), (r, t)


def test_boundary_has_the_entry_points():
    from freud_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for sym in ("sae_label_files", "sae_label_keys"):
        assert sym in E.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", hdr), sym
    for name, code in MEASURES.items():
        assert int(re.search(r"SAE_LABEL_" + name.upper() + r"\s*=\s*(\d+)", hdr).group(1)) == code == E.LABEL_MEASURES[name]
    assert int(re.search(r"#define\s+SAE_LABEL_MAX_CLASSES\s+(\d+)", hdr).group(1)) == E.LABEL_MAX_CLASSES == 4096
    assert int(re.search(r"#define\s+SAE_LABEL_MAX_SLOTS\s+(\d+)", hdr).group(1)) == E.LABEL_MAX_SLOTS == 16
    assert build_units.assert_one_unit_builds("labels.h") == "passes.hip"
    assert callable(E.label_keys) and callable(E.SaeEngine.label_files)


@pytest.fixture
def no_device(tmp_path, monkeypatch):
    """3 files of T = 4 frames, d = 2; any look at the device fails the test."""
    import torch
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((3, 8), np.float32), [4, 2])

    def touched():
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    return str(tmp_path)


def test_arguments_are_checked_without_a_device(no_device):
    from freud_amd import feature_labels as FL
    from freud_amd.engine import FILE_TOP_MAX
    path = no_device
    ok = np.array([0, 1, -1])

    def run(sae="ckpt.pth", **kw):
        if "file_labels" not in kw and "frame_labels" not in kw:
            kw["file_labels"] = ok
        return FL.feature_labels(sae, path, "enc", **kw)

    for raw in (None, "none"):
        with pytest.raises(ValueError, match="need an SAE"):
            run(raw)
    for bad in (0, -1, FILE_TOP_MAX + 1):
        with pytest.raises(ValueError, match="n_top"):
            run(n_top=bad)
    with pytest.raises(ValueError, match="measure"):
        run(measure="jaccard")
    with pytest.raises(ValueError, match="exactly one"):
        FL.feature_labels("ckpt.pth", path, "enc")
    with pytest.raises(ValueError, match="exactly one"):
        run(file_labels=ok, frame_labels=np.zeros((3, 4), np.int64))
    # ids
    with pytest.raises(ValueError, match="-2"):
        run(file_labels=np.array([0, -2, 1]))
    with pytest.raises(ValueError, match=">= n_classes=2"):
        run(file_labels=np.array([0, 2, 1]), n_classes=2)
    with pytest.raises(ValueError, match="duplicate"):
        run(file_labels=np.array([[0, 1], [2, 2], [1, -1]]))
    with pytest.raises(ValueError, match="duplicate"):
        fr = np.full((3, 4, 3), -1)
        fr[2, 3] = [5, 1, 5]
        run(frame_labels=fr)
    run_ok_dups_of_empty = np.array([[0, -1, -1], [-1, -1, -1], [1, 2, -1]])        # (several empty slots are no duplicate)
    with pytest.raises(ValueError, match="class_names"):
        run(file_labels=run_ok_dups_of_empty, class_names=["a", "b"])
    # dtype
    for bad in (np.array([0.0, 1.0, 2.0]), np.array([True, False, True])):
        with pytest.raises(ValueError, match="integers"):
            run(file_labels=bad)
    # shapes
    for bad in (np.zeros(4, np.int64), np.zeros((3, 2, 2), np.int64), np.int64(1)):
        with pytest.raises(ValueError, match="file_labels must be"):
            run(file_labels=bad)
    for bad in (np.zeros(3, np.int64), np.zeros((3, 5), np.int64), np.zeros((2, 4), np.int64), np.zeros((3, 4, 2, 1), np.int64)):
        with pytest.raises(ValueError, match="frame_labels must be"):
            run(frame_labels=bad)
    # limits
    with pytest.raises(ValueError, match="slots"):
        run(file_labels=np.tile(np.arange(17), (3, 1)))
    with pytest.raises(ValueError, match="slots"):
        run(file_labels=np.zeros((3, 0), np.int64))
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_classes"):
            run(file_labels=np.array([-1, -1, -1]), n_classes=bad)
    with pytest.raises(ValueError, match="n_classes=4097"):
        run(file_labels=np.array([0, 4096, 1]))
    with pytest.raises(ValueError, match="n_classes=0"):
        run(file_labels=np.array([-1, -1, -1]))
    with pytest.raises(ValueError, match="class_names"):
        run(class_names=["a", "b", "c"])


def test_valid_arguments_pass_the_checks_and_go_on_to_the_device(no_device):
    """Arguments that break no rule get as far as FilePass's look at the device (a stand-in for the SAE: nothing is loaded)."""
    from freud_amd import feature_labels as FL

    class Sae:                       # what FilePass reads of a freud_amd.models SAE before it asks for the device
        activation_size, n_dict_components = 2, 8

        def _ensure(self, rows):
            raise RuntimeError("not reached")
    for kw in ({"file_labels": np.array([[0, -1, -1], [-1, -1, -1], [1, 2, -1]]), "class_names": ["a", "b", "c"]},
               {"file_labels": np.array([3, 0, 3], np.uint8), "measure": "precision", "n_top": 1024},
               {"frame_labels": np.zeros((3, 4), np.int32), "n_classes": 4096},
               {"frame_labels": np.tile(np.arange(16), (3, 4, 1)), "lengths": np.array([1, 4, 9])}):
        with pytest.raises(AssertionError, match="the device was touched"):
            FL.feature_labels(Sae(), no_device, "enc", **kw)


def test_too_many_frames_are_refused_without_a_device(no_device, monkeypatch):
    from freud_amd import feature_labels as FL
    monkeypatch.setattr(FL, "MAX_FRAMES", 11)          # 3 files x 4 frames
    with pytest.raises(ValueError, match="exceed the 11 frames"):
        FL.feature_labels("ckpt.pth", no_device, "enc", file_labels=np.array([0, 1, 0]))


def test_npz_round_trip_and_lookup_by_name(tmp_path):
    from freud_amd import feature_labels as FL
    A, lc = random_table(6, 24, 40, 3)
    C, K = 6, 4
    names = [f"class{i}" for i in range(C)]
    by_label, by_latent = np_top(A, lc, "recall", K, 0), np_top(A, lc, "recall", K, 1)
    fl = FL.FeatureLabels(40, lc[:C].copy(), A[C].astype(np.int64), *by_label, *by_latent, A[:C].copy(), "recall", names)
    l = int(np.argmax((by_label[0] >= 0).sum(1)))
    want = [(int(p), int(c), float(s)) for p, c, s in zip(by_label[0][l], by_label[1][l], by_label[2][l]) if p >= 0]
    assert want and fl.top_latents(l) == want == fl.top_latents(names[l])
    j = int(np.argmax((by_latent[0] >= 0).sum(1)))
    assert fl.top_labels(j) == [(int(p), int(c), float(s)) for p, c, s in zip(by_latent[0][j], by_latent[1][j], by_latent[2][j]) if p >= 0]
    with pytest.raises(KeyError):
        fl.top_latents("no such class")
    s = fl.summary()
    assert s["n_frames"] == 40 and s["n_classes"] == C and s["n_latents"] == 24 and s["measure"] == "recall" and s["n_top"] == K
    for with_extras in (True, False):
        if not with_extras:
            fl.matrix, fl.class_names = None, None
        path = str(tmp_path / f"fl{int(with_extras)}.npz")
        fl.to_npz(path)
        back = FL.FeatureLabels.from_npz(path)
        assert back.n_frames == 40 and back.measure == "recall"
        for k in FL._FIELDS:
            assert getattr(back, k).tobytes() == getattr(fl, k).tobytes() and getattr(back, k).dtype == getattr(fl, k).dtype, k
        assert (back.matrix is None) == (not with_extras) and back.class_names == (names if with_extras else None)
        if with_extras:
            np.testing.assert_array_equal(back.matrix, A[:C])
            assert back.top_latents(names[l]) == want
