"""CPU: the feature index without a device.

* the host half of freud_amd/csrc/findex.h (the position word, the posted-slot predicate, the serial reference build
  fi_build_serial and fi_verify_serial) compiled with g++ -Wall -Werror into a stand-alone program and replayed against the numpy
  statement (tests/feature_index_reference.py: flatten, mask, stable argsort) on random stores with zero slots, -0.0, int32 and
  int64 indices and indices outside the dictionary, which must be counted and not posted; a row with a repeated index makes the
  verify count non-zero;
* FeatureIndex (numpy only) over an index written from the numpy lists: series against FeatureShards.series and against the
  reference's own activation_tensor_from_indexed answers in tests/golden/collect_features.npz; top_activations and file_max
  against every answer of the real reference top_activations in tests/golden/feature_index.npz;
* the all-negative rule on a hand-made store, the stale-fingerprint refusal, the 2^32 positions refusal from the metadata alone.
Every comparison is exact: integers, and float32 bit patterns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import feature_index_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LAYER = "enc"

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "findex.h"
// in:  int64 rows, K, n_dict, idx32, pos0, limit; uint32 value bits [rows * K]; indices [rows * K] (int32 or int64)
// out: int64 stats[8], bad, starts[n_dict + 1]; uint32 positions[nnz], values[nnz]
template <typename IdxT>
static int run(FILE* in, FILE* out, int64_t rows, int K, int64_t n, uint64_t pos0, uint64_t limit, const std::vector<uint32_t>& bits) {
  std::vector<IdxT> idx((size_t)(rows * K));
  if (fread(idx.data(), sizeof(IdxT), idx.size(), in) != idx.size()) return 2;
  std::vector<int64_t> starts((size_t)n + 1);
  int64_t stats[FI_NSTATS] = {0}, stats2[FI_NSTATS] = {0};
  fi_build_serial<IdxT>(bits.data(), idx.data(), rows, K, n, pos0, starts.data(), nullptr, nullptr, stats);
  std::vector<uint32_t> pos((size_t)starts[n] + 1), val((size_t)starts[n] + 1);
  fi_build_serial<IdxT>(bits.data(), idx.data(), rows, K, n, pos0, starts.data(), pos.data(), val.data(), stats2);
  for (int i = 0; i < FI_NSTATS; ++i) if (stats[i] != stats2[i]) return 3;
  const int64_t bad = fi_verify_serial(starts.data(), n, pos.data(), limit);
  fwrite(stats, 8, FI_NSTATS, out);
  fwrite(&bad, 8, 1, out);
  fwrite(starts.data(), 8, starts.size(), out);
  fwrite(pos.data(), 4, (size_t)starts[n], out);
  fwrite(val.data(), 4, (size_t)starts[n], out);
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  int64_t h[6];
  if (fread(h, 8, 6, in) != 6) return 2;
  std::vector<uint32_t> bits((size_t)(h[0] * h[1]));
  if (fread(bits.data(), 4, bits.size(), in) != bits.size()) return 2;
  const int rc = h[3] ? run<int32_t>(in, out, h[0], (int)h[1], h[2], (uint64_t)h[4], (uint64_t)h[5], bits)
                      : run<int64_t>(in, out, h[0], (int)h[1], h[2], (uint64_t)h[4], (uint64_t)h[5], bits);
  fclose(out);
  return rc;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("fi_host")
    src = d / "fi.cpp"
    src.write_text(_SRC)
    exe = d / "fi"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def _serial(prog, tmp_path, values, indices, n, pos0, limit):
    rows, K = values.shape
    idx32 = indices.dtype == np.int32
    (tmp_path / "in.bin").write_bytes(np.array([rows, K, n, int(idx32), pos0, limit], np.int64).tobytes()
                                      + np.ascontiguousarray(values).view(np.uint32).tobytes() + np.ascontiguousarray(indices).tobytes())
    subprocess.run([prog, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    raw = (tmp_path / "out.bin").read_bytes()
    head = np.frombuffer(raw, np.int64, 9 + n + 1)
    stats, bad, starts = head[:8], int(head[8]), head[9:]
    nnz = int(starts[-1])
    body = np.frombuffer(raw, np.uint32, 2 * nnz, offset=8 * (9 + n + 1))
    return stats, bad, starts, body[:nnz], body[nnz:]


def random_store(seed, rows, K, n, dtype, zero_frac=0.33, out_of_range=0):
    """[rows, K] values / indices: distinct indices per row, about zero_frac of the slots +-0.0, `out_of_range` non-zero slots with
    an index outside [0, n) (one of them negative)."""
    g = np.random.default_rng(seed)
    idx = np.argsort(g.random((rows, n)), axis=1)[:, :K].astype(dtype)
    val = g.normal(0, 1, (rows, K)).astype(np.float32)
    val[val == 0] = 1.0
    z = g.random((rows, K)) < zero_frac
    val[z] = np.where(g.random(int(z.sum())) < 0.2, np.float32(-0.0), np.float32(0.0))
    for c in range(out_of_range):
        r, q = int(g.integers(rows)), int(g.integers(K))
        idx[r, q] = -1 - c if c == 0 else n + c * 1000
        val[r, q] = 2.5
    return val, idx


@pytest.mark.parametrize("seed,rows,K,n,dtype,oor", [(0, 57, 4, 23, np.int64, 0), (1, 200, 4, 96, np.int32, 3), (2, 31, 7, 7, np.int64, 2),
                                                    (3, 40, 1, 5, np.int32, 0), (4, 19, 65, 300, np.int64, 4)])
def test_serial_build_equals_numpy(prog, tmp_path, seed, rows, K, n, dtype, oor):
    val, idx = random_store(seed, rows, K, n, dtype, out_of_range=oor)
    pos0 = 7 * rows
    starts, positions, vbits, st = R.reference_index(val, idx, n, pos0)
    stats, bad, c_starts, c_pos, c_val = _serial(prog, tmp_path, val, idx, n, pos0, pos0 + rows)
    assert [int(s) for s in stats[:4]] == [st["slots"], st["zero_slots"], st["out_of_range"], st["posted"]]
    assert st["out_of_range"] >= min(oor, 1) and st["zero_slots"] > 0
    assert np.array_equal(c_starts, starts) and np.array_equal(c_pos, positions) and np.array_equal(c_val, vbits)
    assert bad == 0 and R.verify_count(starts, positions, pos0 + rows) == 0
    # a limit one short of the last row's position flags exactly that row's slots
    assert R.verify_count(starts, positions, pos0 + rows - 1) == int((positions == pos0 + rows - 1).sum())


def test_duplicate_index_in_a_row_fails_verify(prog, tmp_path):
    val, idx = random_store(5, 20, 4, 12, np.int64, zero_frac=0.0)
    idx[9, 3] = idx[9, 0]
    starts, positions, _vbits, _st = R.reference_index(val, idx, 12)
    _stats, bad, c_starts, c_pos, _c_val = _serial(prog, tmp_path, val, idx, 12, 0, 20)
    assert np.array_equal(c_starts, starts) and np.array_equal(c_pos, positions)
    assert bad == 1 and R.verify_count(starts, positions, 20) == 1


def write_store(folder, values, indices, n, filenames=None, layer=LAYER):
    """values / indices [F, T, K] -> the reference's indexed store files."""
    F, T, K = values.shape
    os.makedirs(folder, exist_ok=True)
    names = [f"f{i}.flac" for i in range(F)] if filenames is None else [str(f) for f in filenames]
    np.save(os.path.join(folder, f"{layer}_activation_values.npy"), np.ascontiguousarray(values, dtype=np.float32).reshape(F, T * K))
    np.save(os.path.join(folder, f"{layer}_feature_indices.npy"), np.ascontiguousarray(indices).reshape(F, T * K))
    with open(os.path.join(folder, f"{layer}_metadata.json"), "w") as f:
        json.dump({"tensor_shape": [T, K], "activation_shape": [T, int(n)], "filenames": names}, f)
    return names


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["topk", "l1"])
def test_series_equals_shards_and_reference(tmp_path, kind):
    from freud_amd.collect_features import FeatureShards
    from freud_amd.feature_index import FeatureIndex
    z = np.load(os.path.join(GOLD, "collect_features.npz"))
    n, K = int(z[f"{kind}_n"]), int(z[f"{kind}_K"])
    sv, si = z[f"{kind}_store_values"], z[f"{kind}_store_indices"]
    F, T = sv.shape[0], sv.shape[1] // K
    write_store(str(tmp_path), sv.reshape(F, T, K), si.reshape(F, T, K), n, z["filenames"])
    starts, positions, vbits, st = R.reference_index(sv.reshape(F * T, K), si.reshape(F * T, K), n)
    R.write_reference_index(str(tmp_path), LAYER)
    ix, sh = FeatureIndex(str(tmp_path), LAYER), FeatureShards(str(tmp_path), LAYER)
    assert ix.nnz == st["posted"] and np.array_equal(ix.counts, np.diff(starts)) and len(ix) == F
    assert ix.metadata["build"]["zero_slots"] == st["zero_slots"] and ix.metadata["index_dtype"] == "int64"
    ref = z[f"{kind}_ref_series"]
    for j in range(n):
        p, v = ix.postings(j)
        assert np.array_equal(p, positions[starts[j]:starts[j + 1]]) and np.array_equal(bits(v), vbits[starts[j]:starts[j + 1]])
        assert np.all(np.diff(p.astype(np.int64)) > 0)
        s = ix.series(j)
        assert s.dtype == np.float32 and np.array_equal(bits(s), bits(sh.series(j))) and np.array_equal(bits(s), bits(ref[j]))
        assert np.array_equal(bits(ix.series(j, [2, 0])), bits(ref[j][[2, 0]]))


@pytest.fixture(scope="module")
def golden_index(tmp_path_factory):
    from freud_amd.feature_index import FeatureIndex
    z = np.load(os.path.join(GOLD, "feature_index.npz"))
    d = str(tmp_path_factory.mktemp("fi_golden"))
    write_store(d, z["values"], z["indices"], int(z["n_dict"]), z["filenames"])
    R.write_reference_index(d, LAYER)
    return z, FeatureIndex(d, LAYER)


def test_golden_series_and_file_max(golden_index):
    z, ix = golden_index
    n, lengths, T = int(z["n_dict"]), z["lengths"], z["values"].shape[1]
    assert ix.counts[9] == 0 and (ix.counts[:9] > 0).all()                       # the latent nobody fires
    for j in range(n):
        assert np.array_equal(bits(ix.series(j)), bits(z["ref_series"][j]))
    for c in np.flatnonzero((z["case_n_top"] == 1) & np.isnan(z["case_min_val"]) & np.isnan(z["case_max_val"])):
        j, absm = int(z["case_feature"][c]), bool(z["case_absolute"][c])
        vals, frames = ix.file_max(j, lengths, absm)
        assert vals.dtype == np.float32 and np.array_equal(vals.astype(np.float64), z["case_max_per_file"][c])
        for f in range(len(ix)):
            a = z["ref_series"][j][f, : min(int(lengths[f]), T)]
            assert frames[f] == (int(np.argmax(np.abs(a))) if absm else int(np.argmax(a)))


def test_golden_top_activations(golden_index):
    z, ix = golden_index
    lengths, names, T = z["lengths"], [str(s) for s in z["filenames"]], z["values"].shape[1]
    nan = lambda v: None if np.isnan(v) else float(v)      # noqa: E731
    silent_only = 0
    for c in range(z["case_feature"].shape[0]):
        j, n_top, absm = int(z["case_feature"][c]), int(z["case_n_top"][c]), bool(z["case_absolute"][c])
        pq, mpf = ix.top_activations(j, n_top, nan(z["case_max_val"][c]), nan(z["case_min_val"][c]), absm, True, lengths)
        want = [int(f) for f in z["case_files"][c] if f >= 0]
        assert [names.index(p[0]) for p in pq] == want, (c, j)
        assert [p[2] for p in pq] == [float(v) for v in z["case_values"][c][:len(want)]]
        assert [p[3] for p in pq] == [float(v) for v in z["case_times"][c][:len(want)]]
        assert mpf == [float(v) for v in z["case_max_per_file"][c]]
        for p, f in zip(pq, want):
            assert np.array_equal(bits(p[1]), bits(z["ref_series"][j][f, : min(int(lengths[f]), T)]))
        silent_only += bool(want) and not np.isnan(z["case_max_val"][c]) and all(v <= 0 for v in z["case_values"][c][:len(want)])
        pq2, none = ix.top_activations(j, n_top, nan(z["case_max_val"][c]), nan(z["case_min_val"][c]), absm, False, lengths)
        assert none is None and [p[0] for p in pq2] == [p[0] for p in pq]
    assert silent_only > 0


def test_all_negative_rule(tmp_path):
    """Frames without a posting are 0.0: a file whose posted values are all negative has its maximum 0.0 at the first frame that
    has no posting; only when every kept frame holds a negative posting does the negative maximum stand."""
    from freud_amd.feature_index import FeatureIndex
    F, T, K, n = 4, 5, 2, 3
    v = np.zeros((F, T, K), np.float32)
    i = np.tile(np.array([0, 1], np.int64), (F, T, 1))
    v[0, :, 0] = [-1, -2, 0, -3, -0.5]            # first unposted frame: 2
    v[1, :, 0] = [-3, -1, -2, -1, -4]             # every frame posted: -1 at frame 1 (the first of the two)
    v[2, :, 0] = [0, -5, 0, 0, 0]                 # frame 0 unposted
    v[3, :, 0] = [-2, -3, -1, 0, 7]               # lengths cut frame 4: 0.0 at frame 3; untrimmed: 7 at frame 4
    write_store(str(tmp_path), v, i, n)
    R.write_reference_index(str(tmp_path), LAYER)
    ix = FeatureIndex(str(tmp_path), LAYER)
    vals, frames = ix.file_max(0)
    assert vals.tolist() == [0.0, -1.0, 0.0, 7.0] and frames.tolist() == [2, 1, 0, 4]
    assert np.array_equal(bits(vals[[0, 2]]), bits(np.zeros(2, np.float32)))               # +0.0
    lengths = np.array([2, 5, 1, 4])
    vals, frames = ix.file_max(0, lengths)
    assert vals.tolist() == [-1.0, -1.0, 0.0, 0.0] and frames.tolist() == [0, 1, 0, 3]
    vals, frames = ix.file_max(0, lengths, absolute_magnitude=True)
    assert vals.tolist() == [-2.0, -4.0, 0.0, -3.0] and frames.tolist() == [1, 4, 0, 1]
    for absm in (False, True):
        dense = R.dense_series(v, i, n)[0]
        want, want_mpf = R.top_activations_dense(dense, ix.filenames, 3, None, None, absm, lengths)
        got, mpf = ix.top_activations(0, 3, absolute_magnitude=absm, return_max_per_file=True, lengths=lengths)
        assert [(g[0], g[2], g[3]) for g in got] == [(w[0], w[2], w[3]) for w in want] and mpf == want_mpf
    vals, frames = ix.file_max(2)                                                           # a latent nobody fires
    assert not vals.any() and not frames.any()


def test_stale_index_is_refused(tmp_path):
    from freud_amd.feature_index import FeatureIndex, index_paths
    val, idx = random_store(8, 3 * 6, 2, 9, np.int64)
    write_store(str(tmp_path), val.reshape(3, 6, 2), idx.reshape(3, 6, 2), 9)
    R.write_reference_index(str(tmp_path), LAYER)
    FeatureIndex(str(tmp_path), LAYER)
    with pytest.raises(ValueError, match="already holds"):
        R.write_reference_index(str(tmp_path), LAYER)
    write_store(str(tmp_path), val.reshape(3, 6, 2), idx.reshape(3, 6, 2), 9, filenames=["a", "b", "c"])     # other filenames
    with pytest.raises(ValueError, match="stale"):
        FeatureIndex(str(tmp_path), LAYER)
    val2, idx2 = random_store(8, 4 * 6, 2, 9, np.int64)
    write_store(str(tmp_path), val2.reshape(4, 6, 2), idx2.reshape(4, 6, 2), 9)                              # other file sizes
    with pytest.raises(ValueError, match="stale"):
        FeatureIndex(str(tmp_path), LAYER)
    R.write_reference_index(str(tmp_path), LAYER, overwrite=True)
    assert len(FeatureIndex(str(tmp_path), LAYER)) == 4
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".partial")]
    assert all(os.path.exists(p) for p in index_paths(str(tmp_path), LAYER).values())


def test_too_many_positions_refused_from_metadata(tmp_path):
    """n_files * T >= 2^32 is refused from the numbers alone: the postings files do not even exist."""
    from freud_amd.feature_index import FeatureIndex, check_positions, index_paths
    check_positions((1 << 32) // 1500, 1500)
    with pytest.raises(ValueError, match=r"2\^32"):
        check_positions(1 << 21, 2048)
    meta = {"format": 1, "n_files": 1 << 21, "T": 2048, "K": 64, "n_dict": 24576, "nnz": 10 ** 12, "index_dtype": "int64", "build": {},
            "fingerprint": {}}
    with open(index_paths(str(tmp_path), LAYER)["metadata"], "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match=r"2\^32"):
        FeatureIndex(str(tmp_path), LAYER)


def test_plan_ranges():
    from freud_amd.feature_index import plan_ranges
    starts = np.array([0, 10, 10, 40, 45, 100], np.int64)
    assert plan_ranges(starts, 10 ** 9, 4) == [(0, 5)]
    r = plan_ranges(starts, 55 * 8 + 4, 4)
    assert r[0][0] == 0 and r[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(r, r[1:])) and len(r) >= 2
    assert all((starts[b] - starts[a]) * 8 + (b - a) * 4 <= 55 * 8 + 4 for a, b in r)
    with pytest.raises(ValueError, match="does not hold"):
        plan_ranges(starts, 54 * 8, 4)


def test_reader_needs_no_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import freud_amd.feature_index as m\n"
            "assert hasattr(m, 'FeatureIndex') and 'torch' not in [k for k, v in sys.modules.items() if v is not None]\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_entry_points_declared_and_exported():
    import re
    from freud_amd import engine
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for name in ("sae_findex_workspace_bytes", "sae_findex_count", "sae_findex_fill", "sae_findex_verify"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in engine.EXPORTED_SYMBOLS
    assert "activations.py:41-58" in text and ":95-101" in text


def test_cli_top(golden_index, tmp_path, capsys):
    from freud_amd import feature_index as FI
    z, ix = golden_index
    folder = os.path.dirname(ix.positions.filename)
    np.save(tmp_path / "lengths.npy", z["lengths"])
    FI.main(["top", "--data_path", folder, "--layer_name", LAYER, "--feature", "0", "--n_files", "5", "--min_val", "0.5",
             "--lengths", str(tmp_path / "lengths.npy")])
    got = json.loads(capsys.readouterr().out)
    want, _ = ix.top_activations(0, 5, None, 0.5, False, False, z["lengths"])
    assert [(g["file"], g["value"], g["time"], g["frames"]) for g in got] == [(w[0], w[2], w[3], w[1].size) for w in want] and len(got) >= 2
