"""CPU: feature collection without a device.

* the host half of freud_amd/csrc/collect.h (the entry word, the ordering predicate and the serial reference cl_collect_serial that
  the kernels' answers are defined by) compiled with g++ -Wall -Werror into a stand-alone program and replayed against
  numpy.argsort(-a, kind="stable")[:K] on rows built to hit every edge: nnz in {0, K - 1, K, K + 1, n}, ties straddling the
  threshold, ties among the positives, a -0.0 pattern, K = 1 and K = n, an n that is no multiple of 64, a column above 65 535;
  indices, value bits (+0.0 padding) and the eight statistics against a numpy count;
* the writer and the reader round trip: serial-select slots fed through the module's file writer by a fake device source, the
  documented files, FeatureShards, the three refusals, overwrite, an interrupted run;
* the replay of tests/golden/collect_features.npz (tests/golden/make_collect_golden.py): the reference's own encode() outputs, its
  activation_tensor_from_indexed and what its MemoryMappedActivationsDataset read from a store this module wrote;
* the boundary: header text, EXPORTED_SYMBOLS, the symbol in the built library, the constants."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import build_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "collect.h"

// argv: data file (int64 rows, n; uint16 bits[rows][n]) K -> per row "idx..." / "valuebits..." lines, then the 8 statistics
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[1], "rb");
  int64_t rows, n;
  if (!fp || fread(&rows, 8, 1, fp) != 1 || fread(&n, 8, 1, fp) != 1) return 2;
  std::vector<uint16_t> bits((size_t)(rows * n));
  if (fread(bits.data(), 2, bits.size(), fp) != bits.size()) return 2;
  fclose(fp);
  const int K = atoi(argv[2]);
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<float> vals(K);
  std::vector<int64_t> idx(K);
  for (int64_t r = 0; r < rows; ++r) {
    cl_collect_serial(bits.data() + r * n, n, K, vals.data(), idx.data(), stats);
    for (int i = 0; i < K; ++i) printf("%lld ", (long long)idx[i]);
    printf("\n");
    for (int i = 0; i < K; ++i) { uint32_t u; memcpy(&u, &vals[i], 4); printf("%08x ", u); }
    printf("\n");
  }
  for (int i = 0; i < 8; ++i) printf("%lld ", (long long)stats[i]);
  printf("\n");
  // the predicate and the entry word
  if (!cl_before(cl_entry(0x3F80, 9), cl_entry(0x3F80, 10)) || !cl_before(cl_entry(0x3F81, 70000), cl_entry(0x3F80, 0))) return 3;
  if (cl_entry_bits(cl_entry(0x8000, 5)) != 0 || cl_entry_bits(cl_entry(0xBF80, 5)) != 0 || cl_entry_col(cl_entry(0x3F80, 70000)) != 70000) return 3;
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("cl")
    src = d / "cl.cpp"
    src.write_text(_SRC)
    exe = d / "cl"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def bits_to_float(bits):
    return (np.asarray(bits, np.uint32) << 16).view(np.float32)


def serial(prog, tmp_path, bits, K):
    """bits uint16 [rows, n] -> (idx int64 [rows, K], value bits uint32 [rows, K], stats int64 [8]) of cl_collect_serial."""
    bits = np.ascontiguousarray(bits, np.uint16)
    rows, n = bits.shape
    data = tmp_path / "rows.bin"
    data.write_bytes(np.array([rows, n], np.int64).tobytes() + bits.tobytes())
    out = subprocess.run([prog, str(data), str(K)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 2 * rows + 1
    idx = np.array([[int(v) for v in out[2 * r].split()] for r in range(rows)], np.int64).reshape(rows, K)
    val = np.array([[int(v, 16) for v in out[2 * r + 1].split()] for r in range(rows)], np.uint32).reshape(rows, K)
    return idx, val, np.array([int(v) for v in out[-1].split()], np.int64)


def oracle(bits, K):
    """The definition: the stable argsort of the latent the bits stand for (-0.0 and every negative pattern: inactive, value 0),
    and the statistics by a numpy count."""
    bits = np.asarray(bits, np.uint16)
    active = (bits >= 1) & (bits <= 0x7FFF)
    a = np.where(active, bits_to_float(bits), np.float32(0))
    idx = np.argsort(-a, axis=1, kind="stable")[:, :K]
    val = np.take_along_axis(a, idx, 1)
    nnz = active.sum(1)
    stored = np.minimum(nnz, K)
    cut = np.zeros(len(bits), np.int64)
    for r in np.flatnonzero(nnz > K):
        cut[r] = int(np.sort(bits[r][active[r]])[::-1][K])
    stats = np.array([len(bits), stored.sum(), (nnz - stored).sum(), (nnz > K).sum(), nnz.max(initial=0), cut.max(initial=0), 0, 0], np.int64)
    return idx.astype(np.int64), val.view(np.uint32), stats


def edge_rows(n, K, seed):
    """Rows of n bf16 patterns around K: nnz in {0, K - 1, K, K + 1, n}, ties across the threshold and among the positives, -0.0."""
    g = np.random.default_rng(seed)
    pos = np.array([0x3F80, 0x3F81, 0x3F00, 0x4000, 0x3E80, 0x0001, 0x7F7F], np.uint16)      # few values: constant ties
    rows = []
    for nnz in sorted({0, max(K - 1, 0), K, min(K + 1, n), n}):
        r = np.zeros(n, np.uint16)
        at = g.permutation(n)[:nnz]
        r[at] = g.choice(pos, nnz)
        rows.append(r)
        r2 = np.zeros(n, np.uint16)
        r2[at] = 0x3F80                                   # every active value equal: the threshold is one long tie
        rows.append(r2)
    r = np.zeros(n, np.uint16)                            # -0.0 and negative patterns are inactive and store +0.0
    r[:: 3] = 0x8000
    r[1:: 5] = 0xBF80
    r[2:: 7] = 0x3F80
    rows.append(r)
    r = g.choice(pos, n)                                  # dense, with zeros sprinkled in
    r[g.permutation(n)[: n // 4]] = 0
    rows.append(r.astype(np.uint16))
    return np.stack(rows)


@pytest.mark.parametrize("n,K", [(8, 1), (8, 8), (100, 7), (100, 99), (100, 100), (257, 32), (1000, 128), (300, 299)])
def test_serial_select_is_the_stable_argsort(prog, tmp_path, n, K):
    bits = edge_rows(n, K, seed=n * 1000 + K)
    idx, val, stats = serial(prog, tmp_path, bits, K)
    widx, wval, wstats = oracle(bits, K)
    np.testing.assert_array_equal(idx, widx)
    np.testing.assert_array_equal(val, wval)
    np.testing.assert_array_equal(stats, wstats)
    assert stats[6] == 0 and stats[7] == 0
    for r in range(len(bits)):
        assert len(set(idx[r].tolist())) == K                       # distinct indices, always
    assert not (val == 0x80000000).any()                            # the padding is +0.0


def test_serial_select_carries_columns_above_65535(prog, tmp_path):
    n, K = 70001, 5
    bits = np.zeros((3, n), np.uint16)
    bits[0, [65535, 65536, 70000, 12]] = [0x3F80, 0x3F80, 0x4000, 0x3F00]
    bits[1, 66000:66010] = 0x3F80                                   # a tie above 65 535 that straddles the threshold
    bits[2, 69999] = 0x8000                                         # a lone -0.0: the row pads from column 0
    idx, val, stats = serial(prog, tmp_path, bits, K)
    widx, wval, wstats = oracle(bits, K)
    np.testing.assert_array_equal(idx, widx)
    np.testing.assert_array_equal(val, wval)
    np.testing.assert_array_equal(stats, wstats)
    assert idx[0].tolist() == [70000, 65535, 65536, 12, 0] and idx[1].tolist() == [66000, 66001, 66002, 66003, 66004]
    assert idx[2].tolist() == [0, 1, 2, 3, 4] and stats[2] == 5 and stats[5] == 0x3F80


# ---------------------------------------------------------------------------------------------------------------------------
# writer / reader
def _latent(F, T, n, seed, density=0.1):
    g = np.random.default_rng(seed)
    vals = np.array([0x3F80, 0x3F00, 0x4000, 0x3E80, 0x3F81], np.uint16)
    bits = np.where(g.random((F, T, n)) < density, g.choice(vals, (F, T, n)), 0).astype(np.uint16)
    bits[0, 0] = 0                                                    # an all-zero row
    bits[0, 1, :3] = 0x8000
    return bits


class FakeSource:
    """Stand-in for the device source of collect_features: batches of (file0, values [nb, T, K], indices [nb, T, K]) from the serial
    select, and the statistics block it would have accumulated."""

    def __init__(self, prog, tmp_path, bits, K, batch, index_dtype=np.int64, die_after=None):
        self.bits, self.K, self.batch, self.index_dtype, self.die_after = bits, K, batch, index_dtype, die_after
        F, T, n = bits.shape
        idx, val, self.stats = serial(prog, tmp_path, bits.reshape(F * T, n), K)
        self.idx, self.val = idx.reshape(F, T, K), val.view(np.float32).reshape(F, T, K)

    def __iter__(self):
        for b, f0 in enumerate(range(0, self.bits.shape[0], self.batch)):
            if self.die_after is not None and b == self.die_after:
                raise KeyboardInterrupt
            yield f0, self.val[f0:f0 + self.batch], self.idx[f0:f0 + self.batch].astype(self.index_dtype)


def _store(prog, tmp_path, out, bits, K, index_dtype="int64", batch=2, die_after=None, overwrite=False):
    from freud_amd import collect_features as CF
    F, T, n = bits.shape
    src = FakeSource(prog, tmp_path, bits, K, batch, CF._INDEX_DTYPES[index_dtype], die_after)
    w = CF.StoreWriter(str(out), "enc", [f"a{i}.flac" for i in range(F)], T, K, n, variant="l1", index_dtype=index_dtype, overwrite=overwrite)
    return CF.write_store(src, w, lambda: src.stats), src


@pytest.mark.parametrize("index_dtype", ["int64", "int32"])
def test_writer_reader_round_trip(prog, tmp_path, index_dtype):
    from freud_amd import collect_features as CF
    F, T, n, K = 5, 6, 40, 12
    bits = _latent(F, T, n, 3)
    out = tmp_path / "store"
    rep, src = _store(prog, tmp_path, out, bits, K, index_dtype)
    assert rep.complete and rep.dropped == 0 and rep.rows == F * T and rep.largest_dropped == 0.0 and rep.max_active <= K
    v = np.load(out / "enc_activation_values.npy")
    i = np.load(out / "enc_feature_indices.npy")
    assert v.dtype == np.float32 and v.shape == (F, T * K) and i.dtype == np.dtype(index_dtype) and i.shape == (F, T * K)
    for name in ("enc_activation_values.npy", "enc_feature_indices.npy"):
        with open(out / name, "rb") as f:
            assert f.read(8) == b"\x93NUMPY\x01\x00"                 # a plain version-1.0 file
    meta = json.load(open(out / "enc_metadata.json"))
    assert set(meta) == {"tensor_shape", "activation_shape", "filenames", "freud_amd"}
    assert meta["tensor_shape"] == [T, K] and meta["activation_shape"] == [T, n] and meta["filenames"] == [f"a{i}.flac" for i in range(F)]
    fa = meta["freud_amd"]
    assert fa["variant"] == "l1" and fa["K"] == K and fa["sorted"] is True and fa["index_dtype"] == index_dtype
    assert [fa["stats"][k] for k in CF.STAT_NAMES] == src.stats.tolist()
    assert rep.bytes_written == sum(os.path.getsize(out / f) for f in os.listdir(out)) and set(rep.paths) == {"values", "indices", "metadata"}
    fs = CF.FeatureShards(str(out), "enc")
    a = np.where((bits >= 1) & (bits <= 0x7FFF), bits_to_float(bits), np.float32(0))
    for f in range(F):
        rv, ri = fs.rows(f)
        assert rv.shape == (T, K) and ri.shape == (T, K)
        np.testing.assert_array_equal(fs.dense(f).view(np.uint32), a[f].view(np.uint32))      # dropped == 0: dense() is the latent
    for j in range(n):
        np.testing.assert_array_equal(fs.series(j), a[:, :, j])
    np.testing.assert_array_equal(fs.series(3, files=[4, 1]), a[[4, 1], :, 3])
    assert len(fs) == F and fs.info["K"] == K


def test_dropping_store_reports_what_was_cut(prog, tmp_path):
    from freud_amd import collect_features as CF
    bits = _latent(3, 4, 40, 5, density=0.6)
    rep, src = _store(prog, tmp_path, tmp_path / "s", bits, 4)
    active = (bits >= 1) & (bits <= 0x7FFF)
    nnz = active.sum(2)
    assert not rep.complete and rep.dropped == int(np.maximum(nnz - 4, 0).sum()) and rep.rows_dropped == int((nnz > 4).sum())
    assert rep.stored + rep.dropped == int(nnz.sum()) and rep.max_active == int(nnz.max()) and rep.largest_dropped > 0
    fs = CF.FeatureShards(str(tmp_path / "s"), "enc")
    a = np.where(active, bits_to_float(bits), np.float32(0))
    top = -np.sort(-a, axis=2)[:, :, :4]
    for f in range(3):
        np.testing.assert_array_equal(fs.rows(f)[0], top[f])


def test_refusals_overwrite_and_an_interrupted_run(prog, tmp_path):
    from freud_amd import collect_features as CF
    from freud_amd.loader import write_shards
    data = tmp_path / "data"
    write_shards(str(data), "enc", np.zeros((2, 8), np.float32), [4, 2])
    out = tmp_path / "out"
    # 1. the output is the input (also through a link or a relative spelling)
    with pytest.raises(ValueError, match="shard directory itself"):
        CF.check_out_folder(str(data), str(data) + "/../data", "enc", "indexed", True)
    with pytest.raises(ValueError, match="shard directory itself"):
        CF.collect_features("ck.pt", str(data), "enc", str(data), k=4)
    # 2. a tensor file in the output
    other = tmp_path / "other"
    write_shards(str(other), "enc", np.zeros((2, 8), np.float32), [4, 2])
    with pytest.raises(ValueError, match="prefers it"):
        CF.collect_features("ck.pt", str(data), "enc", str(other), k=4, overwrite=True)
    # 3. a store is there and overwrite is not set
    bits = _latent(3, 4, 20, 7)
    _store(prog, tmp_path, out, bits, 5)
    with pytest.raises(ValueError, match="already holds"):
        CF.collect_features("ck.pt", str(data), "enc", str(out), k=4)
    with pytest.raises(ValueError, match="already holds"):
        CF.check_out_folder(str(data), str(out), "enc", "tensor", False)
    CF.check_out_folder(str(data), str(out), "enc", "indexed", True)
    with pytest.raises(ValueError, match="needs an SAE"):
        CF.collect_features(None, str(data), "enc", str(tmp_path / "x"), k=4)
    with pytest.raises(ValueError, match="index_dtype"):
        CF.collect_features("ck.pt", str(data), "enc", str(tmp_path / "x"), k=4, index_dtype="int16")
    with pytest.raises(ValueError, match="layout"):
        CF.collect_features("ck.pt", str(data), "enc", str(tmp_path / "x"), k=4, layout="sparse")
    assert not (tmp_path / "x").exists()
    # the writer itself refuses as well: no caller loses a store without saying overwrite
    before = np.load(out / "enc_activation_values.npy")
    bits2 = _latent(4, 4, 20, 8)
    with pytest.raises(ValueError, match="already holds"):
        _store(prog, tmp_path, out, bits2, 3)
    with pytest.raises(ValueError, match="already holds"):
        CF.StoreWriter(str(other), "enc", ["a.flac"], 4, 2, 20, variant="l1", layout="tensor")
    np.testing.assert_array_equal(np.load(out / "enc_activation_values.npy"), before)
    assert os.path.exists(other / "enc_tensors.npy")
    # overwrite replaces
    _store(prog, tmp_path, out, bits2, 3, overwrite=True)
    after = np.load(out / "enc_activation_values.npy")
    assert before.shape == (3, 20) and after.shape == (4, 12) and json.load(open(out / "enc_metadata.json"))["tensor_shape"] == [4, 3]
    # a run that dies before the rename leaves nothing that loads -- not the new store, not the old one
    with pytest.raises(KeyboardInterrupt):
        _store(prog, tmp_path, out, bits, 5, die_after=1, overwrite=True)
    assert os.listdir(out) == []
    with pytest.raises(FileNotFoundError):
        CF.FeatureShards(str(out), "enc")


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's own answers (tests/golden/make_collect_golden.py)
def to_bf16_bits(a):
    """fp32 -> bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.mark.parametrize("kind", ["topk", "l1"])
def test_golden_select_through_the_serial_reference(prog, tmp_path, kind):
    """The project's own select (cl_collect_serial) on the reference's encode() outputs, rounded to the bf16 the engine's latent
    is: TopK -- the slots are, as a set, the reference's (top_indices, top_acts) after the same rounding; L1 -- the slot values are
    the rounded top K values of the reference's latent (rounding is monotone, so the multiset survives whichever member of a tie
    at the threshold is taken), and every slot's value is the latent's at its index."""
    g = np.load(os.path.join(GOLD, "collect_features.npz"))
    n, K = int(g[f"{kind}_n"]), int(g[f"{kind}_K"])
    if kind == "topk":
        acts, tidx = g["topk_top_acts"], g["topk_top_indices"]
        F, T, _ = acts.shape
        lat = np.zeros((F, T, n), np.float32)
        np.put_along_axis(lat, tidx, acts, axis=2)
    else:
        lat = g["l1_latent"]
        F, T, _ = lat.shape
    bits = to_bf16_bits(lat).reshape(F * T, n)
    idx, val, stats = serial(prog, tmp_path, bits, K)
    rounded = bits_to_float(bits)
    np.testing.assert_array_equal(val.view(np.float32), np.take_along_axis(rounded, idx, 1))
    assert all(len(set(r.tolist())) == K for r in idx) and (np.diff(val.view(np.float32), axis=1) <= 0).all()
    if kind == "topk":
        want_v = bits_to_float(to_bf16_bits(acts)).reshape(F * T, K)
        for r in range(F * T):
            assert set(zip(idx[r].tolist(), val.view(np.float32)[r].tolist())) == set(zip(tidx.reshape(F * T, K)[r].tolist(), want_v[r].tolist()))
        assert stats[2] == 0 and stats[1] == F * T * K
    else:
        top = -np.sort(-lat.reshape(F * T, n), axis=1)[:, :K]                   # the reference's own top K values, fp32
        np.testing.assert_array_equal(val.view(np.float32), bits_to_float(to_bf16_bits(top)))
        nnz = (bits >= 1).sum(1)
        assert stats[2] == int(np.maximum(nnz - K, 0).sum()) > 0
        assert stats[5] == int(to_bf16_bits(-np.sort(-lat.reshape(F * T, n), axis=1)[:, K]).max()) == int(g["l1_stats"][5])


@pytest.mark.parametrize("kind", ["topk", "l1"])
def test_golden_replay(tmp_path, kind):
    """The writer and the reader against the reference's own reader.  (The slots in the golden file are the generator's numpy
    argsort of the reference's fp32 outputs: this pins StoreWriter, FeatureShards and what the reference's dataset class and
    activation_tensor_from_indexed made of the store; the select itself is test_golden_select_through_the_serial_reference.)"""
    from freud_amd import collect_features as CF
    g = np.load(os.path.join(GOLD, "collect_features.npz"))
    n, K = int(g[f"{kind}_n"]), int(g[f"{kind}_K"])
    vals, idx = g[f"{kind}_store_values"], g[f"{kind}_store_indices"]           # what the generator wrote through StoreWriter
    F, T = vals.shape[0], vals.shape[1] // K
    names = [str(s) for s in g["filenames"]]
    w = CF.StoreWriter(str(tmp_path), "enc", names, T, K, n, variant=kind)
    stats = g[f"{kind}_stats"]
    CF.write_store([(0, vals.reshape(F, T, K), idx.reshape(F, T, K))], w, lambda: stats)
    fs = CF.FeatureShards(str(tmp_path), "enc")
    # what the reference's MemoryMappedActivationsDataset answered for that store
    assert str(g[f"{kind}_ref_activation_type"]) == "indexed"
    assert g[f"{kind}_ref_activation_shape"].tolist() == [T, n] and len(names) == int(g[f"{kind}_ref_len"])
    rv, ri = fs.rows(0)
    np.testing.assert_array_equal(g[f"{kind}_ref_file0_values"], rv)
    np.testing.assert_array_equal(g[f"{kind}_ref_file0_indices"], ri)
    if kind == "topk":
        acts, tidx = g["topk_top_acts"], g["topk_top_indices"]                  # the reference's encode(): [F, T, k]
        for f in range(F):
            v, i = fs.rows(f)
            for t in range(T):
                assert set(zip(i[t].tolist(), v[t].tolist())) == set(zip(tidx[f, t].tolist(), acts[f, t].tolist()))
                assert (np.diff(v[t]) <= 0).all()
    else:
        lat = g["l1_latent"]                                                    # the reference's dense latent [F, T, n]
        want = np.argsort(-lat, axis=2, kind="stable")[:, :, :K]
        for f in range(F):
            v, i = fs.rows(f)
            np.testing.assert_array_equal(i, want[f])
            np.testing.assert_array_equal(v, np.take_along_axis(lat[f], want[f], 1))
    dense = g[f"{kind}_ref_series"]                                             # activation_tensor_from_indexed, [n, F, T]
    for j in range(n):
        np.testing.assert_array_equal(fs.series(j), dense[j])


# ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_symbol_list_and_constants():
    from freud_amd import collect_features as CF
    from freud_amd import engine
    raw = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert 'numpy.argsort(-a, kind="stable")[:K]' in raw and "activation_tensor_from_indexed" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+sae_collect_files\s*\(", text)
    assert "sae_collect_files" in engine.EXPORTED_SYMBOLS
    engine.build()
    assert hasattr(engine.load(), "sae_collect_files")
    assert int(re.search(r"#define\s+SAE_COLLECT_MAX_K\s+(\d+)", text).group(1)) == engine.COLLECT_MAX_K == CF.COLLECT_MAX_K == 1024
    assert int(re.search(r"SAE_COLLECT_IDX32\s*=\s*(\d+)", text).group(1)) == engine.COLLECT_IDX32 == 1
    src = open(os.path.join(ROOT, "freud_amd", "csrc", "collect.h")).read()
    assert int(re.search(r"#define\s+CL_MAX_K\s+(\d+)", src).group(1)) == 1024
    assert build_units.assert_one_unit_builds("collect.h") == "passes.hip"
    assert callable(engine.SaeEngine.collect_files) and len(CF.STAT_NAMES) == 8
    # loader.py still refuses to train on an indexed store, in its own words
    assert "SAE-encoded 'indexed' shards cannot be trained on" in open(os.path.join(ROOT, "freud_amd", "loader.py")).read()
