"""GPU: the feature index (freud_amd/feature_index.py over include/freud_sae.h's sae_findex_* entry points; kernels in
freud_amd/csrc/findex.h).

The oracle everywhere is tests/feature_index_reference.py: flatten, mask v != 0 and the index range, numpy's stable argsort by
latent.  Every comparison is exact -- integers and float32 bit patterns; files are compared byte for byte.

Internal thresholds of the kernels and where they are crossed:
  * FI_ROWS = 128 rows per block (one wave): 70, 130 and 200 rows are 1 and 2 blocks with a ragged last one; the pass tests run
    450-row batches (4 blocks);
  * one wave's 64 lanes per row chunk: K = 1, 4, 64 (the K <= 64 kernels), 65 (two chunks, 16 rows per round) and 130 (three
    chunks, 10 rows per round: a round count that does not divide the block);
  * FI_SEG = 16 384 latents per LDS segment: n = 16 384 + 128 and, the next multiple, n = 32 768 + 128, entries planted in the
    last latent of a segment and the first of the next;
  * cursors across batches and latent ranges: every entry-point case is also built in two batches and two ranges."""
import os

import numpy as np
import pytest
import torch

from freud_amd import collect_features as CF
from freud_amd import engine as E
from freud_amd import feature_index as FI
from tests import feature_index_reference as R
from tests.test_collect_features_gpu import l1_model, shards, topk_model
from tests.test_feature_index_cpu import LAYER, bits, random_store, write_store

pytestmark = pytest.mark.gpu


def direct_build(val, idx, n, cuts=(), ranges=None, pos0=0):
    """The entry points over val / idx [rows, K], in the batches that `cuts` (row numbers) split it into and the latent `ranges`
    (default: one) -> (starts, positions uint32, value bits uint32, stats dict, err [2]) on the host."""
    rows, K = val.shape
    v, x = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
    edges = [0, *cuts, rows]
    batches = list(zip(edges[:-1], edges[1:]))
    totals = torch.zeros(n, dtype=torch.int64, device="cuda")
    stats = torch.zeros(E.FINDEX_NSTATS, dtype=torch.int64, device="cuda")
    err = torch.zeros(2, dtype=torch.int64, device="cuda")
    for a, b in batches:
        E.findex_count(v[a:b], x[a:b], n, totals, stats)
    starts_dev = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(totals, 0, out=starts_dev[1:])
    starts = starts_dev.cpu().numpy()
    cursor = starts_dev[:-1].clone()
    positions, values = np.zeros(int(starts[-1]), np.uint32), np.zeros(int(starts[-1]), np.uint32)
    max_rows = max(b - a for a, b in batches)
    for j0, j1 in ([(0, n)] if ranges is None else ranges):
        base, cnt = int(starts[j0]), int(starts[j1] - starts[j0])
        pd = torch.full((max(cnt, 1),), -1, dtype=torch.int32, device="cuda")
        vd = torch.full((max(cnt, 1),), -1.0, dtype=torch.float32, device="cuda")
        work = torch.empty(E.findex_workspace_bytes(max_rows, j1 - j0), dtype=torch.uint8, device="cuda")
        for a, b in batches:
            E.findex_fill(v[a:b], x[a:b], n, j0, j1, pos0 + a, cursor, base, pd, vd, work, err)
        E.findex_verify(starts_dev, j0, j1, base, pd, pos0 + rows, err)
        positions[base:base + cnt] = pd[:cnt].cpu().numpy().view(np.uint32)
        values[base:base + cnt] = vd[:cnt].cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    assert torch.equal(cursor, starts_dev[1:])
    return starts, positions, values, dict(zip(E.FINDEX_STAT_NAMES, stats.cpu().numpy().tolist())), err.cpu().numpy().tolist()


def check_against_reference(val, idx, n, pos0=0):
    rows = val.shape[0]
    want = R.reference_index(val, idx, n, pos0)
    for cuts, ranges in (((), None), ((rows // 3,), [(0, n // 2), (n // 2, n)])):
        starts, positions, values, stats, err = direct_build(val, idx, n, cuts, ranges, pos0)
        assert err == [0, 0] and stats == want[3]
        assert np.array_equal(starts, want[0]) and np.array_equal(positions, want[1]) and np.array_equal(values, want[2])


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("rows,K,n", [(200, 4, 96), (130, 1, 64), (130, 64, 256), (130, 65, 256), (70, 130, 256)])
def test_entry_points_against_numpy(rows, K, n, dtype):
    val, idx = random_store(rows + K, rows, K, n, dtype, zero_frac=0.33, out_of_range=3)
    assert 0.2 < (val == 0).mean() < 0.45
    check_against_reference(val, idx, n, pos0=5 * rows)


@pytest.mark.parametrize("n", [E.FINDEX_SEGMENT + 128, 2 * E.FINDEX_SEGMENT + 128])
def test_dictionary_one_step_above_the_lds_segment(n):
    rows, K = 130, 4
    g = np.random.default_rng(n)
    idx = np.stack([g.choice(n, K, replace=False) for _ in range(rows)]).astype(np.int64)
    val = g.normal(0, 1, (rows, K)).astype(np.float32)
    val[g.random((rows, K)) < 0.33] = 0.0
    edges = [s for m in range(1, n // E.FINDEX_SEGMENT + 1) for s in (m * E.FINDEX_SEGMENT - 1, m * E.FINDEX_SEGMENT)]
    for r in range(rows):                       # the last latent of a segment and the first of the next, in rows of both blocks
        for q, j in enumerate(edges[2 * (r % (len(edges) // 2)):][:2]):
            if r % 7 != 5:
                idx[r, q], val[r, q] = j, 1.0 + r
        assert len(set(idx[r])) == K
    starts = R.reference_index(val, idx, n)[0]
    assert all(starts[j + 1] - starts[j] >= 20 for j in edges)
    check_against_reference(val, idx, n)


def _bytes(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder)) if "_postings" in f}


def pass_store(seed=21, F=6, T=150, K=8, n=50, dtype=np.int64):
    """A store whose latent 7 is fired by every row, whose latent 11 nobody fires (10 and 12 are busy), a third of the slots zero."""
    g = np.random.default_rng(seed)
    pool = np.array([j for j in range(n) if j not in (7, 11)])
    idx = np.stack([g.permutation(pool)[:K] for _ in range(F * T)]).astype(dtype)
    val = (g.normal(0, 1, (F * T, K)).astype(np.float32))
    val[val == 0] = 1.0
    val[g.random((F * T, K)) < 0.33] = 0.0
    idx[:, 2], val[:, 2] = 7, np.arange(1, F * T + 1, dtype=np.float32)
    return val.reshape(F, T, K), idx.reshape(F, T, K)


def check_index_files(folder, val, idx, n):
    F, T, K = val.shape
    starts, positions, vbits, st = R.reference_index(val.reshape(F * T, K), idx.reshape(F * T, K), n)
    ix = FI.FeatureIndex(folder, LAYER)
    assert np.array_equal(ix.starts, starts) and np.array_equal(ix.positions, positions) and np.array_equal(bits(ix.values), vbits)
    assert ix.positions.dtype == np.uint32 and ix.values.dtype == np.float32 and ix.starts.dtype == np.int64
    return ix, st


def test_pass_batches_ranges_determinism_overwrite(tmp_path):
    """Cursor carry-over (batch_files 1, 2 and all: 4 row blocks a batch at batch_files = 3), latent ranges, two runs, the report,
    the overwrite refusal: always the same bytes."""
    n = 50
    val, idx = pass_store()
    F, T, K = val.shape
    d = str(tmp_path / "s")
    write_store(d, val, idx, n)
    rep = FI.build_feature_index(d, LAYER, batch_files=3)
    ix, st = check_index_files(d, val, idx, n)
    assert ix.counts[7] == F * T and ix.counts[11] == 0 and ix.counts[10] > 0 and ix.counts[12] > 0
    assert (rep.nnz, rep.zero_slots, rep.slots, rep.out_of_range) == (st["posted"], st["zero_slots"], F * T * K, 0)
    assert (rep.longest_list, rep.longest_latent, rep.empty_lists, rep.sweeps, rep.ranges) == (F * T, 7, 1, 2, [(0, n)])
    first = _bytes(d)
    assert rep.bytes_written == sum(len(b) for b in first.values()) and len(first) == 4
    assert ix.metadata["build"]["zero_slots"] == st["zero_slots"] and ix.metadata["index_dtype"] == "int64"
    with pytest.raises(ValueError, match="already holds"):
        FI.build_feature_index(d, LAYER)
    assert _bytes(d) == first
    for bf in (1, 2, F, 3):                                  # (3 again: the same build twice)
        FI.build_feature_index(d, LAYER, batch_files=bf, overwrite=True)
        now = _bytes(d)
        assert now.keys() == first.keys()
        for k in first:
            if not k.endswith(".json"):
                assert now[k] == first[k], (bf, k)
    assert _bytes(d) == first                                # the metadata too, at the same batch size
    # three latent ranges or more
    one = st["posted"] * 8 + E.findex_workspace_bytes(3 * T, n)
    rep3 = FI.build_feature_index(d, LAYER, batch_files=3, device_budget_bytes=int(one / 2.6), overwrite=True)
    assert len(rep3.ranges) >= 3 and rep3.sweeps == 1 + len(rep3.ranges) and rep3.ranges[0][0] == 0 and rep3.ranges[-1][1] == n
    now = _bytes(d)
    assert all(now[k] == first[k] for k in first if not k.endswith(".json"))
    check_index_files(d, val, idx, n)
    # int32 indices and a subset
    d32 = str(tmp_path / "s32")
    write_store(d32, val, idx.astype(np.int32), n)
    rep32 = FI.build_feature_index(d32, LAYER, batch_files=2, subset_size=5)
    ix32, _ = check_index_files(d32, val[:5], idx[:5], n)
    assert rep32.n_files == 5 and len(ix32) == 5 and ix32.metadata["index_dtype"] == "int32"


def test_duplicate_index_fails_the_build(tmp_path):
    val, idx = pass_store(seed=22, F=3, T=40)
    idx[1, 17, 5] = idx[1, 17, 0]
    val[1, 17, 5] = val[1, 17, 0] = 2.0
    d = str(tmp_path / "s")
    write_store(d, val, idx, 50)
    before = sorted(os.listdir(d))
    with pytest.raises(ValueError, match="the store has duplicate indices in a row"):
        FI.build_feature_index(d, LAYER, batch_files=2)
    assert sorted(os.listdir(d)) == before


@pytest.mark.parametrize("kind", ["topk", "l1"])
def test_end_to_end_from_collect_features(tmp_path, kind):
    """collect_features on a tiny SAE, build_feature_index, then every latent's series against FeatureShards.series and
    top_activations against the reference rule applied to those series."""
    n, T, F, K = 256, 50, 6, 8
    g = np.random.default_rng(31)
    x = g.normal(0, 1, (F, T, 256)).astype(np.float32)
    sae = topk_model(n, K, seed=5) if kind == "topk" else l1_model(n, seed=8, bias=-1.2)
    path = shards(tmp_path / "data", x)
    out = str(tmp_path / "out")
    crep = CF.collect_features(sae, path, "enc", out, k=K, batch_files=4)
    if kind == "l1":
        assert crep.dropped > 0                                              # a K that drops latents
    rep = FI.build_feature_index(out, "enc", batch_files=4)
    fs, ix = CF.FeatureShards(out, "enc"), FI.FeatureIndex(out, "enc")
    assert rep.nnz == crep.stored and rep.nnz + rep.zero_slots == F * T * K and rep.out_of_range == 0
    lengths = np.array([50, 31, 50, 70, 3, 1])
    fired = 0
    for j in range(n):
        s = fs.series(j)
        assert np.array_equal(bits(ix.series(j)), bits(s))
        fired += bool(s.any())
        for absm, mn in ((False, None), (True, 0.05)):
            want, wmpf = R.top_activations_dense(s, fs.filenames, 4, None, mn, absm, lengths)
            got, mpf = ix.top_activations(j, 4, None, mn, absm, True, lengths)
            assert [(p[0], p[2], p[3]) for p in got] == [(p[0], p[2], p[3]) for p in want] and mpf == wmpf
            assert all(np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(got, want))
    assert fired > n // 4


def test_cli_build(tmp_path, capsys):
    import json
    val, idx = pass_store(seed=23, F=3, T=40)
    d = str(tmp_path / "s")
    write_store(d, val, idx, 50)
    FI.main(["build", "--data_path", d, "--layer_name", LAYER, "--batch_files", "2"])
    rep = json.loads(capsys.readouterr().out)
    _ix, st = check_index_files(d, val, idx, 50)
    assert rep["nnz"] == st["posted"] and rep["zero_slots"] == st["zero_slots"] and rep["sweeps"] == 2
    with pytest.raises(ValueError, match="already holds"):
        FI.main(["build", "--data_path", d, "--layer_name", LAYER])
