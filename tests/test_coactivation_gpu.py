"""GPU: the feature co-activation (freud_amd/coactivation.py over include/freud_sae.h's sae_coact_files / sae_coact_neighbor_keys).

The reference is the engine's own encode() per file: threshold at > 0, trim, Z^T Z in torch, summed over the files as int64 (the
product itself runs in float64 on the device, where 0/1 operands and sums below 2^53 are exact; torch has no int64 matmul there).
The full matrix must be EQUAL.  The neighbour tables must equal the numpy restatement (lexsort by score descending, count
descending, partner ascending; score = (num.astype(f8) / den.astype(f8)).astype(f4)) exactly, for all three measures.

L1 weights: the recipe of tests/test_feature_stats_gpu.py (unit-norm +-1/16 columns: the renormalisation is a fixed point) with the
bias centred at -1.5, so a latent fires on about 7 % of the frames and pairs both co-fire and never co-fire."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import coactivation as CO
from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    b = g.normal(-1.5, 0.3, n).astype(np.float32)
    return W, b


def l1_model(d, n, seed):
    W, b = l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_model(d, n, k, seed, bias=None, multi=False):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi), max_rows=1500)
    if bias is not None:
        sd = sae.state_dict()
        sd["encoder.bias"] = torch.full((n,), float(bias))
        sae.load_state_dict(sd)
    return sae


def shards(path, x):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(np.float32), [T, d])
    return str(path)


def dense_latent(sae, xf):
    if isinstance(sae, L1AutoEncoder):
        return sae.encode(xf).latent.clone()
    enc = sae.encode(xf)
    dense = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda")
    dense.scatter_(1, enc.top_indices, enc.top_acts.float())
    return dense


def ref_counts(sae, x, lengths):
    n = sae.n_dict_components
    C = torch.zeros(n, n, dtype=torch.int64, device="cuda")
    for f in range(x.shape[0]):
        Z = (dense_latent(sae, torch.from_numpy(x[f]).cuda())[: int(lengths[f])] > 0).double()
        C += (Z.T @ Z).to(torch.int64)
    return C.cpu().numpy()


def np_scores(C, measure):
    n = C.shape[0]
    C = C.astype(np.int64)
    dii = np.diag(C)
    if measure == "jaccard":
        den = dii[:, None] + dii[None, :] - C
    elif measure == "cond":
        den = np.broadcast_to(dii[:, None], (n, n))
    else:
        den = np.ones((n, n), np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (C.astype("f8") / den.astype("f8")).astype("f4")


def np_neighbors(C, measure, K):
    n = C.shape[0]
    S = np_scores(C, measure)
    nb = np.full((n, K), -1, np.int64)
    cn = np.zeros((n, K), np.int64)
    sc = np.full((n, K), np.nan, np.float32)
    for i in range(n):
        j = np.flatnonzero((C[i] > 0) & (np.arange(n) != i))
        order = j[np.lexsort((j, -C[i, j].astype(np.int64), -S[i, j].astype(np.float64)))][:K]
        m = len(order)
        nb[i, :m], cn[i, :m], sc[i, :m] = order, C[i, order], S[i, order]
    return nb, cn, sc


def check_preconditions(C):
    """Both zero and non-zero off-diagonal counts, and at least one tied score."""
    n = C.shape[0]
    off = ~np.eye(n, dtype=bool)
    assert (C[off] == 0).any() and (C[off] > 0).any()
    S = np_scores(C, "jaccard")
    live = off & (C > 0)
    assert any(len(np.unique(S[i][live[i]])) < live[i].sum() for i in range(n)), "no tied scores"


def check_tables(co, C, measure, K):
    nb, cn, sc = np_neighbors(C, measure, K)
    np.testing.assert_array_equal(co.neighbors, nb)
    np.testing.assert_array_equal(co.counts, cn)
    assert co.scores.dtype == np.float32 and co.scores.tobytes() == sc.tobytes()
    assert co.neighbors.dtype == np.int64 and co.counts.dtype == np.int64


def check_against_stats(co, st):
    C = co.matrix.astype(np.int64)
    np.testing.assert_array_equal(np.diag(C), st.fire_count)
    np.testing.assert_array_equal(co.fire_count, st.fire_count)
    np.testing.assert_array_equal(C, C.T)
    assert C.sum() == (np.arange(st.l0_hist.shape[0], dtype=np.int64) ** 2 * st.l0_hist).sum()
    assert co.n_frames == st.n_frames


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l1_small(tmp_path_factory):
    """d = 256, n = 300 (no multiple of any tile; three 128-wide tile rows: diagonal, off-diagonal and mirrored tiles), T = 50,
    F = 7 in batches of 3: three calls, the last one partial, 150 rows per call (no multiple of the K step), trimmed lengths."""
    d, n, T, F = 256, 300, 50, 7
    g = np.random.default_rng(7)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = T
    sae = l1_model(d, n, seed=5)
    path = shards(tmp_path_factory.mktemp("l1small"), x)
    C = ref_counts(sae, x, L)
    return sae, path, L, C


def test_l1_small_matrix_is_exact(l1_small):
    sae, path, L, C = l1_small
    check_preconditions(C)
    co = CO.feature_coactivation(sae, path, "enc", lengths=L, batch_files=3, return_counts=True)
    assert co.matrix.dtype == np.int32 and co.matrix.shape == C.shape
    np.testing.assert_array_equal(co.matrix.astype(np.int64), C)
    assert co.n_frames == int(L.sum())
    check_against_stats(co, FST.feature_stats(sae, path, "enc", lengths=L, batch_files=3))
    again = CO.feature_coactivation(sae, path, "enc", lengths=L, batch_files=3, return_counts=True)
    for k in ("matrix", "neighbors", "counts", "scores", "fire_count"):
        assert getattr(co, k).tobytes() == getattr(again, k).tobytes(), k


@pytest.mark.parametrize("measure", ["jaccard", "cond", "count"])
@pytest.mark.parametrize("K", [1, 16, 320])
def test_neighbor_tables_equal_numpy(l1_small, measure, K):
    """K = 320 > n - 1 leaves empty slots in every row."""
    sae, path, L, C = l1_small
    co = CO.feature_coactivation(sae, path, "enc", n_neighbors=K, measure=measure, lengths=L, batch_files=3)
    assert co.matrix is None
    check_tables(co, C, measure, K)
    if K > C.shape[0] - 1:
        assert (co.neighbors[:, -1] == -1).all() and (co.counts[:, -1] == 0).all() and np.isnan(co.scores[:, -1]).all()
    j = int(np.argmax((co.neighbors >= 0).sum(1)))
    assert co.top(j) == [(int(p), int(c), float(s)) for p, c, s in zip(co.neighbors[j], co.counts[j], co.scores[j]) if p >= 0]


def test_neighbor_selection_in_row_blocks_with_a_partial_last_one(l1_small, monkeypatch):
    """The key buffer of 128 rows: blocks of 128, 128 and 44 rows of n = 300 (n = 40 960 ends on a 10-row block of its 819)."""
    sae, path, L, C = l1_small
    n = C.shape[0]
    monkeypatch.setattr(CO, "KEY_BLOCK", 128 * n)
    assert n % (CO.KEY_BLOCK // n) not in (0, n)
    co = CO.feature_coactivation(sae, path, "enc", n_neighbors=16, measure="jaccard", lengths=L, batch_files=3)
    check_tables(co, C, "jaccard", 16)


def test_l1_long_files(tmp_path):
    d, n, T, F = 256, 1024, 1500, 3
    g = np.random.default_rng(11)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = T
    sae = l1_model(d, n, seed=2)
    path = shards(tmp_path, x)
    C = ref_counts(sae, x, L)
    check_preconditions(C)
    co = CO.feature_coactivation(sae, path, "enc", lengths=L, batch_files=2, return_counts=True)
    np.testing.assert_array_equal(co.matrix.astype(np.int64), C)
    check_tables(co, C, "jaccard", 16)
    check_against_stats(co, FST.feature_stats(sae, path, "enc", lengths=L, batch_files=2))
    # without lengths every frame counts
    full = CO.feature_coactivation(sae, path, "enc", batch_files=2, return_counts=True)
    np.testing.assert_array_equal(full.matrix.astype(np.int64), ref_counts(sae, x, np.full(F, T)))
    assert full.n_frames == F * T


def test_topk_exact_against_encode(tmp_path):
    d, n, k, T, F = 256, 4096, 32, 50, 9
    sae = topk_model(d, n, k, seed=9, bias=-1.5)
    g = np.random.default_rng(9)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = T
    path = shards(tmp_path, x)
    # rows with fewer than k positive pre-activations: their selection holds zeros, which are not active
    acts = sae.encode(torch.from_numpy(x[0]).cuda()).top_acts
    assert bool((acts == 0).any()) and bool((acts > 0).any())
    C = ref_counts(sae, x, L)
    check_preconditions(C)
    co = CO.feature_coactivation(sae, path, "enc", lengths=L, batch_files=4, return_counts=True)
    np.testing.assert_array_equal(co.matrix.astype(np.int64), C)
    check_tables(co, C, "jaccard", 16)
    st = FST.feature_stats(sae, path, "enc", lengths=L, batch_files=4)
    assert st.l0_hist[:k].sum() > 0
    check_against_stats(co, st)


def test_multi_topk_follows_encode(tmp_path):
    d, n, k, T, F = 256, 2048, 16, 300, 4
    sae = topk_model(d, n, k, seed=3, multi=True)
    x = np.random.default_rng(3).normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path, x)
    C = ref_counts(sae, x, np.full(F, T))
    co = CO.feature_coactivation(sae, path, "enc", batch_files=3, return_counts=True, measure="cond")
    np.testing.assert_array_equal(co.matrix.astype(np.int64), C)
    check_tables(co, C, "cond", 16)
    assert C.sum() <= F * T * k * k, "the k selection of encode(), not the 4k one"


def test_larger_shape_on_the_device_twice():
    """d = 256, n = 16 384, 4 x 1500 frames in one call, the table kept on the device: equal to the float64 product of the stored
    latent's mask, two runs bitwise identical, the keys of a row block as the host formula gives them."""
    d, n, T, F = 256, 16384, 1500, 4
    W, b = l1_weights(d, n, seed=13)
    eng = E.SaeEngine("l1", d, n, F * T + 144)
    eng.set_params({"decoder.weight": W, "encoder_bias": b})
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, T, d, generator=g).cuda()
    lens = torch.randint(1, T + 1, (F,), generator=g, dtype=torch.int32)
    lens[0] = T
    lens_dev = lens.cuda()
    tables = [torch.zeros(n, n, dtype=torch.int32, device="cuda") for _ in range(2)]
    for t in tables:
        eng.coact_files(x, t, lens_dev)
    torch.cuda.synchronize()
    assert torch.equal(tables[0], tables[1])
    eng.eval(x.reshape(F * T, d))
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (F * T, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    lat = torch.as_tensor(_Alias(), device="cuda")[:, :n].view(torch.bfloat16)
    keep = (torch.arange(T)[None, :] < lens[:, None]).reshape(F * T).cuda()
    Z = ((lat > 0) & keep[:, None]).double()
    want = (Z.T @ Z).to(torch.int32)
    del Z
    assert torch.equal(tables[0], want)
    assert bool((want == 0).any()) and int(want.max()) > 1
    # the neighbour tables of the device table, against numpy on a few rows
    nb, cn, sc = CO.neighbor_tables(tables[0], n, 16, "jaccard")
    Ch = want.cpu().numpy()
    rows = [0, 1, 127, 128, 8191, n - 1]
    S = np_scores(Ch, "jaccard")
    for i in rows:
        j = np.flatnonzero((Ch[i] > 0) & (np.arange(n) != i))
        order = j[np.lexsort((j, -Ch[i, j].astype(np.int64), -S[i, j].astype(np.float64)))][:16]
        m = len(order)
        assert nb[i, :m].tolist() == order.tolist() and (nb[i, m:] == -1).all(), i
        assert cn[i, :m].tolist() == Ch[i, order].tolist() and sc[i, :m].tobytes() == S[i, order].tobytes(), i
    eng.close()


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_coactivation(variant):
    d, n, T, F = 256, 1024, 50, 4

    def make():
        if variant == "l1":
            W, b = l1_weights(d, n, seed=1)
            eng = E.SaeEngine("l1", d, n, 1500, recon_alpha=1e2)
            eng.set_params({"decoder.weight": W, "encoder_bias": b})
        else:
            torch.manual_seed(1)
            eng = E.SaeEngine("topk", d, n, 1500, k=16, optimizer="adam")
            g = torch.Generator().manual_seed(1)
            We = torch.randn(n, d, generator=g) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32),
                            "W_dec": We.numpy().copy(), "b_dec": np.zeros(d, np.float32)})
        return eng

    a, b = make(), make()
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(2)).cuda()
    table = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    for eng in (a, b):
        eng.eval(x.reshape(F * T, d))
    a.coact_files(x, table)
    torch.cuda.synchronize()
    assert int(table.sum()) > 0 and torch.equal(table, table.T)
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="co-activation"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="co-activation"):
            a.topk_indices_tensor(F * T, "cuda")
    # a following training step is bitwise the same step as in a context that never ran the pass
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert a.metrics().tobytes() == b.metrics().tobytes()
    # bad shapes are rejected before anything is enqueued: the table keeps its sentinel
    sentinel = torch.full_like(table, 7)
    with pytest.raises(E.EngineError, match="max_rows"):
        a.coact_files(torch.randn(40, 50, d).cuda(), sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    table = torch.full((1024, 1024), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.coact_files(torch.randn(2, 100, 256).cuda(), table)
    torch.cuda.synchronize()
    assert bool((table == 7).all())
    eng.close()


def test_neighbor_keys_arguments():
    n = 64
    table = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    keys = torch.full((n * n,), 7, dtype=torch.int64, device="cuda")
    for row0, rows, measure in ((0, 0, 0), (-1, 4, 0), (60, 5, 0), (0, 4, 3), (0, 4, -1)):
        with pytest.raises(E.EngineError):
            E.coact_neighbor_keys(table, n, row0, rows, measure, keys)
    torch.cuda.synchronize()
    assert bool((keys == 7).all())


def test_cli_matches_the_function(tmp_path):
    d, n, T, F = 256, 512, 50, 12
    sae = l1_model(d, n, seed=3)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": d,
                            "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    g = np.random.default_rng(4)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path / "data", x)
    L = g.integers(1, T + 1, F)
    np.save(tmp_path / "len.npy", L)
    out = tmp_path / "coact.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.coactivation", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--lengths", str(tmp_path / "len.npy"), "--batch_files", "5", "--n_neighbors", "8", "--measure", "cond",
                        "--counts", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    rng = torch.get_rng_state()
    want = CO.feature_coactivation(str(ck), path, "enc", n_neighbors=8, measure="cond", lengths=L, batch_files=5, return_counts=True)
    assert torch.equal(torch.get_rng_state(), rng)
    got = CO.CoActivation.from_npz(str(out))
    for k in ("fire_count", "neighbors", "counts", "scores", "matrix"):
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
    assert got.n_frames == want.n_frames == int(L.sum()) == summary["n_frames"]
    assert got.measure == "cond" == summary["measure"]
    assert summary["dead"] == int((want.fire_count == 0).sum()) and summary["n_neighbors"] == 8
    assert summary["pairs_reported"] == int((want.neighbors >= 0).sum())
