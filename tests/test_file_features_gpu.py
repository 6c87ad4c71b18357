"""GPU: the file features (freud_amd/file_features.py over include/freud_sae.h's sae_file_top_features) -- the reference's
top_activations_for_audio (utils/activations.py:135-209) for every file of a shard directory.

* the select kernel alone through the C ABI on synthetic keys against numpy.lexsort: column counts around the wave size, several
  blocks' worth and the largest dictionary (163 840), 1 / 3 / 33 files, n_top from 1 to the maximum; key populations all distinct,
  five distinct values (latent order decides at the threshold), all equal, none positive, exactly n_top - 1 positive; run twice,
  bitwise equal;
* raw mode against the reference's own answers (tests/golden/file_features_raw.npz), fp32 and fp16 shards, a partial last batch;
* L1 and TopK bit-exact against the restated rule (value descending, first frame ascending, latent ascending, positive only)
  applied to the engine's own encode() latents, on the fused streaming epilogue and on the stored-latent path, trimmed lengths;
* top_activations_for_file against file_features and encode(); the RNG, the context after a pass, the CLI.

L1 weights as in test_feature_search_gpu.py: every column has 256 entries of +-1/16, so its norm is exactly 1 and the in-place
renormalisation every L1 forward starts with is a bit-exact fixed point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import file_features as FF
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "file_features_raw.npz")
pytestmark = pytest.mark.gpu

ZERO = np.uint64(0x80000000)          # ord(0.0): the high half of a zero-valued key


# ---------------------------------------------------------------------------------------------------------------------------
def lexsort_select(keys, n_top, flags):
    """keys [F, ncols] uint64 -> latents int32 [F, n_top] (-1), keys uint64 [F, n_top] (0): numpy's answer."""
    F, ncols = keys.shape
    lat = np.full((F, n_top), -1, np.int32)
    out = np.zeros((F, n_top), np.uint64)
    cols = np.arange(ncols)
    for f in range(F):
        ok = keys[f] != 0
        if flags & E.FILE_TOP_POSITIVE:
            ok &= (keys[f] >> np.uint64(32)) > ZERO
        c = cols[ok]
        order = c[np.lexsort((c, ~keys[f][ok]))][:n_top]        # key descending, then latent ascending
        lat[f, : len(order)] = order
        out[f, : len(order)] = keys[f][order]
    return lat, out


def positive_keys(g, shape):
    hi = g.integers(0x80000001, 0xFF800000, shape, dtype=np.uint64)
    return (hi << np.uint64(32)) | g.integers(0, 1 << 32, shape, dtype=np.uint64)


def nonpositive_keys(g, shape):
    """zero-valued keys (frame 0 and later frames) and negative values"""
    hi = np.where(g.random(shape) < 0.5, ZERO, g.integers(0x00800000, 0x80000000, shape, dtype=np.uint64)).astype(np.uint64)
    return (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - g.integers(0, 1500, shape, dtype=np.uint64))


def populations(g, F, ncols, n_top):
    shape = (F, ncols)
    mixed = np.where(g.random(shape) < 0.5, positive_keys(g, shape), nonpositive_keys(g, shape))
    mixed[:, :: 7] = positive_keys(g, shape)[:, :: 7]
    yield "distinct, signed, no flag", mixed, 0
    yield "distinct, positive", positive_keys(g, shape), E.FILE_TOP_POSITIVE
    five = np.concatenate([positive_keys(g, (4,)), nonpositive_keys(g, (1,))])
    yield "five values", five[g.integers(0, 5, shape)], E.FILE_TOP_POSITIVE
    yield "five values, no flag", five[g.integers(0, 5, shape)], 0
    yield "all equal", np.full(shape, positive_keys(g, (1,))[0]), E.FILE_TOP_POSITIVE
    yield "none positive", nonpositive_keys(g, shape), E.FILE_TOP_POSITIVE
    few = nonpositive_keys(g, shape)
    m = min(n_top - 1, ncols)
    for f in range(F):
        few[f, g.permutation(ncols)[:m]] = positive_keys(g, (m,))
    yield "n_top - 1 positive", few, E.FILE_TOP_POSITIVE


def run_select(keys, n_top, flags):
    F, ncols = keys.shape
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    lat = torch.full((F, n_top), 7, dtype=torch.int32, device="cuda")
    out = torch.full((F, n_top), 7, dtype=torch.int64, device="cuda")
    E.file_top_features(kd, F, ncols, n_top, flags, lat, out)
    torch.cuda.synchronize()
    return lat.cpu().numpy(), out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("ncols,n_files,n_top", [(1, 1, 1), (1, 3, 7), (63, 3, 7), (64, 3, 64), (65, 33, 7), (65, 1, 1024),
                                                 (1000, 33, 64), (1000, 3, 1024), (4096, 1, 1), (4096, 3, 1024),
                                                 (163840, 1, 7), (163840, 3, 1024), (163840, 33, 64)])
def test_select_kernel_against_lexsort(ncols, n_files, n_top):
    g = np.random.default_rng(ncols * 131 + n_files * 17 + n_top)
    for name, keys, flags in populations(g, n_files, ncols, n_top):
        keys = np.ascontiguousarray(keys, np.uint64)
        want_lat, want_keys = lexsort_select(keys, n_top, flags)
        lat, out = run_select(keys, n_top, flags)
        np.testing.assert_array_equal(lat, want_lat, err_msg=name)
        np.testing.assert_array_equal(out, want_keys, err_msg=name)
        lat2, out2 = run_select(keys, n_top, flags)
        assert lat.tobytes() == lat2.tobytes() and out.tobytes() == out2.tobytes(), f"{name}: two runs differ"
        if name == "none positive":
            assert (lat == -1).all() and (out == 0).all()
        if name == "n_top - 1 positive":
            m = min(n_top - 1, ncols)
            assert ((lat >= 0).sum(1) == m).all()


def test_select_argument_checks_enqueue_nothing():
    keys = torch.zeros(4 * 10, dtype=torch.int64, device="cuda")
    lat = torch.full((4, 3), 7, dtype=torch.int32, device="cuda")
    out = torch.full((4, 3), 7, dtype=torch.int64, device="cuda")
    big = torch.full((E.FILE_TOP_MAX + 1,), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="n_top"):
        E.file_top_features(keys, 1, 10, 0, 0, lat, out)
    with pytest.raises(E.EngineError, match="n_top"):
        E.file_top_features(keys, 1, 10, E.FILE_TOP_MAX + 1, 0, big.to(torch.int32), big)
    with pytest.raises(E.EngineError, match="flags"):
        E.file_top_features(keys, 4, 10, 3, 2, lat, out)
    lib = E.load()
    assert lib.sae_file_top_features(None, 4, 10, 3, 0, lat.data_ptr(), out.data_ptr(), None) != 0
    assert lib.sae_file_top_features(keys.data_ptr(), 0, 10, 3, 0, lat.data_ptr(), out.data_ptr(), None) != 0
    assert lib.sae_file_top_features(keys.data_ptr(), 4, 0, 3, 0, lat.data_ptr(), out.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((lat == 7).all()) and bool((out == 7).all())


# ---------------------------------------------------------------------------------------------------------------------------
def shards(tmp_path, x, dtype=np.float32, name="enc", filenames=None):
    F, T, d = x.shape
    write_shards(str(tmp_path), name, x.reshape(F, T * d).astype(dtype), [T, d], filenames=filenames)
    return str(tmp_path)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_raw_mode_matches_reference_golden(tmp_path, dtype):
    g = np.load(GOLD)
    x, L = g["x"], g["lengths"]
    names = [str(f) for f in g["filenames"]]
    path = shards(tmp_path, x, dtype, filenames=names)
    rng_before = torch.get_rng_state()
    for n_top in sorted(set(g["case_top_n"].tolist())):
        ff = FF.file_features(None, path, "enc", n_top, lengths=L, batch_files=4)      # 6 files: the last batch is partial
        assert ff.latents.shape == (x.shape[0], n_top) and ff.filenames == names
        for c in np.nonzero(g["case_top_n"] == n_top)[0]:
            f = int(g["case_file"][c])
            want = [int(i) for i in g["case_idx"][c] if i >= 0]
            m = len(want)
            ctx = f"file {f} top_n={n_top}"
            assert ff.latents[f, :m].tolist() == want and (ff.latents[f, m:] == -1).all(), ctx
            assert ff.values[f, :m].tolist() == [float(v) for v in g["case_values"][c][:m]] and np.isnan(ff.values[f, m:]).all(), ctx
            assert ff.frames[f, :m].tolist() == [int(t) for t in g["case_frames"][c][:m]] and (ff.frames[f, m:] == -1).all(), ctx
            assert ff.times[f, :m].tolist() == [int(t) * FF.TIMESTEP_S for t in g["case_frames"][c][:m]] and np.isnan(ff.times[f, m:]).all(), ctx
            assert [r[0] for r in ff.top(names[f])] == want
    assert torch.equal(torch.get_rng_state(), rng_before), "the pass must leave the global torch RNG as it found it"


# ---------------------------------------------------------------------------------------------------------------------------
def l1_model(d, n, seed, max_rows=1500):
    g = np.random.default_rng(seed)
    nz, v = 256, 1 / 16
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:nz], j] = np.where(g.random(nz) < 0.5, -v, v)
    b = (g.normal(0, 0.3, n) - 3.0).astype(np.float32)        # sparse (about 0.2 % of a frame's latents are positive): short files
    #                                                            have fewer positive latents than 64 slots
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=max_rows)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def dense_latent(sae, xf):
    """encode() of one file [T, d] (CUDA) as a dense fp32 [T, n] on the device."""
    enc = sae.encode(xf)
    if hasattr(enc, "latent"):
        return enc.latent.float()
    dense = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda")
    dense.scatter_(1, enc.top_indices, enc.top_acts.float())
    return dense


def per_file_max(sae, x, lengths):
    """V, A [F, n]: the maximum of every latent's trimmed series and its FIRST frame (no reliance on argmax's tie order)."""
    V, A = [], []
    for f in range(x.shape[0]):
        lat = dense_latent(sae, torch.from_numpy(x[f]).cuda())[: int(lengths[f])]
        v = lat.max(0).values
        rows = torch.arange(lat.shape[0], device="cuda")[:, None].expand_as(lat)
        a = torch.where(lat == v[None], rows, lat.shape[0]).min(0).values
        V.append(v.cpu().numpy())
        A.append(a.cpu().numpy())
    return np.stack(V), np.stack(A)


def restated(V, A, n_top):
    """The issue's restatement of the reference on per-file maxima: value descending, first frame ascending, latent ascending;
    only values > 0."""
    F, n = V.shape
    lat = np.full((F, n_top), -1, np.int64)
    val = np.full((F, n_top), np.nan, np.float32)
    fr = np.full((F, n_top), -1, np.int64)
    cols = np.arange(n)
    for f in range(F):
        c = cols[V[f] > 0]
        order = c[np.lexsort((c, A[f][c], -V[f][c].astype(np.float64)))][:n_top]
        m = len(order)
        lat[f, :m], val[f, :m], fr[f, :m] = order, V[f][order], A[f][order]
    return lat, val, fr


def check(ff, lat, val, fr):
    np.testing.assert_array_equal(ff.latents, lat)
    np.testing.assert_array_equal(ff.frames, fr)
    np.testing.assert_array_equal(ff.values, val)
    np.testing.assert_array_equal(ff.times, np.where(fr >= 0, fr * FF.TIMESTEP_S, np.nan))


@pytest.mark.parametrize("T,F,batch,n", [(1500, 7, 6, 16384), (50, 9, 4, 1024)])
def test_l1_bit_exact_against_restated_rule(tmp_path, T, F, batch, n):
    d = 256
    g = np.random.default_rng(T + F)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F).astype(np.int64)
    L[0], L[1] = T, 1
    sae = l1_model(d, n, seed=F)
    path = shards(tmp_path, x)
    V, A = per_file_max(sae, x, L)
    assert ((V > 0).sum(1) < 64).any() and ((V > 0).sum(1) > 64).any(), "files with fewer and with more positive latents than slots"
    for n_top in (1, 64):
        ff = FF.file_features(sae, path, "enc", n_top, lengths=L, batch_files=batch)
        check(ff, *restated(V, A, n_top))


@pytest.fixture(scope="module")
def topk_model():
    torch.manual_seed(9)
    return TopKAutoEncoder(256, TopKAutoEncoderConfig(n_dict_components=4096, k=8), max_rows=1500)


@pytest.mark.parametrize("T,n_tops", [(50, (1, 64)), (3, (1024,))])
def test_topk_bit_exact_against_restated_rule(tmp_path, topk_model, T, n_tops):
    F, d = 9, 256
    g = np.random.default_rng(T)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F).astype(np.int64)
    L[0] = T
    path = shards(tmp_path, x)
    V, A = per_file_max(topk_model, x, L)
    for n_top in n_tops:
        ff = FF.file_features(topk_model, path, "enc", n_top, lengths=L, batch_files=4)
        check(ff, *restated(V, A, n_top))
        if T == 3:
            got = (ff.latents >= 0).sum(1)
            assert got.max() <= 24 and (ff.latents[:, 24:] == -1).all() and got.min() >= 1


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l1", "topk", "raw"])
def test_top_activations_for_file(tmp_path, topk_model, kind):
    T, F, d = 50, 5, 256
    g = np.random.default_rng(3)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = np.array([50, 17, 1, 33, 70])
    sae = {"l1": lambda: l1_model(d, 1024, seed=2), "topk": lambda: topk_model, "raw": lambda: None}[kind]()
    path = shards(tmp_path, x)
    top_n = 12
    rng_before = torch.get_rng_state()
    ff = FF.file_features(sae, path, "enc", top_n, lengths=L, batch_files=2)
    for f in range(F):
        idx, series = FF.top_activations_for_file(sae, x[f], top_n, length=int(L[f]))
        Lf = min(int(L[f]), T)
        assert idx == [int(j) for j in ff.latents[f] if j >= 0] and len(series) == len(idx)
        full = torch.from_numpy(x[f]) if sae is None else dense_latent(sae, torch.from_numpy(x[f]).cuda()).cpu()
        for r, (j, s) in enumerate(zip(idx, series)):
            assert s.dtype == torch.float32 and s.device.type == "cpu" and s.shape == (Lf,)
            assert torch.equal(s, full[:Lf, j])
            assert float(s.max()) == float(ff.values[f, r]) and int(s.argmax()) == int(ff.frames[f, r])
    assert torch.equal(torch.get_rng_state(), rng_before)


def test_context_state_after_a_pass(tmp_path):
    d, n, T, F = 256, 1024, 50, 4
    sae = l1_model(d, n, seed=1)
    eng = sae._ensure(1500)
    x = np.random.default_rng(0).normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path, x)
    xd = torch.from_numpy(x).cuda()
    eng.eval(xd.reshape(F * T, d))
    before = eng.get_params()
    lat_a = sae.encode(xd[0]).latent.clone()
    FF.file_features(sae, path, "enc", 5)
    for getter in (eng.latent_buffer, eng.latent_colmax, eng.metrics):
        with pytest.raises(E.EngineError, match="feature search"):
            getter()
    for k, v in eng.get_params().items():
        np.testing.assert_array_equal(v, before[k])
    assert torch.equal(sae.encode(xd[0]).latent, lat_a)
    eng.metrics()


def test_cli_writes_a_loadable_file(tmp_path):
    g = np.random.default_rng(2)
    x = g.normal(0, 1, (11, 30, 24)).astype(np.float32)
    path = shards(tmp_path / "data", x)
    L = g.integers(1, 40, 11)
    np.save(tmp_path / "len.npy", L)
    out = tmp_path / "ff.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.file_features", "--sae", "none", "--data_path", path, "--layer_name", "enc",
                        "--n_top", "30", "--lengths", str(tmp_path / "len.npy"), "--batch_files", "4", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert len(r.stdout.strip().splitlines()) == 1 and "11 files x top 30" in r.stdout
    got = FF.FileFeatures.from_npz(str(out))
    want = FF.file_features(None, path, "enc", 30, lengths=L)
    for k in ("latents", "values", "frames", "times"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
    assert got.filenames == want.filenames and (got.latents[:, :24] >= 0).all() and (got.latents[:, 24:] == -1).all()
