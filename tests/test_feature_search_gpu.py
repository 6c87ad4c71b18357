"""GPU: the feature search (freud_amd/feature_search.py over include/freud_sae.h's sae_search_*) against the reference's
top_activations (utils/activations.py:61-132).

* raw mode against the reference's own answers (tests/golden/search_raw.npz, make_search_golden.py), fp32 and fp16 shards;
* L1 and TopK latents, bit-exact against the reference loop transliterated here and applied to the engine's own encode() latents
  of every file, on the fused streaming epilogue (enough rows per batch) and on the stored-latent path (small batches, the last
  partial batch), T = 1500 and T = 50, trimmed lengths, filters, n_files above the file count;
* d = 1280, n = 40960: the fused keys equal an unfused path (sae_eval per file + a column max / argmax of the stored latent);
* the context after a search; the CLI.

L1 weights: every column has 256 (1024 at d >= 1024) entries of +-1/16 (+-1/32), so its norm is exactly 1 and the in-place
renormalisation every L1 forward starts with (l1autoencoder.py:71-73) is a bit-exact fixed point: the search and the
comparison encodes see the same weights however many forwards run in between."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import feature_search as FS
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "search_raw.npz")
pytestmark = pytest.mark.gpu


def ref_table(V, A, n_top, mn=None, mx=None):
    """The reference loop's answer for every latent: V, A = per-file max / first argmax [F, n] -> files, values, frames [n, n_top]."""
    F, n = V.shape
    ok = np.ones_like(V, dtype=bool)
    if mx is not None:
        ok &= V.astype(np.float64) <= mx
    if mn is not None:
        ok &= V.astype(np.float64) >= mn
    key = np.where(ok, -V.astype(np.float64), np.inf)
    order = np.argsort(key, axis=0, kind="stable")[:n_top]           # stable: equal values keep file order
    files = np.full((n, n_top), -1, np.int64)
    vals = np.full((n, n_top), np.nan, np.float32)
    frames = np.full((n, n_top), -1, np.int64)
    m = min(n_top, F)
    cols = np.arange(n)
    for r in range(m):
        f = order[r]
        good = ok[f, cols]
        files[good, r] = f[good]
        vals[good, r] = V[f[good], cols[good]]
        frames[good, r] = A[f[good], cols[good]]
    # the passing files come first in every column (key inf sorts last), so the rows above are dense
    return files, vals, frames


def per_file_max(series_list):
    V = np.stack([s.max(0).values.numpy() for s in series_list])
    A = np.stack([s.argmax(0).numpy() for s in series_list])
    return V, A


def check_atlas(atlas, files, vals, frames):
    np.testing.assert_array_equal(atlas.file_idx, files)
    np.testing.assert_array_equal(atlas.frames, frames)
    np.testing.assert_array_equal(atlas.values, vals)
    want_t = np.where(frames >= 0, frames * FS.TIMESTEP_S, np.nan)
    np.testing.assert_array_equal(atlas.times, want_t)


def l1_model(d, n, seed, max_rows=1500):
    g = np.random.default_rng(seed)
    nz, v = (1024, 1 / 32) if d >= 1024 else (256, 1 / 16)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:nz], j] = np.where(g.random(nz) < 0.5, -v, v)
    b = (g.normal(0, 0.3, n)).astype(np.float32)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=max_rows)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def shards(tmp_path, x, dtype=np.float32, name="enc", filenames=None):
    F, T, d = x.shape
    write_shards(str(tmp_path), name, x.reshape(F, T * d).astype(dtype), [T, d], filenames=filenames)
    return str(tmp_path)


def l1_series(sae, x, lengths):
    out = []
    for f in range(x.shape[0]):
        lat = sae.encode(torch.from_numpy(x[f]).cuda()).latent.float().cpu()
        out.append(lat[: lengths[f]])
    return out


def topk_series(sae, x, lengths):
    out = []
    for f in range(x.shape[0]):
        enc = sae.encode(torch.from_numpy(x[f]).cuda())
        dense = torch.zeros(x.shape[1], sae.n_dict_components, device="cuda")
        dense.scatter_(1, enc.top_indices, enc.top_acts.float())
        out.append(dense.cpu()[: lengths[f]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_raw_mode_matches_reference_golden(tmp_path, dtype):
    g = np.load(GOLD)
    x, L = g["x"], g["lengths"]
    path = shards(tmp_path, x, dtype, filenames=[str(f) for f in g["filenames"]])
    cases = {}
    for c in range(len(g["case_feature"])):
        key = (int(g["case_n_top"][c]), int(g["case_absolute"][c]), float(g["case_min_val"][c]), float(g["case_max_val"][c]))
        cases.setdefault(key, []).append(c)
    rng_before = torch.get_rng_state()
    for (n_top, absm, mn, mx), idx in cases.items():
        atlas = FS.search_features(None, path, "enc", n_top, absolute_magnitude=bool(absm),
                                   min_val=None if np.isnan(mn) else mn, max_val=None if np.isnan(mx) else mx,
                                   lengths=L, batch_files=3, max_per_file_features=range(x.shape[2]))
        for c in idx:
            j = int(g["case_feature"][c])
            want = [int(f) for f in g["case_files"][c] if f >= 0]
            m = len(want)
            ctx = f"n_top={n_top} abs={absm} min={mn} max={mx} feature={j}"
            assert atlas.file_idx[j, :m].tolist() == want and (atlas.file_idx[j, m:] == -1).all(), ctx
            assert atlas.values[j, :m].tolist() == [float(v) for v in g["case_values"][c][:m]], ctx
            assert atlas.times[j, :m].tolist() == [float(t) for t in g["case_times"][c][:m]], ctx
            assert atlas.max_per_file[j].tolist() == [float(v) for v in g["case_max_per_file"][c]], ctx
            assert [r[0] for r in atlas.top(j)] == [str(g["filenames"][f]) for f in want]
    assert torch.equal(torch.get_rng_state(), rng_before), "the search must leave the global torch RNG as it found it"


@pytest.mark.parametrize("T,F,batch,n", [(1500, 7, 6, 16384), (1500, 5, 1, 4096), (50, 200, 200, 16384), (50, 9, 4, 1024)])
def test_l1_bit_exact_against_reference_loop(tmp_path, T, F, batch, n):
    d = 256
    g = np.random.default_rng(T + F)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F).astype(np.int64)
    L[0] = T
    sae = l1_model(d, n, seed=F)
    path = shards(tmp_path, x)
    V, A = per_file_max(l1_series(sae, x, L))
    for n_top, mn, mx in [(5, None, None), (F + 3, 0.5, 2.5)]:
        atlas = FS.search_features(sae, path, "enc", n_top, lengths=L, batch_files=batch, min_val=mn, max_val=mx,
                                   max_per_file_features=[0, n - 1])
        check_atlas(atlas, *ref_table(V, A, n_top, mn, mx))
        np.testing.assert_array_equal(atlas.max_per_file, V[:, [0, n - 1]].T)
    # abs mode on a latent >= 0 is the plain mode
    atlas = FS.search_features(sae, path, "enc", 3, lengths=L, batch_files=batch, absolute_magnitude=True)
    check_atlas(atlas, *ref_table(V, A, 3))


@pytest.mark.parametrize("T,F,batch", [(1500, 5, 2), (50, 9, 9)])
def test_topk_bit_exact_against_reference_loop(tmp_path, T, F, batch):
    d, n, k = 256, 4096, 32
    torch.manual_seed(F)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k), max_rows=1500)
    g = np.random.default_rng(F)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F).astype(np.int64)
    path = shards(tmp_path, x)
    V, A = per_file_max(topk_series(sae, x, L))
    assert (V == 0).any(), "some latent never fires in some file: value 0 at frame 0"
    atlas = FS.search_features(sae, path, "enc", 4, lengths=L, batch_files=batch, max_per_file_features=[1, 7])
    check_atlas(atlas, *ref_table(V, A, 4))
    np.testing.assert_array_equal(atlas.max_per_file, V[:, [1, 7]].T)


def test_d384_search_equals_generic_encoder(tmp_path):
    """At d = 384 eval runs the fused forward; the search runs the generic encoder GEMM -- compared here against a force_generic
    context's encode()."""
    d, n, T, F = 384, 3072, 1500, 4
    sae = l1_model(d, n, seed=5)
    ref = l1_model(d, n, seed=5)
    ref._engine_kw["force_generic"] = True
    ref._eng.close()
    ref._eng = None
    ref._ensure(1500)
    ref.load_state_dict(sae.state_dict())
    g = np.random.default_rng(9)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = np.full(F, T)
    path = shards(tmp_path, x)
    V, A = per_file_max(l1_series(ref, x, L))
    atlas = FS.search_features(sae, path, "enc", 3, batch_files=4)
    check_atlas(atlas, *ref_table(V, A, 3))


def test_large_shape_fused_equals_unfused_and_is_deterministic():
    d, n, T, F = 1280, 40960, 1500, 16
    sae = l1_model(d, n, seed=11, max_rows=F * T)
    eng = sae._eng
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, T, d, generator=g).cuda()
    lens = torch.randint(1, T + 1, (F,), generator=g, dtype=torch.int32)
    lens[0] = T
    lens_dev = lens.cuda()
    k1 = torch.empty(F * n, dtype=torch.int64, device="cuda")
    k2 = torch.empty_like(k1)
    ku = torch.empty_like(k1)
    # the fused epilogue never writes the latent: a latent left by an eval of OTHER data must survive the two fused searches,
    # and only the stored-latent path overwrites it (so the comparison below is fused against unfused, not fallback against itself)
    sae.encode(torch.randn(F * T, d, generator=g).cuda())
    left = sae._latent_view(F * T)
    saved = left.clone()
    eng.search_files(x, k1, lens_dev)
    eng.search_files(x, k2, lens_dev)
    torch.cuda.synchronize()
    assert torch.equal(left, saved), "the latent buffer was written: the fused epilogue did not run"
    eng.search_files(x, ku, lens_dev, unfused=True)
    torch.cuda.synchronize()
    assert not torch.equal(left, saved), "the stored-latent path left the latent buffer alone"
    assert torch.equal(k1, k2), "two runs of the fused search differ"
    assert torch.equal(k1, ku), "fused and stored-latent search differ"
    # sae_eval per file + the key of a column max / argmax on the stored latent
    for f in range(F):
        lat = sae.encode(x[f]).latent[: int(lens[f])]
        v, a = lat.max(0).values.float(), lat.cpu().float().argmax(0)
        bits = v.cpu().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
        ordv = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits | 0x80000000)
        want = (ordv << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - a.numpy().astype(np.uint64))
        got = k1[f * n:(f + 1) * n].cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(got, want, err_msg=f"file {f}")


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_state_after_search(variant):
    d, n, T, F = 256, 1024, 50, 4
    if variant == "l1":
        sae = l1_model(d, n, seed=1)
    else:
        torch.manual_seed(1)
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=16), max_rows=1500)
    eng = sae._eng
    x = torch.randn(F, T, d).cuda()
    eng.eval(x.reshape(F * T, d))
    before = eng.get_params()
    step, m1, m2 = eng.get_opt_state()
    nfsf = eng.get_topk_state() if variant == "topk" else None
    keys = torch.empty(F * n, dtype=torch.int64, device="cuda")
    eng.search_files(x, keys)
    torch.cuda.synchronize()
    with pytest.raises(E.EngineError, match="feature search"):
        eng.latent_buffer()
    with pytest.raises(E.EngineError, match="feature search"):
        eng.latent_colmax()
    with pytest.raises(E.EngineError, match="feature search"):
        eng.metrics()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="feature search"):
            eng.topk_indices_tensor(F * T, "cuda")
        np.testing.assert_array_equal(eng.get_topk_state(), nfsf)
    for k, v in eng.get_params().items():
        np.testing.assert_array_equal(v, before[k])
    s2, n1, n2 = eng.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k], m1[k]) and np.array_equal(n2[k], m2[k]) for k in m1)
    # the next forward is unaffected: same latent as before the search
    first = (lambda o: o.latent) if variant == "l1" else (lambda o: o.top_acts)
    lat_a = first(sae.encode(x[0])).clone()
    eng.eval(x.reshape(F * T, d))
    lat_b = first(sae.encode(x[0]))
    assert torch.equal(lat_a, lat_b)
    eng.metrics()
    # bad shapes are rejected before anything is enqueued: the output keeps its sentinel
    big = torch.randn(40, 50, d).cuda()              # 2000 rows > max_rows
    keys2 = torch.full((40 * n,), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="max_rows"):
        eng.search_files(big, keys2)
    torch.cuda.synchronize()
    assert bool((keys2 == 7).all())
    with pytest.raises(E.EngineError, match="n_top"):
        E.search_merge(keys, None, F, n, 0, 0, 0, 0.0, 0.0, keys2, torch.zeros(40 * n, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert bool((keys2 == 7).all())


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    keys = torch.full((2 * 1024,), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.search_files(torch.randn(2, 100, 256).cuda(), keys)
    torch.cuda.synchronize()
    assert bool((keys == 7).all())
    eng.close()


def test_cli_matches_search_features(tmp_path):
    g = np.random.default_rng(2)
    x = g.normal(0, 1, (11, 30, 24)).astype(np.float32)
    data = tmp_path / "data"
    path = shards(data, x)
    L = g.integers(1, 40, 11)
    np.save(tmp_path / "len.npy", L)
    out = tmp_path / "atlas.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "freud_amd.feature_search", "--sae", "none", "--data_path", path, "--layer_name", "enc",
                    "--n_files", "4", "--absolute", "--min_val", "-1.5", "--lengths", str(tmp_path / "len.npy"), "--out", str(out)],
                   check=True, cwd=ROOT, env=env, timeout=300)
    got = np.load(out)
    want = FS.search_features(None, path, "enc", 4, absolute_magnitude=True, min_val=-1.5, lengths=L)
    for k in ("values", "file_idx", "frames", "times"):
        np.testing.assert_array_equal(got[k], getattr(want, k), err_msg=k)
    assert got["filenames"].tolist() == want.filenames
    # the reference's tuple shape through top_activations: (audio_file, series, value, time)
    pq, mpf = FS.top_activations(None, path, "enc", 3, 4, None, -1.5, True, True, lengths=L)
    assert [p[0] for p in pq] == [want.filenames[f] for f in want.file_idx[3] if f >= 0]
    for p, f in zip(pq, want.file_idx[3]):
        assert p[1].shape[0] == min(int(L[f]), 30) and torch.equal(p[1], torch.from_numpy(x[f, : p[1].shape[0], 3]))
    assert len(mpf) == 11


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_sae_search_against_reference_golden(tmp_path, kind):
    """The reference's own L1AutoEncoder / TopKAutoEncoder latents and its top_activations over them (search_{kind}.npz), against
    the search of the engine loaded with the recorded weights: per-file values within bf16 tolerance; files wherever a file's
    value is farther than twice the tolerance from every other candidate's (the topk_tiefree precedent), frames wherever the
    series maximum stands that far above the best other frame."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"search_{kind}.npz"))
    x, L, margin, flip = g["x"], g["lengths"], g["margin"], g["flip"]
    F, T, d = x.shape
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w_")}
    if kind == "l1":
        n = w["decoder.weight"].shape[1]
        sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n))
    else:
        n = w["W_dec"].shape[0]
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=int(g["k"])))
    sae.load_state_dict(w)
    path = shards(tmp_path, x, filenames=[str(f) for f in g["filenames"]])
    tol = lambda v: 0.03 + 0.01 * np.abs(v)                   # bf16 operands, K = 32: a few bf16 ulps of |x| |w| summed
    groups = {}
    for c in range(len(g["case_feature"])):
        groups.setdefault((int(g["case_n_top"][c]), int(g["case_absolute"][c]), float(g["case_min_val"][c]),
                           float(g["case_max_val"][c])), []).append(c)
    checked_files = checked_frames = 0
    for (n_top, absm, mn, mx), idx in groups.items():
        atlas = FS.search_features(sae, path, "enc", n_top, absolute_magnitude=bool(absm), min_val=None if np.isnan(mn) else mn,
                                   max_val=None if np.isnan(mx) else mx, lengths=L, batch_files=4, max_per_file_features=range(n))
        for c in idx:
            j = int(g["case_feature"][c])
            P = g["case_max_per_file"][c].astype(np.float64)
            ctx = f"{kind} n_top={n_top} abs={absm} min={mn} max={mx} latent={j}"
            # (TopK: where the k-th and (k+1)-th pre-activations of a kept frame are within bf16 rounding of each other, the
            # selection itself may differ -- those (file, latent) pairs are left out, and so is the order of their latent)
            stable = ~flip[:, j]
            assert np.all(np.abs(atlas.max_per_file[j] - P)[stable] <= tol(P)[stable]), ctx
            if not stable.all():
                continue
            ok = np.ones(F, bool)
            if not np.isnan(mn):
                ok &= P >= mn
            if not np.isnan(mx):
                ok &= P <= mx
            near = (not np.isnan(mn) and np.any(np.abs(P - mn) <= tol(P))) or (not np.isnan(mx) and np.any(np.abs(P - mx) <= tol(P)))
            want = [int(f) for f in g["case_files"][c] if f >= 0]
            if not near:
                assert int((atlas.file_idx[j] >= 0).sum()) == len(want), ctx
            R = np.abs(P)
            for r, f in enumerate(want):
                others = [h for h in range(F) if h != f and ok[h]]
                if near or any(abs(R[f] - R[h]) <= 2 * tol(R[f]) for h in others):
                    continue
                assert atlas.file_idx[j, r] == f, ctx
                assert abs(atlas.values[j, r] - g["case_values"][c][r]) <= tol(g["case_values"][c][r]), ctx
                checked_files += 1
                if margin[f, j] > 2 * tol(R[f]):
                    assert atlas.times[j, r] == g["case_times"][c][r], ctx
                    checked_frames += 1
    assert checked_files > 300 and checked_frames > 150 and flip.mean() < 0.5, (checked_files, checked_frames, flip.mean())


def test_cli_with_checkpoint_matches_search_features(tmp_path):
    """--sae CKPT end to end (init_sae_from_checkpoint, then the L1 search) against search_features in this process; the caller's
    RNG survives a search from a checkpoint path (the model is built with a random initialisation first)."""
    d, n, T, F = 256, 4096, 50, 12
    sae = l1_model(d, n, seed=3)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": d,
                            "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    g = np.random.default_rng(4)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path / "data", x)
    out = tmp_path / "atlas.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run([sys.executable, "-m", "freud_amd.feature_search", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                    "--n_files", "3", "--max_val", "2.0", "--batch_files", "5", "--out", str(out)], check=True, cwd=ROOT, env=env, timeout=300)
    got = np.load(out)
    rng = torch.get_rng_state()
    want = FS.search_features(str(ck), path, "enc", 3, max_val=2.0, batch_files=5)
    assert torch.equal(torch.get_rng_state(), rng)
    for k in ("values", "file_idx", "frames", "times"):
        np.testing.assert_array_equal(got[k], getattr(want, k), err_msg=k)
    assert (got["file_idx"][:, 0] >= 0).any()
