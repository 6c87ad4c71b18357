"""GPU: feature collection (freud_amd/collect_features.py over include/freud_sae.h's sae_collect_files).

The oracle everywhere is the stable argsort of encode()'s own latent (TopK: the scatter of its selection): indices exactly equal,
values bit-equal (+0.0 padding), the statistics equal to a numpy count.  bf16 latents tie constantly, which is what exercises the
rule.

L1 weights: d = 256 and every entry of a column is +-1/16, so a column's norm is exactly 1 and the in-place renormalisation every
L1 forward starts with is a bit-exact fixed point: every forward sees the same weights.

Internal thresholds: the L1 kernel (freud_amd/csrc/collect.h, collect_l1_kernel) has no threshold on n_p or K -- one workgroup
size, one load form, no register-resident variant.  Its only second path is chosen per ROW by the data: a row with more than K
active latents takes the threshold search.  Both sides of that (nnz == K and nnz == K + 1 included, wherever they occur) are in
test_l1_fast_path_and_mix; the dense case is test_l1_dense_overflow_and_maximum_k.  The TopK kernel has one path."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import collect_features as CF
from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
D = 256


def l1_weights(n, seed):
    g = np.random.default_rng(seed)
    return np.where(g.random((D, n)) < 0.5, np.float32(-1 / 16), np.float32(1 / 16)).astype(np.float32)


def l1_model(n, seed, bias):
    sae = L1AutoEncoder(D, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    b = np.broadcast_to(np.asarray(bias, np.float32), (n,)).copy()
    sae.load_state_dict({"decoder.weight": torch.from_numpy(l1_weights(n, seed)), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_model(n, k, seed, bias=None, multi_topk=False):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(D, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi_topk), max_rows=1500)
    if bias is not None:
        sd = sae.state_dict()
        sd["encoder.bias"] = torch.full((n,), float(bias))
        sae.load_state_dict(sd)
    return sae


def shards(path, x, dtype=np.float32):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(dtype), [T, d])
    return str(path)


def latent_bits(sae, x):
    """encode() of every file of x (a numpy array or a CUDA tensor [F, T, d]) as bf16 bit patterns, uint16 [F, T, n]."""
    out = []
    for f in range(x.shape[0]):
        xf = x[f] if torch.is_tensor(x) else torch.from_numpy(x[f]).cuda()
        if isinstance(sae, L1AutoEncoder):
            lat = sae.encode(xf).latent.float()
        else:
            enc = sae.encode(xf)
            lat = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda")
            lat.scatter_(1, enc.top_indices, enc.top_acts.float())
        b16 = lat.to(torch.bfloat16)
        assert torch.equal(b16.float(), lat)                 # the latent IS bf16: nothing rounds here
        out.append(b16.view(torch.int16).cpu().numpy().view(np.uint16))
    return np.stack(out)


def oracle(bits, K):
    """(indices int64 [F, T, K], value bits uint32 [F, T, K], stats int64 [8], nnz [F, T]) by numpy."""
    a = (bits.astype(np.uint32) << 16).view(np.float32)
    active = (bits >= 1) & (bits <= 0x7FFF)
    assert (a[~active] == 0).all()                           # post-ReLU / a selection: nothing negative but -0.0
    idx = np.argsort(-a, axis=-1, kind="stable")[..., :K]
    val = np.take_along_axis(a, idx, -1).copy()
    val[val == 0] = 0.0
    nnz = active.sum(-1)
    stored = np.minimum(nnz, K)
    srt = -np.sort(-np.where(active, bits, 0).astype(np.int64), axis=-1)
    cut = srt[..., K] if K < bits.shape[-1] else np.zeros_like(nnz)
    stats = np.array([nnz.size, stored.sum(), (nnz - stored).sum(), (nnz > K).sum(), nnz.max(), cut.max(), 0, 0], np.int64)
    return idx.astype(np.int64), val.view(np.uint32), stats, nnz


def run_collect(sae, x, K, batch, index_dtype=torch.int64):
    """The engine call over x [F, T, d] (numpy or CUDA tensor) in batches of `batch` files -> (values, indices, stats) on the host."""
    F, T, _ = x.shape
    eng = sae._ensure(batch * T)
    vals = torch.full((F, T, K), -7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((F, T, K), -7, dtype=index_dtype, device="cuda")
    stats = torch.zeros(8, dtype=torch.int64, device="cuda")
    for f0 in range(0, F, batch):
        xb = x[f0:f0 + batch] if torch.is_tensor(x) else torch.from_numpy(x[f0:f0 + batch]).cuda()
        eng.collect_files(xb.contiguous(), K, vals[f0:f0 + batch], idx[f0:f0 + batch], stats)
    torch.cuda.synchronize()
    return vals.cpu().numpy(), idx.cpu().numpy(), stats.cpu().numpy()


def check(sae, x, K, batch, index_dtype=torch.int64):
    bits = latent_bits(sae, x)
    widx, wval, wstats, nnz = oracle(bits, K)
    vals, idx, stats = run_collect(sae, x, K, batch, index_dtype)
    print(f"K={K} nnz min/median/max = {nnz.min()}/{int(np.median(nnz))}/{nnz.max()}  stats = {stats.tolist()}")
    np.testing.assert_array_equal(idx.astype(np.int64), widx)
    np.testing.assert_array_equal(vals.view(np.uint32), wval)
    np.testing.assert_array_equal(stats, wstats)
    return bits, nnz, (vals, idx, stats)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 32, 100])
def test_l1_fast_path_and_mix(K):
    """n = 1000 (padded columns), 9 files of T = 50 in batches of 4 (200 and 50 rows: a ragged last batch, no multiple of 128).
    K columns carry a bias of 1/256 and the others -2.3: a near-silent file fires exactly those K, ordinary files about K / 2 + 10,
    a loud file well over 100 -- rows with fewer than K, exactly K and more than K active latents."""
    n, T, F = 1000, 50, 9
    g = np.random.default_rng(K)
    bias = np.full(n, -2.3, np.float32)
    bias[g.permutation(n)[:K]] = 1 / 256
    x = g.normal(0, 1, (F, T, D)).astype(np.float32)
    x *= np.array([1, 1, 1e-4, 1, 2.5, 1, 1, 0.5, 1], np.float32)[:, None, None]
    sae = l1_model(n, seed=K, bias=bias)
    _, nnz, _ = check(sae, x, K, batch=4)
    assert (nnz == K).any() and (nnz > K).any() and (K == 1 or (nnz < K).any())
    assert (nnz[2] == K).all()


@pytest.mark.parametrize("bias", [0.0, -2.5])
def test_l1_dense_overflow_and_maximum_k(bias):
    """n = 4352 (17 blocks of 256), K = 1024, 40 files of T = 8.  Zero bias: every row drops about half its latents; a strongly
    negative bias: few positives and long padding."""
    n, T, F, K = 4352, 8, 40, 1024
    g = np.random.default_rng(11)
    x = g.normal(0, 1, (F, T, D)).astype(np.float32)
    sae = l1_model(n, seed=3, bias=bias)
    _, nnz, (_, _, stats) = check(sae, x, K, batch=16)
    if bias == 0.0:
        assert (nnz > K).all() and stats[2] > F * T * 800 and stats[5] > 0
    else:
        assert (nnz < 200).all() and stats[2] == 0 and stats[5] == 0


def test_l1_whole_row():
    n, T, F = 256, 50, 3
    x = np.random.default_rng(2).normal(0, 1, (F, T, D)).astype(np.float32)
    sae = l1_model(n, seed=4, bias=0.0)
    _, _, (_, idx, stats) = check(sae, x, 256, batch=2)
    assert stats[2] == 0 and (np.sort(idx, axis=-1) == np.arange(n)).all()          # the whole row, sorted: a permutation


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_l1_index_width(index_dtype):
    """n = 66 048: only columns above 65 535 can fire, so every stored active index must exceed 65 535."""
    n, T, F, K = 66048, 8, 2, 32
    bias = np.full(n, -100.0, np.float32)
    bias[65536:] = -1.0
    x = np.random.default_rng(6).normal(0, 1, (F, T, D)).astype(np.float32)
    sae = l1_model(n, seed=5, bias=bias)
    _, nnz, (vals, idx, _) = check(sae, x, K, batch=2, index_dtype=index_dtype)
    assert (nnz > K).any() and (vals > 0).any()
    assert (idx[vals > 0] > 65535).all() and (idx[vals == 0] < K).all()


@pytest.mark.parametrize("bias,K,multi", [(None, 32, False), (None, 8, False), (-1.5, 32, False), (-1.5, 8, False), (None, 32, True),
                                          (-1.5, 8, True)])
def test_topk(bias, K, multi):
    """k = 32.  Zero bias: every row has at least k positives; a bias of -1.5 leaves a handful per row, so the selection holds the
    engine's zeros (lowest columns) -- they come out behind the positives, in column order, as +0.0.  multi_topk: its k selection."""
    n, k, T, F = 1000, 32, 50, 9
    x = np.random.default_rng(8).normal(0, 1, (F, T, D)).astype(np.float32)
    sae = topk_model(n, k, seed=2, bias=bias, multi_topk=multi)
    bits, nnz, (vals, idx, stats) = check(sae, x, K, batch=4)
    if bias is None:
        assert (nnz == k).all() and stats[2] == F * T * (k - K)
    else:
        assert (nnz < k).all() and (nnz > 0).any() and (vals == 0).any()


def test_statistics_against_feature_stats(tmp_path):
    n, T, F, K = 1000, 50, 9, 32
    g = np.random.default_rng(9)
    x = g.normal(0, 1, (F, T, D)).astype(np.float32)
    sae = l1_model(n, seed=7, bias=-1.85)
    path = shards(tmp_path / "data", x)
    st = FST.feature_stats(sae, path, "enc", batch_files=4)
    rep = CF.collect_features(sae, path, "enc", str(tmp_path / "out"), k=K, batch_files=4)
    assert rep.rows == F * T and rep.stored + rep.dropped == int(st.fire_count.sum())
    assert rep.max_active == int(np.flatnonzero(st.l0_hist).max())
    assert rep.rows_dropped == int(st.l0_hist[K + 1:].sum()) and 0 < rep.rows_dropped < F * T
    assert not rep.complete and rep.largest_dropped > 0


def _bytes(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_pass_end_to_end(tmp_path):
    """The files as documented (int64 and int32), fp16 shards, subset_size, layout="tensor", determinism over runs and batch sizes,
    the CLI in a fresh process.  (Shards on disk are fp32 or fp16; a bf16 batch reaches the engine only as a tensor:
    test_bf16_input.)"""
    n, T, F, K = 1000, 50, 9, 32
    g = np.random.default_rng(10)
    x = g.normal(0, 1, (F, T, D)).astype(np.float32)
    sae = l1_model(n, seed=8, bias=-1.85)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": D, "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    path = shards(tmp_path / "data", x)
    bits = latent_bits(sae, x)
    widx, wval, wstats, _ = oracle(bits, K)
    rng = torch.get_rng_state()
    rep = CF.collect_features(sae, path, "enc", str(tmp_path / "a"), k=K, batch_files=4)
    assert torch.equal(torch.get_rng_state(), rng)
    v, i = np.load(tmp_path / "a" / "enc_activation_values.npy"), np.load(tmp_path / "a" / "enc_feature_indices.npy")
    assert v.dtype == np.float32 and i.dtype == np.int64 and v.shape == i.shape == (F, T * K)
    np.testing.assert_array_equal(i.reshape(F, T, K), widx)
    np.testing.assert_array_equal(v.view(np.uint32).reshape(F, T, K), wval)
    meta = json.load(open(tmp_path / "a" / "enc_metadata.json"))
    assert meta["tensor_shape"] == [T, K] and meta["activation_shape"] == [T, n] and len(meta["filenames"]) == F
    assert [meta["freud_amd"]["stats"][s] for s in CF.STAT_NAMES] == wstats.tolist() and meta["freud_amd"]["variant"] == "l1"
    assert [rep.rows, rep.stored, rep.dropped, rep.rows_dropped, rep.max_active] == wstats[:5].tolist()
    assert rep.bytes_written == sum(len(b) for b in _bytes(tmp_path / "a").values())
    fs = CF.FeatureShards(str(tmp_path / "a"), "enc")
    a = (bits.astype(np.uint32) << 16).view(np.float32)
    j = int(np.argmax((bits[0] > 0).sum(0)))
    top = np.sort(a, axis=-1)[..., -K]                              # a latent's value is stored wherever it is above the row's K-th
    np.testing.assert_array_equal(fs.series(j)[a[..., j] > top], a[..., j][a[..., j] > top])
    # two runs and two batch sizes: the same bytes
    CF.collect_features(sae, path, "enc", str(tmp_path / "b"), k=K, batch_files=4)
    CF.collect_features(sae, path, "enc", str(tmp_path / "c"), k=K, batch_files=9)
    assert _bytes(tmp_path / "a") == _bytes(tmp_path / "b") == _bytes(tmp_path / "c")
    # int32 indices, a subset
    CF.collect_features(sae, path, "enc", str(tmp_path / "i32"), k=K, index_dtype="int32", subset_size=5, batch_files=2)
    i32 = np.load(tmp_path / "i32" / "enc_feature_indices.npy")
    assert i32.dtype == np.int32 and i32.shape == (5, T * K)
    np.testing.assert_array_equal(i32.reshape(5, T, K), widx[:5])
    np.testing.assert_array_equal(np.load(tmp_path / "i32" / "enc_activation_values.npy"), v[:5])
    # fp16 shards
    x16 = x.astype(np.float16)
    p16 = shards(tmp_path / "data16", x16, np.float16)
    CF.collect_features(sae, p16, "enc", str(tmp_path / "h"), k=K, batch_files=4)
    hidx, hval, _, _ = oracle(latent_bits(sae, torch.from_numpy(x16).cuda()), K)
    np.testing.assert_array_equal(np.load(tmp_path / "h" / "enc_feature_indices.npy").reshape(F, T, K), hidx)
    np.testing.assert_array_equal(np.load(tmp_path / "h" / "enc_activation_values.npy").view(np.uint32).reshape(F, T, K), hval)
    # the dense form equals encode() to the bit
    rt = CF.collect_features(sae, path, "enc", str(tmp_path / "t"), layout="tensor", batch_files=4)
    dense = np.load(tmp_path / "t" / "enc_tensors.npy")
    assert dense.dtype == np.float32 and dense.shape == (F, T * n) and set(rt.paths) == {"tensors", "metadata"}
    np.testing.assert_array_equal(dense.view(np.uint32).reshape(F, T, n), a.view(np.uint32))
    assert json.load(open(tmp_path / "t" / "enc_metadata.json"))["tensor_shape"] == [T, n]
    with pytest.raises(ValueError, match="prefers it"):
        CF.collect_features(sae, path, "enc", str(tmp_path / "t"), k=K, overwrite=True)
    # argument rules that need the model
    with pytest.raises(ValueError, match="l0_hist"):
        CF.collect_features(sae, path, "enc", str(tmp_path / "z"))
    with pytest.raises(ValueError, match="min"):
        CF.collect_features(sae, path, "enc", str(tmp_path / "z"), k=1001)
    assert not (tmp_path / "z").exists()
    # the CLI in a fresh process, with the reference's config keys
    cfg = {"whisper_model": "tiny", "sae_model": str(ck), "layer_name": "enc", "batch_size": 4, "data_path": path, "device": "cuda",
           "out_folder": str(tmp_path / "cli"), "dl_max_workers": 0, "collect_max": None}
    with open(tmp_path / "cfg.json", "w") as f:
        json.dump(cfg, f)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.collect_features", "--config", str(tmp_path / "cfg.json"), "--k", str(K)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["rows"] == F * T and out["dropped"] == rep.dropped and out["K"] == K and out["complete"] is False
    cli, ref = _bytes(tmp_path / "cli"), _bytes(tmp_path / "a")
    assert cli["enc_activation_values.npy"] == ref["enc_activation_values.npy"] and cli["enc_feature_indices.npy"] == ref["enc_feature_indices.npy"]


def test_topk_pass_defaults_to_the_models_k(tmp_path):
    n, k, T, F = 1000, 32, 50, 5
    x = np.random.default_rng(12).normal(0, 1, (F, T, D)).astype(np.float32)
    sae = topk_model(n, k, seed=3)
    path = shards(tmp_path / "data", x)
    rep = CF.collect_features(sae, path, "enc", str(tmp_path / "o"), batch_files=2)
    assert rep.K == k and rep.complete and rep.variant == "topk"
    widx, wval, _, _ = oracle(latent_bits(sae, x), k)
    fs = CF.FeatureShards(str(tmp_path / "o"), "enc")
    np.testing.assert_array_equal(np.asarray(fs.indices).reshape(F, T, k), widx)
    np.testing.assert_array_equal(np.asarray(fs.values).view(np.uint32).reshape(F, T, k), wval)
    with pytest.raises(ValueError, match="model's k"):
        CF.collect_features(sae, path, "enc", str(tmp_path / "p"), k=k + 1)
    with pytest.raises(ValueError, match="dense L1 form"):
        CF.collect_features(sae, path, "enc", str(tmp_path / "p"), layout="tensor")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bf16_and_fp16_input(dtype):
    n, T, F, K = 1000, 50, 3, 32
    x = torch.randn(F, T, D, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    sae = l1_model(n, seed=9, bias=-1.85)
    check(sae, x, K, batch=2)


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_collection(variant):
    n, T, F, K = 1024, 50, 4, 16

    def make():
        if variant == "l1":
            eng = E.SaeEngine("l1", D, n, 1500, recon_alpha=1e2)
            eng.set_params({"decoder.weight": l1_weights(n, 1), "encoder_bias": np.full(n, -1.0, np.float32)})
        else:
            eng = E.SaeEngine("topk", D, n, 1500, k=16, optimizer="adam")
            We = torch.randn(n, D, generator=torch.Generator().manual_seed(1)) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32),
                            "W_dec": We.numpy().copy(), "b_dec": np.zeros(D, np.float32)})
        return eng

    a, b = make(), make()
    x = torch.randn(F, T, D, generator=torch.Generator().manual_seed(2)).cuda()
    for eng in (a, b):
        if variant == "topk":                               # moments and num_frames_since_fired are set.  (L1: a step would leave
            eng.step(x.reshape(F * T, D), 1e-3)             # columns off unit norm, and EVERY L1 forward renormalises them in place)
        eng.eval(x.reshape(F * T, D))
    before = a.get_params()
    step, m1, m2 = a.get_opt_state()
    fired = a.get_topk_state().copy() if variant == "topk" else None
    vals = torch.empty(F, T, K, device="cuda")
    idx = torch.empty(F, T, K, dtype=torch.int64, device="cuda")
    stats = torch.zeros(8, dtype=torch.int64, device="cuda")
    a.collect_files(x, K, vals, idx, stats)
    torch.cuda.synchronize()
    assert int(stats[0]) == F * T and int(stats[6]) == 0 and int(stats[7]) == 0
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(), lambda: a.multi_topk_buffers(F * T, "cuda"),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, D, device="cuda"))):
        with pytest.raises(E.EngineError, match="feature collection"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="feature collection"):
            a.topk_indices_tensor(F * T, "cuda")
        assert np.array_equal(a.get_topk_state(), fired)
    for k, v in a.get_params().items():
        assert v.tobytes() == before[k].tobytes(), k
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k], m1[k]) and np.array_equal(n2[k], m2[k]) for k in m1)
    a.eval(x.reshape(F * T, D))                             # the getters are back after the next forward
    a.latent_buffer()
    for eng in (a, b):                                      # the next training step is the step of a context that never collected
        eng.step(x.reshape(F * T, D), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k

    # every argument error: SAE_ERR_INVALID, and stats still zero -- nothing was enqueued
    lib, vp = a._lib, C.c_void_p
    z = torch.zeros(8 + 1, dtype=torch.int64, device="cuda")
    sv, si = torch.full_like(vals, 7), torch.full_like(idx, 7)
    INVALID = -1                                           # include/freud_sae.h: SAE_ERR_INVALID

    def raw(xp=x.data_ptr(), n_files=F, rows=T, dt=E.DTYPE["float32"], K=K, flags=0, v=sv.data_ptr(), i=si.data_ptr(), s=z.data_ptr()):
        return lib.sae_collect_files(a._ctx, vp(xp), n_files, rows, dt, K, flags, vp(v), vp(i), vp(s), vp(torch.cuda.current_stream().cuda_stream))

    k_max = 16 if variant == "topk" else n
    for bad in (dict(K=0), dict(K=-1), dict(K=k_max + 1), dict(K=E.COLLECT_MAX_K + 1), dict(flags=2), dict(flags=-1), dict(xp=None), dict(v=None),
                dict(i=None), dict(s=None), dict(s=z.data_ptr() + 4), dict(n_files=0), dict(rows=0), dict(n_files=40), dict(dt=99)):
        assert raw(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((z == 0).all()) and bool((sv == 7).all()) and bool((si == 7).all())
    assert raw() == 0 and raw(flags=E.COLLECT_IDX32) == 0
    torch.cuda.synchronize()
    assert int(z[0]) == 2 * F * T
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", D, 1024, 512, precision="fp8")
    stats = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.collect_files(torch.randn(2, 100, D).cuda(), 8, torch.empty(2, 100, 8, device="cuda"),
                          torch.empty(2, 100, 8, dtype=torch.int64, device="cuda"), stats)
    torch.cuda.synchronize()
    assert bool((stats == 0).all())
    eng.close()
