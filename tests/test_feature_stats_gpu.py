"""GPU: the feature statistics (freud_amd/feature_stats.py over include/freud_sae.h's sae_stats_files).

* L1 and TopK against the engine's own encode() latents of every file, reduced here in float64: counts, maxima, the L0
  histogram and the frame count equal, the sums within 1e-5; T = 1500 and T = 50, trimmed lengths, a last partial batch, the fused
  epilogue (enough rows per batch) and the stored-latent path (small batches, SAE_STATS_UNFUSED);
* d = 1280, n = 40960: fused against unfused, the invariants, two runs bitwise identical;
* TopK rows with fewer than k positive pre-activations, and a multi_topk model;
* the reference's own top_activations answers (tests/golden/search_{l1,topk}.npz): the top-1 value is act_max;
* the context afterwards; the CLI.

L1 weights: every column has 256 (1024 at d >= 1024) entries of +-1/16 (+-1/32), so its norm is exactly 1 and the in-place
renormalisation every L1 forward starts with is a bit-exact fixed point: every forward sees the same weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FIELDS = ("fire_count", "act_sum", "act_sq_sum", "act_max", "l0_hist")


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    nz, v = (1024, 1 / 32) if d >= 1024 else (256, 1 / 16)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:nz], j] = np.where(g.random(nz) < 0.5, -v, v)
    b = g.normal(0, 0.3, n).astype(np.float32)
    return W, b


def l1_model(d, n, seed, max_rows=1500):
    W, b = l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=max_rows)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def shards(path, x, dtype=np.float32):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(dtype), [T, d])
    return str(path)


def dense_latent(sae, xf):
    """encode() of one file as a dense float32 CUDA tensor [T, n] (TopK: the scatter of the selection)."""
    if isinstance(sae, L1AutoEncoder):
        return sae.encode(xf).latent.clone()
    enc = sae.encode(xf)
    dense = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda")
    dense.scatter_(1, enc.top_indices, enc.top_acts.float())
    return dense


def ref_stats(sae, x, lengths):
    n = sae.n_dict_components
    fire = torch.zeros(n, dtype=torch.int64, device="cuda")
    s = torch.zeros(n, dtype=torch.float64, device="cuda")
    q = torch.zeros_like(s)
    mx = torch.zeros(n, device="cuda")
    hist = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    frames = 0
    for f in range(x.shape[0]):
        lat = dense_latent(sae, torch.from_numpy(x[f]).cuda())[: int(lengths[f])]
        act = lat > 0
        fire += act.sum(0)
        s += lat.double().sum(0)
        q += (lat.double() ** 2).sum(0)
        mx = torch.maximum(mx, lat.max(0).values)
        hist += torch.bincount(act.sum(1), minlength=n + 1)
        frames += lat.shape[0]
    return FST.FeatureStats(frames, fire.cpu().numpy(), s.cpu().numpy(), q.cpu().numpy(), mx.cpu().numpy(), hist.cpu().numpy())


def check_invariants(st):
    assert st.l0_hist.sum() == st.n_frames
    assert (np.arange(st.l0_hist.shape[0]) * st.l0_hist).sum() == st.fire_count.sum()


def check_exact(got, want, ctx=""):
    assert got.n_frames == want.n_frames, ctx
    np.testing.assert_array_equal(got.fire_count, want.fire_count, err_msg=ctx)
    np.testing.assert_array_equal(got.act_max, want.act_max, err_msg=ctx)
    np.testing.assert_array_equal(got.l0_hist, want.l0_hist, err_msg=ctx)
    np.testing.assert_allclose(got.act_sum, want.act_sum, rtol=1e-5, atol=1e-30, err_msg=ctx)
    np.testing.assert_allclose(got.act_sq_sum, want.act_sq_sum, rtol=1e-5, atol=1e-30, err_msg=ctx)
    check_invariants(got)


def check_same(a, b, ctx=""):
    """Two paths of the same data: integers and maxima identical, sums to 1e-5."""
    assert a.n_frames == b.n_frames, ctx
    for k in ("fire_count", "act_max", "l0_hist"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{ctx} {k}")
    np.testing.assert_allclose(a.act_sum, b.act_sum, rtol=1e-5, err_msg=ctx)
    np.testing.assert_allclose(a.act_sq_sum, b.act_sq_sum, rtol=1e-5, err_msg=ctx)


def check_bitwise(a, b):
    assert a.n_frames == b.n_frames
    for k in FIELDS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F,batch,n,trim", [(1500, 7, 6, 16384, True), (50, 200, 200, 16384, False), (50, 9, 4, 1024, True)])
def test_l1_exact_against_encode(tmp_path, T, F, batch, n, trim):
    """(1500, 7, 6): a fused batch of 6 files, then a last partial batch of 1 (stored latent); (50, 200, 200): fused; (50, 9, 4):
    small batches.  Every case also runs with the stored-latent path forced."""
    d = 256
    g = np.random.default_rng(T + F)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F) if trim else np.full(F, T)
    L[0] = T
    sae = l1_model(d, n, seed=F)
    path = shards(tmp_path, x)
    want = ref_stats(sae, x, L)
    assert want.dead().any() or want.fire_count.min() < want.n_frames
    lens = L if trim else None
    fused = FST.feature_stats(sae, path, "enc", lengths=lens, batch_files=batch)
    check_exact(fused, want, "fused")
    unfused = FST.feature_stats(sae, path, "enc", lengths=lens, batch_files=batch, unfused=True)
    check_exact(unfused, want, "unfused")
    check_same(fused, unfused)
    check_bitwise(fused, FST.feature_stats(sae, path, "enc", lengths=lens, batch_files=batch))


def test_large_shape_fused_equals_unfused_and_is_deterministic():
    d, n, T, F = 1280, 40960, 1500, 4
    W, b = l1_weights(d, n, seed=11)
    eng = E.SaeEngine("l1", d, n, F * T + 256)
    eng.set_params({"decoder.weight": W, "encoder_bias": b})
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, T, d, generator=g).cuda()
    lens = torch.randint(1, T + 1, (F,), generator=g, dtype=torch.int32)
    lens[0] = T
    lens_dev = lens.cuda()
    nb = E.stats_layout(n)["bytes"]
    blocks = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(3)]
    # the fused epilogue never writes the latent: a latent left by an eval of other data survives it, and only the stored-latent
    # path overwrites it (so the comparison below is fused against unfused, not one path against itself)
    eng.eval(torch.randn(F * T, d, generator=g).cuda())
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (F * T, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    left = torch.as_tensor(_Alias(), device="cuda")
    saved = left.clone()
    eng.stats_files(x, blocks[0], lens_dev)
    eng.stats_files(x, blocks[1], lens_dev)
    torch.cuda.synchronize()
    assert torch.equal(left, saved), "the latent buffer was written: the fused epilogue did not run"
    eng.stats_files(x, blocks[2], lens_dev, unfused=True)
    torch.cuda.synchronize()
    assert not torch.equal(left, saved), "the stored-latent path left the latent buffer alone"
    st = [FST.FeatureStats.from_block(bl.cpu().numpy(), n) for bl in blocks]
    check_bitwise(st[0], st[1])
    check_same(st[0], st[2], "fused vs unfused")
    check_invariants(st[0])
    assert st[0].n_frames == int(lens.sum())
    eng.close()


def topk_model(d, n, k, seed, bias=None, multi=False):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi), max_rows=1500)
    if bias is not None:
        sd = sae.state_dict()
        sd["encoder.bias"] = torch.full((n,), float(bias))
        sae.load_state_dict(sd)
    return sae


@pytest.mark.parametrize("T,F,batch,trim", [(1500, 5, 2, True), (50, 9, 9, False)])
def test_topk_exact_against_encode(tmp_path, T, F, batch, trim):
    d, n, k = 256, 4096, 32
    sae = topk_model(d, n, k, seed=F, bias=-1.5)
    g = np.random.default_rng(F)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F) if trim else np.full(F, T)
    path = shards(tmp_path, x)
    # rows where fewer than k pre-activations are positive: their selection holds zeros, which do not count
    acts = sae.encode(torch.from_numpy(x[0]).cuda()).top_acts
    assert bool((acts == 0).any()) and bool((acts > 0).any())
    want = ref_stats(sae, x, L)
    assert want.l0_hist[:k].sum() > 0
    got = FST.feature_stats(sae, path, "enc", lengths=L if trim else None, batch_files=batch)
    check_exact(got, want)
    check_bitwise(got, FST.feature_stats(sae, path, "enc", lengths=L if trim else None, batch_files=batch))


def test_multi_topk_follows_encode(tmp_path):
    d, n, k, T, F = 256, 2048, 16, 300, 4
    sae = topk_model(d, n, k, seed=3, multi=True)
    x = np.random.default_rng(3).normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path, x)
    want = ref_stats(sae, x, np.full(F, T))
    got = FST.feature_stats(sae, path, "enc", batch_files=3)
    check_exact(got, want)
    assert got.l0_hist[k + 1:].sum() == 0, "the k selection of encode(), not the 4k one"


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_act_max_is_the_reference_top1(tmp_path, kind):
    """The reference's top_activations (search_{kind}.npz): for every case without filters and abs mode, its top-1 value is the
    latent's maximum over the trimmed data -- act_max, within the bf16 tolerance test_feature_search_gpu.py applies."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"search_{kind}.npz"))
    x, L, flip = g["x"], g["lengths"], g["flip"]
    d = x.shape[2]
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w_")}
    if kind == "l1":
        sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=w["decoder.weight"].shape[1]))
    else:
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=w["W_dec"].shape[0], k=int(g["k"])))
    sae.load_state_dict(w)
    st = FST.feature_stats(sae, shards(tmp_path, x), "enc", lengths=L, batch_files=4)
    check_invariants(st)
    assert st.n_frames == int(np.minimum(L, x.shape[1]).sum())
    tol = lambda v: 0.03 + 0.01 * abs(v)
    checked = 0
    for c in range(len(g["case_feature"])):
        if g["case_absolute"][c] or not np.isnan(g["case_min_val"][c]) or not np.isnan(g["case_max_val"][c]):
            continue
        j = int(g["case_feature"][c])
        if flip[:, j].any():            # (TopK: a selection that bf16 rounding may flip)
            continue
        top1 = float(g["case_values"][c][0])
        assert abs(float(st.act_max[j]) - top1) <= tol(top1), (kind, j, st.act_max[j], top1)
        checked += 1
    assert checked >= 10, checked


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_stats(variant):
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
    block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device="cuda")
    for eng in (a, b):
        eng.eval(x.reshape(F * T, d))
    a.stats_files(x, block)
    torch.cuda.synchronize()
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="statistics"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="statistics"):
            a.topk_indices_tensor(F * T, "cuda")
    # a following training step is bitwise the same step as in a context that never ran the statistics
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert a.metrics().tobytes() == b.metrics().tobytes()
    # bad shapes are rejected before anything is enqueued: the block keeps its sentinel
    sentinel = torch.full_like(block, 7)
    with pytest.raises(E.EngineError, match="max_rows"):
        a.stats_files(torch.randn(40, 50, d).cuda(), sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    block = torch.full((E.stats_layout(1024)["bytes"],), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.stats_files(torch.randn(2, 100, 256).cuda(), block)
    torch.cuda.synchronize()
    assert bool((block == 7).all())
    eng.close()


def test_cli_matches_feature_stats(tmp_path):
    d, n, T, F = 256, 2048, 50, 12
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
    out = tmp_path / "stats.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.feature_stats", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--lengths", str(tmp_path / "len.npy"), "--batch_files", "5", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    rng = torch.get_rng_state()
    want = FST.feature_stats(str(ck), path, "enc", lengths=L, batch_files=5)
    assert torch.equal(torch.get_rng_state(), rng)
    check_bitwise(FST.FeatureStats.from_npz(str(out)), want)
    assert summary["n_frames"] == want.n_frames == int(L.sum())
    assert summary["dead"] == int(want.dead().sum())
    assert summary["l0_mean"] == pytest.approx(want.l0_mean())
    assert summary["dense_over_10pct"] == int((want.frequency() > 0.1).sum())
