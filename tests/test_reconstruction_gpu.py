"""GPU: the reconstruction report (freud_amd/reconstruction.py over include/freud_sae.h's sae_recon_files; freud_amd/csrc/recon.h).

1. the residual: L1 to the bit against x - decode(encode(x).latent) on counted rows and 0 elsewhere (float32 and float16 shards,
   padded and ragged shapes); TopK against the float64 decode of the selection within (k + 2) 2^-24 (|b_dec| + sum |a| |w|) plus the
   one fp32 subtraction;
2. every sum against the float64 reference of tests/reconstruction_reference.py within its bounds -- the 256-tile and the 128-tile
   GEMM (force_gemm128, odd tile counts), many tiles (n = 16384), a last partial batch, TopK with rows of fewer than k positives, a
   multi_topk model -- each L1 case also with SAE_RECON_UNFUSED, and the two against each other;
3. act_sq_sum and n_frames against feature_stats of the same data; fvu() against the float64 formula;
4. the report predicts a real ablation: manipulate_features(scale 0) of four latents against ablation();
5. d = 1280, n = 40960: two runs bitwise identical; batch_files 4 against 9;
6. the context afterwards, the refusals; 7. the CLI.

Which GEMM kernel ran the L1 attribution is read from the engine's brackets: recon_attr_stream (gemm256s.h) or recon_attr (the tile
forms); the two n = 16384 cases have the 2048 tiles of 256 x 256 the streaming form needs, the others do not.

L1 weights: columns of exactly unit norm (256 entries of +-1/16; 1024 of +-1/32 at d >= 1024; 64 of +-1/8 below d = 256), so the
in-place renormalisation every L1 forward starts with is a bit-exact fixed point: every forward sees the same weights."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd import reconstruction as RC
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.manipulate import manipulate_features
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder
from tests import reconstruction_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24


def bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    nz, v = (1024, 1 / 32) if d >= 1024 else (256, 1 / 16) if d >= 256 else (64, 1 / 8)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:nz], j] = np.where(g.random(nz) < 0.5, -v, v)
    return W, g.normal(0, 0.3, n).astype(np.float32)


def l1_model(d, n, seed, **engine_kw):
    W, b = l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    if engine_kw:                                   # (re-created with the same parameters by the next _ensure that needs more rows)
        sae._engine_kw.update(engine_kw)
        sae._ensure(sae._max_rows + 1)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_model(d, n, k, seed, bias=None, multi=False, hot=()):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi), max_rows=1500)
    sd = sae.state_dict()
    sd["b_dec"] = 0.05 * torch.randn(d)
    if bias is not None:
        sd["encoder.bias"] = torch.full((n,), float(bias))
    for j in hot:
        sd["encoder.bias"][j] = 1.2
    sae.load_state_dict(sd)
    return sae


def is_l1(sae):
    return isinstance(sae, L1AutoEncoder)


def dense_latent(sae, xf):
    """encode() as a dense float32 CUDA tensor [..., n] (TopK: the scatter of the selection)."""
    if is_l1(sae):
        return sae.encode(xf).latent.clone()
    enc = sae.encode(xf)
    return torch.zeros(*xf.shape[:-1], sae.n_dict_components, device="cuda").scatter_(-1, enc.top_indices, enc.top_acts.float())


def operand(sae):
    """The bf16 decoder operand [n][d] of the engine's CURRENT weights."""
    p = sae._eng.get_params()
    return R.bf16(np.ascontiguousarray(p["decoder.weight"].T) if is_l1(sae) else p["W_dec"])


def make_data(F, T, d, seed, trim, dtype=np.float32, spread=False):
    """N(0, 1) frames and trimmed lengths.  spread: every frame scaled by a factor in [0.9, 1.7] and the lengths cut by at most 8 --
    for the few frames of the small TopK case: the bias of -1.5 leaves about 19 positive pre-activations per unit-scale frame (fewer
    than k = 32) and about 150 at 1.7, so some rows are short AND 400 frames still fire over 90 % of 4096 latents."""
    g = np.random.default_rng(seed)
    x = g.normal(0, 1, (F, T, d))
    if spread:
        x = x * g.uniform(0.9, 1.7, (F, T, 1))
    x = x.astype(dtype)                              # (float16: the shard values ARE the data)
    L = (g.integers(T - 8, T, F) if spread else g.integers(1, T, F)) if trim else np.full(F, T)
    L[0] = T
    return x, L


def run_report(sae, x, L, batch, unfused=False, want_resid=True):
    """The pass through SaeEngine.recon_files in batches of files, as reconstruction_report walks them -> (report, resid [F][T][d])."""
    F, T, d = x.shape
    eng = sae._ensure(-(-min(batch, F) * T // 256) * 256)
    n = eng.n
    block = torch.zeros(E.recon_layout(n, d)["bytes"], dtype=torch.uint8, device="cuda")
    file_out = torch.zeros(F, 2, dtype=torch.float64, device="cuda")
    resid = torch.full((F, T, d), float("nan"), device="cuda") if want_resid else None
    lens = torch.from_numpy(np.asarray(L, np.int32)).cuda() if L is not None else None
    for f0 in range(0, F, batch):
        f1 = min(f0 + batch, F)
        eng.recon_files(torch.from_numpy(x[f0:f1]).cuda(), block, file_out[f0:f1], lens[f0:f1] if lens is not None else None,
                        resid=resid[f0:f1] if want_resid else None, unfused=unfused)
    torch.cuda.synchronize()
    return RC.ReconstructionReport.from_block(block.cpu().numpy(), n, d, file_out.cpu().numpy()), resid


def make_reference(sae, x, resid, L, most_fire=True):
    ref = R.reference(x, resid, lambda f: dense_latent(sae, torch.from_numpy(x[f]).cuda()), operand(sae), L,
                      "l1" if is_l1(sae) else "topk", device="cuda")
    assert not most_fire or ref.fired.mean() >= 0.9, ref.fired.mean()
    assert ref.n_frames < x.shape[0] * x.shape[1] or (np.asarray(L) == x.shape[1]).all()
    return ref


def check_l1_residual(sae, x, L, batch, resid):
    F, T, d = x.shape
    for f0 in range(0, F, batch):
        f1 = min(f0 + batch, F)
        xb = torch.from_numpy(x[f0:f1]).cuda()
        want = xb.float() - sae.decode(sae.encode(xb).latent)
        counted = (torch.arange(T, device="cuda")[None, :] < torch.from_numpy(np.asarray(L[f0:f1])).cuda()[:, None])
        got = resid[f0:f1]
        assert np.array_equal(bits(got[counted]), bits(want[counted])), (f0, "counted rows")
        assert bool((got[~counted] == 0).all()) and not bool(torch.signbit(got[~counted]).any()), (f0, "rows that do not count")
        assert float(want[counted].abs().max()) > 0


# ---- 1 + 2, L1
L1_CASES = {
    # name: (d, n, T, F, batch, dtype, engine keywords, batches that stream)
    "f32_256_1024": (256, 1024, 50, 9, 4, np.float32, {}, 0),
    "f16_256_1024": (256, 1024, 50, 9, 4, np.float16, {}, 0),
    "ragged_200_300": (200, 300, 77, 3, 2, np.float32, {}, 0),
    "gemm128_500_1000": (500, 1000, 50, 5, 3, np.float32, {"force_gemm128": True}, 0),
    "many_tiles_16384": (256, 16384, 50, 200, 200, np.float32, {}, 1),        # 40 x 64 = 2560 tiles
    "partial_batch_16384": (256, 16384, 1500, 7, 6, np.float32, {}, 1),       # 36 x 64 tiles, then one file alone on the tile form
}


def attr_launches(sae, fn):
    """(streaming, tile) launches of the attribution GEMM during fn(), from the engine's brackets."""
    eng = sae._eng
    eng.profile(2)
    eng.kernel_times()
    out = fn()
    kt = eng.kernel_times()
    eng.profile(0)
    return out, kt.get("recon_attr_stream", (0.0, 0))[1], kt.get("recon_attr", (0.0, 0))[1]


@pytest.mark.parametrize("name", sorted(L1_CASES))
def test_l1_residual_and_sums(name):
    d, n, T, F, batch, dtype, kw, streams = L1_CASES[name]
    n_batches = -(-F // batch)
    sae = l1_model(d, n, seed=F, **kw)
    x, L = make_data(F, T, d, seed=T + F, trim=True, dtype=dtype)
    rep, resid = run_report(sae, x, L, batch)
    check_l1_residual(sae, x, L, batch, resid)
    ref = make_reference(sae, x, resid, L)
    assert ref.n_frames == int(L.sum()) < F * T
    R.check_report(rep, ref, f"{name} fused")
    (unf, resid_u), s_launches, t_launches = attr_launches(sae, lambda: run_report(sae, x, L, batch, unfused=True))
    assert (s_launches, t_launches) == (0, n_batches), "SAE_RECON_UNFUSED keeps the attribution on the tile forms"
    assert torch.equal(resid.view(torch.int32), resid_u.view(torch.int32))
    R.check_report(unf, ref, f"{name} unfused")
    R.check_same(rep, unf, ref, f"{name} fused vs unfused")
    # without resid_dev the sums are the same to the bit; and the streaming kernel ran exactly where its conditions hold
    again, s_launches, t_launches = attr_launches(sae, lambda: run_report(sae, x, L, batch, want_resid=False)[0])
    R.check_bitwise(rep, again)
    assert (s_launches, t_launches) == (streams, n_batches - streams)


# ---- 1 + 2, TopK
def check_topk_residual(sae, x, L, resid, k):
    F, T, d = x.shape
    p = sae._eng.get_params()
    Wd, bd = R.bf16(p["W_dec"]).astype(np.float64), p["b_dec"].astype(np.float64)
    saw_short_row = False
    for f in range(F):
        enc = sae.encode(torch.from_numpy(x[f]).cuda())
        idx, acts = enc.top_indices.cpu().numpy(), enc.top_acts.cpu().numpy().astype(np.float64)
        saw_short_row |= bool((acts == 0).any())
        rows = Wd[idx]                                                     # [T, k, d]
        want = bd + (acts[:, :, None] * rows).sum(1)
        bound = (k + 2) * U24 * (np.abs(bd) + (np.abs(acts)[:, :, None] * np.abs(rows)).sum(1))
        rw = x[f].astype(np.float64) - want
        tol = bound * (1 + U24) + U24 * (np.abs(rw) + bound)               # (+ the one fp32 subtraction on x - x_hat)
        got = resid[f].cpu().numpy().astype(np.float64)
        Lf = int(L[f])
        assert (np.abs(got[:Lf] - rw[:Lf]) <= tol[:Lf]).all(), f
        assert (got[Lf:] == 0).all(), f
    return saw_short_row


@pytest.mark.parametrize("T,F,batch", [(1500, 5, 2), (50, 9, 9)])
def test_topk_residual_and_sums(T, F, batch):
    d, n, k = 256, 4096, 32
    sae = topk_model(d, n, k, seed=F, bias=-1.5)
    x, L = make_data(F, T, d, seed=F, trim=True, spread=T < 100)
    rep, resid = run_report(sae, x, L, batch)
    assert check_topk_residual(sae, x, L, resid, k), "some rows should have fewer than k positive pre-activations"
    ref = make_reference(sae, x, resid, L)
    R.check_report(rep, ref, f"topk {T} {F} {batch}")
    R.check_bitwise(rep, run_report(sae, x, L, batch)[0])


def test_multi_topk_follows_the_k_selection():
    d, n, k, T, F = 256, 2048, 16, 300, 4
    sae = topk_model(d, n, k, seed=3, multi=True)
    x, L = make_data(F, T, d, seed=3, trim=True)
    rep, resid = run_report(sae, x, L, 3)
    assert sae.encode(torch.from_numpy(x[0]).cuda()).top_indices.shape[-1] == k
    R.check_report(rep, make_reference(sae, x, resid, L), "multi_topk")


# ---- 3. consistency with what exists
def shards(path, x):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d), [T, d])
    return str(path)


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_library_call_agrees_with_feature_stats(tmp_path, kind):
    d, T, F, batch = 256, 50, 9, 4
    sae = l1_model(d, 1024, seed=2) if kind == "l1" else topk_model(d, 4096, 32, seed=2, bias=-1.5)
    x, L = make_data(F, T, d, seed=21, trim=True)
    path = shards(tmp_path, x)
    rep = RC.reconstruction_report(sae, path, "enc", lengths=L, batch_files=batch)
    R.check_bitwise(rep, run_report(sae, x, L, batch)[0])             # the library walks the batches as run_report does
    assert len(rep.filenames) == F and rep.file_sse.shape == (F,)
    st = FST.feature_stats(sae, path, "enc", lengths=L, batch_files=batch)
    assert rep.n_frames == st.n_frames == int(L.sum())
    np.testing.assert_allclose(rep.act_sq_sum, st.act_sq_sum, rtol=1e-5, atol=1e-30)
    resc = rep.rescale()
    assert np.isfinite(resc[st.fire_count > 0]).all() and np.isnan(resc[st.fire_count == 0]).all()


def test_topk_fvu_against_the_float64_formula():
    d, n, k, T, F = 256, 4096, 32, 50, 6
    sae = topk_model(d, n, k, seed=8)
    x, L = make_data(F, T, d, seed=8, trim=False)
    rep, resid = run_report(sae, x, None, F)
    x64, r64 = x.reshape(F * T, d).astype(np.float64), resid.cpu().numpy().reshape(F * T, d).astype(np.float64)
    N = F * T
    assert rep.n_frames == N
    tv = ((x64 - x64.mean(0)) ** 2).sum()
    want = (r64 ** 2).sum() / tv
    # sum_r_sq: rtol 128 u.  Per dimension tv_i = sxx - sx^2 / N with |d sxx| <= 128 u sxx, |d sx| <= 128 u sum |x|
    e_sx = 128 * R.U * np.abs(x64).sum(0)
    tol_tv = (128 * R.U * (x64 ** 2).sum(0) + (2 * np.abs(x64.sum(0)) * e_sx + e_sx ** 2) / N).sum()
    tol = want * (128 * R.U + tol_tv / tv) * 1.001
    print(f"fvu {rep.fvu()!r}, float64 {want!r}, |difference| / bound = {abs(rep.fvu() - want) / tol:.3g}")
    assert abs(rep.fvu() - want) <= tol
    assert 0 < rep.fvu() < 1.5
    np.testing.assert_allclose(rep.file_nmse(), (r64 ** 2).reshape(F, -1).sum(1) / (x64 ** 2).reshape(F, -1).sum(1), rtol=256 * R.U)


# ---- 4. the report predicts a real ablation
@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_ablation_predicts_manipulate_scale_zero(kind):
    d, T, F = 256, 50, 4
    n = 1024 if kind == "l1" else 4096
    latents = (0, n - 1, 127, 128)
    sae = l1_model(d, n, seed=4) if kind == "l1" else topk_model(d, n, 32, seed=4, hot=latents)
    x, _ = make_data(F, T, d, seed=4, trim=False)
    rep, resid = run_report(sae, x, None, F)
    ref = make_reference(sae, x, resid, np.full(F, T), most_fire=False)      # (four named latents are checked, and each must fire)
    d_p = R.round_up(d, 128)
    abl = rep.ablation()
    xc = torch.from_numpy(x).cuda()
    x64 = x.astype(np.float64)
    for j in latents:
        m = manipulate_features(sae, xc, [(j, "scale")], [[0.0]])
        std, man = m.standard_decoded.cpu().numpy().astype(np.float64), m.manipulated_decoded[0].cpu().numpy().astype(np.float64)
        real = ((x64 - man) ** 2).sum() - ((x64 - std) ** 2).sum()
        A, Q = ref.A[j], ref.values["act_sq_sum"][j] * ref.values["dec_norm_sq"][j]
        assert ref.fired[j] and Q > 0, j
        tol = 2.0 ** -8 * A + (d_p + 136) * 2.0 ** -22 * (A + Q)
        print(f"{kind} latent {j}: ablation {abl[j]!r}, real {real!r}, |difference| / bound = {abs(abl[j] - real) / tol:.3g}")
        assert abs(abl[j] - real) <= tol, j
        assert abs(real) > tol, "the ablation should be larger than its own bound, or the test shows nothing"


# ---- 5. determinism and batching
def test_large_shape_is_deterministic_and_unfused_agrees():
    d, n, T, F = 1280, 40960, 1500, 4
    W, b = l1_weights(d, n, seed=11)
    eng = E.SaeEngine("l1", d, n, F * T + 256)
    eng.set_params({"decoder.weight": W, "encoder_bias": b})
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, T, d, generator=g)
    lens = torch.randint(1, T, (F,), generator=g, dtype=torch.int32)
    lens[0] = T
    xd, lens_dev = x.cuda(), lens.cuda()
    lay = E.recon_layout(n, d)
    outs = []
    for unfused in (False, False, True):
        block = torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda")
        fo = torch.zeros(F, 2, dtype=torch.float64, device="cuda")
        resid = torch.empty(F, T, d, device="cuda")
        eng.recon_files(xd, block, fo, lens_dev, resid=resid, unfused=unfused)
        torch.cuda.synchronize()
        outs.append((RC.ReconstructionReport.from_block(block.cpu().numpy(), n, d, fo.cpu().numpy()), resid))
    R.check_bitwise(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))

    def dense(f):
        eng.eval(xd[f])
        ptr, ld = eng.latent_buffer()

        class _Alias:
            __cuda_array_interface__ = {"shape": (T, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
        return torch.as_tensor(_Alias(), device="cuda").view(torch.bfloat16)[:, :n].float()
    w_op = R.bf16(np.ascontiguousarray(eng.get_params()["decoder.weight"].T))
    ref = R.reference(x.numpy(), outs[0][1], dense, w_op, lens.numpy(), "l1", device="cuda")
    assert ref.n_frames == int(lens.sum()) and ref.fired.mean() >= 0.9
    R.check_report(outs[0][0], ref, "d=1280 n=40960")
    R.check_same(outs[0][0], outs[2][0], ref, "fused vs unfused")
    eng.close()


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_batch_size_does_not_matter(kind):
    d, T, F = 256, 50, 9
    sae = l1_model(d, 1024, seed=5) if kind == "l1" else topk_model(d, 4096, 32, seed=5, bias=-1.5)
    x, L = make_data(F, T, d, seed=5, trim=True, spread=kind == "topk")
    a, resid = run_report(sae, x, L, 4)
    b, _ = run_report(sae, x, L, 9)
    R.check_same(a, b, make_reference(sae, x, resid, L), "batch_files 4 vs 9")


# ---- 6. the context
@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_the_pass(variant):
    d, n, T, F = 256, 1024, 50, 4

    def make():
        if variant == "l1":
            W, b = l1_weights(d, n, seed=1)
            eng = E.SaeEngine("l1", d, n, 1500, recon_alpha=1e2)
            eng.set_params({"decoder.weight": W, "encoder_bias": b})
        else:
            eng = E.SaeEngine("topk", d, n, 1500, k=16, optimizer="adam")
            g = torch.Generator().manual_seed(1)
            We = torch.randn(n, d, generator=g) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32),
                            "W_dec": We.numpy().copy(), "b_dec": np.zeros(d, np.float32)})
        return eng

    a, b = make(), make()
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(2)).cuda()
    lay = E.recon_layout(n, d)
    block = torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda")
    fo = torch.zeros(F, 2, dtype=torch.float64, device="cuda")
    for eng in (a, b):
        eng.eval(x.reshape(F * T, d))
    a.recon_files(x, block, fo, torch.tensor([T, 7, T, 1], dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert int(np.frombuffer(block.cpu().numpy(), np.int64, 1)[0]) == 2 * T + 8
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="reconstruction report"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="reconstruction report"):
            a.topk_indices_tensor(F * T, "cuda")
    # a following training step is bitwise the step of a context that never ran the pass
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert a.metrics().tobytes() == b.metrics().tobytes()
    # refusals come before anything is enqueued: the outputs keep their sentinels
    sb, sf = torch.full_like(block, 7), torch.full_like(fo, -77.0)
    sr = torch.full((40 * 50 * d,), -77.0, device="cuda")
    big = torch.randn(40, 50, d).cuda()
    with pytest.raises(E.EngineError, match="max_rows"):
        a.recon_files(big, sb, torch.full((40, 2), -77.0, dtype=torch.float64, device="cuda"), resid=sr)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (C.c_void_p(x.data_ptr()), F, T, E.DTYPE["float32"], None)
    assert a._lib.sae_recon_files(a._ctx, *args, 2, C.c_void_p(sb.data_ptr()), C.c_void_p(sf.data_ptr()), None, st) == -1      # unknown flag
    assert a._lib.sae_recon_files(a._ctx, *args, 0, None, C.c_void_p(sf.data_ptr()), None, st) == -1                          # null block
    assert a._lib.sae_recon_files(a._ctx, *args, 0, C.c_void_p(sb.data_ptr()), None, None, st) == -1                          # null file_out
    assert a._lib.sae_recon_files(a._ctx, *args, 0, C.c_void_p(sb.data_ptr() + 4), C.c_void_p(sf.data_ptr()), None, st) == -1  # alignment
    torch.cuda.synchronize()
    assert bool((sb == 7).all()) and bool((sf == -77.0).all()) and bool((sr == -77.0).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    block = torch.full((E.recon_layout(1024, 256)["bytes"],), 7, dtype=torch.uint8, device="cuda")
    fo = torch.full((2, 2), -77.0, dtype=torch.float64, device="cuda")
    resid = torch.full((2 * 100 * 256,), -77.0, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.recon_files(torch.randn(2, 100, 256).cuda(), block, fo, resid=resid)
    torch.cuda.synchronize()
    assert bool((block == 7).all()) and bool((fo == -77.0).all()) and bool((resid == -77.0).all())
    eng.close()


# ---- 7. the CLI
def test_cli_matches_the_library_call(tmp_path):
    d, n, T, F = 256, 2048, 50, 12
    sae = l1_model(d, n, seed=3)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": d,
                            "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    x, L = make_data(F, T, d, seed=4, trim=True)
    path = shards(tmp_path / "data", x)
    np.save(tmp_path / "len.npy", L)
    out = tmp_path / "report.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.reconstruction", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--lengths", str(tmp_path / "len.npy"), "--batch_files", "5", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    rng = torch.get_rng_state()
    want = RC.reconstruction_report(str(ck), path, "enc", lengths=L, batch_files=5)
    assert torch.equal(torch.get_rng_state(), rng)
    back = RC.ReconstructionReport.from_npz(str(out))
    R.check_bitwise(back, want)
    assert back.filenames == want.filenames and len(back.filenames) == F
    assert summary["n_frames"] == want.n_frames == int(L.sum())
    assert summary["fvu"] == pytest.approx(want.fvu()) and summary["top_latent"] == want.top_latents(1)[0][0]
