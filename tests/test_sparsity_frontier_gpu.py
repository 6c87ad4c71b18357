"""GPU: the sparsity frontier (freud_amd/sparsity_frontier.py over include/freud_sae.h's sae_frontier_files).

The reference is the float64 rule of tests/frontier_reference.py on the operands as the engine holds them: the slots
sae_collect_files returns for the same files, the bf16-valued operand rows, the delivered x and the fp32 b_dec.  Every bound is the
one stated there; before anything is compared, at least 99 % of the counted frames must be decided at every threshold.

L1 weights: d = 256 and every entry of a column is +-1/16, so a column's norm is exactly 1, the in-place renormalisation of every
L1 forward is a bit-exact fixed point and the operand rows are the columns themselves.  TopK: seeded tied dictionaries with a random
b_dec on frames planted from the dictionary (planted()): the thresholds are crossed in large steps and every frame's e_s rises again.

Files of T = 37 frames, 5 files, batches of 2 (74, 74 and 37 rows: a ragged last batch) unless a test says otherwise.

Internal thresholds of freud_amd/csrc/frontier.h and the tests on each side of them:
* slot chunk FR_CHUNK = 32 norms (m = 0 .. K): K = 1 and 17 stay inside the first chunk, K = 32 puts ONE norm into a second chunk,
  K = 64 and 256 end one norm past a full chunk (test_topk, test_l1);
* gather depth FR_DEPTH = 4: K = 1 (fewer slots than the depth), 17 (a remainder of 1), 32 (none);
* rows per workgroup FR_UNIT = 32, 4 waves: 74 rows = two full units and one of 10, 37 rows = one full and one of 5 (a wave with one
  row, waves with two); test_lengths has units whose rows all lie beyond a file's length;
* the d_p forms: 256 (generic, 2 column pairs per lane: the L1 and TopK tests, and d = 200 padded to it), 384 and 768 (the
  compile-time forms 3 and 6; test_geometry, 5 files each so that the cap on undecided frames leaves room for one), 1280 shares
  the code of 384 / 768 and is not run here;
* the 128-row blocks of the dimension sums: 74 rows (one block), batch_files = 5 in test_invariance (185 rows: two);
* padding slots: test_topk with a low encoder bias, test_l1 (row L0 on both sides of K)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import reconstruction as RC
from freud_amd import sparsity_frontier as SF
from freud_amd.loader import write_shards
from tests import frontier_reference as R
from tests.frontier_cases import F, T, collect, counted_rows, data, frontier, l1_model, planted, topk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TAUS = (0.5, 0.2, 0.1, 0.05)


def check(sae, w_op, b, x, K, batch, taus=TAUS, lengths=None, k_full=None, ctx=""):
    """One run against the rule.  x: numpy [F, T, d] in the dtype the engine is to see.  k_full: a K at which collect returns every
    active latent of a row (the count behind rows_cut / active_cut)."""
    Fn, Tn, d = x.shape
    xd = torch.from_numpy(x).cuda()
    xf = xd.float().cpu().numpy().reshape(Fn * Tn, d)                       # the delivered x, widened exactly
    vals, idx, _ = collect(sae, xd, K, batch)
    keep = counted_rows(Fn, Tn, lengths)
    ref = R.reference(vals[keep], idx[keep], w_op, xf[keep], b)
    R.assert_decidable(ref, taus, ctx)                                     # from the reference alone, before any comparison
    fr, raw = frontier(sae, xd, K, taus, batch, lengths)
    assert fr.n_frames == int(keep.sum())
    R.check_sse(fr.sse, ref, ctx)
    for t, tau in enumerate(taus):
        assert int(fr.budget[t].sum()) == fr.n_frames
        R.check_hist(fr.budget[t], ref, tau, f"{ctx} tau={tau}")
    # the denominator: fp32 sums of at most 128 rows (32 per wave, 4 waves: 35 roundings), then float64
    x64 = xf[keep].astype(np.float64)
    for got, want, mag in ((fr.sum_x, x64.sum(0), np.abs(x64).sum(0)), (fr.sum_x_sq, (x64 * x64).sum(0), (x64 * x64).sum(0))):
        assert (np.abs(got - want) <= 36 * R.U * mag + 1e-300).all()
    if k_full is not None:
        fv, _, _ = collect(sae, xd, k_full, batch)
        nnz = (fv[keep] > 0).sum(1)
        assert fr.rows_cut == int((nnz > K).sum()) and fr.active_cut == int(np.maximum(nnz - K, 0).sum())
    return fr, ref, raw, (vals, idx, keep, xf)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17, 32])
def test_topk(K):
    n, k = 1024, 32
    sae, w_op, b = topk_model(256, n, k, seed=31)
    x = planted(w_op, b, 131)
    fr, ref, _, (_, _, keep, xf) = check(sae, w_op, b, x, K, batch=2, k_full=k, ctx=f"topk K={K}")
    if K == k:
        assert (np.diff(ref.E, axis=1) > 0).any(1).all()                        # every frame's curve rises somewhere
        assert np.count_nonzero(fr.budget[2]) >= 4 and 0 < fr.budget[3][K + 1] < F * T
    e0 = ((xf.astype(np.float64) - b.astype(np.float64)) ** 2).sum()
    assert abs(fr.sse[0] - e0) <= ref.sse_bound()[0]
    assert fr.rows_cut <= F * T and (K < k or fr.active_cut == 0)


def test_topk_full_k_against_the_reconstruction_report(tmp_path):
    """At K = k the last point of the curve is the reconstruction report's squared error: the same latent, the same operand rows,
    x - (b + sum) there and (x - b) - sum here -- K + 1 roundings per element on the same magnitudes either way, so the tolerance is
    the frontier's bound at s = K twice over, plus the report's own 128-row fp32 partials (35 roundings)."""
    n, k = 1024, 32
    sae, w_op, b = topk_model(256, n, k, seed=31)
    x = planted(w_op, b, 131)
    write_shards(str(tmp_path), "enc", x.reshape(F, -1), [T, 256])
    fr = SF.sparsity_frontier(sae, str(tmp_path), "enc", batch_files=2)
    assert fr.K == k and fr.thresholds.tolist() == [np.float32(t) for t in SF.DEFAULT_THRESHOLDS]
    rep = RC.reconstruction_report(sae, str(tmp_path), "enc", batch_files=2)
    vals, idx, _ = collect(sae, torch.from_numpy(x).cuda(), k, 2)
    ref = R.reference(vals, idx, w_op, x.reshape(F * T, 256), b)
    tol = 2 * ref.sse_bound()[k] + 36 * R.U * rep.sse()
    print(f"sse[K] {fr.sse[k]:.6e} report {rep.sse():.6e} diff {abs(fr.sse[k] - rep.sse()):.3e} tol {tol:.3e}")
    assert abs(fr.sse[k] - rep.sse()) <= tol
    assert fr.n_frames == rep.n_frames and fr.total_variance() == pytest.approx(rep.total_variance(), rel=1e-5)
    assert fr.fvu(k) == pytest.approx(rep.fvu(), rel=1e-4)
    fr2, _ = frontier(sae, torch.from_numpy(x).cuda(), k, SF.DEFAULT_THRESHOLDS, 2)
    assert fr2.sse.tobytes() == fr.sse.tobytes() and fr2.budget.tobytes() == fr.budget.tobytes()      # the module is the engine calls


@pytest.mark.parametrize("multi", [False, True])
def test_topk_padding_slots(multi):
    """An encoder bias of -1.5 leaves a handful of positives per row: the selection holds the engine's zeros, the slots behind the
    positives are padding (+0.0) and the curve is flat there.  multi_topk: its k selection."""
    n, k, K = 1024, 32, 32
    sae, w_op, b = topk_model(256, n, k, seed=20, bias=-1.5, multi_topk=multi)
    x = planted(w_op, b, 120)
    # (the curve of these frames levels out near 10 % of e_0: the thresholds keep clear of that plateau)
    fr, _, _, (vals, _, _, _) = check(sae, w_op, b, x, K, batch=2, taus=(0.5, 0.25, 0.15, 0.03), k_full=k, ctx="topk padding")
    nnz = (vals > 0).sum(1)
    assert (nnz < k).any() and (nnz > 0).any() and fr.rows_cut == 0 and fr.active_cut == 0
    assert (fr.sse[int(nnz.max()):] == fr.sse[int(nnz.max())]).all()            # nothing changes behind the last positive of any row


@pytest.mark.parametrize("K", [64, 256])
def test_l1(K, tmp_path):
    """n = 512.  A quiet file, ordinary files and a loud one put the rows' L0 on both sides of K = 64; at K = 256 =
    SAE_FRONTIER_MAX_K most rows end in padding."""
    n = 512
    sae, w_op, b = l1_model(n, seed=5, bias=-1.2)
    x = data(256, 10, scale=[1, 0.3, 1, 2.5, 1])
    fr, ref, _, (vals, _, _, xf) = check(sae, w_op, b, x, K, batch=2, k_full=n, ctx=f"l1 K={K}")
    full, _, _ = collect(sae, torch.from_numpy(x).cuda(), n, 2)
    nnz = (full > 0).sum(1)
    if K == 64:
        assert (nnz < K).any() and (nnz > K).any() and 0 < fr.rows_cut < F * T
    write_shards(str(tmp_path / "d"), "enc", x.reshape(F, -1), [T, 256])
    from freud_amd import collect_features as CF
    rep = CF.collect_features(sae, str(tmp_path / "d"), "enc", str(tmp_path / "o"), k=K, batch_files=2)
    assert fr.active_cut == rep.dropped and fr.rows_cut == rep.rows_dropped
    rc = RC.reconstruction_report(sae, str(tmp_path / "d"), "enc", batch_files=2)
    assert abs(fr.sse[0] - rc.file_energy.sum()) <= 2 * ref.sse_bound()[0]       # b = 0: e_0 = |x|^2, two fp32 summation orders


@pytest.mark.parametrize("d,dtype,seed", [(200, np.float32, 23), (384, np.float32, 32), (768, np.float32, 20), (256, np.float16, 31)])
def test_geometry(d, dtype, seed):
    sae, w_op, b = topk_model(d, 1024, 32, seed=seed)
    x = planted(w_op, b, seed + 100).astype(dtype)
    check(sae, w_op, b, x, 17, batch=2, k_full=32, ctx=f"d={d} {np.dtype(dtype).name}")


def test_lengths():
    """Trimmed files, one of a single frame: 4 of the 5 files end early, and whole 32-row units lie beyond a length."""
    sae, w_op, b = topk_model(256, 1024, 32, seed=31)
    x = planted(w_op, b, 131)
    L = [37, 1, 20, 50, 5]
    fr, _, _, _ = check(sae, w_op, b, x, 32, batch=2, lengths=L, k_full=32, ctx="lengths")
    assert fr.n_frames == 37 + 1 + 20 + 37 + 5


def test_invariance():
    sae, w_op, b = topk_model(256, 1024, 32, seed=23, bias=-0.5)
    x = planted(w_op, b, 123)
    K = 32
    runs = {bf: check(sae, w_op, b, x, K, batch=bf, k_full=32, ctx=f"batch_files={bf}") for bf in (1, 2, 5)}
    fr, ref, raw, _ = runs[2]
    again, raw2 = frontier(sae, torch.from_numpy(x).cuda(), K, TAUS, 2)
    assert raw2 == raw                                                          # two runs: the same bytes
    for bf in (1, 5):
        o = runs[bf][0]
        assert o.budget.tobytes() == fr.budget.tobytes() and (o.n_frames, o.rows_cut, o.active_cut) == (fr.n_frames, fr.rows_cut, fr.active_cut)
        assert (np.abs(o.sse - fr.sse) <= 2 * ref.sse_bound()).all()
        assert np.allclose(o.sum_x, fr.sum_x, rtol=0, atol=72 * R.U * np.abs(x).sum((0, 1)).max())
    # the curve's prefix: a run at K' is the first K' + 1 entries of the run at K, to the bit
    for Kp in (1, 17):
        short, _ = frontier(sae, torch.from_numpy(x).cuda(), Kp, TAUS, 2)
        assert short.sse.tobytes() == fr.sse[:Kp + 1].tobytes()


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_state_and_argument_rules(variant):
    n, K, Fn = 1024, 16, 4
    g = np.random.default_rng(1)

    def make():
        if variant == "l1":
            eng = E.SaeEngine("l1", 256, n, 1500, recon_alpha=1e2)
            W = np.where(g.random((256, n)) < 0.5, np.float32(-1 / 16), np.float32(1 / 16)).astype(np.float32)
            eng.set_params({"decoder.weight": W, "encoder_bias": np.full(n, -1.0, np.float32)})
        else:
            eng = E.SaeEngine("topk", 256, n, 1500, k=16, optimizer="adam")
            We = torch.randn(n, 256, generator=torch.Generator().manual_seed(1)) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32),
                            "W_dec": We.numpy().copy(), "b_dec": np.zeros(256, np.float32)})
        return eng

    a = make()
    x = torch.randn(Fn, T, 256, generator=torch.Generator().manual_seed(2)).cuda()
    if variant == "topk":
        a.step(x.reshape(Fn * T, 256), 1e-3)
    a.eval(x.reshape(Fn * T, 256))
    before = a.get_params()
    step, m1, m2 = a.get_opt_state()
    fired = a.get_topk_state().copy() if variant == "topk" else None
    tau = np.array([0.5, 0.1], np.float32)
    nbytes = E.frontier_layout(2, K, 256)["bytes"]
    block = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    a.frontier_files(x, K, tau, block)
    torch.cuda.synchronize()
    assert int(block[:8].view(torch.int64)[0]) == Fn * T
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, 256, device="cuda"))):
        with pytest.raises(E.EngineError, match="sparsity frontier"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="sparsity frontier"):
            a.topk_indices_tensor(Fn * T, "cuda")
        assert np.array_equal(a.get_topk_state(), fired)
    for k_, v in a.get_params().items():
        assert v.tobytes() == before[k_].tobytes(), k_
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k_], m1[k_]) and np.array_equal(n2[k_], m2[k_]) for k_ in m1)
    a.eval(x.reshape(Fn * T, 256))                              # the getters are back after the next forward
    a.latent_buffer()

    # every argument error: SAE_ERR_INVALID before anything ran -- the block is still zero
    lib, vp = a._lib, C.c_void_p
    z = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    INVALID = -1                                               # include/freud_sae.h: SAE_ERR_INVALID

    def raw(xp=x.data_ptr(), n_files=Fn, rows=T, dt=E.DTYPE["float32"], K=K, taus=(0.5, 0.1), n_tau=None, flags=0, blk=z.data_ptr()):
        arr = (C.c_float * max(len(taus), 1))(*taus)
        return lib.sae_frontier_files(a._ctx, vp(xp), n_files, rows, dt, None, K, arr if taus is not None else None,
                                      len(taus) if n_tau is None else n_tau, flags, vp(blk), vp(torch.cuda.current_stream().cuda_stream))

    k_max = 16 if variant == "topk" else 256
    for bad in (dict(K=0), dict(K=-1), dict(K=k_max + 1), dict(K=E.FRONTIER_MAX_K + 1), dict(taus=(0.1,) * 9), dict(taus=(0.0,)), dict(taus=(1.0,)),
                dict(taus=(float("nan"),)), dict(taus=(0.5, -0.1)), dict(n_tau=-1), dict(flags=1), dict(xp=None), dict(blk=None),
                dict(blk=z.data_ptr() + 4), dict(n_files=0), dict(rows=0), dict(n_files=60), dict(dt=99)):
        assert raw(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((z == 0).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert int(z[:8].view(torch.int64)[0]) == Fn * T
    a.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    block = torch.zeros(E.frontier_layout(1, 8, 256)["bytes"], dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.frontier_files(torch.randn(2, 100, 256).cuda(), 8, [0.5], block)
    torch.cuda.synchronize()
    assert bool((block == 0).all())
    eng.close()


def test_cli(tmp_path):
    n, K = 512, 24
    sae, _, _ = l1_model(n, seed=8, bias=-1.2)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": 256, "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    x = data(256, 14)
    write_shards(str(tmp_path / "d"), "enc", x.reshape(F, -1), [T, 256])
    rng = torch.get_rng_state()
    fr = SF.sparsity_frontier(sae, str(tmp_path / "d"), "enc", K=K, thresholds=(0.5, 0.25), batch_files=2)
    assert torch.equal(torch.get_rng_state(), rng)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.sparsity_frontier", "--sae", str(ck), "--data_path", str(tmp_path / "d"), "--layer_name",
                        "enc", "--K", str(K), "--thresholds", "0.5,0.25", "--batch_files", "2", "--out", str(tmp_path / "f.npz")],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["K"] == K and out["n_frames"] == F * T and out["fvu"] == fr.summary()["fvu"]
    back = SF.SparsityFrontier.from_npz(str(tmp_path / "f.npz"))
    assert back.sse.tobytes() == fr.sse.tobytes() and back.budget.tobytes() == fr.budget.tobytes()
