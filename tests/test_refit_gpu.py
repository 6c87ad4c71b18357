"""GPU: the refit frontier (freud_amd/refit.py over include/freud_sae.h's sae_refit_files).

Three references, each for what it can say:
* the float64 rule of tests/refit_reference.py (pivot ratios, least squares on every prefix) within its derived bounds -- after the
  cap on undecided frames has been asserted from the reference alone;
* the Gram trace against the float64 Gram matrix within gamma(d_p) sum |w w| (the MFMA's order is not specified, its error is);
* refit_chol.h's rf_row_serial, compiled for the host and fed the engine's OWN G, c and e_0: everything after the MFMA to the bit.

Files of T = 37 frames, 5 files, batches of 2 (74, 74 and 37 rows: a ragged last batch).  The model builders are those of
tests/frontier_cases.py.  L1: d = 256, +-1/16 columns, n = 512.  TopK: d = 128, n = 512, k = 64 on planted()
frames; one case each at d_p = 384 and 768.  K = 1, 17, 31 / 32 / 33 (the MFMA tile edge), 64, 65 (a lane's second row), 128 (L1)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import pursuit as PU
from freud_amd import refit as RF
from freud_amd import sparsity_frontier as SF
from tests import frontier_reference as FR
from tests import refit_reference as R
from tests.frontier_cases import F, T, collect, counted_rows, data, frontier, l1_model, planted, topk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TAUS = (0.5, 0.1)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return R.build_serial(tmp_path_factory.mktemp("rf"), ROOT)


def refit(sae, x, K, taus, batch, lengths=None, support=None, gram=True):
    """The engine calls over x (a CUDA tensor [F, T, d]) in batches of `batch` files -> (RefitFrontier, the block's bytes, the trace
    as numpy arrays over all rows)."""
    Fn, Tn, d = x.shape
    eng = sae._ensure(batch * Tn)
    tau = SF.check_thresholds(taus)
    block = torch.zeros(E.refit_layout(tau.size, K, d, eng.n)["bytes"], dtype=torch.uint8, device="cuda")
    lens = torch.from_numpy(np.asarray(lengths, np.int32)).cuda() if lengths is not None else None
    rows = Fn * Tn
    tr = {"coef": torch.full((rows, K), 7.0, device="cuda"), "err": torch.full((rows, K + 1), 7.0, device="cuda"),
          "dep": torch.full((rows, K), 7, dtype=torch.uint8, device="cuda")}
    if gram:
        tr["gram"] = torch.full((rows, K + 1, K), 7.0, device="cuda")
    sup = None if support is None else torch.from_numpy(np.ascontiguousarray(support, np.int32)).cuda().reshape(rows, K)
    for f0 in range(0, Fn, batch):
        r0, r1 = f0 * Tn, min(Fn, f0 + batch) * Tn
        eng.refit_files(x[f0:f0 + batch].contiguous(), K, tau, block, lens[f0:f0 + batch] if lens is not None else None,
                        support=None if sup is None else sup[r0:r1], trace={k: v[r0:r1] for k, v in tr.items()})
    torch.cuda.synchronize()
    host = block.cpu().numpy()
    return RF.RefitFrontier.from_block(host, K, tau, d, eng.n), host.tobytes(), {k: v.cpu().numpy() for k, v in tr.items()}


def check(prog, tmp_path, sae, w_op, b, x, K, batch=2, taus=TAUS, lengths=None, support=None, ctx=""):
    """One run against the three references.  support: None (the encoder's slots) or int [F * T, K]."""
    Fn, Tn, d = x.shape
    d_p = R.round_up(d, 128)
    n = w_op.shape[0]
    xd = torch.from_numpy(x).cuda()
    xf = xd.float().cpu().numpy().reshape(Fn * Tn, d)
    keep = counted_rows(Fn, Tn, lengths)
    if support is None:
        vals, idx, _ = collect(sae, xd, K, batch)
        active = vals != 0
    else:
        idx = np.asarray(support, np.int64).reshape(Fn * Tn, K)
        active = (idx >= 0) & (idx < n)
        vals = None
    idx_safe = np.where(active, idx, 0)
    w_rows = w_op[idx_safe] * active[..., None]
    r0 = R.r0_fp32(xf, b)
    fs = R.frames(w_rows[keep], active[keep], r0[keep])
    dec = R.assert_decided(fs, ctx)                                        # from the reference alone, before any comparison
    ratios = np.concatenate([f.ratio[~np.isnan(f.ratio)] for f in fs]) if fs else np.zeros(0)
    print(f"{ctx}: kept ratios >= {ratios[ratios > R.DEP].min() if (ratios > R.DEP).any() else float('nan'):.3g}, "
          f"dependent ratios <= {ratios[ratios <= R.DEP].max() if (ratios <= R.DEP).any() else float('nan'):.3g}")

    rf, raw, tr = refit(sae, xd, K, taus, batch, lengths, support)
    assert rf.n_frames == int(keep.sum())
    # rows that do not count: an all-zero trace
    for k in ("coef", "err", "dep", "gram"):
        assert not tr[k][~keep].any()
    gram, coef, err, dep = tr["gram"][keep], tr["coef"][keep], tr["err"][keep], tr["dep"][keep].astype(bool)
    act, wk, r0k = active[keep], w_rows[keep].astype(np.float64), r0[keep].astype(np.float64)

    # the Gram trace and c within their bounds; both triangles equal; inactive slots exactly 0
    G64 = np.einsum("rsd,rtd->rst", wk, wk)
    gb = R.gamma(d_p) * np.einsum("rsd,rtd->rst", np.abs(wk), np.abs(wk))
    gerr = np.abs(gram[:, :K] - G64)
    print(f"{ctx}: Gram worst |err| / bound = {(gerr / np.maximum(gb, 1e-300)).max():.3e}")
    assert (gerr <= gb).all()
    assert (gram[:, :K] == gram[:, :K].transpose(0, 2, 1)).all()
    c64 = np.einsum("rsd,rd->rs", wk, r0k)
    cb = R.gamma(d_p // 64 + 32) * np.einsum("rsd,rd->rs", np.abs(wk), np.abs(r0k))
    assert (np.abs(gram[:, K] - c64) <= cb).all()

    # e_0 bit-equal to the frontier's
    e0 = R.serial_e0(prog, tmp_path, xf[keep], b)
    assert (err[:, 0].view(np.uint32) == e0.view(np.uint32)).all()

    # everything downstream of the MFMA to the bit
    rep = R.serial_replay(prog, tmp_path, gram, err[:, 0], act)
    assert (rep["e"].view(np.uint32) == err.view(np.uint32)).all()
    assert (rep["a"].view(np.uint32) == coef.view(np.uint32)).all()
    assert (rep["dep"].astype(bool) == dep).all()
    nkept = (act & ~dep).sum(1)
    np.testing.assert_array_equal(rf.kept, np.bincount(nkept, minlength=K + 1))

    # the curve against the float64 rule
    E64 = np.array([f.e for f in fs])
    B = np.array([f.curve_bound(d_p) for f in fs])
    cerr = np.abs(err - E64)
    print(f"{ctx}: curve worst |err| / bound = {(cerr[dec] / B[dec]).max():.3e}, worst |err| / e_0 = {(cerr[dec] / E64[dec][:, :1]).max():.3e}")
    assert (cerr[dec] <= B[dec]).all()
    kept64 = np.array([f.kept for f in fs])
    assert ((act & ~dep)[dec] == kept64[dec]).all()
    assert (np.diff(err, axis=1) <= 0).all() and (err >= 0).all()
    und = (~dec).sum()
    # the sums: per-frame bounds, 35 roundings of the unit partials, the undecided frames by their whole e_0
    slack = B[dec].sum(0) + 36 * R.U * err.sum(0) + (E64[~dec][:, :1].sum() if und else 0.0)
    assert (np.abs(rf.sse - E64.sum(0)) <= slack).all()
    # e_final: the directly computed error of the traced coefficients, and SSE_FINAL
    res = r0k - np.einsum("rs,rsd->rd", coef.astype(np.float64), wk)
    ef64 = (res * res).sum(1)
    fb = np.array([f.final_bound(d_p) for f in fs])
    assert (np.abs(ef64 - err[:, K])[dec] <= fb[dec]).all()
    assert abs(rf.sse_final - rf.sse[K]) <= fb[dec].sum() + 72 * R.U * rf.sse[0] + (E64[~dec][:, 0].sum() if und else 0.0)

    # the integer fields from the trace
    first = np.zeros_like(act)
    for r in range(len(act)):
        seen = set()
        for s in range(K):
            if act[r, s] and idx_safe[keep][r, s] not in seen:
                first[r, s] = True
                seen.add(idx_safe[keep][r, s])
    ik = idx_safe[keep]
    np.testing.assert_array_equal(rf.slots, np.bincount(ik[first], minlength=n))
    np.testing.assert_array_equal(rf.neg, np.bincount(ik[act & (coef < 0)], minlength=n))
    np.testing.assert_array_equal(rf.dep, np.bincount(ik[act & dep], minlength=n))
    if support is None:
        k_ = act & ~dep
        bins = R.serial_bins(prog, tmp_path, (coef[k_] / vals[keep][k_]).astype(np.float32))
        np.testing.assert_array_equal(rf.ratio, np.bincount(bins, minlength=36))
        assert rf.bad_index == 0
    else:
        assert not rf.ratio.any()
        assert rf.bad_index == int(((idx[keep] != -1) & ~act).sum())
    # budgets: the frontier's predicate on the engine's own curve
    for t, tau in enumerate(taus):
        lim = (np.float32(tau) * err[:, :1]).astype(np.float32)
        hit = err <= lim
        np.testing.assert_array_equal(rf.budget[t], np.bincount(np.where(hit.any(1), hit.argmax(1), K + 1), minlength=K + 2))
    x64 = xf[keep].astype(np.float64)
    assert (np.abs(rf.sum_x - x64.sum(0)) <= 36 * R.U * np.abs(x64).sum(0) + 1e-300).all()
    return rf, raw, tr, dict(vals=vals, idx=idx, keep=keep, xf=xf, fs=fs, dec=dec, B=B)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 17, 31, 32, 33, 64, 65, 128])
def test_l1(prog, tmp_path, K):
    sae, w_op, b = l1_model(512, seed=7, bias=0.0)
    x = data(256, 100 + K)
    rf, _, _, aux = check(prog, tmp_path, sae, w_op, b, x, K, ctx=f"l1 K={K}")
    # least-squares optimality against the encoder's own curve on the same batches
    fr, _ = frontier(sae, torch.from_numpy(x).cuda(), K, TAUS, 2)
    ref = FR.reference(aux["vals"], aux["idx"], w_op, aux["xf"], b)
    slack = aux["B"].sum(0) + ref.sse_bound() + 72 * R.U * fr.sse
    print(f"l1 K={K}: refit / encoder sse at K = {rf.sse[K] / fr.sse[K]:.4f}")
    assert (rf.sse <= fr.sse + slack).all() and rf.sse[0] == fr.sse[0]
    assert rf.sum_x.tobytes() == fr.sum_x.tobytes() and rf.sum_x_sq.tobytes() == fr.sum_x_sq.tobytes()


@pytest.mark.parametrize("K", [1, 17, 31, 32, 33, 64])
def test_topk(prog, tmp_path, K):
    sae, w_op, b = topk_model(128, 512, 64, seed=31)
    x = planted(w_op, b, 131)
    rf, _, _, aux = check(prog, tmp_path, sae, w_op, b, x, K, ctx=f"topk K={K}")
    fr, _ = frontier(sae, torch.from_numpy(x).cuda(), K, TAUS, 2)
    ref = FR.reference(aux["vals"], aux["idx"], w_op, aux["xf"], b)
    assert (rf.sse <= fr.sse + aux["B"].sum(0) + ref.sse_bound() + 72 * R.U * fr.sse).all() and rf.sse[0] == fr.sse[0]


@pytest.mark.parametrize("d", [384, 768])
def test_geometry(prog, tmp_path, d):
    sae, w_op, b = topk_model(d, 512, 32, seed=40 + d)
    x = planted(w_op, b, 140 + d)
    check(prog, tmp_path, sae, w_op, b, x, 32, ctx=f"topk d={d}")
    check(prog, tmp_path, sae, w_op, b, x.astype(np.float16), 17, ctx=f"topk d={d} f16")


def test_given_support_and_pursuit(prog, tmp_path):
    """A given support: duplicates and -1 slots planted at known places, out-of-range indices counted; then the pursuit's own trace
    as the support -- pursuit with a final orthogonal projection cannot end above the pursuit."""
    n, K = 512, 20
    sae, w_op, b = topk_model(128, n, 64, seed=31)
    x = planted(w_op, b, 131)
    g = np.random.default_rng(5)
    sup = np.stack([g.permutation(n)[:K] for _ in range(F * T)]).astype(np.int32)
    sup[:, 7] = sup[:, 2]                      # a duplicate in every frame
    sup[::3, 4] = -1                           # empty slots
    sup[1::5, 9] = n + 3                       # out of range, above
    sup[2::7, 11] = -5                         # out of range, below
    rf, _, tr, aux = check(prog, tmp_path, sae, w_op, b, x, K, support=sup, ctx="given")
    assert tr["dep"][:, 7].all() and not tr["dep"][:, [0, 1, 2, 3, 5, 6]].any() and not tr["coef"][:, 7].any()
    assert (np.diff(tr["err"], axis=1)[:, 7] == 0).all() and (np.diff(tr["err"][::3], axis=1)[:, 4] == 0).all()
    assert rf.bad_index == len(range(1, F * T, 5)) + len(range(2, F * T, 7)) and rf.dep.sum() == F * T
    # the pursuit's picks as the support
    xd = torch.from_numpy(x).cuda()
    pidx, _pval, perr = PU.pursuit_encode(sae, xd, K)
    idx, coef, err = RF.refit_encode(sae, xd, support=pidx)
    assert idx.shape == (F, T, K) and (idx == pidx).all()
    pe, re_ = perr.cpu().numpy().reshape(F * T, K + 1).astype(np.float64), err.cpu().numpy().reshape(F * T, K + 1).astype(np.float64)
    sup2 = pidx.cpu().numpy().reshape(F * T, K)
    act2 = sup2 >= 0
    fs = R.frames(w_op[np.where(act2, sup2, 0)] * act2[..., None], act2, R.r0_fp32(x.reshape(F * T, -1), b))
    B = np.array([f.curve_bound(128)[K] + f.final_bound(128) for f in fs])
    # In exact arithmetic the least-squares error on the picks is at most the error of the pursuit's own coefficients.  The pursuit's
    # e_K is the fp32 norm of its fp32 residual: K + 2 roundings per element on magnitudes <= |r_0| + sum |a_i| |w_i|, and every
    # |a_i| |w_i| is a projection of a residual no longer than r_0, so |dr|_2 <= (K + 2) U (K + 1) sqrt(e_0) and its e_K lies within
    # [2 (K + 2) (K + 1) U + gamma(C + 8)] e_0 of the exact one (C + 8: a lane's chain and the butterfly of pursuit.h).
    P_SLACK = (2 * (K + 2) * (K + 1) * R.U + R.gamma(128 // 64 + 8)) * pe[:, 0]
    assert (re_[:, K] <= pe[:, K] + B + P_SLACK).all()
    assert (np.abs(re_[:, 0] - pe[:, 0]) <= 2 * R.gamma(128 // 64 + 32) * pe[:, 0]).all()      # (two fixed orders of the same sum)
    rf2, _, tr2 = refit(sae, xd, K, (), 2, support=sup2, gram=False)
    assert rf2.sse_final <= pe[:, K].sum() + B.sum() + P_SLACK.sum()
    print(f"pursuit + projection: sum e_final / sum pursuit e_K = {rf2.sse_final / pe[:, K].sum():.4f}")
    assert (tr2["err"].view(np.uint32) == err.cpu().numpy().reshape(F * T, K + 1).view(np.uint32)).all()
    assert (tr2["coef"].view(np.uint32) == coef.cpu().numpy().reshape(F * T, K).view(np.uint32)).all()


def test_given_support_l1_without_a_forward(prog, tmp_path):
    """A fresh L1 context and a given support: no encoder has run, the operand rows come from the pass's own weight preparation."""
    n, K = 512, 33
    sae, w_op, b = l1_model(n, seed=9, bias=0.0)
    g = np.random.default_rng(6)
    sup = np.stack([g.permutation(n)[:K] for _ in range(F * T)]).astype(np.int32)
    sup[:, 32] = sup[:, 0]                     # a duplicate across the tile edge
    rf, _, tr, _ = check(prog, tmp_path, sae, w_op, b, data(256, 77), K, support=sup, ctx="given l1")
    assert tr["dep"][:, 32].all() and rf.dep.sum() == F * T and rf.bad_index == 0


def test_lengths_trimming(prog, tmp_path):
    sae, w_op, b = topk_model(128, 512, 64, seed=31)
    x = planted(w_op, b, 131)
    lengths = [37, 1, 20, 50, 33]              # (50: longer than the file -- trimmed to T)
    rf, _, _, aux = check(prog, tmp_path, sae, w_op, b, x, 17, lengths=lengths, ctx="lengths")
    assert rf.n_frames == 37 + 1 + 20 + 37 + 33


def test_determinism_batches_and_prefix():
    sae, w_op, b = l1_model(512, seed=7, bias=0.0)
    xd = torch.from_numpy(data(256, 164)).cuda()
    rf, raw, tr = refit(sae, xd, 64, TAUS, 2)
    rf_b, raw_b, tr_b = refit(sae, xd, 64, TAUS, 2)
    assert raw == raw_b and all(tr[k].tobytes() == tr_b[k].tobytes() for k in tr)          # two runs: equal bytes
    for batch in (1, 5):
        o, _, t = refit(sae, xd, 64, TAUS, batch)
        assert all(tr[k].tobytes() == t[k].tobytes() for k in tr), batch                   # the trace
        for name in ("n_frames", "bad_index"):
            assert getattr(o, name) == getattr(rf, name)
        for name in ("budget", "kept", "slots", "neg", "dep", "ratio"):
            np.testing.assert_array_equal(getattr(o, name), getattr(rf, name), err_msg=f"{name} batch={batch}")
    # the prefix: a run at K' = 17 over the same batches
    o17, _, t17 = refit(sae, xd, 17, TAUS, 2)
    assert o17.sse.tobytes() == rf.sse[:18].tobytes()
    assert t17["err"].tobytes() == np.ascontiguousarray(tr["err"][:, :18]).tobytes()
    assert t17["dep"].tobytes() == np.ascontiguousarray(tr["dep"][:, :17]).tobytes()


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_contract(variant):
    """The getters refuse after the pass, the training state around it is bitwise unchanged, the context stays usable; every argument
    error returns SAE_ERR_INVALID with nothing enqueued."""
    n, Fn, K = 512, 2, 16
    if variant == "l1":
        a = E.SaeEngine("l1", 256, n, 1500, optimizer="adam")
        g = np.random.default_rng(7)
        W = np.where(g.random((256, n)) < 0.5, np.float32(-1 / 16), np.float32(1 / 16)).astype(np.float32)
        a.set_params({"decoder.weight": W, "encoder_bias": np.full(n, -1.0, np.float32)})
    else:
        a = E.SaeEngine("topk", 256, n, 1500, k=16, optimizer="adam")
        We = torch.randn(n, 256, generator=torch.Generator().manual_seed(1)) / 16
        a.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32), "W_dec": We.numpy().copy(),
                      "b_dec": np.zeros(256, np.float32)})
    x = torch.randn(Fn, T, 256, generator=torch.Generator().manual_seed(2)).cuda()
    if variant == "topk":
        a.step(x.reshape(Fn * T, 256), 1e-3)
    a.eval(x.reshape(Fn * T, 256))
    before = a.get_params()
    step, m1, m2 = a.get_opt_state()
    fired = a.get_topk_state().copy() if variant == "topk" else None
    tau = np.array([0.5, 0.1], np.float32)
    nbytes = E.refit_layout(2, K, 256, n)["bytes"]
    block = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    a.refit_files(x, K, tau, block)
    torch.cuda.synchronize()
    assert int(block[:8].view(torch.int64)[0]) == Fn * T
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, 256, device="cuda"))):
        with pytest.raises(E.EngineError, match="refit frontier"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="refit frontier"):
            a.topk_indices_tensor(Fn * T, "cuda")
        assert np.array_equal(a.get_topk_state(), fired)
    for k_, v in a.get_params().items():
        assert v.tobytes() == before[k_].tobytes(), k_
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k_], m1[k_]) and np.array_equal(n2[k_], m2[k_]) for k_ in m1)
    a.eval(x.reshape(Fn * T, 256))
    a.latent_buffer()
    a.step(x.reshape(Fn * T, 256), 1e-3)
    torch.cuda.synchronize()

    lib, vp = a._lib, C.c_void_p
    z = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    INVALID = -1                                               # include/freud_sae.h: SAE_ERR_INVALID

    def raw(xp=x.data_ptr(), n_files=Fn, rows=T, dt=E.DTYPE["float32"], K=K, taus=(0.5, 0.1), n_tau=None, flags=0, blk=z.data_ptr(), sup=None,
            trace=(None, None, None, None)):
        arr = (C.c_float * max(len(taus), 1))(*taus)
        return lib.sae_refit_files(a._ctx, vp(xp), n_files, rows, dt, None, K, arr, len(taus) if n_tau is None else n_tau, flags, vp(sup), vp(blk),
                                   *(vp(p) for p in trace), vp(torch.cuda.current_stream().cuda_stream))

    te = torch.zeros(Fn * T * (K + 1), dtype=torch.float32, device="cuda")
    k_over = 17 if variant == "topk" else n + 1                # K > k (TopK), K > n_dict and > MAX_K (L1)
    for bad in (dict(K=0), dict(K=-1), dict(K=E.REFIT_MAX_K + 1), dict(K=k_over), dict(taus=(0.1,) * 9), dict(taus=(0.0,)), dict(taus=(1.0,)),
                dict(taus=(float("nan"),)), dict(taus=(0.5, -0.1)), dict(n_tau=-1), dict(flags=1), dict(xp=None), dict(blk=None),
                dict(blk=z.data_ptr() + 4), dict(n_files=0), dict(rows=0), dict(n_files=60), dict(dt=99),
                dict(trace=(None, te.data_ptr() + 2, None, None)), dict(sup=te.data_ptr() + 2)):
        assert raw(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((z == 0).all()) and bool((te == 0).all())
    assert raw(trace=(None, te.data_ptr(), None, None)) == 0
    torch.cuda.synchronize()
    assert int(z[:8].view(torch.int64)[0]) == Fn * T and bool((te != 0).any())
    a.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    block = torch.zeros(E.refit_layout(1, 8, 256, 1024)["bytes"], dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.refit_files(torch.randn(2, 100, 256).cuda(), 8, [0.5], block)
    torch.cuda.synchronize()
    assert bool((block == 0).all())
    eng.close()


def test_module_surface(tmp_path):
    from freud_amd.loader import write_shards
    sae, w_op, b = topk_model(128, 512, 64, seed=31)
    x = planted(w_op, b, 131)
    write_shards(str(tmp_path), "enc", x.reshape(F, -1), [T, 128])
    rf = RF.refit_frontier(sae, str(tmp_path), "enc", K=17, thresholds=TAUS, batch_files=2)
    rf2, _, _ = refit(sae, torch.from_numpy(x).cuda(), 17, TAUS, 2)
    assert rf.sse.tobytes() == rf2.sse.tobytes() and rf.ratio.tobytes() == rf2.ratio.tobytes() and rf.sse_final == rf2.sse_final
    fr = SF.sparsity_frontier(sae, str(tmp_path), "enc", K=17, thresholds=TAUS, batch_files=2)
    pu = PU.pursuit_frontier(sae, str(tmp_path), "enc", K=17, thresholds=TAUS, batch_files=2)
    dec = rf.decompose(fr, pu)
    np.testing.assert_allclose(dec["coefficient_gap"] + dec["support_gap"], pu.amortisation_gap(fr), atol=1e-12)
    assert (dec["coefficient_gap"] >= -1e-6).all() and dec["coefficient_gap"][17] > 0
    idx, coef, err = RF.refit_encode(sae, torch.from_numpy(x).cuda(), K=17)
    assert idx.shape == (F, T, 17) and coef.shape == (F, T, 17) and err.shape == (F, T, 18)
    assert rf.summary()["n_frames"] == F * T
