"""GPU: the pursuit frontier (freud_amd/pursuit.py over include/freud_sae.h's sae_pursuit_files).

The reference is tests/pursuit_reference.py: the float64 rule, and the teacher-forced replay of the engine's own trace -- the float64
residual rebuilt from (trace_idx, trace_val) -- against which every pick, stop, coefficient and norm is held to the bound derived
there from the kernel's roundings.  No row is exempt from those; only the comparison with the float64 rule's own picks is restricted
to the rows the rule decides, and at least 95 % of the counted rows must be decided before anything is compared.

Models are the frontier tests' (tests/frontier_cases.py): L1 with +-1/16 columns at d = 256, TopK tied unit rows with a
random b_dec, frames from planted() with nplant = K.  Files of T = 37 frames, 5 files in batches of 2 (74, 74 and 37 rows) unless a
test says otherwise.

Shapes and the branches they reach (freud_amd/csrc/pursuit.h, gemm_launch.h):
* d = 256, n = 512, 185 rows in batches of 74 / 74 / 37: the generic d_p form (2 column pairs per lane), a row grid padded to 256 and
  n_p = 512 -- the 256-edge tile grid, whole tiles of padding rows;
* d = 96, n = 320, 300 rows (T = 60): d padded to 128, n_p = 384 -- an odd number of 128-column tiles, so the 128-edge tile grid, and a
  ragged last column tile (columns 320 .. 383 are never eligible);
* 512 rows (16 files of T = 32), n = 512: the 256-edge grid with no padding row;
* d_p = 384 and 768: the step kernel's compile-time forms 3 and 6;
* K = 1, 6, 32, and K = 256 = SAE_PURSUIT_MAX_K once at n = 512."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd import pursuit as P
from freud_amd import sparsity_frontier as SF
from freud_amd.config import TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import TopKAutoEncoder
from tests import pursuit_reference as R
from tests.frontier_cases import F, T, collect, counted_rows, frontier, l1_model, planted, topk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
TAUS = (0.5, 0.2, 0.1, 0.05)


def pursue(sae, x, K, taus, batch, lengths=None, trace=True):
    """The engine calls over x (a CUDA tensor [F, T, d]) in batches of `batch` files -> (PursuitFrontier, the block's bytes,
    idx [F*T, K], val [F*T, K], err [F*T, K + 1])."""
    Fn, Tn, d = x.shape
    eng = sae._ensure(batch * Tn) if hasattr(sae, "_ensure") else sae
    tau = SF.check_thresholds(taus)
    block = torch.zeros(E.pursuit_layout(tau.size, K, d, eng.n)["bytes"], dtype=torch.uint8, device="cuda")
    lens = torch.from_numpy(np.asarray(lengths, np.int32)).cuda() if lengths is not None else None
    idx = torch.full((Fn * Tn, K), -7, dtype=torch.int32, device="cuda")
    val = torch.full((Fn * Tn, K), -7.0, dtype=torch.float32, device="cuda")
    err = torch.full((Fn * Tn, K + 1), -7.0, dtype=torch.float32, device="cuda")
    for f0 in range(0, Fn, batch):
        r0, r1 = f0 * Tn, min(Fn, f0 + batch) * Tn
        eng.pursuit_files(x[f0:f0 + batch].contiguous(), K, tau, block, lens[f0:f0 + batch] if lens is not None else None,
                          trace=(idx[r0:r1], val[r0:r1], err[r0:r1]) if trace else None)
    torch.cuda.synchronize()
    host = block.cpu().numpy()
    return P.PursuitFrontier.from_block(host, K, tau, d, eng.n), host.tobytes(), idx.cpu().numpy(), val.cpu().numpy(), err.cpu().numpy()


def check(sae, w_op, b, x, K, batch, taus=TAUS, lengths=None, ctx="", encoder_k=None):
    """One run against the replay of its own trace; every check of cases 2 and 4.  x: numpy or torch (CPU) [F, T, d] in the dtype the
    engine sees."""
    Fn, Tn, d = x.shape
    xd = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).cuda()
    xf = xd.float().cpu().numpy().reshape(Fn * Tn, d)
    keep = counted_rows(Fn, Tn, lengths)
    pf, raw, idx, val, err = pursue(sae, xd, K, taus, batch, lengths)
    n = w_op.shape[0]
    # uncounted rows: -1 / +0.0 / 0 and nothing else
    assert (idx[~keep] == -1).all() and (val[~keep].view(np.uint32) == 0).all() and (err[~keep].view(np.uint32) == 0).all()
    assert pf.n_frames == int(keep.sum())
    rp = R.Replay(idx[keep], val[keep], w_op, xf[keep], b)
    e = err[keep]
    print(f"{ctx}: rows {keep.sum()}, picks {int((idx[keep] >= 0).sum())}, worst value err/bound "
          f"{np.nanmax(np.abs(val[keep] - rp.a64) / rp.ab):.3e}, worst e err/bound {np.max(np.abs(e - rp.E) / np.maximum(rp.Eb, 1e-300)):.3e}, "
          f"worst (best - at)/(2 eta) {np.nanmax((rp.best - rp.at) / (2 * rp.eta)):.3e}")
    assert not rp.shape_violations().any(), ctx
    assert not rp.choice_violations().any(), (ctx, np.argwhere(rp.choice_violations())[:5])
    assert not rp.stop_violations().any(), (ctx, np.nonzero(rp.stop_violations())[0][:5])
    assert not rp.value_violations().any(), (ctx, np.argwhere(rp.value_violations())[:5])
    assert not rp.err_violations(e).any(), (ctx, np.argwhere(rp.err_violations(e))[:5])
    # the block: SSE within the fold bound of the fp64 sum of trace_err, the integer fields recomputed from the trace exactly
    esum = e.astype(np.float64).sum(0)
    assert (np.abs(pf.sse - esum) <= R.fold_bound(esum)).all(), ctx
    budget, steps, picks = R.derived(idx[keep], e, SF.check_thresholds(taus), n, K)
    assert np.array_equal(pf.budget, budget) and np.array_equal(pf.steps, steps) and np.array_equal(pf.picks, picks), ctx
    # IN_SUPPORT from the engine's own collect of the same rows (every active latent of a row)
    kc = encoder_k if encoder_k is not None else min(n, E.COLLECT_MAX_K)
    cv, ci, _ = collect(sae, xd, kc, batch)
    want = np.zeros(K, np.int64)
    for r in np.nonzero(keep)[0]:
        act = set(ci[r][cv[r] > 0].tolist())
        for s in range(K):
            want[s] += int(idx[r, s] in act)
    assert np.array_equal(pf.in_support, want), (ctx, pf.in_support.tolist(), want.tolist())
    return pf, raw, (idx, val, err, keep, xf, rp)


@functools.lru_cache(maxsize=None)
def models(kind):
    if kind == "l1":
        return l1_model(512, seed=5, bias=-1.2)
    if kind == "topk":
        return topk_model(256, 512, 32, seed=31)
    d, n = {"topk96": (96, 320), "topk384": (384, 768), "topk768": (768, 1024)}[kind]
    return topk_model(d, n, 32, seed=23)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the exact case
def exact_model(d=256, n=128):
    """Scaled one-hot decoder rows with bf16-exact entries: row j = c_j e_{2 j + 1}, c_j in {1, 1.5}; row 9 is a copy of row 5.
    b_dec holds quarters."""
    g = np.random.default_rng(77)
    W = np.zeros((n, d), np.float32)
    c = np.where(g.random(n) < 0.5, np.float32(1.0), np.float32(1.5))
    W[np.arange(n), 2 * np.arange(n) + 1] = c
    W[9] = W[5]
    b = (g.integers(-8, 9, d) / 4).astype(np.float32)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=8), max_rows=1500)
    sae.load_state_dict({"W_dec": torch.from_numpy(W), "b_dec": torch.from_numpy(b), "encoder.weight": torch.from_numpy(W.copy()),
                         "encoder.bias": torch.zeros(n)})
    return sae, W, b


def test_exact_case():
    sae, W, b = exact_model()
    n, d = W.shape
    g = np.random.default_rng(78)
    rows = F * T
    amps = np.array([8, 4, 2, 1], np.float32)
    js = np.empty((rows, 4), np.int64)
    x = np.tile(b, (rows, 1))
    pool = np.array([j for j in range(n) if j not in (5, 9)])
    for r in range(rows):
        js[r] = g.permutation(pool)[:4]
        if r % 7 == 0:
            js[r, r % 4] = 5                       # (the duplicated direction, at every rank)
        x[r] = b + (amps[:, None] * W[js[r]]).sum(0)
    # pick order: the score of a planted atom is amplitude x scale -- 8, 12 > 4, 6 > 2, 3 > 1, 1.5: the planted order whatever the scales
    planted_as_9 = 3
    x[planted_as_9] = b + (amps[:, None] * W[[9, 30, 31, 32]]).sum(0)
    js[planted_as_9] = [5, 30, 31, 32]             # planted through row 9, picked as row 5: the lower index of two identical rows
    zero_row, neg_row = 11, 12
    x[zero_row] = b
    x[neg_row] = b - W[0]
    K = 6
    pf, _, idx, val, err = pursue(sae, torch.from_numpy(x.reshape(F, T, d)).cuda(), K, TAUS, 2)
    normal = np.ones(rows, bool)
    normal[[zero_row, neg_row]] = False
    assert np.array_equal(idx[normal, :4], js[normal]) and (idx[normal, 4:] == -1).all()
    assert np.array_equal(val[normal, :4], np.tile(amps, (normal.sum(), 1))) and (val[normal, 4:].view(np.uint32) == 0).all()
    assert (err[normal, 4:].view(np.uint32) == 0).all() and (err[normal, :4] > 0).all()        # e_4 == 0 to the bit, and held
    for r in (zero_row, neg_row):
        assert (idx[r] == -1).all() and (val[r].view(np.uint32) == 0).all() and (err[r] == err[r, 0]).all()
    assert err[zero_row, 0] == 0 and err[neg_row, 0] == float((W[0] ** 2).sum())
    assert pf.steps[4] == normal.sum() and pf.steps[0] == 2 and pf.steps.sum() == rows == pf.n_frames
    assert pf.picks[9] == 0 and pf.picks[5] == (js[normal] == 5).sum() and pf.picks.sum() == 4 * normal.sum()
    assert pf.sse[4] == 0 + float(err[neg_row, 0]) and pf.sse[K] == pf.sse[4]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. + 4. near-optimal choice, legitimate stops, values, norms, the block -- on every counted row
@pytest.mark.parametrize("kind,dtype,K", [("l1", "float32", 6), ("l1", "bfloat16", 1), ("topk", "float32", 32), ("topk", "bfloat16", 6)])
def test_choice_and_values(kind, dtype, K):
    sae, w_op, b = models(kind)
    x = torch.from_numpy(planted(w_op, b, 140 + K, nplant=K)).to(getattr(torch, dtype))
    pf, _, (idx, _, _, keep, _, _) = check(sae, w_op, b, x, K, batch=2, ctx=f"{kind} {dtype} K={K}", encoder_k=32 if kind == "topk" else None)
    assert (idx[keep][:, 0] >= 0).all()
    # the denominators are the frontier's own fold: bit-equal on the same files and batches
    fr, _ = frontier(sae, x.cuda(), min(K, 32), TAUS, 2)
    assert fr.sum_x.tobytes() == pf.sum_x.tobytes() and fr.sum_x_sq.tobytes() == pf.sum_x_sq.tobytes() and fr.n_frames == pf.n_frames


def test_max_K():
    """K = 256 = SAE_PURSUIT_MAX_K at n = 512: far more steps than planted atoms, so latents repeat and the error keeps falling."""
    sae, w_op, b = models("topk")
    x = planted(w_op, b, 160, files=2, nplant=6)
    pf, _, (idx, _, err, keep, _, _) = check(sae, w_op, b, x, 256, batch=2, ctx="K=256", encoder_k=32)
    assert any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in idx[keep])   # repeated picks exist


# ---------------------------------------------------------------------------------------------------------------------------
# 3. exact greedy on the rows the float64 rule decides
@pytest.mark.parametrize("kind,K,files,rows_per_file,batch", [("topk", 6, F, T, 2), ("topk96", 4, 5, 60, 5), ("topk384", 6, F, T, 2),
                                                              ("topk768", 6, F, T, 2), ("l1", 6, 16, 32, 16)])
def test_exact_greedy_on_decided_rows(kind, K, files, rows_per_file, batch):
    sae, w_op, b = models(kind)
    x = planted(w_op, b, 170 + K, files=files, rows_per_file=rows_per_file, nplant=K)
    d = x.shape[2]
    xf = x.reshape(-1, d)
    i64, v64, _, _, _ = R.greedy64(w_op, xf, b, K)
    dec = R.Replay(i64, v64, w_op, xf, b).decided()
    print(f"{kind} K={K}: decided {dec.mean():.4f} of {len(dec)} rows")
    assert dec.mean() >= R.MIN_DECIDED                                          # from the reference alone, before any comparison
    _, _, idx, val, err = pursue(sae, torch.from_numpy(x).cuda(), K, TAUS, batch)
    assert np.array_equal(idx[dec], i64[dec])
    rp = R.Replay(idx, val, w_op, xf, b)
    assert not (rp.shape_violations().any() or rp.choice_violations().any() or rp.stop_violations().any() or rp.value_violations().any()
                or rp.err_violations(err).any())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. invariance
def test_invariance():
    sae, w_op, b = models("topk")
    x = torch.from_numpy(planted(w_op, b, 180, nplant=6)).cuda()
    K = 6
    runs = {bf: pursue(sae, x, K, TAUS, bf) for bf in (1, 2, 5)}
    again = pursue(sae, x, K, TAUS, 2)
    assert again[1] == runs[2][1] and all(a.tobytes() == c.tobytes() for a, c in zip(again[2:], runs[2][2:]))     # two runs: the same bytes
    pf = runs[2][0]
    for bf in (1, 5):
        o = runs[bf]
        assert all(a.tobytes() == c.tobytes() for a, c in zip(o[2:], runs[2][2:]))                               # the trace
        for name in ("budget", "steps", "picks", "in_support"):
            assert getattr(o[0], name).tobytes() == getattr(pf, name).tobytes(), name
        assert o[0].n_frames == pf.n_frames
        assert (np.abs(o[0].sse - pf.sse) <= 2 * R.fold_bound(pf.sse)).all()
    no_trace = pursue(sae, x, K, TAUS, 2, trace=False)
    assert no_trace[1] == runs[2][1] and (no_trace[2] == -7).all()                                                # the trace is optional


def test_lengths():
    """A file shorter than T, a file of one frame, and one whose rows fill a whole 32-row unit beyond its length (T = 37 with length 5:
    rows 5 .. 36)."""
    sae, w_op, b = models("topk")
    x = planted(w_op, b, 190, nplant=6)
    L = [37, 1, 20, 50, 5]
    pf, _, _ = check(sae, w_op, b, x, 6, batch=2, lengths=L, ctx="lengths", encoder_k=32)
    assert pf.n_frames == 37 + 1 + 20 + 37 + 5


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the contract
@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_state_and_argument_rules(variant):
    n, K, Fn = 1024, 16, 4
    g = np.random.default_rng(1)
    if variant == "l1":
        a = E.SaeEngine("l1", 256, n, 1500, recon_alpha=1e2)
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
    nbytes = E.pursuit_layout(2, K, 256, n)["bytes"]
    block = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    a.pursuit_files(x, K, tau, block)
    torch.cuda.synchronize()
    assert int(block[:8].view(torch.int64)[0]) == Fn * T
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, 256, device="cuda"))):
        with pytest.raises(E.EngineError, match="pursuit frontier"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="pursuit frontier"):
            a.topk_indices_tensor(Fn * T, "cuda")
        assert np.array_equal(a.get_topk_state(), fired)
    for k_, v in a.get_params().items():
        assert v.tobytes() == before[k_].tobytes(), k_
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k_], m1[k_]) and np.array_equal(n2[k_], m2[k_]) for k_ in m1)
    # the context stays usable: a frontier pass, an evaluation (the getters are back) and a train step
    fb = torch.zeros(E.frontier_layout(2, K, 256)["bytes"], dtype=torch.uint8, device="cuda")
    a.frontier_files(x, K, tau, fb)
    a.eval(x.reshape(Fn * T, 256))
    a.latent_buffer()
    a.step(x.reshape(Fn * T, 256), 1e-3)
    torch.cuda.synchronize()
    assert int(fb[:8].view(torch.int64)[0]) == Fn * T

    # every argument error: SAE_ERR_INVALID before anything ran -- the block and the trace are untouched
    lib, vp = a._lib, C.c_void_p
    z = torch.zeros(nbytes + 8, dtype=torch.uint8, device="cuda")
    tr = [torch.zeros(Fn * T * K, dtype=torch.int32, device="cuda"), torch.zeros(Fn * T * K, dtype=torch.float32, device="cuda"),
          torch.zeros(Fn * T * (K + 1), dtype=torch.float32, device="cuda")]
    INVALID = -1                                               # include/freud_sae.h: SAE_ERR_INVALID

    def raw(xp=x.data_ptr(), n_files=Fn, rows=T, dt=E.DTYPE["float32"], K=K, taus=(0.5, 0.1), n_tau=None, flags=0, blk=z.data_ptr(),
            trace=(None, None, None)):
        arr = (C.c_float * max(len(taus), 1))(*taus)
        return lib.sae_pursuit_files(a._ctx, vp(xp), n_files, rows, dt, None, K, arr, len(taus) if n_tau is None else n_tau, flags, vp(blk),
                                     *(vp(p) for p in trace), vp(torch.cuda.current_stream().cuda_stream))

    p = [t.data_ptr() for t in tr]
    for bad in (dict(K=0), dict(K=-1), dict(K=E.PURSUIT_MAX_K + 1), dict(taus=(0.1,) * 9), dict(taus=(0.0,)), dict(taus=(1.0,)),
                dict(taus=(float("nan"),)), dict(taus=(0.5, -0.1)), dict(n_tau=-1), dict(flags=1), dict(xp=None), dict(blk=None),
                dict(blk=z.data_ptr() + 4), dict(n_files=0), dict(rows=0), dict(n_files=60), dict(dt=99),
                dict(trace=(p[0], None, None)), dict(trace=(p[0], p[1], None)), dict(trace=(None, p[1], p[2])),
                dict(trace=(p[0] + 2, p[1], p[2]))):
        assert raw(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((z == 0).all()) and all(bool((t == 0).all()) for t in tr)
    assert raw(trace=tuple(p)) == 0
    torch.cuda.synchronize()
    assert int(z[:8].view(torch.int64)[0]) == Fn * T and bool((tr[0] != 0).any())
    a.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    block = torch.zeros(E.pursuit_layout(1, 8, 256, 1024)["bytes"], dtype=torch.uint8, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.pursuit_files(torch.randn(2, 100, 256).cuda(), 8, [0.5], block)
    torch.cuda.synchronize()
    assert bool((block == 0).all())
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the Python surface
def test_module_encode_and_cli(tmp_path):
    sae, w_op, b = models("topk")
    K, k = 32, 32
    x = planted(w_op, b, 200, nplant=K)
    write_shards(str(tmp_path / "d"), "enc", x.reshape(F, -1), [T, 256])
    rng = torch.get_rng_state()
    pf = P.pursuit_frontier(sae, str(tmp_path / "d"), "enc", batch_files=2)
    assert torch.equal(torch.get_rng_state(), rng)
    assert pf.K == k and pf.thresholds.tolist() == [np.float32(t) for t in SF.DEFAULT_THRESHOLDS]            # the default K is check_K's
    xd = torch.from_numpy(x).cuda()
    direct, raw, idx, val, err = pursue(sae, xd, K, SF.DEFAULT_THRESHOLDS, 2)
    for name in ("sse", "sum_x", "sum_x_sq", "budget", "steps", "picks", "in_support"):
        assert getattr(pf, name).tobytes() == getattr(direct, name).tobytes(), name                          # the module is the engine calls

    # pursuit_encode: the trace, for a 2-D and a 3-D tensor
    i2, v2, e2 = P.pursuit_encode(sae, xd.reshape(F * T, 256), K)
    i3, v3, e3 = P.pursuit_encode(sae, xd, K)
    assert i2.shape == (F * T, K) and i3.shape == (F, T, K) and e3.shape == (F, T, K + 1) and i2.dtype == torch.int32
    for got2, got3, want in ((i2, i3, idx), (v2, v3, val), (e2, e3, err)):
        assert got2.cpu().numpy().tobytes() == want.tobytes() and got3.cpu().numpy().tobytes() == want.tobytes()

    # compare(frontier): on THIS data -- frames planted from K = k atoms of the dictionary itself, read through a tied encoder whose
    # cross-talk picks latents that raise the error (tests/test_sparsity_frontier_gpu.py) -- the greedy code is at least as good as the
    # encoder's at every budget, within the value bounds.  A property of the data chosen, asserted on this case only.
    fr = SF.sparsity_frontier(sae, str(tmp_path / "d"), "enc", K=K, batch_files=2)
    cmp_ = pf.compare(fr)
    assert cmp_.shape == (K + 1, 2) and np.array_equal(pf.amortisation_gap(fr), cmp_[:, 0] - cmp_[:, 1])
    rp = R.Replay(idx, val, w_op, x.reshape(F * T, 256), b)
    slack = (rp.Eb.sum(0) + R.fold_bound(pf.sse)) / pf.total_variance()
    print("encoder FVU", cmp_[[1, 4, 16, 32], 0], "pursuit FVU", cmp_[[1, 4, 16, 32], 1])
    assert (cmp_[:, 1] <= cmp_[:, 0] + 2 * slack).all()
    assert cmp_[0, 0] == pytest.approx(cmp_[0, 1], rel=1e-5)                                                 # budget 0: the same e_0

    # the CLI round trip
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "topk", "activation_size": 256,
                            "autoencoder_config": {"n_dict_components": 512, "k": k}}, "model": sae.state_dict()}, str(ck))
    fr.to_npz(str(tmp_path / "f.npz"))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.pursuit", "--sae", str(ck), "--data_path", str(tmp_path / "d"), "--layer_name", "enc",
                        "--K", str(K), "--batch_files", "2", "--frontier", str(tmp_path / "f.npz"), "--out", str(tmp_path / "p.npz")],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["K"] == K and out["n_frames"] == F * T and out["fvu"] == pf.summary()["fvu"] and "amortisation_gap" in out
    back = P.PursuitFrontier.load(str(tmp_path / "p.npz"))
    assert back.sse.tobytes() == pf.sse.tobytes() and back.picks.tobytes() == pf.picks.tobytes() and back.K == K
