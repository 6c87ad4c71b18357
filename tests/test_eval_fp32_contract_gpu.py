"""The contract and the edges of the fp32 evaluation forward (sae_set_eval_precision(SAE_PREC_FP32); freud_amd/csrc/eval_fp32.h):

  A  what the context answers after an fp32 evaluation (the bf16 forward's getters refuse, the rest stays valid), that a bf16
     evaluation afterwards is the one a fresh context runs, and the row limit;
  B  the smallest L1 shape past the former fixed cap of 16 384 latent partial sums;
  C  the selection edges of the fp32 TopK forward -- exact ties at the boundary (lowest column first), ties across 256-column
     chunks and waves, fewer than k positive entries, a ragged last chunk -- against a float64 forward written out below;
  D  fp32 evaluations between training steps: the training state is the one the bf16 evaluation (L1) / no evaluation at all
     (TopK) leaves, bit for bit.

The references here are plain float64 (numpy / torch on the CPU); the tolerances are the project's for this path (1e-4 on the
losses, 1e-4 / 1e-6 on the per-feature maxima: tests/test_eval_fp32_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import sae_oracle as O

pytestmark = pytest.mark.gpu

TOPK_KEYS = ("encoder.weight", "encoder.bias", "W_dec", "b_dec")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# ---- float64 references -------------------------------------------------------------------------------------------------
def l1_ref64(x, W, b, alpha):
    """L1AutoEncoder.forward (l1autoencoder.py:69-95) in float64 on weights that are already column-normalised."""
    x, W, b = (torch.as_tensor(np.asarray(t)).double() for t in (x, W, b))
    c = torch.relu(x @ W + b)
    e2 = (c @ W.t() - x) ** 2
    keep = x != -1.0
    return {"recon": alpha * float(e2[keep].sum() / keep.sum()), "l1": float(c.sum(1).mean()), "mse": float(e2.mean()),
            "count": float(keep.sum()), "colmax": c.max(0).values.numpy()}


def topk_pre64(x, P, src=None):
    """relu((x - b_dec) W_enc^T + b_enc) in float64, and the same before the ReLU.  src: column j of the model is a copy of the
    unique column src[j] -- those are computed once and gathered, so that copies are equal to the last bit."""
    x = torch.as_tensor(np.asarray(x)).double().reshape(-1, P["b_dec"].shape[0])
    We, be = torch.as_tensor(np.asarray(P["encoder.weight"])).double(), torch.as_tensor(np.asarray(P["encoder.bias"])).double()
    s_in = x - torch.as_tensor(np.asarray(P["b_dec"])).double()
    if src is None:
        z = s_in @ We.t() + be
    else:
        src = torch.as_tensor(np.asarray(src))
        uniq = torch.unique(src)
        first = torch.full((int(uniq.max()) + 1,), -1, dtype=torch.long)
        for j in reversed(range(len(src))):                # the lowest column holding each unique latent
            first[src[j]] = j
        assert torch.equal(We[first[src]], We) and torch.equal(be[first[src]], be)        # the copies ARE copies
        zu = s_in @ We[first[uniq]].t() + be[first[uniq]]
        pos = torch.zeros(int(uniq.max()) + 1, dtype=torch.long)
        pos[uniq] = torch.arange(len(uniq))
        z = zu[:, pos[src]]
    return torch.relu(z), z


def topk_ref64(x3, P, k, multi, src=None):
    """TopKAutoEncoder.forward (topkautoencoder.py:72-151) without a dead mask in float64; equal values are taken lowest column
    first (a stable descending sort).  x3: [B][T][d]."""
    B, T, d = x3.shape
    x = torch.as_tensor(np.asarray(x3)).double().reshape(B * T, d)
    Wd, bd = torch.as_tensor(np.asarray(P["W_dec"])).double(), torch.as_tensor(np.asarray(P["b_dec"])).double()
    pre, z = topk_pre64(x, P, src)
    order = torch.sort(pre, dim=1, descending=True, stable=True).indices
    x3d = x.reshape(B, T, d)
    tv = float(((x3d - x3d.mean(0)) ** 2).sum())
    tv = 1.0 if tv == 0.0 else tv

    def run(kk):
        dense = torch.zeros_like(pre).scatter_(1, order[:, :kk], torch.gather(pre, 1, order[:, :kk]))
        e2 = float(((dense @ Wd + bd - x) ** 2).sum())
        return dense, e2

    dense, e2 = run(k)
    out = {"fvu": e2 / tv, "mse": e2 / x.numel(), "multi": 0.0, "pre": pre, "z": z, "dense": dense}
    if multi:
        dense, e2m = run(4 * k)
        out["multi"] = e2m / tv
        out["dense"] = dense
    out["colmax"] = out["dense"].max(0).values.numpy()
    return out


def assert_boundary_gaps(pre, z, kk, tol=1e-4):
    """The condition on the inputs (not a tolerance): at every row's selection boundary the fp32 forward must see the order the
    float64 one sees.  Equal values there are equal in both (copied latents); DISTINCT values next to the boundary must be more
    than `tol` apart relatively.  Rows with fewer than kk positive entries select every positive entry: there no entry may
    sit within 1e-3 of the ReLU's kink, unless it is exactly on it."""
    s = torch.sort(pre, dim=1, descending=True).values
    for r in range(pre.shape[0]):
        hi, lo = float(s[r, kk - 1]), float(s[r, kk])
        row = s[r]
        if hi != lo:
            assert hi - lo > tol * hi, (r, kk, hi, lo)
        else:
            above, below = row[row > hi], row[row < hi]
            if len(above):
                assert float(above.min()) - hi > tol * float(above.min()), (r, kk, "above the tied value")
            if len(below) and hi > 0:
                assert hi - float(below.max()) > tol * hi, (r, kk, "below the tied value")
        if int((pre[r] > 0).sum()) <= kk:
            zr = z[r]
            near = (zr.abs() < 1e-3) & (zr != 0)
            assert not bool(near.any()), (r, kk, "an entry within 1e-3 of zero")


def check_topk_eval(eng, x3, P, k, multi, src=None):
    """fp32 eval of x3 against topk_ref64: the input condition, the losses at 1e-4, the maxima at 1e-4 / 1e-6 and their zero
    pattern.  Returns the reference."""
    ref = topk_ref64(x3, P, k, multi, src)
    assert_boundary_gaps(ref["pre"], ref["z"], k)
    if multi:
        assert_boundary_gaps(ref["pre"], ref["z"], 4 * k)
    M, n = ref["pre"].shape
    met = torch.zeros(8, device="cuda")
    cmx = torch.full((n,), -1.0, device="cuda")
    eng.set_eval_precision("fp32")
    eng.eval_into(x3.cuda(), met, cmx)
    m, cm = met.cpu().numpy(), cmx.cpu().numpy()
    print("\nfvu %.8g ref %.8g | mse %.8g ref %.8g | multi %.8g ref %.8g | max colmax err %.3g | zero pattern differs in %d columns"
          % (m[0], ref["fvu"], m[2], ref["mse"], m[6], ref["multi"], np.abs(cm - ref["colmax"]).max(), ((cm == 0) != (ref["colmax"] == 0)).sum()))
    assert m[0] == pytest.approx(ref["fvu"], rel=1e-4)
    assert m[1] == 0.0
    assert m[2] == pytest.approx(ref["mse"], rel=1e-4)
    assert m[6] == (pytest.approx(ref["multi"], rel=1e-4) if multi else 0.0)
    assert np.array_equal(cm == 0, ref["colmax"] == 0), np.nonzero((cm == 0) != (ref["colmax"] == 0))[0]
    np.testing.assert_allclose(cm, ref["colmax"], rtol=1e-4, atol=1e-6)
    np.testing.assert_array_equal(eng.latent_colmax(), cm)
    return ref


def check_l1_eval(eng, x, alpha, m=None, cm=None):
    """metrics() / latent_colmax() of the fp32 evaluation just run against the float64 forward on the weights the engine holds
    right after it (the in-place normalisation has happened: they are the weights it multiplied by)."""
    p = eng.get_params()
    ref = l1_ref64(x.float().cpu().numpy(), p["decoder.weight"], p["encoder_bias"], alpha)
    m = eng.metrics() if m is None else m
    cm = eng.latent_colmax() if cm is None else cm
    print("\nrecon %.8g ref %.8g | l1 %.8g ref %.8g | mse %.8g ref %.8g | count %.0f ref %.0f | max colmax err %.3g"
          % (m[0], ref["recon"], m[1], ref["l1"], m[2], ref["mse"], m[4], ref["count"], np.abs(cm - ref["colmax"]).max()))
    assert m[0] == pytest.approx(ref["recon"], rel=1e-4)
    assert m[1] == pytest.approx(ref["l1"], rel=1e-4)
    assert m[2] == pytest.approx(ref["mse"], rel=1e-4)
    assert m[4] == pytest.approx(ref["count"], rel=1e-4)
    np.testing.assert_allclose(cm, ref["colmax"], rtol=1e-4, atol=1e-6)
    return p


# ---- models and data ------------------------------------------------------------------------------------------------------
def _l1_data(M, d, g, masked=30, rank=64):
    x = (torch.relu(torch.randn(M, rank, generator=g)) * 0.1) @ torch.randn(rank, d, generator=g)
    if masked:
        x.view(-1)[torch.randint(0, x.numel(), (masked,), generator=g)] = -1.0
    return x


def _l1_model(d, n, g):
    return {"decoder.weight": (torch.randn(d, n, generator=g) / d ** 0.5).numpy(), "encoder_bias": (0.01 * torch.randn(n, generator=g)).numpy()}


def _topk_model(d, n, g):
    We = torch.randn(n, d, generator=g) / d ** 0.5
    Wd = torch.randn(n, d, generator=g)
    Wd /= Wd.norm(dim=1, keepdim=True)
    return {"encoder.weight": We, "encoder.bias": 0.01 * torch.randn(n, generator=g), "W_dec": Wd, "b_dec": 0.01 * torch.randn(d, generator=g)}


def _topk_data(M, d, g):
    return torch.relu(torch.randn(M, 48, generator=g)) @ torch.randn(48, d, generator=g) * 0.2


def _make(kind, seed, max_rows=256):
    from freud_amd.engine import SaeEngine
    g = torch.Generator().manual_seed(seed)
    if kind == "l1":
        d, n = 64, 256
        eng = SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=max_rows, optimizer="adam", recon_alpha=1e4)
        P = _l1_model(d, n, g)
    else:
        d, n = 128, 512
        eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=max_rows, optimizer="adam", k=8, auxk_alpha=0.03125,
                        multi_topk=kind == "topk_multi")
        eng.set_topk_options(1e6, max_rows)
        P = {kk: v.numpy() for kk, v in _topk_model(d, n, g).items()}
    eng.set_params(P)
    return eng, P, d, n, g


def _data(kind, M, d, g):
    return _l1_data(M, d, g) if kind == "l1" else _topk_data(M, d, g)


def _check_fp32_eval(kind, eng, x):
    if kind == "l1":
        check_l1_eval(eng, x, 1e4)
    else:
        P = {kk: torch.tensor(v) for kk, v in eng.get_params().items()}
        ref = topk_ref64(x[None], P, 8, kind == "topk_multi")
        assert_boundary_gaps(ref["pre"], ref["z"], 8)
        if kind == "topk_multi":
            assert_boundary_gaps(ref["pre"], ref["z"], 32)
        m = eng.metrics()
        assert m[0] == pytest.approx(ref["fvu"], rel=1e-4) and m[2] == pytest.approx(ref["mse"], rel=1e-4)
        assert m[6] == (pytest.approx(ref["multi"], rel=1e-4) if kind == "topk_multi" else 0.0)
        np.testing.assert_allclose(eng.latent_colmax(), ref["colmax"], rtol=1e-4, atol=1e-6)


def _bf16_getters(kind, eng, M, n):
    """Everything a bf16 forward leaves, as host arrays."""
    torch.cuda.synchronize()
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}

    out = {"latent": torch.as_tensor(_Alias(), device="cuda")[:, :n].cpu().numpy().copy(), "colmax": eng.latent_colmax(), "metrics": eng.metrics()}
    if kind != "l1":
        out["indices"] = eng.topk_indices_tensor(M, "cuda").cpu().numpy().copy()
    if kind == "topk_multi":
        dense, idx = eng.multi_topk_buffers(M, "cuda")
        out["multi_dense"], out["multi_indices"] = dense.view(torch.int16).cpu().numpy().copy(), idx.cpu().numpy().copy()
    return out


# ---- A: the state after an fp32 evaluation -----------------------------------------------------------------------------------
STATE_SEED = {"l1": 3, "topk": 3, "topk_multi": 4}
LIMIT_SEED = {"l1": 3, "topk": 4, "topk_multi": 7}


@pytest.mark.parametrize("kind", ["l1", "topk", "topk_multi"])
def test_after_an_fp32_eval_the_bf16_getters_refuse_and_a_bf16_eval_is_a_fresh_one(kind):
    from freud_amd.engine import EngineError
    # (seeds: the first from 3 on for which the 100 / 256 rows of the fp32 evaluation keep the gap that assert_boundary_gaps asks for)
    eng, P, d, n, g = _make(kind, STATE_SEED[kind])
    x1, x2 = _data(kind, 256, d, g).cuda(), _data(kind, 100, d, g).cuda()
    eng.forward_backward(x1)
    ngrad = n * d + n if kind == "l1" else 2 * n * d + n + d
    grads = eng.debug_read(2, ngrad)
    eng.set_eval_precision("fp32")
    eng.eval(x2)
    refusing = [eng.latent_buffer, lambda: eng.debug_read(0, 256 * n), lambda: eng.debug_read(1, 256 * d), lambda: eng.debug_read(8, 256 * d),
                lambda: eng.debug_read(9, 256 * n)]
    if kind != "l1":
        refusing += [lambda: eng.topk_indices_tensor(100, "cuda"), lambda: eng.debug_read(3, 256 * 8)]
    if kind == "topk_multi":
        refusing += [lambda: eng.multi_topk_buffers(100, "cuda")]
    for call in refusing:
        with pytest.raises(EngineError, match="fp32"):
            call()
    # what stays valid: the fp32 forward's own metrics and maxima, the gradients of the training forward, the state, decode()
    _check_fp32_eval(kind, eng, x2.cpu())
    assert np.array_equal(eng.debug_read(2, ngrad), grads)
    step, m1, _ = eng.get_opt_state()
    assert step == 0 and all(not v.any() for v in m1.values())
    if kind != "l1":
        assert eng.get_topk_state().shape == (n,)
    p = eng.get_params()
    lat = torch.relu(torch.randn(100, n, generator=g))
    xh = torch.empty(100, d, device="cuda")
    eng.decode(lat.cuda(), xh)
    torch.cuda.synchronize()
    want = lat.double() @ torch.tensor(p["decoder.weight"]).double().t() if kind == "l1" else \
        lat.double() @ torch.tensor(p["W_dec"]).double() + torch.tensor(p["b_dec"]).double()
    assert _rel(xh.cpu().numpy(), want.numpy()) < 1e-2
    with pytest.raises(EngineError, match="fp32"):          # (decode() is no forward: the getters still refuse)
        eng.latent_buffer()
    # a bf16 evaluation brings every getter back, bitwise as in a context that ran nothing else
    eng.set_eval_precision("bf16")
    eng.eval(x1)
    got = _bf16_getters(kind, eng, 256, n)
    fresh, _, _, _, _ = _make(kind, STATE_SEED[kind])
    fresh.set_params(p)
    fresh.eval(x1)
    want = _bf16_getters(kind, fresh, 256, n)
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    eng.close()
    fresh.close()


@pytest.mark.parametrize("kind", ["l1", "topk", "topk_multi"])
def test_fp32_eval_obeys_the_row_limit(kind):
    """More rows than max_rows: refused like every other forward, before anything is allocated or enqueued; the context then
    still evaluates max_rows rows correctly.  (No getter is called after the refused call.)"""
    from freud_amd.engine import EngineError
    eng, P, d, n, g = _make(kind, LIMIT_SEED[kind])
    xs = _data(kind, 320, d, g)
    eng.set_eval_precision("fp32")
    with pytest.raises(EngineError, match="max_rows"):
        eng.eval(xs.cuda())
    x = xs[:256].contiguous()
    eng.eval(x.cuda())
    _check_fp32_eval(kind, eng, x)
    eng.close()


# ---- B: past the former cap of the latent partial sums -----------------------------------------------------------------------
def test_fp32_eval_l1_past_16384_partial_sums():
    """d = 64, n = 16 384, M = 16 448: 64 column blocks x 257 row blocks = 16 448 partial sums of the latent, the smallest shape
    past the 16 384 the buffer once held (such a shape was refused after the first GEMM was enqueued)."""
    from freud_amd.engine import SaeEngine
    d, n, M = 64, 16384, 16448
    g = torch.Generator().manual_seed(d + n)
    P = _l1_model(d, n, g)
    x = _l1_data(M, d, g)
    eng = SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=M, optimizer="adam", recon_alpha=1e4)
    eng.set_params(P)
    eng.set_eval_precision("fp32")
    met = torch.zeros(8, device="cuda")
    cmx = torch.zeros(n, device="cuda")
    eng.eval_into(x.cuda(), met, cmx)
    torch.cuda.synchronize()
    check_l1_eval(eng, x, 1e4, met.cpu().numpy(), cmx.cpu().numpy())
    eng.close()


# ---- C: selection edges ----------------------------------------------------------------------------------------------------
def _topk_engine(d, n, k, M, T, multi, P):
    from freud_amd.engine import SaeEngine
    eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=M, optimizer="adam", k=k, auxk_alpha=0.03125, multi_topk=multi)
    eng.set_topk_options(1e6, T)
    eng.set_params({kk: np.ascontiguousarray(v.numpy()) for kk, v in P.items()})
    return eng


SEED_A = 0


def case_a(seed=SEED_A):
    """n = 1000 = 2 x 500: every latent twice (encoder row and bias; the decoder rows differ, so the loss sees which copy was
    taken), at random columns.  k = 7: the 7th and 8th largest of every row are the two copies of one latent."""
    d, n, M = 128, 1000, 96
    g = torch.Generator().manual_seed(seed)
    P = _topk_model(d, n, g)
    src = torch.cat([torch.arange(500), torch.arange(500)])[torch.randperm(n, generator=g)]
    first = torch.full((500,), -1, dtype=torch.long)
    for j in reversed(range(n)):
        first[src[j]] = j
    P["encoder.weight"] = P["encoder.weight"][first[src]].contiguous()
    P["encoder.bias"] = P["encoder.bias"][first[src]].contiguous()
    x3 = _topk_data(M, d, g).reshape(2, 48, d)
    return P, src, x3


def test_fp32_topk_boundary_tie_in_every_row():
    d, n, k, M = 128, 1000, 7, 96
    P, src, x3 = case_a()
    eng = _topk_engine(d, n, k, M, 48, True, P)
    ref = check_topk_eval(eng, x3, P, k, True, src)
    s = torch.sort(ref["pre"], dim=1, descending=True).values
    assert bool((s[:, k - 1] == s[:, k]).all()) and bool((s[:, k - 1] > 0).all())       # the boundary splits a pair in every row
    assert bool((s[:, 4 * k - 1] != s[:, 4 * k]).all())
    eng.close()


def case_b():
    """n = 1000, k = 8.  Latents on orthonormal directions, so every row's pre-activations are set by hand: six `strong` latents,
    a pair A at columns 63 / 64 (a wave boundary), a pair B at 255 / 256 (a chunk boundary), a value five times at columns 250,
    300, 383, 384, 520 (three chunks; 383 / 384 is a wave boundary), and a background far below all of them.  Rows of kind
    0: 7 strong values above pair A -> column 63 only;  1: the same with pair B -> column 255 only;  2..5: 7, 6, 5, 4 values above
    the five-fold one -> its first 1, 2, 3, 4 columns.  The five-fold value differs from row kind to row kind, largest where one
    column is taken: the per-feature maxima then say which kind of row took which column, and columns 64, 256 and 520 stay 0."""
    d, n, k, M = 128, 1000, 8, 96
    g = torch.Generator().manual_seed(1)
    Q, _ = torch.linalg.qr(torch.randn(d, d, generator=g))
    strong, A, B, F = [5, 100, 200, 400, 600, 700, 999], [63, 64], [255, 256], [250, 300, 383, 384, 520]
    We = 0.02 * torch.randn(n, d, generator=g)            # the background: |pre| of a few 1e-2
    for i, j in enumerate(strong):
        We[j] = Q[:, i]
    for j in A:
        We[j] = Q[:, 7]
    for j in B:
        We[j] = Q[:, 8]
    for j in F:
        We[j] = Q[:, 9]
    Wd = torch.randn(n, d, generator=g)
    Wd /= Wd.norm(dim=1, keepdim=True)
    P = {"encoder.weight": We, "encoder.bias": torch.zeros(n), "W_dec": Wd, "b_dec": 0.01 * torch.randn(d, generator=g)}
    coef = torch.zeros(M, 10)
    for r in range(M):
        kind = r % 6
        above = [7, 7, 7, 6, 5, 4][kind]
        coef[r, :above] = 2.0 + 0.1 * torch.arange(above) + 0.01 * torch.rand(1, generator=g)
        coef[r, 7 + min(kind, 2)] = 1.0 + 0.05 * (6 - kind) + 0.01 * torch.rand(1, generator=g)
    x = coef @ Q[:, :10].t() + P["b_dec"] + 0.01 * torch.randn(M, d, generator=g)
    src = torch.arange(n)
    src[64], src[256] = 63, 255
    src[torch.tensor(F)] = 250
    return P, src, x.reshape(2, 48, d), (strong, A, B, F)


def test_fp32_topk_ties_across_chunks_and_waves():
    d, n, k, M = 128, 1000, 8, 96
    P, src, x3, (strong, A, B, F) = case_b()
    eng = _topk_engine(d, n, k, M, 48, False, P)
    ref = check_topk_eval(eng, x3, P, k, False, src)
    # the fixture is what its description says: which columns the reference took in each kind of row
    taken = ref["dense"] > 0
    for r in range(M):
        kind = r % 6
        want = strong[:[7, 7, 7, 6, 5, 4][kind]] + ([63] if kind == 0 else [255] if kind == 1 else F[:kind - 1])
        assert sorted(torch.nonzero(taken[r]).flatten().tolist()) == sorted(want), r
    cm = ref["colmax"]
    assert cm[64] == 0 and cm[256] == 0 and cm[520] == 0 and cm[250] > cm[300] > cm[383] > cm[384] > 0
    eng.close()


@pytest.mark.parametrize("live", [5, 8])
def test_fp32_topk_fewer_than_k_positive_entries(live):
    """k = 8, b_enc = -100 on all but `live` latents (0 there).  live = 5: no row has k positive entries -- the selection keeps
    the positive ones only.  live = 8: row 1 is b_dec plus the sum of the eight live encoder rows: exactly k positive entries.
    Row 0 is b_dec itself in both: nothing is positive."""
    d, n, k, M = 128, 1000, 8, 96
    g = torch.Generator().manual_seed(20 + live)
    P = _topk_model(d, n, g)
    P["encoder.weight"] = P["encoder.weight"] * d ** 0.5 / 4          # rows of norm ~ 2.8: live pre-activations of order 1
    cols = torch.tensor([3, 255, 256, 700, 999, 64, 511, 512][:live])
    P["encoder.bias"] = torch.full((n,), -100.0)
    P["encoder.bias"][cols] = 0.0
    x = _topk_data(M, d, g)
    x[0] = P["b_dec"]
    if live == 8:
        x[1] = P["b_dec"] + P["encoder.weight"][cols].sum(0) / 8
    x3 = x.reshape(2, 48, d)
    for multi in (False, True):
        eng = _topk_engine(d, n, k, M, 48, multi, P)
        ref = check_topk_eval(eng, x3, P, k, multi)
        eng.close()
    npos = (ref["pre"] > 0).sum(1)
    assert int(npos[0]) == 0 and int(npos.max()) <= live and int(npos[2:].min()) < k and int(npos.max()) >= 3
    if live == 8:
        assert int(npos[1]) == k
    assert set(np.nonzero(ref["colmax"])[0].tolist()) <= set(cols.tolist())


def test_fp32_topk_maxima_in_the_ragged_last_chunk():
    """n = 1000: columns 768 .. 999 are the last, ragged 256-column chunk.  A bias of +1 on columns 900 .. 999 puts most of the
    selection (k and 4k) there; the reference says so.  (Seed: the first from 4 on that keeps the gap assert_boundary_gaps asks for
    and whose reference takes the very last column at k as well as at 4k.)"""
    d, n, k, M = 128, 1000, 8, 96
    g = torch.Generator().manual_seed(17)
    P = _topk_model(d, n, g)
    P["encoder.bias"][900:] += 1.0
    x3 = _topk_data(M, d, g).reshape(2, 48, d)
    for multi in (False, True):
        eng = _topk_engine(d, n, k, M, 48, multi, P)
        ref = check_topk_eval(eng, x3, P, k, multi)
        eng.close()
        sel = ref["dense"] > 0
        assert float(sel[:, 768:].sum()) > 0.5 * float(sel.sum()) and bool(sel[:, 990:].any()) and ref["colmax"][999] > 0


# ---- D: fp32 evaluations between training steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,M", [(64, 256, 512), (384, 1024, 512), (512, 1024, 768)])
def test_fp32_eval_between_l1_steps_leaves_the_bf16_evals_training_state(d, n, M):
    """step, step, eval(xv), eval(xv), step, step.  Every forward of the reference normalises the master in place, so the two
    evaluations matter to the run -- and in the same way whichever arithmetic they use: parameters and both moments are bitwise
    those of the run with bf16 evaluations (d <= 384: the folded weight preparation, prep_weights_l1 followed by
    settle_weights in the fp32 path)."""
    from freud_amd.engine import SaeEngine
    g = torch.Generator().manual_seed(d + 1)
    W0 = torch.empty(d, n)
    torch.nn.init.orthogonal_(W0, generator=g)
    b0 = 0.01 * torch.randn(n, generator=g)
    x = _l1_data(M, d, g, masked=0, rank=16)
    xv = _l1_data(M, d, g, masked=30, rank=16)
    lr, alpha = 1e-3, 1e4

    def run(prec):
        eng = SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=M, optimizer="adam", recon_alpha=alpha)
        eng.set_params({"decoder.weight": W0.numpy(), "encoder_bias": b0.numpy()})
        eng.set_eval_precision(prec)
        xd, xvd = x.cuda(), xv.cuda()
        eng.step(xd, lr)
        eng.step(xd, lr)
        for _ in range(2):
            eng.eval(xvd)
            if prec == "fp32":
                p = check_l1_eval(eng, xv, alpha)
                assert np.abs(np.linalg.norm(p["decoder.weight"], axis=0) - 1).max() < 1e-5
        eng.step(xd, lr)
        eng.step(xd, lr)
        p = eng.get_params()
        _, m1, v1 = eng.get_opt_state()
        eng.close()
        return [p["decoder.weight"], p["encoder_bias"], m1["decoder.weight"], m1["encoder_bias"], v1["decoder.weight"], v1["encoder_bias"]]

    a, o = run("fp32"), run("bf16")
    for i, (u, v) in enumerate(zip(a, o)):
        assert np.array_equal(u, v), (i, np.abs(u - v).max())
    # and the run is the reference's: the oracle's steps with the two in-place normalisations at the evaluation points
    W, b, st = W0.clone(), b0.clone(), O.OptState()
    for i in range(4):
        if i == 2:
            W.copy_(O.normalize_columns(O.normalize_columns(W)))
        O.l1_train_step(x, W, b, st, recon_alpha=alpha, lr=lr, clip_thresh=1.0, optimizer="adam")
    print("\nfinal W rel-L2 to the oracle %.3g, b %.3g" % (_rel(a[0], W.numpy()), _rel(a[1], b.numpy())))
    assert _rel(a[0], W.numpy()) < 1e-3


def test_fp32_eval_between_topk_steps_does_not_touch_the_training_state():
    """TopK with AuxK and a dead threshold of 600 frames (latents that did not fire in steps 1 and 2 are dead from step 3 on):
    step, step, eval(xv), eval(xv), step, step leaves parameters, moments and num_frames_since_fired bitwise as the four steps
    alone do.  The validation batch is 32 rows, and the seed is the one of 9 .. 99 whose rows keep the widest gap at the selection
    boundary (1.6e-3) on the oracle's weights after two steps; the condition itself is asserted on the engine's weights."""
    from freud_amd.engine import SaeEngine
    d, n, k, M = 256, 1024, 16, 512
    g = torch.Generator().manual_seed(97)
    P = _topk_model(d, n, g)
    P["W_dec"] = P["encoder.weight"] / P["encoder.weight"].norm(dim=1, keepdim=True)
    x, xv = _topk_data(M, d, g), _topk_data(32, d, g)

    def run(evals):
        eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=M, optimizer="adam", k=k, auxk_alpha=0.03125)
        eng.set_topk_options(600.0, M)
        eng.set_params({kk: v.numpy() for kk, v in P.items()})
        eng.set_eval_precision("fp32")
        xd, xvd = x.cuda(), xv.cuda()
        dead = []
        for i in range(4):
            if i == 2 and evals:
                for _ in range(2):
                    eng.eval(xvd)
                    Pn = {kk: torch.tensor(v) for kk, v in eng.get_params().items()}
                    ref = topk_ref64(xv[None], Pn, k, False)
                    assert_boundary_gaps(ref["pre"], ref["z"], k)
                    m = eng.metrics()
                    print("\nfvu %.8g ref %.8g | mse %.8g ref %.8g" % (m[0], ref["fvu"], m[2], ref["mse"]))
                    assert m[0] == pytest.approx(ref["fvu"], rel=1e-4) and m[2] == pytest.approx(ref["mse"], rel=1e-4)
                    np.testing.assert_allclose(eng.latent_colmax(), ref["colmax"], rtol=1e-4, atol=1e-6)
            dead.append(int((eng.get_topk_state() > 600).sum()))
            eng.step(xd, 1e-3)
        p = eng.get_params()
        _, m1, v1 = eng.get_opt_state()
        out = [p[kk] for kk in TOPK_KEYS] + [m1[kk] for kk in TOPK_KEYS] + [v1[kk] for kk in TOPK_KEYS] + [eng.get_topk_state()]
        eng.close()
        return out, dead

    (a, dead), (o, _) = run(True), run(False)
    assert dead[2] > 0 and dead[3] > 0, dead            # the AuxK pass ran in steps 3 and 4
    for i, (u, v) in enumerate(zip(a, o)):
        assert np.array_equal(u, v), (i, np.abs(u.astype(np.float64) - v).max())
