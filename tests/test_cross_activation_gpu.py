"""GPU: the cross-activation (freud_amd/cross_activation.py over include/freud_sae.h's sae_cross_mask_files / sae_cross_update /
sae_cross_keys).

The reference is the engine's own encode() per file, the method of tests/test_coactivation_gpu.py with its weight recipes:
threshold at > 0, then Za[:len - l].T @ Zb[l:len] in float64 on the device (0/1 operands and sums below 2^53 are exact), summed over
the files as int64; a column of ones on either side gives the margins out of the same product.  Tables and margins must be EQUAL;
the partner tables must equal the numpy restatement of tests/cross_activation_reference.py (lexsort by score descending, count
descending, partner ascending; score = (num.astype(f8) / den.astype(f8)).astype(f4)) exactly, for all four measures in both
orientations.

Which shapes reach which update path (coact.h's K split: the fewest K ranges that give 1024 workgroups).  The small shapes -- 3 x 2
tiles (n_a = 300, n_b = 200), 3 x 33 tiles against the TopK dictionary -- have far fewer than 1024 tiles: with batch_files = 3 or 7
(150 or 350 rows: 2 or 3 K steps) K is split and the tiles are added with integer atomics; with batch_files = 1 (50 rows: one K
step) one range is left and the plain read-modify-write runs.  The device-only shape, 33 x 129 = 4257 tiles over 47 K steps, runs
unsplit on the plain path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import coactivation as CO
from freud_amd import cross_activation as CX
from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd.loader import write_shards
from tests import cross_activation_reference as REF
from tests.test_coactivation_gpu import dense_latent, l1_model, l1_weights, shards, topk_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

D, NA, NB, T, F = 256, 300, 200, 50, 7
ARRAYS = CX._FIELDS + ("tables",)


def active(sae, x):
    """bool CUDA [F, T, n]: encode() of every file, thresholded at > 0."""
    return torch.stack([dense_latent(sae, torch.from_numpy(np.ascontiguousarray(x[f])).cuda()) > 0 for f in range(x.shape[0])])


def ref_table(Za, Zb, lengths, lag):
    """[(n_a + 1), (n_b + 1)] int64: per file Za[:len - l].T @ Zb[l:len] in float64 on the device, a column of ones on either side."""
    out = torch.zeros(Za.shape[2] + 1, Zb.shape[2] + 1, dtype=torch.int64, device="cuda")
    for f in range(Za.shape[0]):
        n = int(lengths[f])
        if n - lag <= 0:
            continue
        ones = torch.ones(n - lag, 1, dtype=torch.float64, device="cuda")
        A = torch.cat([Za[f, :n - lag].double(), ones], 1)
        B = torch.cat([Zb[f, lag:n].double(), ones], 1)
        out += (A.T @ B).to(torch.int64)
    return out.cpu().numpy()


def check_lag(cx, l, want):
    X, fa, fb, n_pairs = REF.split(want)
    assert cx.tables.dtype == np.int32
    np.testing.assert_array_equal(cx.tables[l].astype(np.int64), X)
    np.testing.assert_array_equal(cx.fire_a[l], fa)
    np.testing.assert_array_equal(cx.fire_b[l], fb)
    assert int(cx.n_pairs[l]) == n_pairs
    assert cx.fire_a.dtype == cx.fire_b.dtype == cx.n_pairs.dtype == np.int64


def check_partners(cx, l, want, measure, K, excl):
    for by_b, got in ((0, (cx.partners_a, cx.counts_a, cx.scores_a)), (1, (cx.partners_b, cx.counts_b, cx.scores_b))):
        nb, cn, sc = REF.partners(want, measure, K, by_b, excl)
        np.testing.assert_array_equal(got[0][l], nb)
        np.testing.assert_array_equal(got[1][l], cn)
        assert got[2].dtype == np.float32 and got[2][l].tobytes() == sc.tobytes()
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64


def same_arrays(a, b):
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """d = 256, n_a = 300 and n_b = 200 (n + 1 no multiple of 128: 3 tile rows, 2 tile columns), T = 50, F = 7 in batches of 3:
    150 rows per call (no multiple of the K step), the last batch partial; random lengths with two full files, each followed by
    another file.  The masks of both dictionaries, computed once."""
    g = np.random.default_rng(7)
    x = g.normal(0, 1, (F, T, D)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = L[3] = T
    a, b = l1_model(D, NA, seed=5), l1_model(D, NB, seed=6)
    path = shards(tmp_path_factory.mktemp("cxsmall"), x)
    return {"a": a, "b": b, "x": x, "L": L, "path": path, "Za": active(a, x), "Zb": active(b, x)}


def test_self_lag_0_is_the_coactivation_table(small):
    s = small
    cx = CX.cross_activation(s["a"], s["path"], "enc", lags=(0,), lengths=s["L"], batch_files=3, return_counts=True)
    co = CO.feature_coactivation(s["a"], s["path"], "enc", lengths=s["L"], batch_files=3, return_counts=True)
    st = FST.feature_stats(s["a"], s["path"], "enc", lengths=s["L"], batch_files=3)
    assert cx.tables.shape == (1, NA, NA) and cx.tables[0].tobytes() == co.matrix.tobytes()
    np.testing.assert_array_equal(cx.fire_a[0], st.fire_count)
    np.testing.assert_array_equal(cx.fire_b[0], st.fire_count)
    assert int(cx.n_pairs[0]) == st.n_frames == int(s["L"].sum())
    assert cx.same_dictionary and cx.measure == "jaccard"
    # the latent itself is no partner at lag 0; the jaccard partners are those of the co-activation pass
    assert not (cx.partners_a[0] == np.arange(NA)[:, None]).any() and not (cx.partners_b[0] == np.arange(NA)[:, None]).any()
    for got in (cx.partners_a[0], cx.partners_b[0]):
        np.testing.assert_array_equal(got, co.neighbors)
    assert cx.scores_a[0].tobytes() == co.scores.tobytes()
    check_lag(cx, 0, ref_table(s["Za"], s["Za"], s["L"], 0))


def test_self_lags(small):
    s = small
    Za, L = s["Za"], s["L"]
    lags = (1, 3, T - 1, T)
    want = [ref_table(Za, Za, L, l) for l in lags]
    # from the reference alone: file boundaries matter, lengths matter, and some lag has both empty and filled cells
    flat, keep = Za.reshape(1, F * T, NA), (torch.arange(T)[None, :] < torch.from_numpy(L)[:, None]).reshape(1, F * T, 1).cuda()
    inner = lambda t: t[:-1, :-1]
    assert any((inner(ref_table(flat & keep, flat & keep, [F * T], l)) != inner(w)).any() for l, w in zip(lags, want))
    assert any((inner(ref_table(Za, Za, np.full(F, T), l)) != inner(w)).any() for l, w in zip(lags, want))
    assert any((w[:-1, :-1] == 0).any() and (w[:-1, :-1] > 0).any() for w in want)
    K = NA + 20                                          # room for every partner: a reported diagonal cannot fall off the list
    cx = CX.cross_activation(s["a"], s["path"], "enc", lags=lags, n_neighbors=K, lengths=L, batch_files=3, return_counts=True)
    assert cx.lags.tolist() == list(lags)
    for l, w in enumerate(want):
        check_lag(cx, l, w)
        check_partners(cx, l, w, "jaccard", K, 0)
    assert not cx.tables[3].any() and int(cx.n_pairs[3]) == 0 and not cx.fire_a[3].any() and (cx.partners_a[3] == -1).all()
    assert int(cx.n_pairs[2]) == int((L == T).sum()) >= 2
    # at l > 0 the diagonal is the latent's persistence and is reported wherever it is not zero
    persists = np.diag(want[0][:-1, :-1]) > 0
    assert persists.any() and ((cx.partners_a[0] == np.arange(NA)[:, None]).any(1) == persists).all()


def test_l1_against_topk_on_the_same_shards(small):
    s = small
    n_b, k = 4096, 32
    b = topk_model(D, n_b, k, seed=9, bias=-1.5)
    acts = b.encode(torch.from_numpy(s["x"][0]).cuda()).top_acts
    assert bool((acts == 0).any()) and bool((acts > 0).any())          # selected zeros: not active
    Zb = active(b, s["x"])
    cx = CX.cross_activation(s["a"], s["path"], "enc", sae_b=b, lags=(0, 2), lengths=s["L"], batch_files=3, return_counts=True)
    assert not cx.same_dictionary and cx.tables.shape == (2, NA, n_b)
    for l, lag in enumerate((0, 2)):
        w = ref_table(s["Za"], Zb, s["L"], lag)
        check_lag(cx, l, w)
        check_partners(cx, l, w, "jaccard", 16, 0)
    back = CX.cross_activation(b, s["path"], "enc", sae_b=s["a"], lags=(0,), lengths=s["L"], batch_files=3, return_counts=True)
    np.testing.assert_array_equal(back.tables[0], cx.tables[0].T)
    np.testing.assert_array_equal(back.fire_a[0], cx.fire_b[0])
    np.testing.assert_array_equal(back.fire_b[0], cx.fire_a[0])
    np.testing.assert_array_equal(back.partners_a[0], cx.partners_b[0])


def test_two_layers(small, tmp_path, monkeypatch):
    """B reads its own directory: d = 128, fp16 shards, the same filenames; an L1 dictionary on one, a TopK one on the other."""
    s = small
    d_b, n_b, k = 128, 1024, 16
    names = [f"file_{i:06d}.flac" for i in range(F)]
    g = np.random.default_rng(21)
    xb = g.normal(0, 1, (F, T, d_b)).astype(np.float16)
    write_shards(str(tmp_path / "mid"), "mid", xb.reshape(F, T * d_b), [T, d_b], names)
    b = topk_model(d_b, n_b, k, seed=4, bias=-1.5)
    Zb = active(b, xb)
    cx = CX.cross_activation(s["a"], s["path"], "enc", sae_b=b, data_path_b=str(tmp_path / "mid"), layer_name_b="mid", lags=(0, 3),
                             n_neighbors=8, measure="lift", lengths=s["L"], batch_files=3, return_counts=True)
    for l, lag in enumerate((0, 3)):
        w = ref_table(s["Za"], Zb, s["L"], lag)
        assert (w[:-1, :-1] > 0).any()
        check_lag(cx, l, w)
        check_partners(cx, l, w, "lift", 8, 0)
    # directories that do not hold the same files are refused before any engine call
    write_shards(str(tmp_path / "renamed"), "mid", xb.reshape(F, T * d_b), [T, d_b], names[:-1] + ["other.flac"])
    write_shards(str(tmp_path / "fewer"), "mid", xb[:-1].reshape(F - 1, T * d_b), [T, d_b], names[:-1])
    write_shards(str(tmp_path / "longer"), "mid", np.zeros((F, (T + 1) * d_b), np.float16), [T + 1, d_b], names)

    def called(*a, **k):
        raise AssertionError("an engine call before the directories were compared")
    monkeypatch.setattr(E.SaeEngine, "cross_mask_files", called)
    monkeypatch.setattr(E, "cross_update", called)
    for folder in ("renamed", "fewer", "longer"):
        with pytest.raises(ValueError, match="director"):
            CX.cross_activation(s["a"], s["path"], "enc", sae_b=b, data_path_b=str(tmp_path / folder), layer_name_b="mid",
                                lengths=s["L"], batch_files=3)


def test_batching_and_two_runs_are_bitwise_identical(small):
    s = small
    runs = [CX.cross_activation(s["a"], s["path"], "enc", sae_b=s["b"], lags=(0, 1, 3), lengths=s["L"], batch_files=bf, return_counts=True)
            for bf in (3, 1, 7, 3)]
    for r in runs[1:]:
        same_arrays(runs[0], r)
    check_lag(runs[0], 2, ref_table(s["Za"], s["Zb"], s["L"], 3))


@pytest.fixture(scope="module")
def small_tables(small):
    s = small
    return [ref_table(s["Za"], s["Zb"], s["L"], l) for l in (0, 1)]


@pytest.mark.parametrize("measure", sorted(REF.MEASURES))
@pytest.mark.parametrize("K", [1, 16, max(NA, NB) + 20])
def test_partner_tables_equal_numpy(small, small_tables, measure, K):
    """Both orientations; K = 320 exceeds either side and leaves empty slots in every row."""
    s = small
    assert any(REF.has_tied_scores(small_tables[0], measure, by_b, 0) for by_b in (0, 1)), "no tied scores"
    cx = CX.cross_activation(s["a"], s["path"], "enc", sae_b=s["b"], lags=(0, 1), n_neighbors=K, measure=measure, lengths=s["L"],
                             batch_files=3)
    assert cx.tables is None and cx.measure == measure
    for l, w in enumerate(small_tables):
        check_partners(cx, l, w, measure, K, 0)
    if K > max(NA, NB):
        for p, c, sc in ((cx.partners_a, cx.counts_a, cx.scores_a), (cx.partners_b, cx.counts_b, cx.scores_b)):
            assert (p[..., -1] == -1).all() and (c[..., -1] == 0).all() and np.isnan(sc[..., -1]).all()
    i = int(np.argmax((cx.partners_a[1] >= 0).sum(1)))
    assert cx.top(i, lag=1) == [(int(p), int(c), float(v)) for p, c, v in zip(cx.partners_a[1, i], cx.counts_a[1, i], cx.scores_a[1, i])
                                if p >= 0]


def _stored_mask(eng, x2, n):
    """bool CUDA [rows, n]: the bf16 latent the context stores for x2, > 0."""
    eng.eval(x2)
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (x2.shape[0], ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Alias(), device="cuda")[:, :n].view(torch.bfloat16) > 0


def test_larger_shape_on_the_device():
    """TopK n_a = 4096 against L1 n_b = 16 384, 4 x 1500 frames in one call, lags (0, 5), the tables kept on the device: equal to
    the float64 product of the stored latents' masks.  33 x 129 tiles: the unsplit, non-atomic path (the small shapes above split K)."""
    d, n_a, n_b, k, Tl, Fl = 256, 4096, 16384, 32, 1500, 4
    rows = Fl * Tl
    g = torch.Generator().manual_seed(1)
    We = torch.randn(n_a, d, generator=g) / 16
    a = E.SaeEngine("topk", d, n_a, rows + 144, k=k, optimizer="adam")
    a.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.full(n_a, -1.5, np.float32), "W_dec": We.numpy().copy(),
                  "b_dec": np.zeros(d, np.float32)})
    W, bias = l1_weights(d, n_b, seed=13)
    b = E.SaeEngine("l1", d, n_b, rows + 144)
    b.set_params({"decoder.weight": W, "encoder_bias": bias})
    x = torch.randn(Fl, Tl, d, generator=g).cuda()
    lens = torch.randint(1, Tl + 1, (Fl,), generator=g, dtype=torch.int32)
    lens[0] = Tl
    lens_dev = lens.cuda()
    lags = (0, 5)
    one_a, one_b = E.cross_mask_bytes(n_a, rows), E.cross_mask_bytes(n_b, rows)
    assert one_a == 4224 * 6016 and one_b == 16512 * 6016
    ma = torch.empty(one_a, dtype=torch.int8, device="cuda")
    mb = torch.empty(2 * one_b, dtype=torch.int8, device="cuda")
    tables = torch.zeros(2, n_a + 1, n_b + 1, dtype=torch.int32, device="cuda")
    a.cross_mask_files(x, ma, E.CROSS_SOURCE, (), lens_dev)
    b.cross_mask_files(x, mb, E.CROSS_TARGET, lags, lens_dev)
    for l in range(2):
        E.cross_update(ma, n_a, mb[l * one_b:(l + 1) * one_b], n_b, rows, tables[l])
    torch.cuda.synchronize()
    # every padding byte of a mask is zero
    assert not ma.view(4224, 6016)[n_a + 1:].any() and not ma.view(4224, 6016)[:, rows:].any()
    assert not mb.view(2, 16512, 6016)[:, n_b + 1:].any() and not mb.view(2, 16512, 6016)[:, :, rows:].any()
    x2 = x.reshape(rows, d)
    Za, Zb = _stored_mask(a, x2, n_a).view(Fl, Tl, n_a), _stored_mask(b, x2, n_b).view(Fl, Tl, n_b)
    for l, lag in enumerate(lags):
        want = torch.from_numpy(ref_table(Za, Zb, lens.numpy(), lag)).cuda()
        assert torch.equal(tables[l].to(torch.int64), want), lag
        assert bool((want[:-1, :-1] == 0).any()) and int(want[:-1, :-1].max()) > 1
        assert int(want[-1, -1]) == int((lens - lag).clamp(min=0).sum())
    a.close()
    b.close()


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_the_masks(variant):
    d, n, Tc, Fc = 256, 1024, 50, 4

    def make(**kw):
        if variant == "l1":
            W, b = l1_weights(d, n, seed=1)
            eng = E.SaeEngine("l1", d, n, 1500, recon_alpha=1e2, **kw)
            eng.set_params({"decoder.weight": W, "encoder_bias": b})
        else:
            eng = E.SaeEngine("topk", d, n, 1500, k=16, optimizer="adam", **kw)
            We = torch.randn(n, d, generator=torch.Generator().manual_seed(1)) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32), "W_dec": We.numpy().copy(),
                            "b_dec": np.zeros(d, np.float32)})
        return eng

    a, b = make(), make()
    x = torch.randn(Fc, Tc, d, generator=torch.Generator().manual_seed(2)).cuda()
    rows = Fc * Tc
    one = E.cross_mask_bytes(n, rows)
    masks = torch.empty(3 * one, dtype=torch.int8, device="cuda")
    table = torch.zeros(n + 1, n + 1, dtype=torch.int32, device="cuda")
    for eng in (a, b):
        eng.eval(x.reshape(rows, d))
    a.cross_mask_files(x, masks, E.CROSS_SOURCE | E.CROSS_TARGET, (0, 1))
    E.cross_update(masks[:one], n, masks[2 * one:], n, rows, table)
    torch.cuda.synchronize()
    assert int(table[-1, -1]) == Fc * (Tc - 1) and int(table[:-1, :-1].sum()) > 0
    assert torch.equal(masks[:one], masks[one:2 * one])                  # the source mask is the target mask at lag 0
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="cross-activation"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="cross-activation"):
            a.topk_indices_tensor(rows, "cuda")
    # a following training step is bitwise the same step as in a context that never ran the pass
    for eng in (a, b):
        eng.step(x.reshape(rows, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for key in pa:
        assert pa[key].tobytes() == pb[key].tobytes(), key
    assert a.metrics().tobytes() == b.metrics().tobytes()

    # every bad argument is refused before anything is enqueued: the mask and the table keep their sentinels
    masks.fill_(7)
    table.fill_(7)
    both = E.CROSS_SOURCE | E.CROSS_TARGET
    for sides, lags, match in ((both, (0, 32768), "outside"), (both, (-1,), "outside"), (both, tuple(range(9)), "n_lags"),
                               (both, (2, 5, 2), "twice"), (both, (), "n_lags"), (E.CROSS_SOURCE, (1,), "n_lags"), (0, (), "sides"),
                               (4, (1,), "sides")):
        with pytest.raises(E.EngineError, match=match):
            a.cross_mask_files(x, masks, sides, lags)
    with pytest.raises(E.EngineError, match="max_rows"):
        a.cross_mask_files(torch.randn(40, 50, d).cuda(), torch.full((3 * E.cross_mask_bytes(n, 2000),), 7, dtype=torch.int8, device="cuda"),
                           both, (0, 1))
    with pytest.raises(E.EngineError, match="masks_bytes"):
        a.cross_mask_files(x, masks[:3 * one - 1], both, (0, 1))
    lag_arr = (E.C.c_int32 * 2)(0, 1)
    xp, sp = E.C.c_void_p(x.data_ptr()), E.C.c_void_p(torch.cuda.current_stream().cuda_stream)
    null_calls = [(a._ctx, None, E.C.c_void_p(masks.data_ptr())), (a._ctx, xp, None), (None, xp, E.C.c_void_p(masks.data_ptr()))]
    for ctx, xarg, marg in null_calls:
        assert a._lib.sae_cross_mask_files(ctx, xarg, Fc, Tc, 0, None, both, lag_arr, 2, marg, masks.numel(), sp) != 0
    assert a._lib.sae_cross_mask_files(a._ctx, xp, Fc, Tc, 0, None, both, None, 2, E.C.c_void_p(masks.data_ptr()), masks.numel(), sp) != 0
    with pytest.raises(E.EngineError, match="mask_b"):
        E.cross_update(masks[:one], n, masks[:one - 1], n, rows, table)
    with pytest.raises(E.EngineError):
        E.cross_update(masks[:one], n, masks[one:2 * one], n, 0, table)
    with pytest.raises(E.EngineError, match="aligned"):
        E.cross_update(masks[:one], n, masks[1:one + 1], n, rows, table)
    keys = torch.full(((n + 1) * n,), 7, dtype=torch.int64, device="cuda")
    for measure, by_b, excl, row0, nr in ((4, 0, 0, 0, 4), (-1, 0, 0, 0, 4), (0, 2, 0, 0, 4), (0, 0, 2, 0, 4), (0, 0, 0, -1, 4),
                                          (0, 0, 0, n - 2, 3), (0, 1, 0, 0, 0)):
        with pytest.raises(E.EngineError):
            E.cross_keys(table, n, n, measure, by_b, excl, row0, nr, keys)
    torch.cuda.synchronize()
    assert bool((masks == 7).all()) and bool((table == 7).all()) and bool((keys == 7).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    masks = torch.full((2 * E.cross_mask_bytes(1024, 200),), 7, dtype=torch.int8, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.cross_mask_files(torch.randn(2, 100, 256).cuda(), masks, E.CROSS_SOURCE | E.CROSS_TARGET, (1,))
    torch.cuda.synchronize()
    assert bool((masks == 7).all())
    eng.close()


def test_cli_matches_the_function(small, tmp_path):
    s = small
    cks = []
    for name, sae, n in (("a", s["a"], NA), ("b", s["b"], NB)):
        cks.append(str(tmp_path / f"{name}.pth"))
        torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": D,
                                "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}}, "model": sae.state_dict()}, cks[-1])
    np.save(tmp_path / "len.npy", s["L"])
    out = tmp_path / "cross.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.cross_activation", "--sae", cks[0], "--sae_b", cks[1], "--data_path", s["path"],
                        "--layer_name", "enc", "--lengths", str(tmp_path / "len.npy"), "--batch_files", "3", "--n_neighbors", "8",
                        "--measure", "lift", "--lags", "0,2", "--counts", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    rng = torch.get_rng_state()
    want = CX.cross_activation(cks[0], s["path"], "enc", sae_b=cks[1], lags=(0, 2), n_neighbors=8, measure="lift", lengths=s["L"],
                               batch_files=3, return_counts=True)
    assert torch.equal(torch.get_rng_state(), rng)
    got = CX.CrossActivation.from_npz(str(out))
    same_arrays(got, want)
    check_lag(got, 1, ref_table(s["Za"], s["Zb"], s["L"], 2))
    assert got.measure == "lift" == summary["measure"] and got.same_dictionary is False and summary["same_dictionary"] is False
    assert summary["n_a"] == NA and summary["n_b"] == NB and summary["n_neighbors"] == 8
    assert [e["lag"] for e in summary["lags"]] == [0, 2] and summary["lags"][0]["n_pairs"] == int(s["L"].sum())
    assert summary == {"out": str(out), **want.summary()}
