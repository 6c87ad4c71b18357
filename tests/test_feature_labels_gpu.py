"""GPU: the feature labels (freud_amd/feature_labels.py over include/freud_sae.h's sae_label_files / sae_label_keys).

The oracle is numpy on what freud_amd.models encode() returns: A = onehot(labels on the counted frames).T @ (encode(x) > 0) in int64
with the "any" column appended, label_count by bincount.  Table, label counts and fire counts must be EQUAL; the two key tables
must equal the numpy restatement (lexsort by score descending, count descending, index ascending; score = np.float32(np.float64(num)
/ np.float64(den))) exactly, for all four measures.  Weights and shards follow tests/test_coactivation_gpu.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import coactivation as CO
from freud_amd import engine as E
from freud_amd import feature_labels as FL
from freud_amd import feature_stats as FST
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MEASURES = ("f1", "precision", "recall", "count")


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    b = g.normal(-1.5, 0.3, n).astype(np.float32)
    return W, b


def l1_model(d, n, seed):
    W, b = l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_model(d, n, k, seed, bias=None, multi=False):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi), max_rows=1500)
    if bias is not None:
        sd = sae.state_dict()
        sd["encoder.bias"] = torch.full((n,), float(bias))
        sae.load_state_dict(sd)
    return sae


def shards(path, x):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(np.float32), [T, d])
    return str(path)


def active_mask(sae, x):
    """encode(x[f]) > 0 of every file: bool [F, T, n] on the host."""
    out = []
    for f in range(x.shape[0]):
        xf = torch.from_numpy(x[f]).cuda()
        if isinstance(sae, L1AutoEncoder):
            z = sae.encode(xf).latent > 0
        else:
            enc = sae.encode(xf)
            z = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda").scatter_(1, enc.top_indices, enc.top_acts.float()) > 0
        out.append(z.cpu().numpy())
    return np.stack(out)


def oracle(Z, labels, L, C):
    """Z bool [F, T, n], labels int [F, T, S], L [F] -> (A int64 [C + 1, n], label_count int64 [C + 1])."""
    F, T, n = Z.shape
    keep = np.arange(T)[None, :] < np.asarray(L)[:, None]
    onehot = np.zeros((F, T, C + 1), np.int64)
    for s in range(labels.shape[2]):
        f, t = np.nonzero(labels[:, :, s] >= 0)
        onehot[f, t, labels[f, t, s]] = 1
    onehot[:, :, C] = 1
    onehot *= keep[:, :, None]
    A = onehot.reshape(F * T, C + 1).T @ Z.reshape(F * T, n).astype(np.int64)
    ids = labels[keep]
    lc = np.bincount(ids[ids >= 0], minlength=C)
    return A, np.concatenate([lc, [int(keep.sum())]]).astype(np.int64)


def np_scores(A, lc, measure):
    Cn = A.shape[0] - 1
    a = A[:Cn].astype(np.int64)
    fire = np.broadcast_to(A[Cn].astype(np.int64)[None, :], a.shape)
    lcb = np.broadcast_to(lc[:Cn].astype(np.int64)[:, None], a.shape)
    num, den = {"f1": (2 * a, fire + lcb), "precision": (a, fire), "recall": (a, lcb), "count": (a, np.ones_like(a))}[measure]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (num.astype(np.float64) / den.astype(np.float64)).astype(np.float32)


def np_top(A, lc, measure, K, by_latent):
    Cn = A.shape[0] - 1
    cnt = A[:Cn].astype(np.int64)
    S = np_scores(A, lc, measure)
    if by_latent:
        cnt, S = cnt.T, S.T
    rows = cnt.shape[0]
    nb = np.full((rows, K), -1, np.int64)
    cn = np.zeros((rows, K), np.int64)
    sc = np.full((rows, K), np.nan, np.float32)
    for i in range(rows):
        j = np.flatnonzero(cnt[i] > 0)
        order = j[np.lexsort((j, -cnt[i, j], -S[i, j].astype(np.float64)))][:K]
        m = len(order)
        nb[i, :m], cn[i, :m], sc[i, :m] = order, cnt[i, order], S[i, order]
    return nb, cn, sc


def check_counts(fl, A, lc):
    Cn = A.shape[0] - 1
    assert fl.matrix.dtype == np.int32 and fl.matrix.shape == (Cn, A.shape[1])
    np.testing.assert_array_equal(fl.matrix.astype(np.int64), A[:Cn])
    np.testing.assert_array_equal(fl.fire_count, A[Cn])
    np.testing.assert_array_equal(fl.label_count, lc[:Cn])
    assert fl.n_frames == int(lc[Cn]) and fl.label_count.dtype == np.int64 and fl.fire_count.dtype == np.int64


def check_tables(fl, A, lc, measure, K):
    Cn = A.shape[0] - 1
    for got, by_latent, k in (((fl.label_latents, fl.label_counts, fl.label_scores), 0, K),
                              ((fl.latent_labels, fl.latent_counts, fl.latent_scores), 1, min(K, Cn))):
        nb, cn, sc = np_top(A, lc, measure, k, by_latent)
        np.testing.assert_array_equal(got[0], nb)
        np.testing.assert_array_equal(got[1], cn)
        assert got[2].dtype == np.float32 and got[2].tobytes() == sc.tobytes()
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64


def random_labels(g, F, T, S, C, empty=0.3):
    """[F, T, S]: distinct ids per frame, slots emptied with probability `empty`."""
    lab = np.argsort(g.random((F, T, max(C, S))), axis=-1)[:, :, :S].astype(np.int64)
    lab[lab >= C] = -1
    lab[g.random((F, T, S)) < empty] = -1
    return lab


ALL = ("matrix", "label_count", "fire_count", "label_latents", "label_counts", "label_scores", "latent_labels", "latent_counts",
       "latent_scores")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l1_small(tmp_path_factory):
    """d = 256, n = 300 (no multiple of a tile: three tile columns), T = 50, F = 7 in batches of 3: three calls, the last one partial,
    150 rows per call (two K steps: the K split with atomic adds), ragged lengths that include 1 and T, C = 5 with some -1."""
    d, n, T, F, Cn = 256, 300, 50, 7, 5
    g = np.random.default_rng(7)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(2, T, F)
    L[0], L[3] = T, 1
    sae = l1_model(d, n, seed=5)
    path = shards(tmp_path_factory.mktemp("l1small"), x)
    Z = active_mask(sae, x)
    lab = random_labels(g, F, T, 1, Cn)
    A, lc = oracle(Z, lab, L, Cn)
    return sae, path, L, Z, lab[:, :, 0], A, lc


def test_l1_small_table_is_exact(l1_small):
    sae, path, L, Z, lab, A, lc = l1_small
    assert (lab == -1).any() and (A[:5] == 0).any() and (A[:5] > 1).any()
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, n_classes=5, lengths=L, batch_files=3, return_counts=True)
    check_counts(fl, A, lc)
    assert fl.n_frames == int(L.sum())
    st = FST.feature_stats(sae, path, "enc", lengths=L, batch_files=3)
    np.testing.assert_array_equal(fl.fire_count, st.fire_count)
    co = CO.feature_coactivation(sae, path, "enc", lengths=L, batch_files=3, return_counts=True)
    np.testing.assert_array_equal(fl.fire_count, np.diag(co.matrix).astype(np.int64))
    check_tables(fl, A, lc, "f1", 16)
    for bf in (3, 7):
        again = FL.feature_labels(sae, path, "enc", frame_labels=lab, n_classes=5, lengths=L, batch_files=bf, return_counts=True)
        for k in ALL:
            assert getattr(fl, k).tobytes() == getattr(again, k).tobytes(), (bf, k)


@pytest.mark.parametrize("Cn", [1, 127, 128, 130])
def test_tile_edges_in_the_label_dimension(l1_small, Cn):
    """C + 1 = 2, 128 (one full tile row), 129 and 131 (the "any" row, then labels too, spill into a second tile row)."""
    sae, path, L, Z, _lab, _A, _lc = l1_small
    g = np.random.default_rng(Cn)
    lab = random_labels(g, Z.shape[0], Z.shape[1], 1, Cn, empty=0.1)
    lab[0, :3, 0] = [Cn - 1, 0, Cn - 1]                    # (file 0 counts all its frames: the last class is seen)
    A, lc = oracle(Z, lab, L, Cn)
    assert A[Cn - 1].sum() > 0
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, n_top=4, lengths=L, batch_files=3, return_counts=True)
    assert fl.n_classes == Cn
    check_counts(fl, A, lc)
    check_tables(fl, A, lc, "f1", 4)


def test_slots_and_file_labels(l1_small):
    """S = 3 with empty slots: file_labels [F, S] equals the same labels broadcast by hand into frame_labels [F, T, S]."""
    sae, path, L, Z, _lab, _A, _lc = l1_small
    F, T, _n = Z.shape
    per_file = np.array([[0, 4, -1], [-1, -1, -1], [2, -1, 3], [-1, 1, -1], [4, 0, 2], [1, -1, -1], [-1, -1, 0]])
    frame = np.ascontiguousarray(np.broadcast_to(per_file[:, None, :], (F, T, 3)))
    A, lc = oracle(Z, frame, L, 5)
    a = FL.feature_labels(sae, path, "enc", file_labels=per_file, n_classes=5, lengths=L, batch_files=3, return_counts=True)
    b = FL.feature_labels(sae, path, "enc", frame_labels=frame, n_classes=5, lengths=L, batch_files=3, return_counts=True)
    check_counts(a, A, lc)
    check_tables(a, A, lc, "f1", 16)
    for k in ALL:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    # one id per file, [F]: a class per file, as ESC-50 gives it
    one = np.array([0, 1, 2, 3, 4, 0, -1])
    A1, lc1 = oracle(Z, np.broadcast_to(one[:, None, None], (F, T, 1)), L, 5)
    check_counts(FL.feature_labels(sae, path, "enc", file_labels=one, lengths=L, batch_files=3, return_counts=True), A1, lc1)


def test_topk_exact_against_encode(tmp_path):
    d, n, k, T, F, Cn = 256, 4096, 32, 50, 9, 6
    sae = topk_model(d, n, k, seed=9, bias=-1.5)
    g = np.random.default_rng(9)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(1, T + 1, F)
    L[0] = T
    path = shards(tmp_path, x)
    # rows with fewer than k positive pre-activations: their selection holds zeros, which are not active
    acts = sae.encode(torch.from_numpy(x[0]).cuda()).top_acts
    assert bool((acts == 0).any()) and bool((acts > 0).any())
    lab = random_labels(g, F, T, 2, Cn)
    A, lc = oracle(active_mask(sae, x), lab, L, Cn)
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, measure="precision", lengths=L, batch_files=4, return_counts=True)
    check_counts(fl, A, lc)
    check_tables(fl, A, lc, "precision", 16)
    np.testing.assert_array_equal(fl.fire_count, FST.feature_stats(sae, path, "enc", lengths=L, batch_files=4).fire_count)


def test_multi_topk_follows_encode(tmp_path):
    d, n, k, T, F, Cn = 256, 2048, 16, 300, 4, 3
    sae = topk_model(d, n, k, seed=3, multi=True)
    g = np.random.default_rng(3)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path, x)
    lab = random_labels(g, F, T, 1, Cn)
    A, lc = oracle(active_mask(sae, x), lab, np.full(F, T), Cn)
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, batch_files=3, return_counts=True, measure="recall")
    check_counts(fl, A, lc)
    check_tables(fl, A, lc, "recall", 16)
    assert A[Cn].sum() <= F * T * k, "the k selection of encode(), not the 4k one"


def test_both_sides_of_the_k_split_on_the_device_twice():
    """The rule of sae_label_files: ksplit = min(ceil(1024 / tiles), K steps) with tiles = (round_up(C + 1, 128) / 128) x (n_p / 128).
    n = 16 384, 4 x 1500 frames in one call (47 K steps): C = 1023 gives 8 x 128 = 1024 tiles, ksplit 1, the plain-store path;
    C = 5 gives 128 tiles, ksplit 8, the atomic path.  Both on the device, twice, bitwise, against the float64 product of the
    operands (0 / 1 values and sums below 2^53 are exact there; torch has no integer matmul on the device)."""
    d, n, T, F = 256, 16384, 1500, 4
    W, b = l1_weights(d, n, seed=13)
    eng = E.SaeEngine("l1", d, n, F * T + 144)
    eng.set_params({"decoder.weight": W, "encoder_bias": b})
    g = torch.Generator().manual_seed(0)
    x = torch.randn(F, T, d, generator=g).cuda()
    lens = torch.randint(1, T + 1, (F,), generator=g, dtype=torch.int32)
    lens[0] = T
    lens_dev = lens.cuda()
    eng.eval(x.reshape(F * T, d))
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (F * T, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    keep = (torch.arange(T)[None, :] < lens[:, None]).reshape(F * T).cuda()
    Z = ((torch.as_tensor(_Alias(), device="cuda")[:, :n].view(torch.bfloat16) > 0) & keep[:, None]).double()
    for Cn, S in ((1023, 2), (5, 1)):
        tiles = -(-(Cn + 1) // 128) * (n // 128)
        assert (min(-(-1024 // tiles), -(-F * T // 128)) == 1) == (Cn == 1023)
        lab = torch.from_numpy(random_labels(np.random.default_rng(Cn), F, T, S, Cn).astype(np.int32)).cuda()
        onehot = torch.zeros(F * T, Cn + 2, dtype=torch.float64, device="cuda")       # (column C + 1 takes the empty slots)
        idx = lab.reshape(F * T, S).long()
        onehot.scatter_(1, torch.where(idx < 0, torch.full_like(idx, Cn + 1), idx), 1.0)
        onehot = onehot[:, :Cn + 1]
        onehot[:, Cn] = 1.0
        onehot *= keep[:, None]
        want = (onehot.T @ Z).to(torch.int32)
        want_lc = onehot.sum(0).to(torch.int64)
        runs = []
        for _ in range(2):
            table = torch.zeros(Cn + 1, n, dtype=torch.int32, device="cuda")
            lcount = torch.zeros(Cn + 1, dtype=torch.int64, device="cuda")
            eng.label_files(x, lab, Cn, table, lcount, lens_dev)
            runs.append((table, lcount))
        torch.cuda.synchronize()
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(runs[0][0], want), Cn
        assert torch.equal(runs[0][1], want_lc), Cn
        assert int(want[:Cn].max()) > 1 and (Cn == 5 or bool((want[:Cn] == 0).any()))
        del onehot, want
    eng.close()


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [1, 16, 8])
def test_key_tables_equal_numpy_in_row_blocks(l1_small, monkeypatch, measure, K):
    """K = 8 = C + 3 and K = 16 ask a latent for more labels than there are: its table is clipped to C columns, with empty slots
    wherever a latent never meets a label.  The key buffer of 600 keys: label rows (n = 300 columns) in blocks of 2, 2 and 1; latent
    rows (C = 5 columns) in blocks of 120, 120 and 60."""
    sae, path, L, Z, lab, A, lc = l1_small
    monkeypatch.setattr(CO, "KEY_BLOCK", 600)
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, n_classes=5, n_top=K, measure=measure, lengths=L, batch_files=3)
    assert fl.matrix is None and fl.measure == measure
    assert fl.label_latents.shape == (5, K) and fl.latent_labels.shape == (300, min(K, 5))
    check_tables(fl, A, lc, measure, K)
    empty = fl.latent_labels == -1
    assert bool(np.isnan(fl.latent_scores[empty]).all()) and bool((fl.latent_counts[empty] == 0).all())
    l = int(np.argmax((fl.label_latents >= 0).sum(1)))
    assert fl.top_latents(l) == [(int(p), int(c), float(s)) for p, c, s in zip(fl.label_latents[l], fl.label_counts[l], fl.label_scores[l]) if p >= 0]


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_the_label_pass(variant):
    d, n, T, F, Cn = 256, 1024, 50, 4, 7

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

    def state(eng):
        step, m1, m2 = eng.get_opt_state()
        out = [np.int64(step).tobytes()] + [v.tobytes() for dct in (eng.get_params(), m1, m2) for v in dct.values()]
        if variant == "topk":
            out.append(eng.get_topk_state().tobytes())
        return out

    a, b = make(), make()
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(2)).cuda()
    # moments and TopK counters that are not their initial zeros.  (No training step in front: every L1 forward, this pass included,
    # renormalises the decoder columns in place as the reference's does, and only the unit-norm +-1/16 columns are its fixed point.)
    g = np.random.default_rng(3)
    shapes = a.param_shapes()
    m1 = {k: g.normal(0, 1e-3, v).astype(np.float32) for k, v in shapes.items()}
    m2 = {k: g.uniform(1e-6, 1e-5, v).astype(np.float32) for k, v in shapes.items()}
    for eng in (a, b):
        eng.set_opt_state(3, m1, m2)
        if variant == "topk":
            eng.set_topk_state(g.integers(0, 1000, n) if eng is a else a.get_topk_state())
        eng.eval(x.reshape(F * T, d))
    before = state(a)
    lab = torch.from_numpy(random_labels(np.random.default_rng(0), F, T, 2, Cn).astype(np.int32)).cuda()
    table = torch.zeros(Cn + 1, n, dtype=torch.int32, device="cuda")
    lcount = torch.zeros(Cn + 1, dtype=torch.int64, device="cuda")
    a.label_files(x, lab, Cn, table, lcount)
    torch.cuda.synchronize()
    assert int(table[:Cn].sum()) > 0 and int(lcount[Cn]) == F * T
    assert state(a) == before
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="feature label pass"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="feature label pass"):
            a.topk_indices_tensor(F * T, "cuda")
    # a co-activation pass after the label pass (the shared mask scratch) still gives its own exact table
    co_a = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    co_b = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    a.coact_files(x, co_a)
    b.coact_files(x, co_b)
    torch.cuda.synchronize()
    assert torch.equal(co_a, co_b) and torch.equal(torch.diagonal(co_a), table[Cn])
    a.eval(x.reshape(F * T, d))
    a.latent_buffer()
    # a following training step is bitwise the same step as in a context that never ran the pass
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    assert state(a) == state(b)
    assert a.metrics().tobytes() == b.metrics().tobytes()
    a.close()
    b.close()


def test_rejections_before_anything_is_enqueued():
    d, n, T, F, Cn = 256, 1024, 50, 2, 4
    lib = E.load()
    x = torch.randn(F, T, d).cuda()
    lab = torch.zeros(F, T, 1, dtype=torch.int32, device="cuda")
    table = torch.full((Cn + 1, n), 7, dtype=torch.int32, device="cuda")
    lcount = torch.full((Cn + 1,), 7, dtype=torch.int64, device="cuda")
    keys = torch.full((n * n,), 7, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def files(eng, xp=p(x), rows=T, labels=p(lab), slots=1, classes=Cn, flags=0, counts=p(table), lc=p(lcount)):
        return lib.sae_label_files(eng._ctx, xp, F, rows, E.DTYPE["float32"], None, labels, slots, classes, flags, counts, lc, None)

    eng8 = E.SaeEngine("l1", d, n, 512, precision="fp8")
    assert files(eng8) != 0 and b"fp8" in lib.sae_last_error()
    eng8.close()
    eng = E.SaeEngine("l1", d, n, 512)
    for kw, word in (({"classes": 0}, b"n_classes"), ({"classes": 4097}, b"n_classes"), ({"slots": 0}, b"n_slots"),
                     ({"slots": 17}, b"n_slots"), ({"flags": 1}, b"flags"), ({"xp": None}, b"null"), ({"labels": None}, b"null"),
                     ({"counts": None}, b"null"), ({"lc": None}, b"null"), ({"rows": 257}, b"max_rows")):
        assert files(eng, **kw) != 0, kw
        assert word in lib.sae_last_error(), (kw, lib.sae_last_error())
    assert lib.sae_label_files(None, p(x), F, T, 0, None, p(lab), 1, Cn, 0, p(table), p(lcount), None) != 0
    with pytest.raises(E.EngineError, match="labels must be"):
        eng.label_files(x, lab.reshape(F * T, 1), Cn, table, lcount)
    with pytest.raises(E.EngineError, match="counts must be"):
        eng.label_files(x, lab, Cn + 1, table, lcount)
    eng.close()
    for row0, rows, measure, by_latent in ((0, 0, 0, 0), (-1, 2, 0, 0), (3, 2, 0, 0), (0, Cn + 1, 0, 0), (n - 1, 2, 0, 1), (0, 2, 4, 0),
                                           (0, 2, -1, 1), (0, 2, 0, 2)):
        with pytest.raises(E.EngineError):
            E.label_keys(table, lcount, Cn, n, measure, by_latent, row0, rows, keys)
    assert lib.sae_label_keys(None, p(lcount), Cn, n, 0, 0, 0, 1, p(keys), None) != 0
    assert lib.sae_label_keys(p(table), p(lcount), 4097, n, 0, 0, 0, 1, p(keys), None) != 0
    torch.cuda.synchronize()
    assert bool((table == 7).all()) and bool((lcount == 7).all()) and bool((keys == 7).all())


def test_cli_matches_the_function(tmp_path):
    d, n, T, F = 256, 512, 50, 12
    sae = l1_model(d, n, seed=3)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": d,
                            "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    g = np.random.default_rng(4)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path / "data", x)
    L = g.integers(1, T + 1, F)
    lab = random_labels(g, F, T, 2, 6)
    names = [f"class{i}" for i in range(6)]
    np.save(tmp_path / "len.npy", L)
    np.save(tmp_path / "lab.npy", lab)
    (tmp_path / "names.json").write_text(json.dumps(names))
    out = tmp_path / "labels.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.feature_labels", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--frame_labels", str(tmp_path / "lab.npy"), "--class_names", str(tmp_path / "names.json"),
                        "--lengths", str(tmp_path / "len.npy"), "--batch_files", "5", "--n_top", "8", "--measure", "recall",
                        "--counts", "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    rng = torch.get_rng_state()
    want = FL.feature_labels(str(ck), path, "enc", frame_labels=lab, class_names=names, n_top=8, measure="recall", lengths=L,
                             batch_files=5, return_counts=True)
    assert torch.equal(torch.get_rng_state(), rng)
    got = FL.FeatureLabels.from_npz(str(out))
    for k in ALL:
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
    assert got.n_frames == want.n_frames == int(L.sum()) == summary["n_frames"]
    assert got.measure == "recall" == summary["measure"] and got.class_names == names
    assert summary == want.summary() | {"out": str(out)}
    assert got.top_latents("class2") == want.top_latents(2)
