"""GPU: the dictionary comparison (freud_amd/dictionary_match.py over include/freud_sae.h's sae_dict_pack / sae_dict_sim_keys) against a
float64 numpy reference: unit vectors and cosines in float64 from the fp32 inputs, neighbours by lexsort (cosine descending, index
ascending).

Shapes (n_a, n_b, d): (300, 260, 100) ragged in every dimension with more than one 256-tile each way; (512, 768, 384) aligned and
multi-tile; (128, 256, 1280) the longest K.

Tolerance of the accuracy test: tol = 3 x 2^-18 (the hi / lo operand split: two lo roundings and the dropped lo.lo term, each at
most 2^-18 sum |a_k b_k| <= 2^-18) + 2^-21 (the normalisation roundings) + 4 x E_acc, E_acc = the largest difference, over the
test's pairs, between a strictly sequential fp32 accumulation (numpy.cumsum in float32) of the 3 d exact products of the split
operands and their float64 sum; the factor 4 covers the unknown summation order of the MFMA.  Plain bf16 operands are off by a few
1e-4 and fail it.

Measured on an MI355X (max |cosine - float64| over the reported pairs, printed by the test): 2.0e-6 at (300, 260, 100) against
tol = 1.55e-5, 1.2e-6 at (512, 768, 384) against 1.73e-5, 1.1e-6 at (128, 256, 1280) against 1.96e-5; norms within 1.3e-7 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from freud_amd import dictionary_match as DM
from freud_amd import engine as E
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

pytestmark = pytest.mark.gpu

SHAPES = [(300, 260, 100), (512, 768, 384), (128, 256, 1280)]
N_PLANTED = 64


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def unit64(W):
    W = np.asarray(W, np.float32).astype(np.float64)
    nrm = np.sqrt((W * W).sum(axis=1))
    return np.divide(W, nrm[:, None], out=np.zeros_like(W), where=nrm[:, None] > 0), nrm


def cos64(A, B):
    return unit64(A)[0] @ unit64(B)[0].T


def np_neighbors(S, K, self_mode):
    """Per row of S (fp32 values are what is ranked) the K best columns: cosine descending, index ascending; -1 / NaN where empty."""
    n_a, n_b = S.shape
    nb = np.full((n_a, K), -1, np.int32)
    cs = np.full((n_a, K), np.nan, np.float32)
    for i in range(n_a):
        j = np.arange(n_b)
        if self_mode:
            j = j[j != i]
        order = j[np.lexsort((j, -S[i, j].astype(np.float64)))][:K]
        nb[i, :len(order)], cs[i, :len(order)] = order, S[i, order]
    return nb, cs


def exact_dictionary(n, d, seed):
    """Every direction: four non-zeros of +-0.5 at seeded positions, scaled by a seeded power of two in [2^-3, 2^3]: norms, unit
    vectors (lo = 0) and every partial sum are exact in any order, cosines are multiples of 0.25 with massive ties."""
    g = np.random.default_rng(seed)
    W = np.zeros((n, d), np.float32)
    for i in range(n):
        W[i, g.permutation(d)[:4]] = np.where(g.random(4) < 0.5, -0.5, 0.5)
    return W * (2.0 ** g.integers(-3, 4, n)).astype(np.float32)[:, None]


def check_exact(m, A, B, K, self_mode):
    S = (cos64(A, B).astype(np.float32) + np.float32(0.0))              # (+ 0.0: a -0.0 of the reference's summation becomes 0.0)
    assert np.array_equal(S.astype(np.float64) * 4, np.round(S.astype(np.float64) * 4)), "the construction is not exact"
    nb, cs = np_neighbors(S, K, self_mode)
    np.testing.assert_array_equal(m.neighbors, nb)
    assert m.neighbors.dtype == np.int32 and m.cosines.dtype == np.float32
    filled = nb >= 0
    np.testing.assert_array_equal(m.cosines[filled].view(np.uint32), cs[filled].view(np.uint32))
    assert np.isnan(m.cosines[~filled]).all()
    un, nrm = unit64(A)
    np.testing.assert_array_equal(m.norms_a, nrm.astype(np.float32))
    assert m.self_mode == self_mode


@pytest.fixture(scope="module")
def exact_pair():
    A, B = exact_dictionary(300, 100, seed=1), exact_dictionary(260, 100, seed=2)
    B[17] = A[5] * 4                    # exact matches across the two dictionaries
    B[203] = -A[5]
    return A, B


@pytest.mark.parametrize("K", [8, 300])
def test_exact_two_dictionaries(exact_pair, K):
    A, B = exact_pair
    m = DM.compare_dictionaries(A, B, n_neighbors=K)
    check_exact(m, A, B, K, False)
    assert m.neighbors[5, 0] == 17 and m.cosines[5, 0] == 1.0
    if K == 300:
        assert (m.neighbors[:, 260:] == -1).all() and (m.neighbors[:, :260] >= 0).all()
        assert m.neighbors[5, 259] == 203 and m.cosines[5, 259] == -1.0        # signed values: no positivity filter


@pytest.mark.parametrize("K", [8, 300])
def test_exact_self_mode(exact_pair, K):
    A = exact_pair[0].copy()
    A[40] = A[7] * 2                    # duplicates of 7, below and above a tile edge
    A[290] = A[7] / 4
    m = DM.compare_dictionaries(A, n_neighbors=K)
    check_exact(m, A, A, K, True)
    assert not (m.neighbors == np.arange(300)[:, None]).any(), "a direction is its own neighbour"
    assert m.top(7)[:2] == [(40, 1.0), (290, 1.0)] and m.top(40)[:2] == [(7, 1.0), (290, 1.0)]
    assert {(7, 40), (7, 290), (40, 290)} <= {tuple(p) for p in m.duplicates(0.999).tolist()}
    if K == 300:
        assert (m.neighbors[:, 299] == -1).all() and (m.neighbors[:, :299] >= 0).all()


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
def gaussian_pair(n_a, n_b, d, seed):
    g = np.random.default_rng(seed)
    B = g.standard_normal((n_b, d)).astype(np.float32)
    A = g.standard_normal((n_a, d)).astype(np.float32)
    rows = g.permutation(n_a)[:N_PLANTED]
    src = g.permutation(n_b)[:N_PLANTED]
    A[rows] = B[src] + np.float32(0.05) * g.standard_normal((N_PLANTED, d)).astype(np.float32)
    return A, B, rows, src


def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def split_operand(W, left):
    u = unit64(W)[0].astype(np.float32)
    hi = bf16_round(u)
    lo = bf16_round(u - hi)
    return np.concatenate([hi, hi, lo] if left else [hi, lo, hi], axis=1)


def accumulation_error(A, B, pairs):
    """E_acc over `pairs` [P, 2]: sequential fp32 accumulation of the exact products of the split operands against their fp64 sum."""
    L, R = split_operand(A, True), split_operand(B, False)
    worst = 0.0
    for c in range(0, len(pairs), 512):
        p = pairs[c:c + 512]
        prod = L[p[:, 0]] * R[p[:, 1]]                                  # bf16 x bf16: exact in fp32
        seq = np.cumsum(prod, axis=1, dtype=np.float32)[:, -1]
        worst = max(worst, float(np.abs(seq.astype(np.float64) - prod.astype(np.float64).sum(axis=1)).max()))
    return worst


_CACHE = {}


def accuracy_case(shape):
    """(inputs, reference, first GPU answer) of a shape, computed once and shared."""
    if shape not in _CACHE:
        n_a, n_b, d = shape
        A, B, rows, src = gaussian_pair(n_a, n_b, d, seed=d)
        _CACHE[shape] = (A, B, rows, src, cos64(A, B), DM.compare_dictionaries(A, B, n_neighbors=8))
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_against_float64(shape):
    n_a, n_b, d = shape
    K = 8
    A, B, rows, src, S, m = accuracy_case(shape)
    nb_ref, _ = np_neighbors(S.astype(np.float32), K, False)
    g = np.random.default_rng(7)
    pairs = np.concatenate([np.stack([np.repeat(np.arange(n_a), K), nb_ref.reshape(-1)], axis=1),
                            np.stack([g.integers(0, n_a, 4096), g.integers(0, n_b, 4096)], axis=1)])
    e_acc = accumulation_error(A, B, pairs)
    tol = 3 * 2.0 ** -18 + 2.0 ** -21 + 4 * e_acc
    assert (m.neighbors >= 0).all() and m.neighbors.shape == (n_a, K)
    rep = np.take_along_axis(S, m.neighbors.astype(np.int64), axis=1)
    err = float(np.abs(m.cosines.astype(np.float64) - rep).max())
    un, nrm = unit64(A)
    nerr = max(float(np.abs(m.norms_a / nrm - 1).max()), float(np.abs(m.norms_b / unit64(B)[1] - 1).max()))
    print(f"\ndictionary match {shape}: max |cosine - float64| = {err:.3e}, tol = {tol:.3e} (E_acc = {e_acc:.3e}), "
          f"max relative norm error = {nerr:.3e}")
    # (a) every reported cosine is that of the reported index
    assert err <= tol, (err, tol)
    # (b) the set is valid: nothing unreported beats the K-th reported cosine by more than 2 tol
    rest = S.copy()
    np.put_along_axis(rest, m.neighbors.astype(np.int64), -np.inf, axis=1)
    excess = float((rest.max(axis=1) - m.cosines[:, K - 1].astype(np.float64)).max())
    assert excess <= 2 * tol, (excess, tol)
    # (c) non-increasing, equal values in index order
    c, j = m.cosines, m.neighbors
    assert (c[:, 1:] <= c[:, :-1]).all()
    assert (j[:, 1:] > j[:, :-1])[c[:, 1:] == c[:, :-1]].all()
    # (d) a planted row finds its source first
    np.testing.assert_array_equal(m.neighbors[rows, 0], src)
    assert (m.cosines[rows, 0] > 0.99).all()
    # (e) norms
    assert nerr <= (d + 2) * 2.0 ** -24, nerr
    assert m.mmcs() == pytest.approx(float(S.max(axis=1).mean()), abs=tol)


# ---- layouts, row blocks, determinism ------------------------------------------------------------------------------------------
def pack(w, n, d, ds, es, side):
    packed = torch.zeros(E.dict_pack_bytes(n, d), dtype=torch.uint8, device="cuda")
    norms = torch.zeros(n, dtype=torch.float32, device="cuda")
    E.dict_pack(w, n, d, ds, es, side, packed, norms)
    return packed, norms


def test_row_and_column_layouts_agree_bitwise():
    n, d = 300, 100
    g = np.random.default_rng(11)
    W = (g.standard_normal((n, d)) * 10.0 ** g.uniform(-2, 2, (n, 1))).astype(np.float32)
    W[13] = 0                                                       # a direction of norm 0 stays the zero vector
    rows = torch.from_numpy(W).cuda()                               # [n][d]: directions contiguous
    cols = torch.from_numpy(np.ascontiguousarray(W.T)).cuda()       # [d][n]: the L1 layout
    for side in (E.DICT_LEFT, E.DICT_RIGHT):
        pr, nr = pack(rows, n, d, d, 1, side)
        pc, nc = pack(cols, n, d, 1, n, side)
        assert torch.equal(pr, pc) and torch.equal(nr, nc)
        assert nr[13].item() == 0.0
        img = pr.view(torch.bfloat16).view(512, 3, 128)
        assert bool((img[n:] == 0).all()) and bool((img[:, :, d:] == 0).all()) and bool((img[13] == 0).all())
        hi_twice = (0, 1) if side == E.DICT_LEFT else (0, 2)
        assert torch.equal(img[:, hi_twice[0]], img[:, hi_twice[1]])
    a = DM.compare_dictionaries(rows, n_neighbors=8)
    b = DM.compare_dictionaries(cols.t(), n_neighbors=8)
    dirs = DM.decoder_directions(cols.t())
    assert (dirs.dir_stride, dirs.elem_stride) == (1, n) and dirs.weights.data_ptr() == cols.data_ptr()
    for k in ("neighbors", "cosines", "norms_a", "norms_b"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes()
    assert (a.cosines[13] == 0).all() and a.neighbors[13].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]


def test_row_blocks_concatenate_bitwise():
    n, d = 300, 100
    g = np.random.default_rng(12)
    W = torch.from_numpy(g.standard_normal((n, d)).astype(np.float32)).cuda()
    pa, _ = pack(W, n, d, d, 1, E.DICT_LEFT)
    pb, _ = pack(W, n, d, d, 1, E.DICT_RIGHT)
    whole = torch.full((n * n,), 7, dtype=torch.int64, device="cuda")
    E.dict_sim_keys(pa, n, pb, n, d, 0, n, True, whole)
    parts = torch.full((n * n,), 9, dtype=torch.int64, device="cuda")
    E.dict_sim_keys(pa, n, pb, n, d, 0, 130, True, parts[:130 * n])
    E.dict_sim_keys(pa, n, pb, n, d, 130, 170, True, parts[130 * n:])
    assert torch.equal(whole, parts)
    k = whole.view(n, n)
    assert bool((torch.diagonal(k) == 0).all()) and int((k == 0).sum()) == n
    assert bool(((k & 0xFFFFFFFF) == 0).all())
    cross = torch.empty(n * n, dtype=torch.int64, device="cuda")
    E.dict_sim_keys(pa, n, pb, n, d, 0, n, False, cross)            # not self mode: the diagonal is a cosine like any other
    assert int((cross == 0).sum()) == 0
    off = ~torch.eye(n, dtype=torch.bool, device="cuda")
    assert torch.equal(cross.view(n, n)[off], k[off])


def test_two_runs_are_bytewise_equal():
    A, B, _rows, _src, _S, first = accuracy_case((512, 768, 384))
    again = DM.compare_dictionaries(A, B, n_neighbors=8)
    for k in ("neighbors", "cosines", "norms_a", "norms_b"):
        assert getattr(first, k).tobytes() == getattr(again, k).tobytes()


# ---- models ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_models_give_their_decoder_directions(variant):
    d, n = 100, 300
    g = np.random.default_rng(21)
    if variant == "l1":
        sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
        W = g.standard_normal((d, n)).astype(np.float32)
        W[:, 200] = W[:, 7]
        sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.zeros(n)})
        want_strides = (1, n)
    else:
        torch.manual_seed(21)
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=8), max_rows=1500)
        sd = sae.state_dict()
        W = g.standard_normal((n, d)).astype(np.float32)
        W[200] = W[7]
        sd["W_dec"] = torch.from_numpy(W)
        sae.load_state_dict(sd)
        want_strides = (d, 1)
    rng = torch.get_rng_state()
    dirs = DM.decoder_directions(sae)
    assert tuple(dirs.weights.shape) == (n, d) and (dirs.dir_stride, dirs.elem_stride) == want_strides
    assert dirs.weights.is_cuda and dirs.weights.dtype == torch.float32
    m = DM.compare_dictionaries(sae)
    t = DM.compare_dictionaries(dirs.weights)
    assert torch.equal(rng, torch.get_rng_state())
    assert m.self_mode and t.self_mode
    for k in ("neighbors", "cosines", "norms_a", "norms_b"):
        assert getattr(m, k).tobytes() == getattr(t, k).tobytes()
    assert [7, 200] in m.duplicates(0.999).tolist()
    assert m.neighbors[7, 0] == 200 and m.neighbors[200, 0] == 7
    # against the float64 reference of the weights the model holds
    S = cos64(dirs.weights.cpu().numpy(), dirs.weights.cpu().numpy())
    rep = np.take_along_axis(S, m.neighbors.astype(np.int64), axis=1)
    assert float(np.abs(m.cosines - rep).max()) < 2e-5


# ---- the C ABI's argument checks ------------------------------------------------------------------------------------------------
def test_argument_checks_return_errors_and_enqueue_nothing():
    lib = E.load()
    n, d = 300, 100
    p = lambda t: C.c_void_p(t.data_ptr())
    w = torch.ones(n, d, device="cuda")
    packed = torch.full((E.dict_pack_bytes(n, d),), 3, dtype=torch.uint8, device="cuda")
    norms = torch.full((n,), 3.0, device="cuda")
    keys = torch.full((n * n,), 7, dtype=torch.int64, device="cuda")
    ok = (p(w), n, d, d, 1, 0, p(packed), p(norms), None)
    bad_pack = [(None,) + ok[1:], ok[:6] + (None,) + ok[7:], ok[:7] + (None, None),
                (p(w), 0, d, d, 1, 0, p(packed), p(norms), None), (p(w), n, 0, d, 1, 0, p(packed), p(norms), None),
                (p(w), (1 << 24) + 1, d, d, 1, 0, p(packed), p(norms), None), (p(w), n, 8193, 8193, 1, 0, p(packed), p(norms), None),
                (p(w), n, d, d, 1, 2, p(packed), p(norms), None), (p(w), n, d, d, 1, -1, p(packed), p(norms), None),
                (p(w), n, d, 0, 1, 0, p(packed), p(norms), None), (p(w), n, d, d, 0, 0, p(packed), p(norms), None)]
    for args in bad_pack:
        assert lib.sae_dict_pack(*args) != 0, args
    oks = (p(packed), n, p(packed), n, d, 0, n, 1, p(keys), None)
    bad_keys = [(None,) + oks[1:], oks[:2] + (None,) + oks[3:], oks[:8] + (None, None),
                (p(packed), 0, p(packed), n, d, 0, 1, 0, p(keys), None), (p(packed), n, p(packed), 0, d, 0, 1, 0, p(keys), None),
                (p(packed), n, p(packed), n, 0, 0, 1, 0, p(keys), None),
                (p(packed), n, p(packed), 260, d, 0, 1, 1, p(keys), None),          # self mode with n_a != n_b
                (p(packed), n, p(packed), n, d, 0, 0, 1, p(keys), None),            # an empty block
                (p(packed), n, p(packed), n, d, -1, 4, 1, p(keys), None),
                (p(packed), n, p(packed), n, d, 296, 5, 1, p(keys), None),          # a block past the end
                (p(packed), n, p(packed), n, d, 0, 4, 2, p(keys), None)]
    for args in bad_keys:
        assert lib.sae_dict_sim_keys(*args) != 0, args
    assert b"rows" in lib.sae_last_error() or b"self" in lib.sae_last_error()
    torch.cuda.synchronize()
    assert bool((packed == 3).all()) and bool((norms == 3.0).all()) and bool((keys == 7).all())
    # the wrappers refuse buffers that are too small before the library sees them
    with pytest.raises(E.EngineError):
        E.dict_pack(w, n, d, d, 1, 0, packed[:-1], norms)
    with pytest.raises(E.EngineError):
        E.dict_pack(w, n, d, d + 1, 1, 0, packed, norms)                            # strides that leave the tensor's storage
    with pytest.raises(E.EngineError):
        E.dict_sim_keys(packed, n, packed, n, d, 0, n, True, keys[:-1])


def test_cli_prints_the_summary_and_writes_the_tables(tmp_path, capsys):
    import json
    d, n = 100, 300
    torch.manual_seed(22)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=8), max_rows=1500)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "topk", "activation_size": d, "autoencoder_config": {"n_dict_components": n, "k": 8}},
                "model": sae.state_dict()}, str(ck))
    out = tmp_path / "match.npz"
    DM.main(["--a", str(ck), "--n-neighbors", "4", "--threshold", "0.5", "--out", str(out)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    want = DM.compare_dictionaries(sae, n_neighbors=4)
    back = DM.DictionaryMatch.from_npz(str(out))
    for k in ("neighbors", "cosines", "norms_a", "norms_b"):
        assert getattr(back, k).tobytes() == getattr(want, k).tobytes()
    assert summary["out"] == str(out) and summary["n_a"] == n and summary["n_b"] == n and summary["self_mode"] is True
    assert summary["n_neighbors"] == 4 and summary["mmcs"] == pytest.approx(want.mmcs()) and summary["matched"] == int(want.matched(0.5).sum())
