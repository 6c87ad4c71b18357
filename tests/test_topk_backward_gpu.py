"""GPU: the CSC sparse backward of the TopK engine (csrc/topk_sparse.h, the default backward at d_p = 384 / 768 / 1280), every element
of its four gradients against the float64 reference and bound of tests/topk_backward_reference.py, on planted batches whose posting
lists have prescribed lengths (0..5, 255..257, 511..513 where M allows, and M).

    case         d, n, k, M, x                         reaches
    base         384, 1000, 8, 700, fp32               NPAIR = 3, ragged M (5 full row blocks + 60 rows), n_p padding
    ragged_d     380, 1000, 8, 333, bf16               d_p = 384 with d % 8 != 0 (scalar topk_prep_x_kernel), padded columns
    wide_k       768, 1500, 72, 300, fp32              NPAIR = 6, kcap > 64: a partly filled second 64-wide index chunk
    large_d      1280, 1100, 8, 130, bf16              NPAIR = 10, one full row block + 2 rows
    segments     384, 33000, 8, 300, fp32              two count segments, three fill segments, the select above 24 576 latents; short
                                                       lists planted at latents 16383, 16384, 32767, 32768 and n - 1
    multi        384, 1000, 8, 700, fp32, multi_topk   passes 0 and 2 in one list: every top-k entry has a same-row twin in the 4k pass,
                                                       the hot latent has 2 M entries
    second_step  the base engine, then M = 200         latents that go from non-empty to empty, fewer row blocks than the step before

The operands are read back from the engine (its own selection, its bf16 d (decoder output) rows -- selector 14 for the multi-TopK
pass --, its fp32 masters); the reference is computed from them, so the test says nothing about the forward and everything about the
seven kernels between the selection and the gradients.  Held per case: the planted coverage on the engine's selection (a precondition
that fails, never skips); selection, dense rows and list values agree; every element of d W_dec, d W_enc, d b_enc, d b_dec inside
its bound; d b_enc on the bf16 grid; empty lists give +0.0 rows and a +0.0 d b_enc to the bit; single-entry lists give
d W_dec[j] = fl32(a g[m]) to the bit.  auxk_alpha = 0 and the default backward throughout."""
import numpy as np
import pytest
import torch

from tests import topk_backward_reference as R

pytestmark = pytest.mark.gpu

BASE = dict(d=384, n=1000, k=8, M=700, x="float32")
CASES = {
    "base": BASE,
    "ragged_d": dict(d=380, n=1000, k=8, M=333, x="bfloat16"),
    "wide_k": dict(d=768, n=1500, k=72, M=300, x="float32"),
    "large_d": dict(d=1280, n=1100, k=8, M=130, x="bfloat16"),
    "segments": dict(d=384, n=33000, k=8, M=300, x="float32", at=(16383, 16384, 32767, 32768, 32999), at_lengths=(3, 5, 2, 1, 6)),
    "multi": dict(BASE, multi=True),
    "second_step": dict(BASE, M2=200, lengths2=(3, 0, 0, 5, 1, 2, 0, 0, 100, 0, 198, 0)),
}
FIRST = 100          # the planted latents start here (above every k - 1: the zero rows select the columns below)


def _split(flat, n, d):
    nd = n * d
    return {"W_enc": flat[:nd].reshape(n, d), "b_enc": flat[nd:nd + n], "W_dec": flat[nd + n:2 * nd + n].reshape(n, d),
            "b_dec": flat[2 * nd + n:2 * nd + n + d]}


def _read_step(eng, case, batch, multi):
    """Everything the backward read and wrote in the step that just ran."""
    d, n, k, M = case["d"], case["n"], case["k"], batch["M"]
    idx = eng.debug_read(3, M * k).reshape(M, k).astype(np.int64)
    dense = eng.debug_read(0, M * n).reshape(M, n)
    out = {"idx_view": eng.topk_indices_tensor(M, "cuda:0").cpu().numpy().astype(np.int64), "dense_nonzero": int((dense != 0).sum())}
    passes = [(idx, np.take_along_axis(dense, idx, 1), eng.debug_read(1, M * d).reshape(M, d))]
    if multi:
        mdense, midx = eng.multi_topk_buffers(M, "cuda:0")
        midx = midx.cpu().numpy().astype(np.int64)
        passes.insert(0, (midx, np.take_along_axis(mdense.float().cpu().numpy(), midx, 1), eng.debug_read(14, M * d).reshape(M, d)))
    out["passes"] = passes
    out["grads"] = _split(eng.debug_read(2, 2 * n * d + n + d), n, d)
    return out


def ran(name):
    from freud_amd.engine import SaeEngine
    spec = CASES[name]
    d, n, k, M, multi = spec["d"], spec["n"], spec["k"], spec["M"], bool(spec.get("multi"))
    lengths = R.allowed_lengths(M) + tuple(spec.get("at_lengths", ()))
    at = list(range(FIRST, FIRST + len(R.allowed_lengths(M)))) + list(spec.get("at", ()))
    case, batch = R.make_case(d, n, k, M, lengths, at, 51, spec["x"])
    batches = [batch]
    if "M2" in spec:
        batches.append(R.make_batch(case, spec["M2"], spec["lengths2"], 77))
    eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=M, optimizer="adam", k=k, auxk_alpha=0.0, multi_topk=multi)
    try:
        eng.set_topk_options(1e9, 1)
        eng.set_params({key: v.numpy() for key, v in case["P"].items()})
        p0 = eng.get_params()                     # the fp32 masters, before any optimizer step (none runs here)
        steps = []
        for b in batches:
            eng.forward_backward(b["x"].reshape(b["M"], 1, d).cuda())
            steps.append(_read_step(eng, case, b, multi))
        p1 = eng.get_params()
    finally:
        eng.close()
    for key in p0:
        assert np.array_equal(R.bits(p0[key]), R.bits(p1[key])), f"forward_backward changed the master {key}"
    last, b = steps[-1], batches[-1]
    ops = R.operands(last["passes"], b["x"], p0["b_dec"], p0["W_dec"], p0["encoder.weight"])
    return {"name": name, "case": case, "batch": b, "step": last, "first": steps[0], "first_batch": batches[0], "ops": ops,
            "ref": R.reference(ops), "multi": multi}


@pytest.fixture(scope="module", params=list(CASES))
def run(request):
    """One engine run per case, shared by the tests below and released before the next case (the segments case holds 0.5 GB)."""
    return ran(request.param)


def test_planted_coverage_holds_on_the_engines_selection(run):
    p = run["step"]["passes"]
    required = None if run["name"] != "second_step" else ()
    L = R.assert_coverage(run["case"], run["batch"], [i for i, _, _ in p], [a for _, a, _ in p], required=required)
    assert np.array_equal(L, run["ref"]["L"])
    if run["name"] == "second_step":               # latents that fired in the step before and have an empty list now, stale rows at hand
        f = run["first"]
        L1 = R.list_lengths([i for i, _, _ in f["passes"]], run["case"]["n"])
        R.assert_coverage(run["case"], run["first_batch"], [i for i, _, _ in f["passes"]], [a for _, a, _ in f["passes"]])
        gone = (L1 > 0) & (L == 0)
        assert gone.sum() >= 100 and f["grads"]["W_dec"][gone].any(1).all() and L1.max() > R.CSC_CHUNK
        assert any(L1[q] > 0 and L[q] == 0 for q in run["case"]["planted"]) and any(L1[q] == 0 and L[q] > 0 for q in run["case"]["planted"])


def test_selection_dense_rows_and_list_values_agree(run):
    """The index view, selector 3 and the dense rows (densified from the compact values the CSC lists were built from) say the same:
    distinct indices inside the dictionary, no non-zero of a dense row outside them, no negative activation; with multi_topk the
    top-k entries are among the same row's 4k selection (a same-row twin in the other pass)."""
    n, st = run["case"]["n"], run["step"]
    idx, a, _ = st["passes"][-1]
    assert np.array_equal(st["idx_view"], idx)
    for i, v, _ in st["passes"]:
        srt = np.sort(i, 1)
        assert i.min() >= 0 and i.max() < n and (srt[:, 1:] != srt[:, :-1]).all()
        assert (v >= 0).all()
    assert st["dense_nonzero"] == int((a != 0).sum())
    if run["multi"]:
        i4, a4, _ = st["passes"][0]
        for m in range(idx.shape[0]):
            twin = {int(j): float(v) for j, v in zip(i4[m], a4[m])}
            assert all(int(j) in twin and twin[int(j)] == float(v) for j, v in zip(idx[m], a[m]) if v > 0), f"row {m}"


def test_every_gradient_element_is_inside_its_bound(run):
    ref, g = run["ref"], run["step"]["grads"]
    msgs = []
    for name in R.GRADS:
        r, tol = ref[name]
        print(f"{run['name']}: d {name}: worst |difference| / tol = {R.worst_ratio(g[name], r, tol).max():.3g}")
        if R.violations(name, g[name], r, tol).any():
            msgs.append(R.report(name, g[name], r, tol, ref["L"]))
    assert not msgs, "\n".join(msgs)


def test_b_enc_is_on_the_bf16_grid(run):
    off = R.off_grid(run["step"]["grads"]["b_enc"])
    assert not off.any(), f"{int(off.sum())} of {off.size} stored d b_enc are no bf16 value, first at latent {int(np.argmax(off))}"


def test_an_empty_list_gives_zero_rows_to_the_bit(run):
    g, empty = run["step"]["grads"], run["ref"]["L"] == 0
    assert empty.sum() > 0
    for name in ("W_dec", "W_enc", "b_enc"):
        b = R.bits(g[name][empty])
        rows = np.flatnonzero(empty)[b.reshape(b.shape[0], -1).any(1)]
        assert not len(rows), f"d {name}: {len(rows)} latents with an empty list hold something else than +0.0, first {rows[:5]}"


def test_a_single_entry_list_gives_the_exact_product(run):
    """d W_dec[j] = 0 + a g[m]: a product of two bf16 values is exact in fp32 (the + 0 turns a product of -0.0 into +0.0, as the
    accumulator does)."""
    n, g, L = run["case"]["n"], run["step"]["grads"], run["ref"]["L"]
    checked = 0
    for idx, a, gp in run["step"]["passes"]:
        m, q = np.nonzero(L[idx] == 1)
        want = (a[m, q][:, None].astype(np.float32) * gp[m]).astype(np.float32) + np.float32(0)
        got = g["W_dec"][idx[m, q]]
        rows = np.flatnonzero((R.bits(got) != R.bits(want)).any(1))
        assert not len(rows), f"{len(rows)} of {len(m)} single-entry lists differ from fl32(a g[m]), first latent {idx[m, q][rows[0]]}"
        checked += len(m)
    assert checked > 0


def test_selector_14_refuses_where_there_is_no_multi_pass():
    from freud_amd.engine import EngineError, SaeEngine
    d, n, k, M = 384, 1024, 8, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, 1, d, generator=g).cuda()
    P = {"encoder.weight": torch.randn(n, d, generator=g).numpy() / d ** 0.5, "encoder.bias": np.zeros(n, np.float32),
         "W_dec": torch.randn(n, d, generator=g).numpy() / d ** 0.5, "b_dec": np.zeros(d, np.float32)}
    for multi in (False, True):
        eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=M, optimizer="adam", k=k, auxk_alpha=0.0, multi_topk=multi)
        try:
            eng.set_topk_options(1e9, 1)
            eng.set_params(P)
            eng.forward_backward(x)
            if not multi:
                with pytest.raises(EngineError, match="multi_topk"):
                    eng.debug_read(14, M * d)
                continue
            dm = eng.debug_read(14, M * d)
            assert dm.any() and not R.off_grid(dm).any()
            with pytest.raises(EngineError, match="capacity"):
                eng.debug_read(14, M * d - 1)
            eng.set_eval_precision("fp32")
            eng.eval(x)
            with pytest.raises(EngineError, match="fp32"):          # like selector 1: the fp32 forward left no bf16 tensors
                eng.debug_read(14, M * d)
        finally:
            eng.close()
    l1 = SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=M, optimizer="adam")
    try:
        with pytest.raises(EngineError, match="multi_topk"):
            l1.debug_read(14, M * d)
    finally:
        l1.close()
