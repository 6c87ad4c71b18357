"""CPU: the per-latent check of tests/topk_backward_reference.py can fail, and fails where it should.  On the planted d = 384,
n = 1000, k = 8, M = 700 case, with the operands of the CPU oracle's forward (engine tie rule), the planted coverage is exact; a
float32 emulation of the sparse backward's arithmetic (per-entry bf16(fp32 dot), fp32 sums in list order and in reversed order,
256-entry partial sums added afterwards) violates the bound on NO element of the four gradients; and each per-latent failure mode of
the seven-kernel pipeline violates it (or the exact checks of the GPU test) on the latents it hits -- the condition that keeps
tests/test_topk_backward_gpu.py, which allows no violation, from passing vacuously."""
import numpy as np
import pytest

from tests import topk_backward_reference as R

D, N, K, M, FIRST = 384, 1000, 8, 700, 100


@pytest.fixture(scope="module")
def one():
    case, batch = R.make_case(D, N, K, M, R.allowed_lengths(M), FIRST, 41)
    ops, idx, a = R.oracle_operands(case, batch)
    return {"case": case, "batch": batch, "ops": ops, "idx": idx, "a": a, "ref": R.reference(ops)}


@pytest.fixture(scope="module")
def two():
    """The same case through two passes (multi-TopK's 4k selection, then the main one)."""
    case, batch = R.make_case(D, N, K, M, R.allowed_lengths(M), FIRST, 41)
    ops, idx, a = R.oracle_operands(case, batch, multi=True)
    return {"case": case, "batch": batch, "ops": ops, "idx": idx, "a": a, "ref": R.reference(ops)}


def latent_of(c, length):
    return c["case"]["planted"][c["batch"]["lengths"].index(length)]


def assert_clean(c, grads):
    for name in R.GRADS:
        ref, tol = c["ref"][name]
        print(f"d {name}: worst |difference| / tol = {R.worst_ratio(grads[name], ref, tol).max():.3g}")
        assert not R.violations(name, grads[name], ref, tol).any(), R.report(name, grads[name], ref, tol, c["ref"]["L"])


def test_planted_coverage_is_exact_on_the_oracle_selection(one, two):
    for c in (one, two):
        L = R.assert_coverage(c["case"], c["batch"], c["idx"], c["a"])
        assert np.array_equal(L, c["ref"]["L"])
    assert sorted(one["batch"]["lengths"]) == list(R.REQUIRED_LENGTHS) and one["ref"]["L"][one["case"]["hot"]] == M
    assert two["ref"]["L"][two["case"]["hot"]] == 2 * M


def test_coverage_check_can_fail(one):
    c = one
    idx = [c["idx"][0].copy()]
    p = latent_of(c, 257)
    m = c["batch"]["rows_of"][c["batch"]["lengths"].index(257)][0]
    idx[0][m][idx[0][m] == p] = N - 1 if N - 1 not in idx[0][m] else N - 2
    with pytest.raises(AssertionError, match=f"planted latent {p}"):
        R.assert_coverage(c["case"], c["batch"], idx, c["a"])
    a = [c["a"][0].copy()]
    a[0][M - 1] = 1.0                            # a zero row whose entries would pass the gate
    with pytest.raises(AssertionError, match="zero row"):
        R.assert_coverage(c["case"], c["batch"], c["idx"], a)


@pytest.mark.parametrize("reverse", [False, True])
def test_emulation_has_no_violation(one, two, reverse):
    for c in (one, two):
        assert_clean(c, R.emulate(c["ops"], reverse=reverse))


def test_bound_is_a_small_fraction_of_the_reference(one):
    """The bound is a small fraction of the reference where it matters: at the median non-zero element of the weight gradients it
    is below 1 % of |ref| (so a lost entry of a short list, 1 / L of the sum, cannot hide)."""
    for name in ("W_dec", "W_enc"):
        ref, tol = one["ref"][name]
        nz = ref != 0
        assert np.median(tol[nz] / np.abs(ref[nz])) < 1e-2, name


def test_last_entry_of_a_list_dropped(one):
    c = one
    named = {latent_of(c, L) for L in (1, 257, 513)}
    hit = set(np.flatnonzero(c["ref"]["L"] % R.CSC_CHUNK == 1))          # (the random latents with a single entry as well)
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="drop_tail"))
    assert named <= set(bad["W_dec"]) <= hit and len(bad["W_dec"]) == len(hit)
    # (d W_enc and d b_enc allow every entry's da its bf16 rounding, 2^-8 |s_t|: over 257 entries that is one entry's worth, so only
    #  d W_dec, whose products are exact, sees ONE lost entry of a long list; all three see the lost entry of a single-entry list)
    for name in ("W_enc", "b_enc"):
        assert latent_of(c, 1) in bad[name] and set(bad[name]) <= hit, name


def test_entries_from_256_on_dropped(one):
    c = one
    hit = sorted([latent_of(c, L) for L in (257, 511, 512, 513)] + [c["case"]["hot"]])
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="drop_from_256"))
    assert list(bad["W_dec"]) == hit
    most = [j for j in hit if j != latent_of(c, 257)]               # (one lost entry of 257: see above)
    for name in ("W_enc", "b_enc"):
        assert set(most) <= set(bad[name]) <= set(hit), name


@pytest.mark.parametrize("length", [2, 256, 513])
def test_one_entry_takes_the_next_rows_g(one, length):
    c = one
    j = latent_of(c, length)
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="next_row", latent=j))
    assert list(bad["W_dec"]) == [j] and set(bad["W_enc"]) <= {j} and (length > 2 or list(bad["W_enc"]) == [j])


def test_ragged_last_row_block_dropped(one):
    c = one
    tail = M // R.CSC_ROWS * R.CSC_ROWS
    in_tail = np.unique(np.asarray(c["idx"][0])[tail:])
    planted_hit = [p for p, rows in zip(c["case"]["planted"], c["batch"]["rows_of"]) if len(rows) and rows.max() >= tail]
    assert planted_hit and c["case"]["hot"] in in_tail
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="drop_ragged_block"))
    assert set(bad["W_dec"]) <= set(in_tail) and set(planted_hit + [c["case"]["hot"]]) <= set(bad["W_dec"])
    assert set(planted_hit + [c["case"]["hot"]]) <= set(bad["W_enc"])
    assert len(bad["W_dec"]) >= 0.9 * len(in_tail)          # (an entry of activation 0 changes nothing in d W_dec)


def test_gate_removed(one):
    """Only the zero-activation entries of the two zero rows see the gate: xs is 0 there, so d W_enc cannot tell; d b_enc of the
    columns 0 .. k - 2 does."""
    c = one
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="no_gate"))
    assert len(bad["W_dec"]) == 0 and len(bad["W_enc"]) == 0
    assert len(bad["b_enc"]) and set(bad["b_enc"]) <= set(range(K - 1))


def test_b_enc_not_rounded(one):
    c = one
    g = R.emulate(c["ops"], mutation="no_round")
    ref, tol = c["ref"]["b_enc"]
    o = np.asarray(g["b_enc"], np.float64)
    assert (np.abs(o - ref) <= tol).all()                    # closer to the reference than the right answer: the bound alone passes it
    live = c["ref"]["L"] > 2                                 # (a sum of bf16 values lands on the bf16 grid now and then)
    assert R.off_grid(g["b_enc"])[live].mean() > 0.75 and R.violations("b_enc", g["b_enc"], ref, tol)[live].mean() > 0.75
    assert not R.off_grid(g["b_enc"])[c["ref"]["L"] == 0].any()


def test_empty_list_keeps_the_previous_step(one):
    c = one
    prev = R.emulate(c["ops"])
    prev = {k: np.roll(v, 1, axis=0) for k, v in prev.items()}     # a step before, in which other latents fired
    empty = np.flatnonzero(c["ref"]["L"] == 0)
    stale = [j for j in empty if prev["W_dec"][j].any()]
    assert latent_of(c, 0) in empty and stale
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="stale_empty", prev=prev))
    assert list(bad["W_dec"]) == stale and set(bad["W_enc"]) <= set(empty) and set(bad["b_enc"]) <= set(empty)


@pytest.mark.parametrize("length", [1, 256, 257])
def test_entry_reads_the_other_passes_g(two, length):
    c = two
    j = latent_of(c, length)
    bad = R.bad_latents(c["ref"], R.emulate(c["ops"], mutation="other_pass", latent=j))
    assert list(bad["W_dec"]) == [j] and list(bad["W_enc"]) == [j]
