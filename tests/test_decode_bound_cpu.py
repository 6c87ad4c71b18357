"""CPU: the decode check of tests/decode_reference.py can fail.  On every shape of tests/test_decode_gpu.py a float32 emulation of the
operation (two K orders, both latent types) has no violating element, and each deliberately wrong answer violates on at least 10 % of
its elements -- the condition that keeps the GPU test, which allows none, from passing vacuously."""
import numpy as np
import pytest
import torch

from tests import decode_reference as R

FLOOR = 0.10


@pytest.fixture(scope="module", params=sorted(R.CASES))
def case(request):
    variant, d, n, M, _max_rows, kw = R.CASES[request.param]
    W, b = R.make_weights(variant, d, n, 21)
    lat = R.make_latent(M, n, 22)
    n_p = R.padded_n(n, kw)
    ref, tol = R.decode_reference(lat, W, b, n_p)
    return {"variant": variant, "lat": lat, "W": W, "b": b, "ref": ref, "tol": tol, "n_p": n_p}


def share(out, c):
    s = R.violations(out, c["ref"], c["tol"], c["b"]).mean()
    print(f"violating share {s:.4f}")
    return s


def test_emulation_has_no_violation(case):
    c = case
    for reverse in (False, True):
        out = R.emulate(c["lat"], c["W"], c["b"], reverse=reverse)
        assert not R.violations(out, c["ref"], c["tol"], c["b"]).any(), R.report(out, c["ref"], c["tol"], c["b"])
    lat16 = torch.from_numpy(c["lat"]).bfloat16()                   # a bf16 latent is taken as is: the same operands, the same reference
    ref16, tol16 = R.decode_reference(lat16, c["W"], c["b"], c["n_p"])
    assert np.array_equal(ref16, c["ref"]) and np.array_equal(tol16, c["tol"])
    out = R.emulate(lat16, c["W"], c["b"], round_latent=False)
    assert not R.violations(out, ref16, tol16, c["b"]).any(), R.report(out, ref16, tol16, c["b"])


def test_non_finite_is_a_violation(case):
    c = case
    out = R.emulate(c["lat"], c["W"], c["b"])
    out[3, 5] = np.nan
    out[4, 6] = np.inf
    bad = R.violations(out, c["ref"], c["tol"], c["b"])
    assert bad[3, 5] and bad[4, 6] and bad.sum() == 2


def test_dropped_last_k_tile(case):
    c = case
    n = c["lat"].shape[1]
    cut = c["lat"].copy()
    cut[:, (n - 1) // 64 * 64:] = 0         # the last 64-column K tile that holds dictionary columns
    assert share(R.emulate(cut, c["W"], c["b"]), c) >= FLOOR


def test_rows_swapped_in_pairs(case):
    c = case
    out = R.emulate(c["lat"], c["W"], c["b"])
    M = out.shape[0] // 2 * 2
    sw = out.copy()
    sw[0:M:2], sw[1:M:2] = out[1:M:2], out[0:M:2]
    assert share(sw, c) >= FLOOR


def test_columns_shifted_by_one(case):
    c = case
    assert share(np.roll(R.emulate(c["lat"], c["W"], None), 1, axis=1) + (0 if c["b"] is None else c["b"]), c) >= FLOOR


def test_bias_omitted(case):
    c = case
    if c["variant"] != "topk":
        return                              # L1 has no decoder bias
    assert share(R.emulate(c["lat"], c["W"], None), c) >= FLOOR


def test_latent_not_rounded(case):
    c = case
    assert share(R.emulate(c["lat"], c["W"], c["b"], round_latent=False), c) >= FLOOR


def test_weights_not_rounded(case):
    c = case
    assert share(R.emulate(c["lat"], c["W"], c["b"], round_weights=False), c) >= FLOOR


def test_output_not_rounded(case):
    """An answer without bf16_round(acc) is CLOSER to the reference than the right one: the bound alone passes it, the bf16-value
    part of the check does not."""
    c = case
    out = R.emulate(c["lat"], c["W"], c["b"], round_out=False)
    assert share(out, c) >= FLOOR
    o = np.asarray(out, np.float64)
    assert (np.abs(o - c["ref"]) <= c["tol"]).all()
