"""GPU: SaeEngine.decode (sae_decode) element by element against the float64 reference and bound of tests/decode_reference.py, at every
kernel launch_gemm can take for it and at the edges of each.

    case (d, n, M; max_rows = M unless named)        reaches
    l1    384 1536 300                               128x128 kernel (d_p / 128 = 3 is odd)
    l1    512 1024 256                               256x256 kernel, whole tiles, M == max_rows == M_p
    l1    500 1000 200                               256x256 kernel, ragged rows, ragged d, K padding
    l1    500 1000 200  force_gemm128                128x128 kernel on the same operands
    l1    200  300  77                               128x128 kernel, n_p = 384, one row block
    l1    384 1000 300  precision fp8                row_pad = 256: d_p = 512, M_p = 512, 256x256 kernel
    topk  256 1024 256                               256x256 kernel, row x k-major operand, bias
    topk  200 1000 130                               256x256 kernel, ragged everything, bias
    topk  768 1536 100                               128x128 kernel (M_p / 128 = 1)
    topk  256 1024 100  max_rows 1500                M_p follows M, not max_rows

Every case decodes a float32 latent, the same latent as bf16 (passed as bf16) and the bf16 values widened to float32.  The latent is
the [:, :n] view of an [M][n + 37] tensor whose other columns are NaN (row stride neither 16-byte aligned nor n_p); the output is the
first M rows of an [M + 2][d] tensor of sentinels.  Weights go in through set_params with no forward before the decode.

Held: no element outside the bound and each one a bf16 value (+ b_dec); the guard rows untouched; the zero row and the one-hot rows to
the bit; the three latent forms to the bit; force_gemm128 against the default to the bit; the refusals; and that a decode between
forward_backward and optimizer_step changes nothing that follows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from tests import decode_reference as R

pytestmark = pytest.mark.gpu
FORMS = ("float32", "bfloat16", "float32_of_bf16")


def _params(variant, W, b, n, d):
    if variant == "l1":
        return {"decoder.weight": np.ascontiguousarray(W.T), "encoder_bias": np.zeros(n, np.float32)}
    enc = torch.randn(n, d, generator=torch.Generator().manual_seed(33)).numpy() / d ** 0.5
    return {"encoder.weight": enc, "encoder.bias": np.zeros(n, np.float32), "W_dec": W, "b_dec": b}


def _wide(lat, dtype):
    """lat [M][n] inside an [M][n + 37] tensor of NaN, on the GPU; the view that is passed to decode."""
    M, n = lat.shape
    wide = torch.full((M, n + 37), float("nan"), dtype=dtype)
    wide[:, :n] = lat
    return wide.cuda()[:, :n]


@functools.lru_cache(maxsize=None)
def decoded(name):
    variant, d, n, M, max_rows, kw = R.CASES[name]
    W, b = R.make_weights(variant, d, n, 31)
    lat32 = torch.from_numpy(R.make_latent(M, n, 32))
    lat16 = lat32.bfloat16()
    eng = E.SaeEngine(variant=variant, d_model=d, n_dict=n, max_rows=max_rows, optimizer="adam", **kw)
    try:
        eng.set_params(_params(variant, W, b, n, d))
        bufs = {}
        for form, lat in zip(FORMS, (lat32, lat16, lat16.float())):
            view = _wide(lat, lat.dtype)
            assert view.stride(0) == n + 37 and view.dtype == lat.dtype
            buf = torch.full((M + 2, d), R.SENTINEL, device="cuda")
            eng.decode(view, buf[:M])
            torch.cuda.synchronize()
            bufs[form] = buf.cpu().numpy()
        p = eng.get_params()                         # after the decode: the master it settled and cast
    finally:
        eng.close()
    Wm = np.ascontiguousarray(p["decoder.weight"].T) if variant == "l1" else p["W_dec"]
    bm = None if variant == "l1" else p["b_dec"]
    assert np.array_equal(R.bits(Wm), R.bits(W)) and (bm is None or np.array_equal(R.bits(bm), R.bits(b))), \
        "decode (or set_params) changed the fp32 master"
    ref, tol = R.decode_reference(lat16, Wm, bm, R.padded_n(n, kw))      # bf16(lat32) is lat16: one reference for the three forms
    return {"variant": variant, "d": d, "n": n, "M": M, "W": Wm, "b": bm, "bufs": bufs, "ref": ref, "tol": tol}


@pytest.fixture(params=sorted(R.CASES))
def run(request):
    return decoded(request.param)


@pytest.mark.parametrize("form", FORMS[:2])
def test_every_element_inside_the_bound(run, form):
    out = run["bufs"][form][:run["M"]]
    bad = R.violations(out, run["ref"], run["tol"], run["b"])
    print(R.report(out, run["ref"], run["tol"], run["b"]))
    assert np.isfinite(out).all() and not bad.any(), R.report(out, run["ref"], run["tol"], run["b"])


def test_guard_rows_keep_the_sentinel(run):
    want = np.float32(R.SENTINEL).view(np.uint32)
    for form in FORMS:
        assert (R.bits(run["bufs"][form][run["M"]:]) == want).all(), form


def test_zero_row_and_one_hot_rows_to_the_bit(run):
    """Row 0 is b_dec (TopK) or +0.0 (L1); a one-hot row at column j is float32(bf16(W[j])) + b_dec in float32: operand indexing and
    the transposed read of W_dec, with no tolerance."""
    b = np.zeros(run["d"], np.float32) if run["b"] is None else run["b"]
    for form in FORMS:
        out = run["bufs"][form]
        assert np.array_equal(R.bits(out[0]), R.bits(b)), f"{form}: zero row"
        for row, j in R.one_hot_rows(run["n"]):
            want = (R.bf16(run["W"][j]) + b).astype(np.float32)
            assert np.array_equal(R.bits(out[row]), R.bits(want)), f"{form}: one-hot row {row} at column {j}"


def test_l1_outputs_are_bf16_values(run):
    if run["variant"] != "l1":
        return
    for form in FORMS:
        assert not (R.bits(run["bufs"][form][:run["M"]]) & 0xFFFF).any(), form


def test_latent_forms_agree_to_the_bit(run):
    """A float32 latent of bf16-representable values and the bf16 latent are the same operand; so is the unrounded float32 latent once
    pad_latent_kernel has rounded it (to nearest even, like torch)."""
    assert np.array_equal(R.bits(run["bufs"]["float32_of_bf16"]), R.bits(run["bufs"]["bfloat16"]))
    assert np.array_equal(R.bits(run["bufs"]["float32"]), R.bits(run["bufs"]["bfloat16"]))


def test_force_gemm128_matches_default_to_the_bit():
    """tests/test_engine_gpu.py::test_gemm256_matches_gemm128 states the contract: same K order per output element."""
    a, b = decoded("l1_500_1000_200"), decoded("l1_500_1000_200_gemm128")
    for form in FORMS:
        assert np.array_equal(R.bits(a["bufs"][form]), R.bits(b["bufs"][form])), form


def test_rejections_launch_nothing():
    """EngineError for M > max_rows, a latent narrower than the dictionary (contiguous, and as a narrow view of a wide tensor, whose row
    stride alone would pass the C side) and a float16 latent (refused in engine.py, like an unsupported activation dtype); the C entry
    point itself for a short row stride and a float16 dtype code.  The output keeps its sentinels, and the context still decodes."""
    d, n, M = 200, 300, 77
    W, _ = R.make_weights("l1", d, n, 31)
    eng = E.SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=M, optimizer="adam")
    eng.set_params(_params("l1", W, None, n, d))
    out = torch.full((M + 1, d), R.SENTINEL, device="cuda")
    lat = torch.from_numpy(R.make_latent(M + 1, n, 32)).cuda()
    with pytest.raises(E.EngineError, match="max_rows"):
        eng.decode(lat, out)
    with pytest.raises(E.EngineError, match="columns"):
        eng.decode(lat[:M, :n - 1].contiguous(), out[:M])
    with pytest.raises(E.EngineError, match="columns"):
        eng.decode(lat[:M, :n - 1], out[:M])
    with pytest.raises(E.EngineError, match="dtype"):
        eng.decode(lat[:M].half(), out[:M])
    lib, stream = E.load(), E._stream_ptr()
    for dtype_code, ld in ((E.DTYPE["float32"], n - 1), (E.DTYPE["float16"], n)):
        assert lib.sae_decode(eng._ctx, C.c_void_p(lat.data_ptr()), dtype_code, ld, M, C.c_void_p(out.data_ptr()), stream) != 0
    torch.cuda.synchronize()
    assert (R.bits(out) == np.float32(R.SENTINEL).view(np.uint32)).all()
    eng.decode(lat[:M], out[:M])
    torch.cuda.synchronize()
    ref, tol = R.decode_reference(lat[:M], W, None, R.padded_n(n))
    assert not R.violations(out[:M], ref, tol).any(), R.report(out[:M], ref, tol)
    eng.close()


STATE_CONTEXTS = {
    "l1_fused": dict(variant="l1", recon_alpha=1e4),
    "l1_generic": dict(variant="l1", recon_alpha=1e4, force_generic=True),
    "topk": dict(variant="topk", k=8, auxk_alpha=0.0, optimizer="adam"),
}


@pytest.mark.parametrize("ctx", sorted(STATE_CONTEXTS))
def test_decode_between_backward_and_update_changes_nothing(ctx):
    """forward_backward(x) -> decode -> optimizer_step -> step(x) against the same without the decode: parameters, both moments,
    metrics() and the TopK firing state are equal to the bit.  decode writes the dpre scratch (dead after the backward), settles the
    lazily normalised L1 master and re-casts Wb / Wd_b from the master the next forward casts again."""
    kw = STATE_CONTEXTS[ctx]
    d, n, M, lr = 384, 1024, 512, 1e-3
    g = torch.Generator().manual_seed(41)
    x = ((torch.relu(torch.randn(M, 32, generator=g)) * 0.1) @ torch.randn(32, d, generator=g)).cuda()
    W, b = R.make_weights(kw["variant"], d, n, 42)
    if kw["variant"] == "l1":
        W = W / np.linalg.norm(W, axis=1, keepdims=True)
    lat = torch.from_numpy(R.make_latent(M, n, 43)).cuda()
    res = []
    for with_decode in (True, False):
        eng = E.SaeEngine(d_model=d, n_dict=n, max_rows=M, **kw)
        eng.set_params(_params(kw["variant"], W, b, n, d))
        eng.forward_backward(x)
        if with_decode:
            out = torch.empty(M, d, device="cuda")
            eng.decode(lat, out)
        eng.optimizer_step(lr)
        eng.step(x, lr)
        step, m1, m2 = eng.get_opt_state()
        got = {"step": np.array([step]), "metrics": eng.metrics().copy()}
        got.update({f"param {k}": v for k, v in eng.get_params().items()})
        got.update({f"exp_avg {k}": v for k, v in m1.items()})
        got.update({f"exp_avg_sq {k}": v for k, v in m2.items()})
        if kw["variant"] == "topk":
            got["topk_state"] = eng.get_topk_state()
        eng.close()
        res.append(got)
    a, b_ = res
    assert np.isfinite(a["metrics"][:3]).all() and a["step"][0] == 2
    for key in a:
        assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint8), np.ascontiguousarray(b_[key]).view(np.uint8)), key
