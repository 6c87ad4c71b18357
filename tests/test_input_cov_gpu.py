"""GPU: the input-covariance kernels (freud_amd/csrc/input_cov.h) through the C ABI (sae_input_cov), held to the rule and the derived
bound of tests/input_cov_reference.py.

Exact cases: integer-valued x in [-8, 8] and an integer centre in [-4, 4] (or NULL) make every partial sum an integer far below 2^53,
so the output must equal the int64 product to the bit in both triangles -- a result in the wrong row, a dropped frame or an operand
0 - c for a frame that does not count cannot hide.  The frames that do not count hold NaN.  The shapes are the smallest that reach
every path: d on both sides of the 16-column instruction tile, of the 32-column wave quarter and of the 64-column tile, d = 384
(21 tiles), d = 2048 (the widest); one frame, three, two units per file, ragged lengths (a length of 0 counts one frame), four units
with tails of two and three frames."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import input_cov_reference as R

pytestmark = pytest.mark.gpu
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
DS = (1, 15, 16, 17, 33, 80, 384)
# a trimmed cross product: every (d, frames) pair, the dtype and the centre cycling through it
EXACT = [(d, fr, ("float32", "float16", "bfloat16")[i % 3], i % 2 == 0) for i, (d, fr) in enumerate(itertools.product(DS, R.FRAME_CASES))]
EXACT.append((2048, "wide", "bfloat16", True))
FRAMES = dict(R.FRAME_CASES, wide=(1, 9, None))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from freud_amd import engine as E
    return E.load()


def _plan(F, T, d):
    out = (C.c_int64 * 4)()
    assert _lib().sae_input_cov_plan(F, T, d, out) == 0
    return tuple(int(v) for v in out)


def _device_sample(x, lengths, dtype, offset=0):
    """x numpy [F, T, d] -> the CUDA tensor in dtype (exact), frames that do not count NaN; offset: its base pointer that many
    elements beyond an allocation's."""
    F, T, d = x.shape
    flat = torch.empty(x.size + offset, dtype=TORCH[dtype], device="cuda")
    dev = flat[offset:].view(F, T, d)
    dev.copy_(torch.from_numpy(x).to("cuda"))
    assert torch.equal(dev.float().cpu(), torch.from_numpy(x).float())
    if lengths is not None:
        for f, c in enumerate(R.counts(F, T, lengths)):
            dev[f, c:] = float("nan")
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda") if lengths is not None else None
    return dev, lens


def _cov(dev, lens, center, ws=None, stream=None, fill=None):
    """sae_input_cov on a resident sample -> the scatter as numpy (center: numpy float64 [d], a CUDA tensor, or None)."""
    lib = _lib()
    F, T, d = (int(v) for v in dev.shape)
    nbytes = lib.sae_input_cov_workspace_bytes(F, T, d)
    assert nbytes == _plan(F, T, d)[1] * _plan(F, T, d)[2] * 64 * 64 * 8
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    c = torch.from_numpy(center).cuda() if isinstance(center, np.ndarray) else center
    out = torch.full((d, d), float("nan"), dtype=torch.float64, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    code = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dev.dtype]          # include/freud_sae.h: SAE_DTYPE_*
    with torch.cuda.stream(s):
        rc = lib.sae_input_cov(_p(dev), F, T, d, code, _p(lens), _p(c), _p(out), _p(ws), ws.numel(), C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sae_last_error().decode()
    s.synchronize()
    return out.cpu().numpy()


def _exact_inputs(d, frames):
    F, T, lengths = FRAMES[frames]
    x, c = R.integer_sample(F, T, d, seed=d * 10 + F)
    return x, c, lengths


@pytest.mark.parametrize("d,frames,dtype,with_center", EXACT, ids=lambda v: str(v))
def test_integer_inputs_give_the_int64_product_to_the_bit(d, frames, dtype, with_center):
    x, c, lengths = _exact_inputs(d, frames)
    c = c if with_center else None
    dev, lens = _device_sample(x, lengths, dtype)
    out = _cov(dev, lens, c)
    assert R.check_exact(out, x, lengths, c) == []
    assert out.tobytes() == np.ascontiguousarray(out.T).tobytes()


def test_the_cases_reach_every_part_of_the_plan():
    """Read from sae_input_cov_plan, not assumed: more than one tile per dimension, more than one segment, a frame count that is no
    multiple of four; and a shape whose segments hold several units (test_several_units_per_segment_exact runs it)."""
    many_tiles = many_segments = odd_count = False
    for d, frames, _dt, _c in EXACT:
        F, T, lengths = FRAMES[frames]
        tile, tiles, segments, ups = _plan(F, T, d)
        assert tiles == (-(-d // tile)) * (-(-d // tile) + 1) // 2 and segments * ups >= F * -(-T // 256) > (segments - 1) * ups
        many_tiles |= d > tile and tiles > 2
        many_segments |= segments > 1
        odd_count |= sum(R.counts(F, T, lengths)) % 4 != 0
    assert many_tiles and many_segments and odd_count
    # a segment of several units: at the widest model three segments share the twelve units
    assert _plan(4, 600, 2048)[3] > 1


def test_odd_d_two_byte_dtype_and_an_odd_base_pointer():
    """Rows that are not 16-byte aligned, from a base pointer one element beyond an allocation's."""
    x, c, lengths = _exact_inputs(33, "ragged")
    dev, lens = _device_sample(x, lengths, "bfloat16", offset=1)
    assert dev.data_ptr() % 4 == 2
    assert R.check_exact(_cov(dev, lens, c), x, lengths, c) == []


def test_several_units_per_segment_exact():
    """d = 2048 over 4 files x 600 frames: 528 tiles, segments of more than one unit, added in ascending order."""
    F, T, d = 4, 600, 2048
    assert _plan(F, T, d)[3] > 1 and _plan(F, T, d)[2] > 1
    x, c = R.integer_sample(F, T, d, seed=5)
    lengths = [600, 77, 513, 256]
    dev, lens = _device_sample(x, lengths, "float16")
    assert R.check_exact(_cov(dev, lens, c), x, lengths, c) == []


def test_gaussian_data_with_a_massive_mean_within_the_derived_bound():
    """fp32 N(0, 1) plus a mean of order 10^3 in two dimensions, the centre the engine's own mean: every element within the bound of
    the high-precision reference formed from the same operands, the diagonal within twice gamma_N A_ii of the moments' centred sum
    of squares (both are fp64 sums of the same N fused squares)."""
    x = R.bound_sample()
    F, T, d = x.shape
    dev, lens = _device_sample(x, R.BOUND_LENGTHS, "float32")
    lib = _lib()
    ws = torch.empty(lib.sae_input_stats_workspace_bytes(F, T, d), dtype=torch.uint8, device="cuda")
    mom = torch.empty(4 * d + 2, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sae_input_moments(_p(dev), F, T, d, 0, _p(lens), _p(mom), _p(ws), ws.numel(), s) == 0
    out = _cov(dev, lens, mom[:d])
    moments = mom.cpu().numpy()
    center, css, N = moments[:d].copy(), moments[d:2 * d], int(moments[4 * d + 1])
    assert N == sum(R.counts(F, T, R.BOUND_LENGTHS)) and abs(center[5]) > 900 and abs(center[17]) > 2000
    a = R.operands(x, R.BOUND_LENGTHS, center)
    ref = R.reference(a)
    bad = R.check(out, x, R.BOUND_LENGTHS, center, ref=ref)
    assert bad == [], bad
    A_ii = np.asarray(np.diag(ref[1]), np.float64) / (1.0 - ref[2])
    gap = np.abs(np.diag(out) - css)
    print("max |S_ii - css_i| / (gamma_N A_ii):", float((gap / (R.gamma(N) * A_ii)).max()))
    assert np.all(gap <= 2.0 * R.gamma(N) * A_ii)


@pytest.mark.parametrize("d,frames,dtype", [(80, "ragged", "float16"), (384, "units", "float32")])
def test_the_bytes_depend_on_the_inputs_alone(d, frames, dtype):
    F, T, lengths = FRAMES[frames]
    x = (np.random.default_rng(d).standard_normal((F, T, d)) * 3).astype(np.float32)
    if dtype == "float16":
        x = x.astype(np.float16).astype(np.float32)
    c = np.random.default_rng(d + 1).standard_normal(d)
    dev, lens = _device_sample(x, lengths, dtype)
    first = _cov(dev, lens, c)
    assert np.isfinite(first).all() and first.tobytes() == np.ascontiguousarray(first.T).tobytes()
    assert R.check(first, x, lengths, c) == []
    assert _cov(dev, lens, c).tobytes() == first.tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert _cov(dev, lens, c, stream=side).tobytes() == first.tobytes()
    assert _cov(dev, lens, c, fill=0xFF).tobytes() == first.tobytes()
    big = torch.empty(_lib().sae_input_cov_workspace_bytes(F, T, d) + 4096, dtype=torch.uint8, device="cuda")
    assert _cov(dev, lens, c, ws=big, fill=0x7F).tobytes() == first.tobytes()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    lib = _lib()
    T, d = 4, 8
    x = torch.zeros((1, T, 2049), dtype=torch.float32, device="cuda")
    need = lib.sae_input_cov_workspace_bytes(1, T, d)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = (C.c_int64 * 4)()
    assert lib.sae_input_cov_workspace_bytes(1, T, 2049) == -1 and lib.sae_input_cov_workspace_bytes(0, T, d) == -1
    assert lib.sae_input_cov_plan(1, T, 2049, plan) == -1 and lib.sae_input_cov_plan(1, T, d, None) == -1
    assert lib.sae_input_cov(_p(x), 1, T, 2049, 0, None, None, _p(out), _p(ws), ws.numel(), s) == -1
    assert "d=2049" in lib.sae_last_error().decode()
    assert lib.sae_input_cov(_p(x), 0, T, d, 0, None, None, _p(out), _p(ws), ws.numel(), s) == -1
    assert lib.sae_input_cov(_p(x), 1, T, d, 7, None, None, _p(out), _p(ws), ws.numel(), s) == -1
    assert "x_dtype 7" in lib.sae_last_error().decode()
    assert lib.sae_input_cov(None, 1, T, d, 0, None, None, _p(out), _p(ws), ws.numel(), s) == -1
    assert lib.sae_input_cov(_p(x), 1, T, d, 0, None, None, None, _p(ws), ws.numel(), s) == -1
    assert lib.sae_input_cov(_p(x), 1, T, d, 0, None, None, _p(out), None, ws.numel(), s) == -1
    assert "null argument" in lib.sae_last_error().decode()
    assert need == 64 * 64 * 8 and lib.sae_input_cov(_p(x), 1, T, d, 0, None, None, _p(out), _p(ws), need - 1, s) == -1
    assert "workspace" in lib.sae_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())
    # the same call with the byte it lacked runs
    assert lib.sae_input_cov(_p(x), 1, T, d, 0, None, None, _p(out), _p(ws), need, s) == 0
    torch.cuda.synchronize()
    assert bool((out.view(-1)[:d * d] == 0.0).all()) and bool((out.view(-1)[d * d:] == 7.0).all())
    from freud_amd import engine as E
    with pytest.raises(E.EngineError, match="d=2049"):
        E.input_cov(x, out, ws)
    with pytest.raises(E.EngineError, match="workspace"):
        E.input_cov(x[:, :, :8].contiguous(), out.view(-1)[:64].view(8, 8), ws[:need - 1])
    with pytest.raises(E.EngineError, match="center"):
        E.input_cov(x[:, :, :8].contiguous(), out.view(-1)[:64].view(8, 8), ws, center=torch.zeros(7, dtype=torch.float64, device="cuda"))
    assert E.input_cov_plan(256, 1500, 384) == {"tile": 64, "tiles": 21, "segments": 96, "units_per_segment": 16}
