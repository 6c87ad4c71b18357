"""GPU: the input-statistics kernels (freud_amd/csrc/input_stats.h through sae_input_moments / sae_input_median) held to the float64
rule and the derived bounds of tests/input_stats_reference.py: min and max to the bit, the moments within their bounds of math.fsum,
and every Weiszfeld step within the single-step bound of the float64 step from the ENGINE's own previous iterate (never a replay of
the whole iteration).  The shapes are the smallest that reach every path: d = 27 (rows that are not 16-byte aligned, less than a
wave), 260 (one vector beyond the 64 lanes in fp32; unaligned rows in the 2-byte dtypes), 384, 1280; T = 37 and 300 (crosses a
256-frame unit); 5 files; with lengths, the frames that do not count hold NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import input_stats_reference as R

pytestmark = pytest.mark.gpu
FILES, ITER = 5, 8
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _lengths(T):
    return [1, T, T + 7, max(1, T // 2), T - 1]


def _sample(d, T, dtype, with_lengths, files=FILES, seed=None):
    """(x numpy float32/float16 [files, T, d] exact in dtype, the CUDA tensor, lengths list or None, int32 CUDA lengths or None)."""
    x = R.gaussian_sample(files, T, d, seed=(d * 1000 + T) if seed is None else seed, dtype="bfloat16" if dtype == "bfloat16" else dtype)
    lengths = _lengths(T)[:files] if with_lengths else None
    dev = torch.from_numpy(x).to("cuda").to(TORCH[dtype])
    assert torch.equal(dev.float().cpu(), torch.from_numpy(x).float())           # the sample is exact in the engine's input format
    if with_lengths:
        for f, l in enumerate(lengths):
            dev[f, min(l, T):] = float("nan")                                        # frames that do not count must not be read
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda") if with_lengths else None
    return x, dev, lengths, lens


def _run(dev, lens, iterations=ITER):
    from freud_amd.input_stats import sample_statistics
    return sample_statistics(dev, lens, iterations)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("with_lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("T", [37, 300])
@pytest.mark.parametrize("d", [27, 260, 384, 1280])
def test_moments_and_every_step_within_bound(d, T, with_lengths, dtype):
    x, dev, lengths, lens = _sample(d, T, dtype, with_lengths)
    moments, path, obj = _run(dev, lens)
    assert path.shape == (ITER + 1, d) and obj.shape == (ITER + 1,)
    bad = R.check_outputs(x, lengths, moments, path, obj)
    assert bad == [], bad


@pytest.mark.parametrize("d,dtype", [(2047, "float32"), (2048, "float32"), (2048, "bfloat16"), (2046, "float16")])
def test_the_widest_rows(d, dtype):
    """d at the limit: eight vectors per lane in fp32, four in a 2-byte dtype, and the scalar form with its largest LDS block."""
    x, dev, lengths, lens = _sample(d, 37, dtype, True, files=2)
    moments, path, obj = _run(dev, lens, 2)
    assert R.check_outputs(x, lengths, moments, path, obj) == []


def test_identical_rows_give_the_row_to_the_bit():
    row = np.float32(np.random.default_rng(7).standard_normal(384) * 3)
    x = np.tile(row, (FILES, 300, 1))
    moments, path, obj = _run(torch.from_numpy(x).cuda(), None)
    assert np.array_equal(path, np.tile(row.astype(np.float64), (ITER + 1, 1))) and np.array_equal(obj, np.zeros(ITER + 1))
    assert R.check_outputs(x, None, moments, path, obj) == []


def test_one_counted_frame():
    x, dev, _l, _lens = _sample(260, 37, "float32", False, files=1)
    lens = torch.tensor([1], dtype=torch.int32, device="cuda")
    moments, path, obj = _run(dev, lens, 3)
    assert moments[4 * 260 + 1] == 1.0
    assert np.array_equal(path, np.tile(x[0, 0].astype(np.float64), (4, 1))) and np.array_equal(obj, np.zeros(4))
    assert R.check_outputs(x, [1], moments, path, obj) == []


def test_one_iteration():
    x, dev, lengths, lens = _sample(384, 37, "float32", True)
    moments, path, obj = _run(dev, lens, 1)
    assert path.shape == (2, 384) and obj.shape == (2,)
    assert R.check_outputs(x, lengths, moments, path, obj) == []


def test_two_calls_and_a_larger_allocation_give_the_same_bits():
    x, dev, lengths, lens = _sample(1280, 300, "bfloat16", True)
    a = _run(dev, lens)
    b = _run(dev, lens)
    big = torch.full((FILES + 3, 300, 1280), float("nan"), dtype=torch.bfloat16, device="cuda")
    big[:FILES].copy_(dev)
    c = _run(big[:FILES], lens)
    for other in (b, c):
        for u, v in zip(a, other):
            assert u.tobytes() == v.tobytes()
    # the scalar form (an odd base pointer) adds the same numbers in the same order as the register form
    flat = torch.empty(dev.numel() + 1, dtype=torch.bfloat16, device="cuda")
    flat[1:].copy_(dev.reshape(-1))
    e = _run(flat[1:].view(FILES, 300, 1280), lens)
    for u, v in zip(a, e):
        assert u.tobytes() == v.tobytes()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    from freud_amd import engine as E
    lib = E.load()
    d, T, it = 2049, 4, 2
    x = torch.zeros((1, T, d), dtype=torch.float32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * d + 2,), 7.0, dtype=torch.float64, device="cuda")
    path = torch.full((it + 1, d), 7.0, dtype=torch.float64, device="cuda")
    obj = torch.full((it + 1,), 7.0, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.sae_input_stats_workspace_bytes(1, T, d) == -1
    assert lib.sae_input_moments(p(x), 1, T, d, 0, None, p(out), p(ws), ws.numel(), s) == -1
    assert "d=2049" in lib.sae_last_error().decode()
    assert lib.sae_input_median(p(x), 1, T, d, 0, None, p(out), 1.0, it, p(path), p(obj), p(ws), ws.numel(), s) == -1
    d = 8
    assert lib.sae_input_median(p(x), 1, T, d, 0, None, p(out), 1.0, 0, p(path), p(obj), p(ws), ws.numel(), s) == -1
    assert "iterations=0" in lib.sae_last_error().decode()
    assert lib.sae_input_median(p(x), 1, T, d, 0, None, p(out), 1.0, 1025, p(path), p(obj), p(ws), ws.numel(), s) == -1
    assert lib.sae_input_median(p(x), 1, T, d, 0, None, p(out), 0.0, it, p(path), p(obj), p(ws), ws.numel(), s) == -1
    assert lib.sae_input_median(p(x), 1, T, d, 7, None, p(out), 1.0, it, p(path), p(obj), p(ws), ws.numel(), s) == -1
    assert lib.sae_input_moments(p(x), 1, T, d, 0, None, p(out), p(ws), 8, s) == -1          # a short workspace
    assert lib.sae_input_moments(p(x), 0, T, d, 0, None, p(out), p(ws), ws.numel(), s) == -1
    torch.cuda.synchronize()
    for t in (out, path, obj):
        assert bool((t == 7.0).all())
    assert bool((ws == 0).all())
    with pytest.raises(E.EngineError, match="d=2049"):
        E.input_moments(torch.zeros((1, T, 2049), device="cuda"), out, ws)
    with pytest.raises(E.EngineError, match="iterations=0"):
        E.input_median(x[:, :, :8].contiguous(), out[:8], 1.0, 0, path, obj, ws)


def test_input_statistics_end_to_end(tmp_path):
    from freud_amd.input_stats import InputStats, input_statistics
    from freud_amd.loader import write_shards
    T, d, files = 37, 27, 6
    x = R.gaussian_sample(files, T, d, seed=11)
    folder = str(tmp_path / "shards")
    write_shards(folder, "enc", x.reshape(files, T * d), [T, d])
    lengths = [1, T, T + 7, 18, 36]
    torch.manual_seed(123)
    before = torch.get_rng_state()
    st = input_statistics(folder, "enc", files=5, lengths=lengths, iterations=ITER)
    assert torch.equal(torch.get_rng_state(), before)
    rows = R.counted_rows(x[:5], lengths)
    mo = R.moments(rows)
    assert (st.n_files, st.n_frames, st.d) == (5, mo["N"], d)
    assert np.all(np.abs(st.mean - mo["mean"]) <= R.mean_bound(mo))
    assert np.all(np.abs(st.var - mo["var"]) <= R.css_bound(mo) / mo["N"] + R.u64 * mo["var"])
    assert np.array_equal(st.min, mo["min"].astype(np.float32)) and np.array_equal(st.max, mo["max"].astype(np.float32))
    assert st.min.dtype == np.float32
    for name in ("mean_sq_norm", "total_variance", "mean_energy_fraction", "norm_scale"):
        assert getattr(st, name) == pytest.approx(mo[name], rel=1e-12), name
    # the same bytes as the engine's path on the same sample; the init value is its float32
    dev = torch.from_numpy(x[:5]).cuda()
    _m, path, obj = _run(dev, torch.tensor(lengths, dtype=torch.int32, device="cuda"))
    assert st.geometric_median64.tobytes() == path[-1].tobytes() and st.objective.tobytes() == obj.tobytes()
    assert st.geometric_median.dtype == np.float32 and np.array_equal(st.geometric_median, path[-1].astype(np.float32))
    assert st.shift == pytest.approx(np.linalg.norm(path[-1] - path[-2]) / mo["sigma"], rel=1e-9)
    assert list(st.top_dims(2)) == [3, 1]
    p = str(tmp_path / "stats.npz")
    st.save(p)
    back = InputStats.load(p)
    assert back.geometric_median.tobytes() == st.geometric_median.tobytes() and back.n_frames == st.n_frames and back.shift == st.shift
    # more files asked for than the directory holds: all of them
    assert input_statistics(folder, "enc", files=99, iterations=1).n_files == files


def test_command_line(tmp_path, capsys):
    import json
    from freud_amd.input_stats import InputStats, input_statistics, main
    from freud_amd.loader import write_shards
    T, d, files = 37, 27, 3
    folder = str(tmp_path / "shards")
    write_shards(folder, "enc", R.gaussian_sample(files, T, d, seed=12).reshape(files, T * d), [T, d])
    lengths = str(tmp_path / "lengths.npy")
    np.save(lengths, np.array([5, 99, 1]))
    out = str(tmp_path / "stats.npz")
    main(["--data-path", folder, "--layer-name", "enc", "--files", "3", "--iterations", "4", "--lengths", lengths, "--out", out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    st = input_statistics(folder, "enc", files=3, iterations=4, lengths=[5, 99, 1])
    assert line["out"] == out and line["n_frames"] == 5 + T + 1 == st.n_frames and line["iterations"] == 4 and line["top_dims"][:2] == [3, 1]
    assert line["shift"] == st.shift and line["mean_energy_fraction"] == st.mean_energy_fraction
    assert InputStats.load(out).geometric_median64.tobytes() == st.geometric_median64.tobytes()
    main(["--data_path", folder, "--layer_name", "enc", "--iterations", "1"])                   # no --out: the summary alone
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["out"] is None
