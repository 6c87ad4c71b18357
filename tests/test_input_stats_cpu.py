"""CPU: the input statistics' rule (tests/input_stats_reference.py) has the properties a geometric median has; its bounds can fail
(an fp32 emulation of the kernels' arithmetic stays inside them, eight mutations of the rule fall outside); the argument rules of
freud_amd.input_stats.input_statistics and of train()'s "init_b_dec" key raise before any device is needed; and exactly one
translation unit builds the kernels."""
import functools

import numpy as np
import pytest

from tests import input_stats_reference as R
from tests.build_units import assert_one_unit_builds


# ---- properties of the rule ---------------------------------------------------------------------------------------------------
def test_symmetric_points_have_their_centre_as_median():
    rng = np.random.default_rng(0)
    centre = rng.standard_normal(9) * 3
    half = rng.standard_normal((40, 9))
    rows = np.concatenate([centre + half, centre - half])
    path, obj = R.weiszfeld(rows, 32)
    assert np.abs(path[-1] - centre).max() < 1e-12
    assert np.all(np.diff(obj) <= 1e-15 * obj[0])


def test_median_stays_with_the_cluster_when_a_fifth_of_the_rows_moves_away():
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((185, 27))
    rows[:37, 0] += 1000.0
    path, obj = R.weiszfeld(rows, 32)
    mean = rows.mean(0)
    assert np.linalg.norm(mean) > 150 and np.linalg.norm(path[-1]) < 2.0
    assert np.all(np.diff(obj) <= 1e-15 * obj[0])        # (non-increasing up to the float64 rounding of the sums)


@pytest.mark.parametrize("d", [27, 260, 384])
def test_objective_does_not_increase_and_the_iteration_settles(d):
    rows = R.counted_rows(R.gaussian_sample(5, 37, d, seed=d))
    mo = R.moments(rows)
    path, obj = R.weiszfeld(rows, 32)
    assert np.all(np.diff(obj) <= 1e-15 * obj[0])
    assert np.linalg.norm(path[-1] - path[-2]) / mo["sigma"] < 1e-9
    assert min(R.distances(rows, m).min() for m in path) >= 0.5 * mo["sigma"] * (0.2 if d == 27 else 1.0)


def test_identical_rows_give_that_row():
    row = np.float32(np.random.default_rng(2).standard_normal(11) * 5)
    rows = np.tile(row.astype(np.float64), (50, 1))
    path, obj = R.weiszfeld(rows, 4)
    assert np.array_equal(path, np.tile(row.astype(np.float64), (5, 1))) and np.array_equal(obj, np.zeros(5))


def test_lengths_trim_and_count():
    x = R.gaussian_sample(3, 5, 4, seed=3)
    rows = R.counted_rows(x, [1, 5, 9])
    assert rows.shape == (11, 4) and np.array_equal(rows[0], x[0, 0]) and np.array_equal(rows[1:6], x[1]) and np.array_equal(rows[6:], x[2])


# ---- the bounds can fail ------------------------------------------------------------------------------------------------------
LENGTHS = [1, 37, 50, 20, 9]


@functools.lru_cache(maxsize=None)
def _case(kind):
    """The inputs of the emulation tests: `offset` carries an 800-offset dimension that dominates the spread and one with a small
    spread (mutations of the subtraction and of the variance), `equal` is one row repeated (the floor is the only thing between it
    and a division by zero)."""
    if kind == "equal":
        x = np.tile(np.float32(np.random.default_rng(4).standard_normal(27)), (5, 37, 1))
    else:
        x = R.gaussian_sample(5, 37, 27, seed=5)
    rows = R.counted_rows(x, LENGTHS)
    return x, rows, R.moments(rows)


def _failures(kind, mutation):
    x, rows, mo = _case(kind)
    out, path, obj = R.emulate(x, LENGTHS, iterations=8, mutation=mutation)
    try:
        return R.check_outputs(x, LENGTHS, out, path, obj, mo=mo, rows=rows)
    except AssertionError as e:             # (a mutant may walk into the singularity: that is a failure of the mutant too)
        return [str(e)]


@pytest.mark.parametrize("kind", ["offset", "equal"])
def test_fp32_emulation_of_the_kernels_stays_inside_the_bounds(kind):
    assert _failures(kind, None) == []


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_rule_falls_outside(mutation):
    kind = "equal" if mutation == "no_floor" else "offset"
    bad = _failures(kind, mutation)
    assert bad, f"{mutation} passes every check: the bounds cannot fail on it"
    expect = {"inverse_square_weight": "m_1", "no_square_root": "J_0", "no_floor": "identical rows", "start_at_zero": "m_0",
              "uncentred_variance": "css", "untrimmed_lengths": "N", "mean_over_files_T": "mean", "m_rounded_to_fp32": "m_"}[mutation]
    assert any(b.startswith(expect) for b in bad), bad


def test_the_fp32_rounding_of_m_is_what_the_800_offset_catches():
    """The same mutation on a sample without the offset passes: it is the massive dimension that makes the rounding visible."""
    x = R.gaussian_sample(5, 37, 27, seed=5, offset_dim=False)
    out, path, obj = R.emulate(x, LENGTHS, iterations=8, mutation="m_rounded_to_fp32")
    assert R.check_outputs(x, LENGTHS, out, path, obj) == []


# ---- argument rules: all before any device --------------------------------------------------------------------------------------
def _shards(tmp_path, n_files=4, T=6, d=8):
    from freud_amd.loader import write_shards
    folder = str(tmp_path / "shards")
    write_shards(folder, "enc", R.gaussian_sample(n_files, T, d, seed=6).reshape(n_files, T * d), [T, d])
    return folder


def test_input_statistics_argument_rules(tmp_path, monkeypatch):
    import torch
    from freud_amd.input_stats import check_budget, input_statistics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    folder = _shards(tmp_path)
    with pytest.raises(ValueError, match="files=0 must be >= 1"):
        input_statistics(folder, "enc", files=0)
    for it in (0, 1025):
        with pytest.raises(ValueError, match=r"iterations=\d+ outside \[1, 1024\]"):
            input_statistics(folder, "enc", iterations=it)
    # 4 files x 6 frames x 8 dims x 4 bytes = 192 bytes per file
    with pytest.raises(ValueError, match=r"over device_budget_bytes=500: files=2 is the most that fits"):
        input_statistics(folder, "enc", device_budget_bytes=500)
    with pytest.raises(ValueError, match="not even one file fits"):
        input_statistics(folder, "enc", device_budget_bytes=100)
    with pytest.raises(ValueError, match=r"lengths must hold one entry per file \(3\)"):
        input_statistics(folder, "enc", files=3, lengths=[1, 2])
    with pytest.raises(ValueError, match="lengths must be >= 1"):
        input_statistics(folder, "enc", lengths=[1, 2, 0, 4])
    # everything checked: only now the device
    with pytest.raises(RuntimeError, match="input statistics run on the GPU"):
        input_statistics(folder, "enc", lengths=[1, 2, 3, 99])
    check_budget(4, 6, 8, 4, 768)
    with pytest.raises(ValueError, match="files=3 is the most"):
        check_budget(4, 6, 8, 4, 767)


def test_input_statistics_refuses_a_wide_model(tmp_path, monkeypatch):
    import torch
    from freud_amd.input_stats import input_statistics
    from freud_amd.loader import write_shards
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    folder = str(tmp_path / "wide")
    write_shards(folder, "enc", np.zeros((1, 2049), np.float32), [1, 2049])
    with pytest.raises(ValueError, match="d=2049"):
        input_statistics(folder, "enc")


def _train_kwargs(**over):
    kw = dict(seed=0, train_folder="x", val_folder="x", device="cpu", run_dir="x", lr=1e-3, weight_decay=0.0, steps=1, clip_thresh=1.0,
              batch_size=1, dl_max_workers=0, log_tb_every=1, save_every=1, val_every=1, start_checkpoint=None,
              whisper_config={"model": "tiny", "layer_name": "l"}, optimizer="adam", scheduler="cosine", scheduler_params={},
              from_disk=True, autoencoder_variant="topk",
              autoencoder_config={"expansion_factor": 2, "k": 4, "auxk_alpha": 0.0, "dead_feature_threshold": 1.0})
    kw.update(over)
    return kw


def test_init_b_dec_key_rules():
    from freud_amd.train_sae import parse_init_b_dec, train
    assert parse_init_b_dec(None, "topk") is None and parse_init_b_dec(None, "l1") is None
    assert parse_init_b_dec("geometric_median", "topk") == {"method": "geometric_median", "files": 256, "iterations": 32}
    assert parse_init_b_dec({"method": "mean", "files": 7}, "topk") == {"method": "mean", "files": 7, "iterations": 32}
    with pytest.raises(ValueError, match="the tied L1 model has no decoder bias"):
        train(**_train_kwargs(autoencoder_variant="l1", init_b_dec="geometric_median"))
    with pytest.raises(ValueError, match="takes method"):
        train(**_train_kwargs(init_b_dec="median"))
    with pytest.raises(ValueError, match="takes method"):
        train(**_train_kwargs(init_b_dec={"method": "mean", "file": 3}))
    with pytest.raises(ValueError, match="takes method"):
        train(**_train_kwargs(init_b_dec={"files": 3}))
    with pytest.raises(ValueError, match="a method name or an object"):
        train(**_train_kwargs(init_b_dec=3))
    with pytest.raises(ValueError, match=r"iterations=0 outside"):
        train(**_train_kwargs(init_b_dec={"method": "mean", "iterations": 0}))
    with pytest.raises(ValueError, match="files=0 must be"):
        train(**_train_kwargs(init_b_dec={"method": "geometric_median", "files": 0}))
    # a good key passes the rules and reaches the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train(**_train_kwargs(init_b_dec={"method": "geometric_median", "files": 3, "iterations": 4}))


def test_stats_round_trip_and_top_dims(tmp_path):
    from freud_amd.input_stats import InputStats, derive
    x = R.gaussian_sample(5, 37, 27, seed=5)
    out, path, obj = R.emulate(x, LENGTHS, iterations=3)
    st = derive(5, 27, out, path, obj)
    mo = _case("offset")[2]
    assert st.n_frames == mo["N"] and st.n_files == 5 and st.d == 27
    for name in ("mean_sq_norm", "total_variance", "mean_energy_fraction", "norm_scale"):
        assert getattr(st, name) == pytest.approx(mo[name], rel=1e-12), name
    assert st.geometric_median.dtype == np.float32 and np.array_equal(st.geometric_median, path[-1].astype(np.float32))
    assert st.shift == pytest.approx(np.linalg.norm(path[-1] - path[-2]) / mo["sigma"], rel=1e-12)
    assert list(st.top_dims(2)) == [3, 1]            # 800 / 0.25 before 800 / 4
    p = str(tmp_path / "stats.npz")
    st.save(p)
    back = InputStats.load(p)
    for f in ("n_files", "n_frames", "d", "mean_sq_norm", "total_variance", "mean_energy_fraction", "norm_scale", "shift"):
        assert getattr(back, f) == getattr(st, f), f
    for f in ("mean", "var", "min", "max", "geometric_median", "geometric_median64", "objective"):
        a, b = getattr(back, f), getattr(st, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f


def test_cli_arguments():
    import argparse
    from freud_amd.file_pass import add_pass_arguments
    ap = argparse.ArgumentParser()
    add_pass_arguments(ap, sae=False, out_required=False)
    a = ap.parse_args(["--data-path", "D", "--layer-name", "L"])
    assert (a.data_path, a.layer_name, a.out, a.lengths) == ("D", "L", None, None) and not hasattr(a, "sae")
    b = argparse.ArgumentParser()
    add_pass_arguments(b)
    assert b.parse_args(["--sae", "S", "--data_path", "D", "--layer_name", "L", "--out", "O"]).data_path == "D"


def test_one_unit_builds_the_kernels():
    assert assert_one_unit_builds("input_stats.h") == "passes.hip"
