"""CPU: the host side of the feature statistics (freud_amd/feature_stats.py): the derived quantities of FeatureStats on hand-built
arrays, the npz round trip, the layout of the engine's output block, argument errors raised before any GPU work, and the new
C-ABI symbol in the library and the header."""
import os
import re

import numpy as np
import pytest

from freud_amd import engine as E
from freud_amd import feature_stats as FST
from freud_amd.loader import write_shards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_stats():
    # 10 frames, 4 latents: latent 0 fires on 5 frames (values 1..5), latent 1 on 1 frame (value 2), latent 2 never,
    # latent 3 on every frame (value 0.5)
    fire = np.array([5, 1, 0, 10], np.int64)
    s = np.array([15.0, 2.0, 0.0, 5.0])
    q = np.array([55.0, 4.0, 0.0, 2.5])
    mx = np.array([5.0, 2.0, 0.0, 0.5], np.float32)
    # latent 1's frame is one of latent 0's: 5 frames with 1 active (latent 3 alone), 4 with 2, 1 with 3
    hist = np.array([0, 5, 4, 1, 0], np.int64)
    return FST.FeatureStats(10, fire, s, q, mx, hist)


def test_derived_quantities():
    st = hand_stats()
    assert st.l0_hist.sum() == st.n_frames
    assert (np.arange(5) * st.l0_hist).sum() == st.fire_count.sum() == 16
    np.testing.assert_array_equal(st.frequency(), [0.5, 0.1, 0.0, 1.0])
    m = st.mean_when_active()
    np.testing.assert_array_equal(m[[0, 1, 3]], [3.0, 2.0, 0.5])
    assert np.isnan(m[2])
    np.testing.assert_array_equal(st.dead(), [False, False, True, False])
    assert st.l0_mean() == pytest.approx(1.6)
    counts, edges, n_dead = st.density_histogram(bins=[-1.5, -0.5, 0.5])
    assert n_dead == 1
    np.testing.assert_array_equal(counts, [1, 2])           # log10 frequency: -1 | -0.301, 0
    counts, edges, _ = st.density_histogram(bins=4)
    assert counts.sum() == 3 and len(edges) == 5
    summ = st.summary()
    assert summ == {"n_frames": 10, "n_latents": 4, "l0_mean": pytest.approx(1.6), "dead": 1, "dense_over_10pct": 2}


def test_empty_stats():
    st = FST.FeatureStats(0, np.zeros(3, np.int64), np.zeros(3), np.zeros(3), np.zeros(3, np.float32), np.zeros(4, np.int64))
    assert np.isnan(st.l0_mean())
    assert st.dead().all() and np.isnan(st.mean_when_active()).all()
    counts, _, n_dead = st.density_histogram(bins=5)
    assert counts.sum() == 0 and n_dead == 3


def test_npz_round_trip(tmp_path):
    st = hand_stats()
    p = str(tmp_path / "s.npz")
    st.to_npz(p)
    back = FST.FeatureStats.from_npz(p)
    assert back.n_frames == st.n_frames and isinstance(back.n_frames, int)
    for k in ("fire_count", "act_sum", "act_sq_sum", "act_max", "l0_hist"):
        a, b = getattr(back, k), getattr(st, k)
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)


def test_block_layout_matches_header():
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    n = 37
    lay = E.stats_layout(n)
    for name, macro in [("n_frames", "N_FRAMES"), ("fire_count", "FIRE_COUNT"), ("act_sum", "ACT_SUM"), ("act_sq_sum", "ACT_SQ_SUM"),
                        ("l0_hist", "L0_HIST"), ("act_max", "ACT_MAX")]:
        m = re.search(rf"#define SAE_STATS_{macro}\(n\) (.+)", text)
        assert m, macro
        expr = m.group(1).replace("(int64_t)", "")
        assert eval(expr, {"n": n}) == lay[name][0], name
    m = re.search(r"#define SAE_STATS_BYTES\(n\) (.+)", text)
    assert eval(m.group(1).replace("(int64_t)", ""), {"n": n}) == lay["bytes"]
    # the fields tile the block without overlap
    fields = [v for k, v in lay.items() if k != "bytes"]
    spans = sorted((off, off + np.dtype(dt).itemsize * cnt) for off, dt, cnt in fields)
    assert spans[0][0] == 0 and spans[-1][1] == lay["bytes"]
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(off % np.dtype(dt).itemsize == 0 for off, dt, _ in fields)


def test_from_block_reads_the_layout():
    n = 5
    lay = E.stats_layout(n)
    blk = np.zeros(lay["bytes"], np.uint8)
    vals = {"n_frames": np.array([42]), "fire_count": np.arange(n), "act_sum": np.linspace(0, 1, n), "act_sq_sum": np.linspace(2, 3, n),
            "l0_hist": np.arange(n + 1) * 7, "act_max": np.linspace(4, 5, n)}
    for k, v in vals.items():
        off, dt, cnt = lay[k]
        blk[off:off + np.dtype(dt).itemsize * cnt] = np.asarray(v, dt).view(np.uint8)
    st = FST.FeatureStats.from_block(blk, n)
    assert st.n_frames == 42
    np.testing.assert_array_equal(st.fire_count, vals["fire_count"])
    np.testing.assert_array_equal(st.act_sum, vals["act_sum"])
    np.testing.assert_array_equal(st.act_sq_sum, vals["act_sq_sum"])
    np.testing.assert_array_equal(st.l0_hist, vals["l0_hist"])
    np.testing.assert_array_equal(st.act_max, vals["act_max"].astype(np.float32))


def _shards(tmp_path, F=4, T=10, d=16):
    x = np.random.default_rng(0).normal(size=(F, T * d)).astype(np.float32)
    write_shards(str(tmp_path), "enc", x, [T, d])
    return str(tmp_path)


def _fake_engine(d, n, precision):
    """A SaeEngine instance that never touched a device: the argument checks read only these attributes."""
    eng = E.SaeEngine.__new__(E.SaeEngine)
    eng.variant, eng.d, eng.n, eng.max_rows, eng.device_id, eng.precision = "l1", d, n, 1500, 0, precision
    eng._ctx = None
    return eng


def test_argument_errors(tmp_path):
    path = _shards(tmp_path)
    eng = _fake_engine(16, 64, "bf16")
    with pytest.raises(ValueError, match="batch_files"):
        FST.feature_stats(eng, path, "enc", batch_files=0)
    with pytest.raises(ValueError, match="one entry per file"):
        FST.feature_stats(eng, path, "enc", lengths=np.array([3, 4]))
    with pytest.raises(ValueError, match=">= 1"):
        FST.feature_stats(eng, path, "enc", lengths=np.array([3, 0, 4, 5]))
    with pytest.raises(ValueError, match="integers"):
        FST.feature_stats(eng, path, "enc", lengths=np.array([3.0, 1.0, 4.0, 5.0]))
    with pytest.raises(ValueError, match="bf16"):
        FST.feature_stats(_fake_engine(16, 64, "fp8"), path, "enc")
    with pytest.raises(ValueError, match="d_model=32"):
        FST.feature_stats(_fake_engine(32, 64, "bf16"), path, "enc")
    with pytest.raises(ValueError, match="need an SAE"):
        FST.feature_stats(None, path, "enc")
    with pytest.raises(TypeError):
        FST.feature_stats(object(), path, "enc")


def test_stats_symbol_exported_and_declared():
    E.build()
    lib = E.load()
    assert hasattr(lib, "sae_stats_files")
    assert "sae_stats_files" in E.EXPORTED_SYMBOLS
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert re.search(r"\bint sae_stats_files\(", text)
    assert "SAE_STATS_UNFUSED = 1" in text and E.STATS_UNFUSED == 1
