"""CPU: the input covariance without a device.

* freud_amd/csrc/input_cov_plan.h compiled for the HOST (g++ -Wall -Werror): every pair i <= j lies in exactly one enumerated tile,
  every unit in exactly one segment, the segments ascending and contiguous, the workspace formula covers the partials and stays within
  the stated bound; freud_amd.input_pca.cov_plan restates the same numbers;
* the reference's bound (tests/input_cov_reference.py) can fail: the emulation of the decomposition passes it and the exact cases,
  each of six mutations of the rule falls outside one of them on the inputs the GPU tests use;
* the host derivations of InputCovariance; the argument and budget refusals, all before any device; the symbols in the header and
  in EXPORTED_SYMBOLS; exactly one translation unit builds the kernels."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import input_cov_reference as R
from tests.build_units import assert_one_unit_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include "input_cov_plan.h"

// plan F T D -> one line of the plan, then "t ti tj" per tile, then "s u0 u1" per segment
int main(int argc, char** argv) {
  if (argc != 4) return 1;
  const long long F = atoll(argv[1]), T = atoll(argv[2]), D = atoll(argv[3]);
  const IcvPlan p = icv_plan(F, T, D);
  printf("%d %d %d %lld %lld %lld %lld %lld %lld\n", ICV_TILE, p.ntd, p.tiles, (long long)p.units_per_file, (long long)p.units,
         (long long)p.units_per_seg, (long long)p.segments, (long long)icv_partial_bytes(p), (long long)ICV_MAX_PARTIAL_BYTES);
  for (int t = 0; t < p.tiles; ++t) {
    int ti, tj;
    icv_tile_of(t, p.ntd, &ti, &tj);
    printf("%d %d %d\n", t, ti, tj);
  }
  for (long long s = 0; s < p.segments; ++s) {
    int64_t u0, u1;
    icv_segment_units(p, s, &u0, &u1);
    printf("%lld %lld %lld\n", s, (long long)u0, (long long)u1);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("icv")
    src = d / "plan.cpp"
    src.write_text(_SRC)
    exe = d / "plan"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


# (n_files, T, d): d = 1, 16, 17, one tile and one beyond, 384, the widest; frame counts below, at and above a segment (at d = 2048
# a segment is a third of the units; at d = 384 it is 16 units of 256 files x 1500 frames; few units give one unit per segment)
PLAN_SHAPES = [(1, 1, 1), (1, 3, 16), (3, 300, 17), (5, 300, 64), (2, 1030, 65), (256, 1500, 384), (256, 1500, 1280), (1, 9, 2048),
               (4, 256, 2048), (4, 257, 2048), (7, 255, 2048), (16, 4096, 384), (17, 4096, 384), (1, 256 * 98, 384), (1, 256 * 98 + 1, 384),
               (65535, 1, 33), (3000, 700, 80)]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plan_header_compiled_for_the_host(prog, shape):
    from freud_amd.input_pca import cov_plan
    F, T, d = shape
    lines = subprocess.run([prog, *map(str, shape)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    tile, ntd, tiles, upf, units, ups, segments, nbytes, max_bytes = (int(v) for v in lines[0].split())
    assert tile == 64 and ntd == -(-d // tile) and tiles == ntd * (ntd + 1) // 2 and upf == -(-T // 256) and units == F * upf
    rows = [tuple(int(v) for v in l.split()) for l in lines[1:]]
    tl, sg = rows[:tiles], rows[tiles:]
    assert len(sg) == segments and [t[0] for t in tl] == list(range(tiles))
    # every pair i <= j in exactly one tile
    cover = np.zeros((d, d), np.int32)
    for _t, ti, tj in tl:
        assert 0 <= ti <= tj < ntd
        blk = cover[ti * tile:(ti + 1) * tile, tj * tile:(tj + 1) * tile]
        blk += np.triu(np.ones(blk.shape, np.int32)) if ti == tj else 1
    assert np.array_equal(cover, np.triu(np.ones((d, d), np.int32)))
    # the segments: ascending, contiguous, none empty, every unit in exactly one
    assert sg[0][1] == 0 and sg[-1][2] == units
    for k, (s, u0, u1) in enumerate(sg):
        assert s == k and u0 < u1 <= u0 + ups and (k == 0 or u0 == sg[k - 1][2])
    # the count: fills the chip where the units allow it, and the partials stay within the stated bound
    assert 1 <= segments <= units and segments * tiles <= max(2048, tiles) and (ups == 1 or -(-units // (ups - 1)) * tiles > 2048)
    assert nbytes == segments * tiles * tile * tile * 8 <= max_bytes == 2048 * 32768
    assert cov_plan(F, T, d) == {"tile": tile, "tiles": tiles, "segments": segments, "units_per_segment": ups, "workspace_bytes": nbytes}


def test_plan_at_the_benchmark_shape_fills_the_chip(prog):
    out = subprocess.run([prog, "256", "1500", "384"], check=True, capture_output=True, text=True).stdout.split("\n")[0].split()
    assert (int(out[2]), int(out[5]), int(out[6])) == (21, 16, 96)          # 21 tiles x 96 segments of 16 units = 2016 workgroups


# ---- the bound can fail ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bound_case():
    x = R.bound_sample()
    rows = R.operands(x, R.BOUND_LENGTHS)
    center = rows.mean(0)                     # (the GPU test takes the engine's own mean; any float64 centre near it serves here)
    return x, center, R.reference(R.operands(x, R.BOUND_LENGTHS, center))


def _bound_failures(mutation):
    x, center, ref = _bound_case()
    return R.check(R.emulate(x, R.BOUND_LENGTHS, center, mutation), x, R.BOUND_LENGTHS, center, ref=ref)


def _exact_failures(mutation, d, frames, with_center=True):
    F, T, lengths = R.FRAME_CASES[frames]
    x, c = R.integer_sample(F, T, d, seed=d * 10 + F)
    c = c if with_center else None
    return R.check_exact(R.emulate(x, lengths, c, mutation), x, lengths, c)


EXACT = [(d, fr) for d in (1, 15, 16, 17, 33, 80, 384) for fr in R.FRAME_CASES]


def test_the_reference_is_wider_than_float64():
    """1 + 2^-60 is no float64 number: the long-double reference holds it, the rational one states its rounding to float64."""
    S, A, e = R.reference(np.array([[1.0], [2.0 ** -30]]))
    if R.LD_OK:
        assert S[0, 0] - 1 == 2.0 ** -60 and A[0, 0] == S[0, 0] and e == R.gamma(2, R.u_ld) < 2.0 ** -62
    else:
        assert float(S[0, 0]) == 1.0 and e == R.u64


def test_the_emulation_stays_inside_the_bound_and_is_exact():
    assert _bound_failures(None) == []
    for d, fr in EXACT:
        assert _exact_failures(None, d, fr) == [], (d, fr)
        assert _exact_failures(None, d, fr, with_center=False) == [], (d, fr)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_rule_falls_outside(mutation):
    where = {"fp32_accumulate": "bound", "center_fp32": "bound", "uncounted_minus_c": ("exact", 17, "ragged"),
             "drop_last_group": ("exact", 33, "long"), "tile_swapped": ("exact", 384, "units"), "unmirrored": ("exact", 15, "three")}[mutation]
    if where == "bound":
        bad = _bound_failures(mutation)
        assert any(b.startswith("bound") for b in bad), f"{mutation} stays inside the bound: it cannot fail"
    else:
        bad = _exact_failures(mutation, where[1], where[2])
        assert bad, f"{mutation} passes the exact case {where[1:]}"
    if mutation == "unmirrored":
        assert any(b.startswith("mirror") for b in _bound_failures(mutation))


def test_the_exact_cases_cover_what_the_mutations_need():
    """A frame count that is no multiple of four, unit tails of one, two and three frames beyond a group of four (what a kernel
    pads), and a file whose length of 0 counts as one frame."""
    assert any(sum(R.counts(F, T, L)) % 4 for F, T, L in R.FRAME_CASES.values())
    tails = {(c - r0) % 4 for F, T, L in R.FRAME_CASES.values() for c in R.counts(F, T, L) for r0 in range(0, c, R.UNIT) if c - r0 < R.UNIT}
    assert {1, 2, 3} <= tails
    assert R.counts(5, 300, [300, 1, 257, 0, 256]) == [300, 1, 257, 1, 256]


def test_the_bound_is_of_the_order_of_float64_rounding():
    x, center, (S, A, e) = _bound_case()
    N = sum(R.counts(*R.BOUND_SHAPE[:2], R.BOUND_LENGTHS))
    lim = R.bound(N, A, e)
    assert N == 681 and float((lim / A).max()) < 682 * 2.0 ** -53 * 1.01 and e <= 2.0 ** -53


# ---- host derivations ----------------------------------------------------------------------------------------------------------------
def _cov(scatter, n_frames=100, center=None, mean=None):
    from freud_amd.input_pca import InputCovariance
    d = scatter.shape[0]
    mean = np.zeros(d) if mean is None else mean
    return InputCovariance(n_files=2, n_frames=n_frames, d=d, center=mean.copy() if center is None else center, mean=mean, scatter=scatter)


def test_a_diagonal_scatter_gives_its_known_curve():
    lam = np.array([1.0, 8.0, 4.0, 2.0, 1.0])                       # descending: 8 4 2 1 1, trace 16
    ic = _cov(np.diag(lam), n_frames=4)
    assert np.array_equal(ic.eigenvalues, [8.0, 4.0, 2.0, 1.0, 1.0])
    assert np.allclose(ic.fvu_curve(), [1.0, 0.5, 0.25, 0.125, 0.0625, 0.0], rtol=0, atol=1e-15)
    assert ic.pca_fvu(0) == 1.0 and ic.pca_fvu(5) == 0.0 and ic.pca_fvu(2) == 0.25
    assert ic.rank_for_fvu(0.25) == 2 and ic.rank_for_fvu(0.2) == 3 and ic.rank_for_fvu(1.0) == 0 and ic.rank_for_fvu(0.0) == 5
    assert ic.participation_ratio == pytest.approx(256.0 / 86.0, rel=1e-15)
    assert np.array_equal(ic.covariance, np.diag(lam) / 4)
    assert np.array_equal(np.abs(ic.components[0]), [0, 1, 0, 0, 0])
    with pytest.raises(ValueError, match="r=6 outside"):
        ic.pca_fvu(6)
    s = ic.summary()
    assert s["center"] == "mean" and s["pca_fvu"] == {} and s["trace"] == 16.0 and "comparable" in s["fvu_about"]
    assert _cov(np.eye(3), center=np.ones(3)).summary()["center"] == "given"
    assert "not comparable" in _cov(np.eye(3), center=np.zeros(3), mean=np.ones(3)).summary()["fvu_about"]


def test_curve_ends_heldout_and_the_clamp():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((200, 40)) * np.linspace(3, 0.1, 40)
    S = a.T @ a
    ic = _cov(S, n_frames=200)
    curve = ic.fvu_curve()
    assert curve[0] == 1.0 and abs(curve[-1]) <= 40 * R.u64 and np.all(np.diff(curve) <= 0)
    tol = 2 * R.solver_error(S) / np.trace(S)
    for r in (0, 1, 7, 40):
        assert abs(ic.heldout_fvu(ic, r) - ic.pca_fvu(r)) <= tol
    assert sorted(ic.summary()["pca_fvu"]) == ["16", "32", "8"]
    # another sample about the same centre: the held-out FVU is at least the other sample's own PCA FVU
    b = rng.standard_normal((150, 40)) * np.linspace(3, 0.1, 40)
    other = _cov(b.T @ b, n_frames=150)
    assert ic.heldout_fvu(other, 5) >= other.pca_fvu(5) - tol
    with pytest.raises(ValueError, match="about THIS sample's centre"):
        ic.heldout_fvu(_cov(S, center=np.ones(40)), 3)
    # a rank-1 scatter: eigenvalues below zero by rounding are clamped
    v = rng.standard_normal(12)
    assert _cov(np.outer(v, v)).eigenvalues.min() == 0.0


def test_save_load_round_trip(tmp_path):
    from freud_amd.input_pca import InputCovariance
    rng = np.random.default_rng(1)
    a = rng.standard_normal((30, 6))
    ic = InputCovariance(n_files=3, n_frames=30, d=6, center=rng.standard_normal(6), mean=a.mean(0), scatter=a.T @ a)
    ic.eigh()
    p = str(tmp_path / "cov.npz")
    ic.save(p)
    back = InputCovariance.load(p)
    assert (back.n_files, back.n_frames, back.d) == (3, 30, 6) and type(back.n_frames) is int
    for f in ("center", "mean", "scatter"):
        assert getattr(back, f).dtype == np.float64 and getattr(back, f).tobytes() == getattr(ic, f).tobytes()
    assert back == ic and back.pca_fvu(2) == ic.pca_fvu(2)


# ---- argument rules: all before any device -----------------------------------------------------------------------------------------
def test_input_covariance_argument_rules(tmp_path, monkeypatch):
    import torch
    from freud_amd.input_pca import cov_extra_bytes, input_covariance
    from freud_amd.loader import write_shards
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    folder = str(tmp_path / "shards")
    write_shards(folder, "enc", R.integer_sample(4, 6, 8, seed=0)[0].reshape(4, 48), [6, 8])
    with pytest.raises(ValueError, match="files=0 must be >= 1"):
        input_covariance(folder, "enc", files=0)
    with pytest.raises(ValueError, match='"mean", "zero" or'):
        input_covariance(folder, "enc", center="median")
    with pytest.raises(ValueError, match="float array"):
        input_covariance(folder, "enc", center=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="float array"):
        input_covariance(folder, "enc", center=np.zeros(8, np.int64))
    # 192 bytes per file; beside them the scatter (512), the moments' block (272) and the workspace (one 32 KiB partial: 4 units)
    extra = cov_extra_bytes(4, 6, 8)
    assert extra == 8 * 8 * 8 + 34 * 8 + 4 * 32768
    with pytest.raises(ValueError, match=rf"beside {extra} bytes of output and workspace, over device_budget_bytes={extra + 500}: files=2 is the most"):
        input_covariance(folder, "enc", device_budget_bytes=extra + 500)
    with pytest.raises(ValueError, match="not even one file fits"):
        input_covariance(folder, "enc", device_budget_bytes=extra)
    with pytest.raises(ValueError, match=r"lengths must hold one entry per file \(3\)"):
        input_covariance(folder, "enc", files=3, lengths=[1, 2])
    # everything checked: only now the device
    with pytest.raises(RuntimeError, match="input covariance runs on the GPU"):
        input_covariance(folder, "enc", lengths=[1, 2, 3, 99])
    wide = str(tmp_path / "wide")
    write_shards(wide, "enc", np.zeros((1, 2049), np.float32), [1, 2049])
    with pytest.raises(ValueError, match="d=2049"):
        input_covariance(wide, "enc")


def test_the_symbols_are_declared_on_both_sides():
    from freud_amd import engine as E
    header = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for name in ("sae_input_cov_workspace_bytes", "sae_input_cov_plan", "sae_input_cov"):
        assert name in E.EXPORTED_SYMBOLS and f" {name}(" in header
    assert all(hasattr(E, n) for n in ("input_cov_workspace_bytes", "input_cov_plan", "input_cov"))


def test_one_unit_builds_the_kernels():
    assert assert_one_unit_builds("input_cov.h") == "passes.hip"
    assert assert_one_unit_builds("input_cov_plan.h") == "passes.hip"
