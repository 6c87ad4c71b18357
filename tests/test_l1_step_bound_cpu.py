"""CPU: the bounds, the partition mirror and the planted inputs of tests/l1_step_reference.py are honest.

* the partition of the fused d = 384 backward covers every (column tile, 32-row step) exactly once and writes exactly the slab pieces
  the reduction adds, for every balanced shape up to 100 tiles x 13 quanta per workgroup x 64 .. 140, 260 and 2048 steps, and for the
  plans of the GPU cases;
* a float32 emulation of the backward on the CPU oracle's forward violates no bound, on one uniform and one balanced plan, and the
  oracle's own forward lies inside the forward bounds; the planted coverage holds there;
* every failure mode of the partition, the piece indexing, the reduction and the gate violates the bounds on the latents it hits;
* the coverage check and the violation check can fail."""
import numpy as np
import pytest

from tests import l1_step_reference as R

EMULATED = ("uniform", "bal_m3")


@pytest.fixture(scope="module")
def emu():
    """name -> (case, operands from the oracle's forward, backward sums, backward reference), computed once."""
    out = {}
    for name in EMULATED:
        case = R.case_of(name)
        ops = R.oracle_operands(case)
        sums = R.backward_sums(ops)
        out[name] = (case, ops, sums, R.backward_reference(ops, case["plan"], sums))
    return out


def test_partition_covers_every_balanced_shape():
    """ntiles 1 .. 100 x m 1 .. 13 x steps 64 .. 140, 260, 2048: exact cover, pieces 0 .. bal_pieces - 1 once each."""
    checked = 0
    for ntiles in range(1, 101):
        for m in range(1, 14):
            for steps in list(range(64, 141)) + [260, 2048]:
                R.check_partition(R.make_plan(1, steps, ntiles, m))
                checked += 1
    assert checked == 100 * 13 * 79


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_partition_of_the_gpu_cases(name):
    plan = R.CASES[name][7]
    wgs = R.partition(plan)
    assert len(wgs) == plan["grid"]
    if plan["balanced"]:
        assert plan["steps"] >= 64 and plan["bal_q"] == (plan["steps"] + 31) // 32 and plan["grid"] <= 256
        assert plan["bal_m"] == (32 * plan["ntiles"] + 255) // 256
        assert all(len(segs) <= 2 for segs in wgs) and R.straddled_tiles(wgs)
    else:
        assert all(len(segs) == 1 for segs in wgs)
    assert (name in ("bal_m3", "bal_scal")) == bool(R.clamped_steps(plan)), "the 68-step batch is the one with a clamped quantum"


def test_partition_mirror_walks_like_the_kernel():
    """The vectorised mirror against the kernel's loop, written out (bwd_fused.h:311-335), on the three balanced GPU shapes."""
    for name in ("bal_m3", "bal_m5", "bal_m12"):
        plan = R.CASES[name][7]
        m, q, steps, ntiles = plan["bal_m"], plan["bal_q"], plan["steps"], plan["ntiles"]
        want = []
        for k in range(plan["grid"]):
            qa, qe, segs = k * m, min(k * m + m, 32 * ntiles), []
            while qa < qe:
                j = qa >> 5
                qb = min(qe, 32 * (j + 1))
                segs.append((j, min((qa - 32 * j) * q, steps), min((qb - 32 * j) * q, steps), k - R.bal_first_wg(j, m)))
                qa = qb
            want.append(segs)
        assert R.partition(plan) == want


def test_loader_rule_against_round_to_nearest():
    x = np.array([-1.0, -1.001, -0.999, -1.0078125, 0.3, 1.0 + 2.0 ** -8, -1.0 - 2.0 ** -9], np.float32)
    got, rne = R.to_bf16_loader(x), R.bf16(x)
    assert got[0] == -1.0 and (got[[1, 2]] != -1.0).all() and (rne[[1, 2]] == -1.0).all()
    assert np.array_equal(got[3:6], rne[3:6]) and got[1] == np.float32(-1.0078125) and got[2] == np.float32(-0.99609375)


@pytest.mark.parametrize("name", EMULATED)
def test_clean_emulation_violates_nothing(emu, name):
    case, ops, sums, ref = emu[name]
    R.assert_coverage(case, ops["c"])
    assert ops["count"] == case["M"] * case["d"] - case["masked"] and case["masked"] >= R.N_MASKED - 2
    fwd = R.forward_reference(ops)
    for key in ("c", "g"):
        assert not R.violations(ops[key], *fwd[key]).any(), R.report(key, ops[key], *fwd[key])
    dW, db = R.emulate(ops, case["plan"])
    assert not R.violations(dW, *ref["dW"]).any(), R.report("dW", dW, *ref["dW"], ref["L"], case["plan"])
    assert not R.violations(db, *ref["db"]).any(), R.report("db", db, *ref["db"], ref["L"], case["plan"])
    assert ref["L"][case["dead"]] == 0 and ref["L"][case["hot"]] == case["M"]
    assert not dW[:, case["dead"]].any() and db[case["dead"]] == 0 and ref["dW"][1][:, case["dead"]].max() == 0
    print(f"\n{name}: worst |difference| / tol   c {R.worst_ratio(ops['c'], *fwd['c']).max():.3f}   g {R.worst_ratio(ops['g'], *fwd['g']).max():.3f}"
          f"   dW {R.worst_ratio(dW, *ref['dW']).max():.3f}   db {R.worst_ratio(db, *ref['db']).max():.3f}")


def _latent(case, kind=None, name=None):
    return next(p for p, v in case["planted"].items() if (kind is None or v[1] == kind) and (name is None or v[0] == name))


def _must_hit(case, ops, ref, mutation):
    """(tile the mutation acts on, latents it must be caught on, tiles the violations must stay in or None), from the case alone."""
    plan, M = case["plan"], case["M"]
    ends, piece = _latent(case, "seg_ends"), _latent(case, "each_piece")
    live = np.flatnonzero(ref["L"] > 0)
    if mutation in ("drop_step", "neighbour_tile"):
        return ends // R.BN, [ends], [ends // R.BN]
    if mutation in ("piece_twice", "piece_missing"):
        return piece // R.BN, [piece], [piece // R.BN]
    if mutation == "drop_last_quantum":
        return None, [case["hot"]] + [p for p, v in case["planted"].items() if v[1] == "row_last"], None
    if mutation == "wrong_piece_count":
        # balanced: tile 0 is reduced with tile 1's count, one piece more, and gets its piece 0 twice; uniform: the last row range is lost
        assert not plan["balanced"] or R.bal_pieces(1, plan["bal_m"]) == R.bal_pieces(0, plan["bal_m"]) + 1
        return None, [case["hot"]] + ([] if plan["balanced"] else [p for p, v in case["planted"].items() if v[1] == "row_last"]), None
    if mutation == "stale_pad_rows":
        assert M % R.FWD_ROWS, "the case has no pad rows"
        return None, [case["hot"]] + [p for p, v in case["planted"].items() if v[1] == "row0"], None
    if mutation == "no_gate":
        return None, [case["dead"]] + list(case["planted"]), None
    if mutation == "no_inv_m":
        return None, list(live), None
    if mutation == "dc_rounded_first":
        # the same two roundings in float64: the latents on which the shift of dW or db is more than 1.2 times the bound
        g, wt, xb = ops["g"].astype(np.float64), ops["wt"].astype(np.float64), ops["xb"].astype(np.float64)
        s = g @ wt.T
        first = np.where(ops["c"] > 0, R.bf16(s).astype(np.float64) + ops["inv_m"], 0.0)
        exact = np.where(ops["c"] > 0, s + ops["inv_m"], 0.0)
        shift_db = (first - exact).sum(0) * ops["scale"]
        shift_dW = xb.T @ (R.bf16(first).astype(np.float64) - exact) * ops["scale"]
        hit = np.flatnonzero((np.abs(shift_db) > 1.2 * ref["db"][1]) | (np.abs(shift_dW) > 1.2 * ref["dW"][1]).any(0))
        assert len(hit) > 0
        return None, list(hit), None
    raise AssertionError(mutation)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("name", EMULATED)
def test_every_failure_mode_violates_the_bound(emu, name, mutation):
    case, ops, sums, ref = emu[name]
    tile, must, stay = _must_hit(case, ops, ref, mutation)
    dW, db = R.emulate(ops, case["plan"], mutation=mutation, tile=tile)
    bad = R.bad_latents(ref, dW, db)
    missed = sorted(set(int(p) for p in must) - set(bad.tolist()))
    assert not missed, f"{mutation}: latents {missed[:10]} ({len(missed)} of {len(must)}) stay inside the bounds"
    if stay is not None:
        assert set((bad // R.BN).tolist()) <= set(stay), f"{mutation} on tile {tile}: violations in tiles {sorted(set((bad // R.BN).tolist()))}"
    if mutation == "no_gate":       # the GPU test's exact check: a dead latent's gradient is +0.0 to the bit
        assert dW[:, case["dead"]].any() and db[case["dead"]] != 0


def test_the_checks_can_fail(emu):
    case, ops, sums, ref = emu["bal_m3"]
    p = _latent(case, "each_piece")
    rows = case["planted"][p][2]
    for change in ((rows[0], p, 0.0), (rows[0], p, 6.0), ((rows[0] + 1) % case["M"], p, 7.0), (3, case["hot"], 0.0), (5, case["dead"], 1.0)):
        c = ops["c"].copy()
        c[change[0], change[1]] = change[2]
        with pytest.raises(AssertionError):
            R.assert_coverage(case, c)
    with pytest.raises(AssertionError):     # a workgroup too few: tile 23 loses its last quanta
        R.check_partition(dict(case["plan"], grid=case["plan"]["grid"] - 1))
    with pytest.raises(AssertionError):     # quanta of two steps reach 64 of the 68 steps
        R.check_partition(dict(case["plan"], bal_q=2))
    dW, db = R.emulate(ops, case["plan"])
    ref_dW, tol_dW = ref["dW"]
    at = np.unravel_index(np.argmax(tol_dW), tol_dW.shape)
    for factor, want in ((0.5, False), (2.0, True)):
        out = ref_dW.copy()
        out[at] += factor * tol_dW[at]
        assert R.violations(out, ref_dW, tol_dW)[at] == want
    out = dW.copy()
    out[7, case["dead"]] = 1e-30            # tol = 0 on a dead latent
    assert R.violations(out, ref_dW, tol_dW)[7, case["dead"]] and "latent %d" % case["dead"] in R.report("dW", out, ref_dW, tol_dW, ref["L"], case["plan"])
    out = db.copy()
    out[p] = np.nan
    assert R.violations(out, *ref["db"])[p]
