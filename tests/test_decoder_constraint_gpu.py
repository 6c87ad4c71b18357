"""GPU: the decoder-norm constraint of TopK training (sae_set_decoder_constraint; freud_amd/csrc/dec_norm.h) against the float64 rule and
the derived bounds of tests/decoder_constraint_reference.py, STAGE BY STAGE -- each stage's input is the engine's own output of the stage
before, so every bound is local (the end-to-end map through Adam is ill-conditioned: a purely parallel gradient row leaves rounding
noise, and Adam's first step turns noise into +-lr).

The harness is the injection of tests/test_optimizer_gpu.py: set_params, set_opt_state(t - 1, m, v), the gradient into
grad_tensor()[:nparams], optimizer_step.  The constraint is switched on AFTER the parameters are in place and with keep_rows, so that the
projection sees the rows as they were planted (unit up to 1e-3 relative), not rows the switch renormalised; the switch's own renorm
and set_params' have a test of their own.  Inputs: the family of tests/optimizer_reference.make_inputs with the rows planted by
decoder_constraint_reference.plant_rows (a zero row, a row without gradient, a row whose gradient is exactly 3 w_j) and, in under 1 % of
the elements, a gradient moved so that its projection does not cancel into the range reference_step refuses (lift_small_projections).

    stage 1  projection   grad_tensor()[:nparams] after the step: W_dec's section element by element against the float64 projection of
                          what was injected (padding included: exactly zero), every other section bit-equal to what was injected
    stage 2  update       m', v', metrics[3] and the step against optimizer_reference.reference_step fed the engine's OWN projected
                          gradient; a second engine WITHOUT the constraint gets the same state and that gradient: its W_enc, b_enc, b_dec
                          and moments equal the first engine's to the bit, its W_dec is the pre-renorm value
    stage 3  renorm       the first engine's W_dec against the float64 renorm of that pre-renorm value; the planted zero row and the
                          padding exactly +0.0 (the padding through sae_param_checksum against a fresh engine's, whose padding is the
                          memset's); every other row's norm within the bound of 1
    stage 4  bf16 copy    an evaluation on the first engine equals, to the bit, that of a fresh engine loaded with its get_params()

    shapes (d, n)   (128, 128) half the lanes idle; (100, 200) padded to 128 x 256; (384, 512) one and a half float4 per lane;
                    (1280, 256) five per lane; (384, 3072) many workgroups.  All six KERNEL_CASES on the first three, three on the others.

Then five real steps (sparse gradients of a real backward), two runs bit-equal, the drift without the constraint; "off is off"; the
refusals.  No tolerance here is a measured number."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import tests.test_optimizer_gpu as OG
from freud_amd import engine as E
from tests import decoder_constraint_reference as D
from tests import optimizer_reference as R

pytestmark = pytest.mark.gpu
SEED = 21
ALL, SOME = OG.ALL, OG.SOME
SHAPES = {(128, 128): ALL, (100, 200): ALL, (384, 512): ALL, (1280, 256): SOME, (384, 3072): SOME}
BY_NAME = {c.name: c for c in R.KERNEL_CASES}
WORST = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sections(d, n):
    """Offsets of the flat padded layout: W_enc [n_p][d_p] | b_enc [n_p] | W_dec [n_p][d_p] | b_dec [d_p]."""
    d_p, n_p = OG.round_up(d, 128), OG.round_up(n, 128)
    nW = d_p * n_p
    return d_p, n_p, nW + n_p, 2 * nW + n_p, 2 * nW + n_p + d_p


def pad2(a, n_p, d_p):
    out = np.zeros((n_p, d_p), np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def grad_flat(eng):
    nparams = eng.grad_layout()[0]
    torch.cuda.synchronize()
    return eng.grad_tensor()[:nparams].cpu().numpy().copy()


def with_grad(g, wd_section, d, n):
    """The gradient dict with W_dec taken from the engine's padded section."""
    d_p, n_p, _, _, _ = sections(d, n)
    return dict(g, W_dec=wd_section.reshape(n_p, d_p)[:n, :d].copy())


def track(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def check_projection(after, before, W, d, n, label):
    """Stage 1 on two flat padded gradient buffers and the (unpadded) rows W the projection used -> the projected section."""
    d_p, n_p, o_wd, o_bd, nparams = sections(d, n)
    assert after.size == before.size == nparams
    for lo, hi, what in ((0, o_wd, "W_enc | b_enc"), (o_bd, nparams, "b_dec")):
        assert np.array_equal(bits(after[lo:hi]), bits(before[lo:hi])), f"{label}: the gradient of {what} was touched"
    Gp, Wp = before[o_wd:o_bd].reshape(n_p, d_p), pad2(W, n_p, d_p)
    got = after[o_wd:o_bd].reshape(n_p, d_p)
    ref, tol = D.project(Gp, Wp), D.project_bound(Gp, Wp, d_p)
    r = D.worst_ratio(got, ref, tol)
    print(f"{label}: projection largest |error| / bound {r:.3f}")
    track("project", r)
    bad = D.violations(got, ref, tol)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} projected elements violate; worst |error| / bound {r:.3g}"
    pad = np.ones((n_p, d_p), bool)
    pad[:n, :d] = False
    assert not got[pad].any() and not np.signbit(got[pad]).any(), f"{label}: the padding of the projected gradient is not +0.0"
    return after[o_wd:o_bd]


def check_update(A, B, ref, c, label, t):
    """Stage 2: engine A (constrained) against the reference fed its projected gradient and against engine B (no constraint)."""
    stepA, mA, vA = A.get_opt_state()
    stepB, mB, vB = B.get_opt_state()
    assert stepA == stepB == t
    for what, got in (("m", mA), ("v", vA)):
        r = R.worst_ratio(got, ref, what)
        print(f"{label}: {what} largest |error| / bound {r:.3f}")
        track("update", r)
        assert not any(b.any() for b in R.violations(got, ref, what).values()), f"{label}: " + R.report(got, ref, what)
    total = float(A.metrics()[3])
    assert abs(total - ref["total"]) <= ref["tol_total"], f"{label}: metrics[3] = {total!r}, float64 norm of the projected gradient {ref['total']!r}"
    assert total == float(B.metrics()[3])
    pA, pB = A.get_params(), B.get_params()
    for k in ("encoder.weight", "encoder.bias", "b_dec"):
        assert np.array_equal(bits(pA[k]), bits(pB[k])), f"{label}: {k} differs from the unconstrained engine's"
    for k in mA:                                                            # the moments are neither projected nor rescaled
        assert np.array_equal(bits(mA[k]), bits(mB[k])) and np.array_equal(bits(vA[k]), bits(vB[k])), f"{label}: a moment of {k} differs"
    assert not any(b.any() for b in R.violations(pB, ref, "p").values()), f"{label}: " + R.report(pB, ref, "p")
    return pA, pB


def check_renorm(WA, W_pre, d, n, label, zero_rows=()):
    """Stage 3: WA against the float64 renorm of the pre-renorm rows."""
    d_p = OG.round_up(d, 128)
    ref, tol = D.renorm(W_pre), D.renorm_bound(W_pre, d_p)
    r = D.worst_ratio(WA, ref, tol)
    print(f"{label}: renorm largest |error| / bound {r:.3f}")
    track("renorm", r)
    bad = D.violations(WA, ref, tol)
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} renormalised elements violate; worst |error| / bound {r:.3g}"
    for j in zero_rows:
        assert not WA[j].any() and not np.signbit(WA[j]).any(), f"{label}: the zero row {j} is not +0.0"
    live = np.ones(n, bool)
    live[list(zero_rows)] = False
    nrm = np.sqrt((WA.astype(np.float64) ** 2).sum(1))
    off = np.abs(nrm - 1.0)
    lim = D.row_norm_bound(W_pre, d_p)
    assert (off <= lim)[live].all(), f"{label}: {int((off > lim)[live].sum())} rows off unit norm, worst {off[live].max():.3g} against {lim[live].min():.3g}"


def check_padding_and_copy(A, d, n, c, x, label):
    """Stage 3's padding and stage 4: a fresh engine with A's parameters has the same checksum (its padding is exactly zero) and
    evaluates to the same bits (it makes its bf16 copies from the master; A's W_dec copy was written by the renorm kernel)."""
    pA = A.get_params()
    Cn = OG.make_engine("topk", d, n, c, {})
    try:
        Cn.set_params(pA)
        assert A.param_checksum()[0] == Cn.param_checksum()[0], f"{label}: the padded master differs from a fresh engine's (non-zero padding)"
        A.eval(x)
        lat_a, met_a = A.debug_read(0, x.shape[0] * n).copy(), A.metrics().copy()
        Cn.eval(x)
        lat_c, met_c = Cn.debug_read(0, x.shape[0] * n).copy(), Cn.metrics().copy()
    finally:
        Cn.close()
    assert np.isfinite(met_a[:3]).all() and met_a[0] > 0
    assert np.array_equal(bits(lat_a), bits(lat_c)), f"{label}: latent bits differ"
    assert np.array_equal(bits(met_a[:3]), bits(met_c[:3])), f"{label}: loss scalars {met_a[:3]} against a fresh engine's {met_c[:3]}"


@pytest.mark.parametrize("d,n,case_name", [(d, n, c.name) for (d, n), cases in SHAPES.items() for c in cases])
def test_constrained_step_stage_by_stage(d, n, case_name):
    c = BY_NAME[case_name]
    label = f"({d}, {n}) {case_name}"
    p, g, m, v = D.plant_rows(*R.make_inputs(OG.shapes_of("topk", d, n), c, SEED))
    g, moved = D.lift_small_projections(p, g, c, OG.round_up(d, 128))     # (the precondition of reference_step; float64 rule only)
    assert moved <= g["W_dec"].size // 100
    nrm0 = np.sqrt((p["W_dec"].astype(np.float64) ** 2).sum(1))
    assert np.abs(nrm0 - 1)[np.arange(n) != D.ZERO_ROW].max() <= 1.001e-3 and nrm0[D.ZERO_ROW] == 0
    assert np.array_equal(g["W_dec"][D.PARALLEL_ROW], np.float32(3) * p["W_dec"][D.PARALLEL_ROW]) and not g["W_dec"][D.ZERO_GRAD_ROW].any()
    x = torch.randn(64, d, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    A, B = OG.make_engine("topk", d, n, c, {}), OG.make_engine("topk", d, n, c, {})
    try:
        OG.load_state(A, "topk", d, n, c, p, g, m, v)
        assert A.decoder_constraint is False
        A.set_decoder_constraint(True, keep_rows=True)
        assert A.decoder_constraint is True
        assert all(np.array_equal(bits(a), bits(p[k])) for k, a in A.get_params().items()), "keep_rows left the rows as they were"
        injected = grad_flat(A)
        assert np.array_equal(bits(injected), bits(OG.padded_flat("topk", d, n, g)))
        A.optimizer_step(c.lr, c.scale)
        # stage 1
        wd = check_projection(grad_flat(A), injected, p["W_dec"], d, n, label)
        g2 = with_grad(g, wd, d, n)
        assert not g2["W_dec"][D.ZERO_ROW].any() and not g2["W_dec"][D.ZERO_GRAD_ROW].any()
        # stage 2
        ref = R.reference_step(p, g2, m, v, c)
        OG.load_state(B, "topk", d, n, c, p, g2, m, v)
        B.optimizer_step(c.lr, c.scale)
        pA, pB = check_update(A, B, ref, c, label, c.t)
        # stage 3
        check_renorm(pA["W_dec"], pB["W_dec"], d, n, label, zero_rows=(D.ZERO_ROW,))
        assert not pB["W_dec"][D.ZERO_ROW].any()
        # stage 3 (padding) and stage 4
        check_padding_and_copy(A, d, n, c, x, label)
    finally:
        A.close()
        B.close()


def test_switching_on_and_set_params_renormalise_rows_of_any_norm():
    """The extra case: the constraint enabled on non-unit rows (norms 2^-40 .. 2^40, one zero row) runs the renorm once; so does
    set_params while it is on.  Both against the float64 renorm of the rows that were given."""
    d, n = 100, 200
    c = R.KERNEL_CASES[0]
    p, _, _, _ = R.make_inputs(OG.shapes_of("topk", d, n), c, SEED)
    rng = np.random.default_rng(SEED)
    W = rng.standard_normal((n, d))
    W = W / np.sqrt((W * W).sum(1, keepdims=True)) * 2.0 ** np.linspace(-40, 40, n)[:, None]
    p["W_dec"] = R.f32(W)
    p["W_dec"][D.ZERO_ROW] = 0.0
    x = torch.randn(64, d, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    A = OG.make_engine("topk", d, n, c, {})
    try:
        A.set_params(p)
        A.set_decoder_constraint(True)
        first = A.get_params()
        for k in ("encoder.weight", "encoder.bias", "b_dec"):
            assert np.array_equal(bits(first[k]), bits(p[k])), k
        d_p = OG.round_up(d, 128)
        ref, tol = D.renorm(p["W_dec"]), D.renorm_bound(p["W_dec"], d_p)
        r = D.worst_ratio(first["W_dec"], ref, tol)
        print(f"switch on, wide norms: renorm largest |error| / bound {r:.3f}")
        assert not D.violations(first["W_dec"], ref, tol).any(), r
        assert not first["W_dec"][D.ZERO_ROW].any() and not np.signbit(first["W_dec"][D.ZERO_ROW]).any()
        assert (np.abs(first["W_dec"].astype(np.float64) - p["W_dec"]) > tol).mean() > 0.9, "the rows were far from unit: the renorm shows"
        check_padding_and_copy(A, d, n, c, x, "switch on, wide norms")
        A.set_params(p)                                  # ... while it is on: the same kernel on the same rows
        again = A.get_params()
        assert np.array_equal(bits(again["W_dec"]), bits(first["W_dec"]))
        A.set_decoder_constraint(True)                   # already on: nothing happens (a second renorm would move the rows by an ulp)
        assert np.array_equal(bits(A.get_params()["W_dec"]), bits(first["W_dec"]))
        A.set_decoder_constraint(False)
        A.set_params(p)
        assert np.array_equal(bits(A.get_params()["W_dec"]), bits(p["W_dec"])) and A.decoder_constraint is False
    finally:
        A.close()


# ---- real steps ---------------------------------------------------------------------------------------------------------------------
RD, RN, RK, RROWS, RSTEPS = 128, 256, 8, 256, 5
# Adam's first steps move every element that has a gradient by about lr, a row by about lr sqrt(d): its norm changes by the order of
# lr^2 d / 2 = 8e-3 at lr = 1e-2 -- three orders above the stage 3 norm bound (2^-23 + 67 U = 4.1e-6).  The test still takes nothing on
# trust: it evaluates the float64 rule without the renorm on the engine's own first gradient and asserts that it crosses the bound.
RLR = 1e-2
RCASE = R.Case("adam", 1, R.BETAS[0], 0.0, 1.0, 1.0, False, lr=RLR)


def real_engine():
    eng = E.SaeEngine(variant="topk", d_model=RD, n_dict=RN, max_rows=RROWS, optimizer="adam", clip_thresh=RCASE.thresh, k=RK)
    eng.set_topk_options(1e12, RROWS)
    return eng


def real_init():
    g = torch.Generator().manual_seed(6)
    We = (torch.randn(RN, RD, generator=g) / math.sqrt(RD)).numpy()
    Wd = We / (np.sqrt((We.astype(np.float64) ** 2).sum(1, keepdims=True)) + D.EPS)
    return {"encoder.weight": R.f32(We), "encoder.bias": np.zeros(RN, np.float32), "W_dec": R.f32(Wd), "b_dec": np.zeros(RD, np.float32)}


def real_batches():
    g = torch.Generator().manual_seed(7)
    return [(torch.relu(torch.randn(RROWS, 16, generator=g)) @ torch.randn(16, RD, generator=g) * 0.3).to(torch.bfloat16).cuda()
            for _ in range(RSTEPS)]


def snapshot(eng):
    step, m, v = eng.get_opt_state()
    return eng.get_params(), m, v, step


def assert_same_state(a, b, what):
    assert a[3] == b[3], what
    for i in range(3):
        for k in a[i]:
            assert np.array_equal(bits(a[i][k]), bits(b[i][k])), (what, "pmv"[i], k)


def run_through_step(constrained, toggled=False):
    eng = real_engine()
    try:
        eng.set_params(real_init())
        if constrained:
            eng.set_decoder_constraint(True)
        if toggled:
            eng.set_decoder_constraint(True, keep_rows=True)
            eng.set_decoder_constraint(False)
        mets = []
        for x in real_batches():
            eng.step(x, RLR)
            mets.append(eng.metrics().copy())
        return snapshot(eng), np.stack(mets)
    finally:
        eng.close()


def test_real_steps_stage_by_stage_and_two_runs_bit_equal():
    """Five steps as forward_backward + optimizer_step with a snapshot of the gradient in between: stages 1-3 on the sparse gradients
    of a real backward.  The same five steps through step() -- twice -- end in the same bits."""
    A, B = real_engine(), real_engine()
    try:
        A.set_params(real_init())
        A.set_decoder_constraint(True)
        for s, x in enumerate(real_batches()):
            label = f"real step {s + 1}"
            c = dataclasses.replace(RCASE, t=s + 1)
            p0, m0, v0, t0 = snapshot(A)
            assert t0 == s
            A.forward_backward(x)
            before = grad_flat(A)
            d_p, n_p, o_wd, o_bd, _ = sections(RD, RN)
            gW = before[o_wd:o_bd].reshape(n_p, d_p)
            assert (np.abs(gW).sum(1) > 0).sum() > RN // 4 and np.abs((gW * pad2(p0["W_dec"], n_p, d_p)).sum(1)).max() > 0      # a real gradient
            A.optimizer_step(RLR, 1.0)
            wd = check_projection(grad_flat(A), before, p0["W_dec"], RD, RN, label)
            g2 = {"encoder.weight": before[:n_p * d_p].reshape(n_p, d_p)[:RN, :RD].copy(), "encoder.bias": before[n_p * d_p:o_wd][:RN].copy(),
                  "W_dec": wd.reshape(n_p, d_p)[:RN, :RD].copy(), "b_dec": before[o_bd:][:RD].copy()}
            ref = R.reference_step(p0, g2, m0, v0, c)
            print(f"{label}: norm of the projected gradient {ref['total']:.4g}, clip coefficient {ref['coef']:.4g}")
            B.set_decoder_constraint(False)
            OG.load_state(B, "topk", RD, RN, c, p0, g2, m0, v0)
            B.optimizer_step(RLR, 1.0)
            pA, pB = check_update(A, B, ref, c, label, s + 1)
            check_renorm(pA["W_dec"], pB["W_dec"], RD, RN, label)
        final = snapshot(A)
    finally:
        A.close()
        B.close()
    one, met1 = run_through_step(True)
    two, met2 = run_through_step(True)
    assert_same_state(one, two, "two runs through step()")
    assert np.array_equal(bits(met1), bits(met2))
    assert_same_state(one, final, "step() against forward_backward + optimizer_step")


def test_without_the_constraint_the_rows_leave_the_norm_bound():
    """The same data, the constraint off: after the five steps at least one row is outside the stage 3 norm bound -- the check above can
    fail.  First the float64 rule without the renorm, on the engine's own first gradient, says so; then the engine does."""
    eng = real_engine()
    try:
        p0 = real_init()
        eng.set_params(p0)
        x0 = real_batches()[0]
        eng.forward_backward(x0)
        flat = grad_flat(eng)
        d_p, n_p, o_wd, o_bd, _ = sections(RD, RN)
        g = {"encoder.weight": flat[:n_p * d_p].reshape(n_p, d_p)[:RN, :RD].copy(), "encoder.bias": flat[n_p * d_p:o_wd][:RN].copy(),
             "W_dec": flat[o_wd:o_bd].reshape(n_p, d_p)[:RN, :RD].copy(), "b_dec": flat[o_bd:][:RD].copy()}
    finally:
        eng.close()
    zeros = {k: np.zeros_like(a) for k, a in p0.items()}
    ref = R.reference_step(p0, g, zeros, zeros, RCASE)
    lim = D.row_norm_bound(p0["W_dec"], OG.round_up(RD, 128))
    drift64 = np.abs(np.sqrt((ref["p"]["W_dec"] ** 2).sum(1)) - 1.0)
    assert (drift64 > 10 * lim).sum() > RN // 4, "lr is large enough: the float64 rule without the renorm leaves the bound in one step"
    (p5, _, _, t5), _ = run_through_step(False)
    assert t5 == RSTEPS
    drift = np.abs(np.sqrt((p5["W_dec"].astype(np.float64) ** 2).sum(1)) - 1.0)
    print(f"unconstrained: {int((drift > lim).sum())} of {RN} rows outside the bound, the worst by {drift.max() / lim.min():.0f} x")
    assert (drift > lim).any()


# ---- off is off -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (R.KERNEL_CASES[0], R.KERNEL_CASES[3]), ids=lambda c: c.name)
def test_off_is_off_for_an_injected_update(case):
    """flat_topk_256_512: an engine whose constraint was never set and one that had it switched on and off again give the same bits as
    the update of tests/test_optimizer_gpu.py."""
    _, variant, d, n, kw, _ = OG.CONFIGS["flat_topk_256_512"]
    c, p, g, m, v = OG.family("flat_topk_256_512", case.name)
    outs = []
    for toggled in (False, True):
        eng = OG.make_engine(variant, d, n, c, kw)
        try:
            OG.load_state(eng, variant, d, n, c, p, g, m, v)
            if toggled:
                eng.set_decoder_constraint(True, keep_rows=True)
                eng.set_decoder_constraint(False)
            before = grad_flat(eng)
            eng.optimizer_step(c.lr, c.scale)
            assert np.array_equal(bits(grad_flat(eng)), bits(before)), "no projection: the gradient buffer is as it was injected"
            outs.append((snapshot(eng), eng.metrics().copy()))
        finally:
            eng.close()
    assert_same_state(outs[0][0], outs[1][0], "never set against switched on and off")
    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))
    p1, m1, v1, step, total = OG.updated("flat_topk_256_512", case.name)
    assert_same_state(outs[0][0], (p1, m1, v1, step), "against the update of tests/test_optimizer_gpu.py")
    assert float(outs[0][1][3]) == total


def test_off_is_off_through_step():
    """step() with the constraint never set and with it switched on and off before the first step: the same step count, metrics (the
    clip norm among them: the sum of squares the backward left is still what the update reads) and state."""
    (a, met_a), (b, met_b) = run_through_step(False), run_through_step(False, toggled=True)
    assert a[3] == b[3] == RSTEPS
    assert np.array_equal(bits(met_a), bits(met_b))
    assert_same_state(a, b, "never set against switched on and off")
    assert (met_a[:, 3] > 0).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_l1_and_fp8_contexts_refuse():
    for kw in ({}, {"precision": "fp8"}):
        eng = E.SaeEngine(variant="l1", d_model=256, n_dict=256, max_rows=256, **kw)
        try:
            with pytest.raises(E.EngineError):
                eng.set_decoder_constraint(True)
            assert eng.decoder_constraint is False
        finally:
            eng.close()


def test_zz_largest_error_to_bound_ratio_per_stage():
    """The figures DESIGN.md quotes (run the file with -s): how much of each derived bound the kernels use at the worst element."""
    for name, w in sorted(WORST.items()):
        print(f"largest |error| / bound, {name}: {w:.3f}")
        assert w <= 1.0
