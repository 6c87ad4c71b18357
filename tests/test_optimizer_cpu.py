"""CPU: the bound of tests/optimizer_reference.py is right and can fail.

Right: on the whole input family torch's own optimizers (torch.nn.utils.clip_grad_norm_, then torch.optim.Adam / torch.optim.RAdam with
foreach=False, fp32, put at step t through their state) and an fp32 numpy emulation of the update (the op order of the engine's
adam_update4 and of its clip coefficient, one rounding per operation; test code, no import of the kernel) stay inside the bound around
the float64 restatement on EVERY element of p, m and v.

Can fail: each of twelve mutations of the emulation leaves the bound on at least one element of every case it applies to.  Which cases a
mutation applies to is decided by the rule, not by the outcome: `APPLIES` below (a mutation of the rectified branch applies to the
rectified cases, one of the clip to the cases on the side of the threshold where it acts, ...).  The family has no case at t = 1000
with betas (0.8, 0.99): there b1^t and b2^t are below 5e-5, the rule has converged and `bias correction at t - 1` changes nothing that
fp32 can see.  `rho_t >= 5` against `> 5` is no mutation here: no integer step has rho_t == 5 (asserted below)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import optimizer_reference as R

F = np.float32
SHAPES = {"decoder.weight": (48, 80), "encoder_bias": (80,)}        # 3920 parameters: 245 groups of 16, every residue of the family
SEED = 20
CASES = {c.name: c for c in R.CPU_CASES}
assert len(CASES) == len(R.CPU_CASES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    p, g, m, v = R.make_inputs(SHAPES, c, SEED)
    return c, p, g, m, v, R.reference_step(p, g, m, v, c)


MUTATIONS = ("bc2_for_its_sqrt", "eps_inside_sqrt", "adam_eps_as_radam", "bias_correction_at_t_minus_1", "rect_omitted",
             "wd_after_moments", "wd_decoupled", "clip_without_min", "clip_by_unscaled_norm", "scale_on_g_not_on_norm",
             "scale_on_norm_not_on_g", "one_group_skipped")
APPLIES = {
    "bc2_for_its_sqrt": lambda c: c.opt == "adam" or c.rectified,
    "eps_inside_sqrt": lambda c: c.opt == "adam" or c.rectified,
    "adam_eps_as_radam": lambda c: c.opt == "adam",
    "bias_correction_at_t_minus_1": lambda c: True,
    "rect_omitted": lambda c: c.rectified,
    "wd_after_moments": lambda c: c.opt == "radam" and c.wd != 0,
    "wd_decoupled": lambda c: c.opt == "radam" and c.wd != 0,
    "clip_without_min": lambda c: not c.clipped,                          # thresh / norm = 4 is applied as it is
    "clip_by_unscaled_norm": lambda c: c.clipped and c.scale != 1.0,      # (not clipped: the unscaled norm is below thresh too)
    "scale_on_g_not_on_norm": lambda c: c.scale != 1.0,                   # the same, and the published norm is unscaled as well
    "scale_on_norm_not_on_g": lambda c: c.scale != 1.0,
    "one_group_skipped": lambda c: True,
}
SKIPPED_GROUP = 4 * 301        # flat elements [1204, 1208)


def emulate(p, g, m, v, c, mutation=None):
    """One update in float32 numpy, every operation rounded once, in the order of the engine's kernels:
        total = sqrtf((float) sum_double(fl(fl(g scale) fl(g scale))));  coef = fminf(thresh / (total + 1e-6f), 1)
        gj = fl(fl(g scale) coef) [+ fl(wd p)];  m += w1 (gj - m);  v = fl(v b2) + fl(fl(w2 gj) gj);  then the three branches.
    -> (p', m', v' as dicts, total)."""
    like = p
    p, g, m, v = (R.flat(d).astype(F) for d in (p, g, m, v))
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    b1, b2 = c.betas
    h = R.host_scalars(c, c.t - 1 if mutation == "bias_correction_at_t_minus_1" else c.t)
    lr, scale, thresh, wd, eps = F(c.lr), F(c.scale), F(c.thresh), F(c.wd), F(c.eps)
    w1, w2, beta2 = F(1.0 - b1), F(1.0 - b2), F(b2)
    with np.errstate(all="ignore"):
        bc1 = F(h["bc1"])
        bc2s = F(h["bc2"]) if mutation == "bc2_for_its_sqrt" else F(np.sqrt(h["bc2"]))
        step_size = F(c.lr / h["bc1"]) if h["bc1"] != 0 else F(np.inf)
        rect, rectify = F(h["rect"]), h["rho_t"] > 5.0
        gs = g if mutation == "scale_on_norm_not_on_g" else g * scale
        gn = g if mutation in ("clip_by_unscaled_norm", "scale_on_g_not_on_norm") else g * scale
        total = np.sqrt(F((gn * gn).astype(np.float64).sum()))
        coef = thresh / (total + F(1e-6))
        if mutation != "clip_without_min":
            coef = min(coef, F(1.0))
        if mutation == "clip_by_unscaled_norm":                 # only the coefficient comes from the unscaled gradient
            total = np.sqrt(F(((g * scale) * (g * scale)).astype(np.float64).sum()))
        gj = gs * coef
        if c.opt == "radam" and c.wd != 0 and mutation not in ("wd_after_moments", "wd_decoupled"):
            gj = gj + wd * p
        if mutation == "wd_decoupled":
            p = p * F(1.0 - c.lr * c.wd)
        m = m + w1 * (gj - m)
        v = v * beta2
        v = v + (w2 * gj) * gj
        num = m + wd * p if mutation == "wd_after_moments" else m
        root = np.sqrt(v + eps) if mutation == "eps_inside_sqrt" else None
        if c.opt == "radam":
            mh = num / bc1
            if rectify:
                adaptive = (F(1.0) / (root if root is not None else np.sqrt(v) + eps)) * bc2s
                upd = (mh * lr) * adaptive
                p = p - (upd if mutation == "rect_omitted" else upd * rect)
            else:
                p = p - mh * lr
        elif mutation == "adam_eps_as_radam":
            p = p + ((-step_size * num) * bc2s) / (np.sqrt(v) + eps)
        else:
            denom = root / bc2s if root is not None else np.sqrt(v) / bc2s + eps
            p = p + (-step_size * num) / denom
    if mutation == "one_group_skipped":
        k = slice(SKIPPED_GROUP, SKIPPED_GROUP + 4)
        p[k], m[k], v[k] = p0[k], m0[k], v0[k]
    assert p.dtype == m.dtype == v.dtype == F and np.asarray(total).dtype == F
    return R.unflat(p, like), R.unflat(m, like), R.unflat(v, like), float(total)


def torch_step(p, g, m, v, c):
    """clip_grad_norm_ and one step of torch's own optimizer at step c.t (its state preloaded with step = t - 1 and the moments)."""
    params = [torch.nn.Parameter(torch.from_numpy(p[k].copy())) for k in p]
    for q, k in zip(params, p):
        q.grad = torch.from_numpy(g[k].copy())
        if c.scale != 1.0:
            q.grad.mul_(c.scale)
    if c.opt == "adam":
        opt = torch.optim.Adam(params, lr=c.lr, betas=c.betas, eps=c.eps, foreach=False)
    else:
        opt = torch.optim.RAdam(params, lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd, foreach=False)
    for q, k in zip(params, p):
        opt.state[q] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": torch.from_numpy(m[k].copy()),
                        "exp_avg_sq": torch.from_numpy(v[k].copy())}
    total = torch.nn.utils.clip_grad_norm_(params, c.thresh, foreach=False)
    opt.step()
    for q in params:
        assert float(opt.state[q]["step"]) == c.t
    return ({k: q.detach().numpy() for q, k in zip(params, p)}, {k: opt.state[q]["exp_avg"].numpy() for q, k in zip(params, p)},
            {k: opt.state[q]["exp_avg_sq"].numpy() for q, k in zip(params, p)}, float(total))


def _all_inside(got, ref, who, name):
    pp, mm, vv, total = got
    bad, n = R.count_violations(pp, mm, vv, ref)
    assert n == 3 * sum(int(np.prod(s)) for s in SHAPES.values()), "every element of p, m and v is compared"
    assert bad == 0, f"{who}, case {name}: " + "; ".join(R.report(x, ref, w) for x, w in ((pp, "p"), (mm, "m"), (vv, "v")))
    if who != "torch":
        assert abs(total - ref["total"]) <= ref["tol_total"], (who, name, total, ref["total"], ref["tol_total"])


def test_the_family_is_what_the_issue_asks_for():
    seen = {"clip": set(), "opt": set(), "t": set(), "betas": set(), "scale": set(), "thresh": set(), "wd": set()}
    for name in CASES:
        c, p, g, m, v, ref = inputs(name)
        assert (ref["coef"] == 1.0) == (not c.clipped) and (ref["coef"] < 1.0) == c.clipped, name    # which side, from the reference
        gf, mf, vf = R.flat(g), R.flat(m), R.flat(v)
        i = np.arange(gf.size)
        assert np.array_equal(gf == 0, i % 16 == 5) and np.array_equal(vf == 0, (i % 32 == 5) | (i % 32 == 25))
        assert ((gf == 0) & (vf == 0) & (mf == 0)).any() and ((gf == 0) & (vf == 0) & (mf != 0)).any()
        big = np.sort(np.abs(gf))[::-1]
        assert np.all(np.abs(gf[8:12]) == big[0]) and big[4] < big[0] / 50, "four elements decide the clip"
        gp = gf.astype(np.float64) * c.scale * ref["coef"]
        sel = (i % 4 == 2) & (i % 64 != 5)
        assert np.array_equal(mf[sel], gp[sel].astype(F)) and sel.mean() > 0.23                      # m = g': g' - m cancels
        for k, val in (("clip", c.clipped), ("opt", (c.opt, c.rectified, c.wd != 0)), ("t", c.t), ("betas", c.betas),
                       ("scale", c.scale), ("thresh", c.thresh), ("wd", c.wd)):
            seen[k].add(val)
    assert seen["clip"] == {True, False} and seen["t"] == {1, 5, 6, 7, 1000} and seen["betas"] == set(R.BETAS)
    assert seen["scale"] == {1.0, 0.5, 1.0 / 3.0} and seen["thresh"] == {1.0, 1e-3, 1e6} and seen["wd"] == {0.0, 0.01}
    assert seen["opt"] >= {("adam", False, False), ("radam", False, False), ("radam", False, True), ("radam", True, False),
                           ("radam", True, True)}
    for c in R.KERNEL_CASES:                  # what every kernel sees on the GPU is part of what is vouched for here
        assert c.name in CASES
    ks = R.KERNEL_CASES
    assert {c.clipped for c in ks} == {True, False} and any(c.scale != 1 for c in ks) and any(c.opt == "adam" for c in ks)
    assert {(c.rectified, c.wd != 0) for c in ks if c.opt == "radam"} >= {(False, False), (True, False), (True, True)}


def test_rectification_switches_at_step_6_and_rho_is_never_5():
    """`rho_t >= 5` and `rho_t > 5` rectify the same steps for both beta2 of the family: no step separates them."""
    for betas in R.BETAS:
        c = R.Case("radam", 1, betas, 0.0, 1.0, 1.0, False)
        rho = [R.host_scalars(c, t)["rho_t"] for t in range(1, 2001)]
        assert all(r != 5.0 for r in rho) and [r > 5.0 for r in rho] == [r >= 5.0 for r in rho]
        assert not rho[4] > 5.0 and rho[5] > 5.0 and min(abs(r - 5.0) for r in rho) > 1e-3


def test_the_build_passes_no_fast_math_flag():
    """The bound counts divide and sqrt as correctly rounded and every rounding as relative: true as long as the build asks for nothing
    else."""
    mk = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "freud_amd", "csrc", "Makefile")).read()
    for flag in ("fast-math", "-Ofast", "unsafe-math", "reciprocal-math", "approx-func", "finite-math", "flush-denormals",
                 "no-hip-fp32-correctly-rounded", "approx-transcendentals", "associative-math", "fp-model", "-cl-"):
        assert flag not in mk, flag


@pytest.mark.parametrize("name", sorted(CASES))
def test_torch_optimizers_stay_inside_the_bound(name):
    """torch's norm is an fp32 sum in an order of the host's choosing: it is held to (n + 3) u, the elements to the bound with the norm's
    error widened by what torch's norm is off (optimizer_reference.py, last paragraph)."""
    c, p, g, m, v, ref = inputs(name)
    got = torch_step(p, g, m, v, c)
    n = sum(a.size for a in p.values())
    off_u = abs(got[3] / ref["total"] - 1.0) / R.U
    assert off_u <= n + 3, (name, got[3], ref["total"])
    print(f"{name}: torch's norm is off by {off_u:.2f} u")
    _all_inside(got, R.reference_step(p, g, m, v, c, norm_extra_u=off_u), "torch", name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_emulation_stays_inside_the_bound(name):
    c, p, g, m, v, ref = inputs(name)
    _all_inside(emulate(p, g, m, v, c), ref, "fp32 emulation", name)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_leaves_the_bound(mutation):
    applies = [n for n in sorted(CASES) if APPLIES[mutation](CASES[n])]
    assert len(applies) >= 3, (mutation, applies)
    for name in applies:
        c, p, g, m, v, ref = inputs(name)
        pp, mm, vv, total = emulate(p, g, m, v, c, mutation)
        bad, n = R.count_violations(pp, mm, vv, ref)
        norm_off = not abs(total - ref["total"]) <= ref["tol_total"]
        if mutation == "scale_on_g_not_on_norm" and not c.clipped:      # coef is 1 either way: it is the published norm that is wrong
            assert norm_off, f"{mutation}, case {name}: the norm {total!r} is inside the bound around {ref['total']!r}"
        else:
            assert bad > 0, f"{mutation}, case {name}: 0 of {n} elements leave the bound"
        print(f"{mutation:30s} {name:40s} {bad:6d} of {n} elements leave the bound{', the norm too' if norm_off else ''}")


def _colnorm_fp32(W):
    """Column norms of W [d_p][n] in float32 in the order of the engine's canonical partial sums: per slab of 32 rows and y in 0..7 a
    chain of four fused multiply-adds over rows y, y + 8, y + 16, y + 24, a tree over the eight, the slabs in order."""
    d_p, n = W.shape
    tot = np.zeros(n, F)
    for s0 in range(0, d_p, 32):
        r = []
        for y in range(8):
            ss = np.zeros(n, F)
            for k in range(4):
                w = W[s0 + y + 8 * k].astype(np.float64)
                ss = (w * w + ss.astype(np.float64)).astype(F)          # fma: the product is exact in double, one rounding
            r.append(ss)
        tot = tot + (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))
    return np.maximum(np.sqrt(tot), F(1e-12))


@pytest.mark.parametrize("name", [c.name for c in R.KERNEL_CASES])
def test_norm_on_load_emulation_stays_inside_the_bound(name):
    """The division by the fp32 column norms in front of the update, taken in the engine's order of summation (d_p = 128 rows; column
    norms from 0.3 to 30, one column all zero): inside the bound with E_pin, and both leaving the division out and leaving E_pin's
    reference un-normalised are far outside."""
    c = CASES[name]
    shapes = {"decoder.weight": (128, 24), "encoder_bias": (24,)}
    p, g, m, v = R.make_inputs(shapes, c, SEED + 1)
    p["decoder.weight"] = (p["decoder.weight"] * np.linspace(0.3, 30.0, 24, dtype=F)).astype(F)
    p["decoder.weight"][:, 7] = 0.0                                       # max(||col||, 1e-12): 0 / 1e-12 = 0
    ref = R.reference_step(p, g, m, v, c, normalise="decoder.weight", d_p=128)
    plain = R.reference_step(p, g, m, v, c)
    pn = dict(p)
    pn["decoder.weight"] = (p["decoder.weight"] / _colnorm_fp32(p["decoder.weight"])).astype(F)
    pp, mm, vv, _ = emulate(pn, g, m, v, c)
    bad, n = R.count_violations(pp, mm, vv, ref)
    assert bad == 0, f"case {name}: " + "; ".join(R.report(x, ref, w) for x, w in ((pp, "p"), (mm, "m"), (vv, "v")))
    bad, _ = R.count_violations(pp, mm, vv, plain)
    assert bad > 1000, f"case {name}: the normalisation is invisible to the bound ({bad} elements)"
    pu, mu, vu, _ = emulate(p, g, m, v, c)
    bad, _ = R.count_violations(pu, mu, vu, ref)
    assert bad > 1000, f"case {name}: an update without the normalisation passes ({bad} elements)"
