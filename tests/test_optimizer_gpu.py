"""GPU: one optimizer update (sae_optimizer_step) of each of the three kernels, element by element against the float64 reference and
the derived bound of tests/optimizer_reference.py.  The update is isolated: set_params and set_opt_state(t - 1, m, v) give the state,
the gradient is written into grad_tensor()[:nparams] in the engine's padded flat layout (zeros in the padding, nothing past nparams:
the loss scalars live there), optimizer_step(lr, grad_scale) recomputes the clip norm from that buffer -- no forward, no GEMM, no bf16.

    kernel   selected by                          shapes (d, n)
    cols     L1, d_p <= 384                       (128, 128) one pass, 8 column blocks;  (256, 384) two passes, 24 column blocks;
                                                  (384, 256) three passes;  (100, 200) padded to 128 x 256
    tiled    L1, d_p > 384; debug_flags 80        (512, 256);  (384, 256)
    flat     L1 debug_flags 79; TopK              L1 (384, 256);  TopK (256, 512);  TopK (384, 3072): 2 362 752 parameters, the update's
                                                  grid-stride loop and the norm kernel's take a second round;  L1 (384, 3072), flag 79:
                                                  1 182 720 parameters, the norm kernel loops, the update does not

Every kernel sees the six cases of optimizer_reference.KERNEL_CASES (Adam, RAdam not rectified, rectified with and without weight
decay, coef == 1 and coef < 1, grad_scale 1, 1/2 and 1/3, every threshold, both betas); the two large shapes see three of them.  Every
element of p, m and v is compared, metrics[3] is compared with the float64 norm, and the step count is t.  No tolerance here is a
measured number.

Further: the three kernels agree to the bit on a rectified RAdam step with weight decay and coef == 1 and on a clipped Adam step;
norm_on_load (step, eval, step) against the reference that normalises the columns in between; the bf16 copies that leave with the update
against a fresh engine's; and the averaging of the loss scalars by grad_scale (once)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from tests import optimizer_reference as R

pytestmark = pytest.mark.gpu
SEED = 20
ROWS = 128

# name -> (kernel, variant, d, n, engine keywords, cases)
ALL, SOME = R.KERNEL_CASES, (R.KERNEL_CASES[0], R.KERNEL_CASES[3], R.KERNEL_CASES[4])
CONFIGS = {
    "cols_128_128": ("cols", "l1", 128, 128, {}, ALL),
    "cols_256_384": ("cols", "l1", 256, 384, {}, ALL),
    "cols_384_256": ("cols", "l1", 384, 256, {}, ALL),
    "cols_100_200": ("cols", "l1", 100, 200, {}, ALL),
    "tiled_512_256": ("tiled", "l1", 512, 256, {}, ALL),
    "tiled_384_256_flag80": ("tiled", "l1", 384, 256, {"debug_flags": 80}, ALL),
    "flat_384_256_flag79": ("flat", "l1", 384, 256, {"debug_flags": 79}, ALL),
    "flat_topk_256_512": ("flat", "topk", 256, 512, {}, ALL),
    "flat_topk_384_3072": ("flat", "topk", 384, 3072, {}, SOME),
    "flat_384_3072_flag79": ("flat", "l1", 384, 3072, {"debug_flags": 79}, SOME),
}
# the two steps the existing 3-step bitwise check never reached
BITWISE_CASES = (R.RECTIFIED_WD_UNCLIPPED, R.KERNEL_CASES[0])
BY_NAME = {c.name: c for c in R.KERNEL_CASES + (R.RECTIFIED_WD_UNCLIPPED,)}


def round_up(v, m):
    return (v + m - 1) // m * m


def shapes_of(variant, d, n):
    if variant == "l1":
        return {"decoder.weight": (d, n), "encoder_bias": (n,)}
    return {"encoder.weight": (n, d), "encoder.bias": (n,), "W_dec": (n, d), "b_dec": (d,)}


def padded_flat(variant, d, n, arrs):
    """The engine's flat layout: L1 W [d_p][n_p] then b [n_p]; TopK W_enc [n_p][d_p], b_enc [n_p], W_dec [n_p][d_p], b_dec [d_p]; zeros
    in the padding."""
    d_p, n_p = round_up(d, 128), round_up(n, 128)
    parts = []
    for k, a in arrs.items():
        if a.ndim == 2:
            w = np.zeros((d_p, n_p) if variant == "l1" else (n_p, d_p), np.float32)
            w[:a.shape[0], :a.shape[1]] = a
        else:
            w = np.zeros(n_p if a.shape[0] == n and k != "b_dec" else d_p, np.float32)
            w[:a.shape[0]] = a
        parts.append(w.reshape(-1))
    return np.concatenate(parts)


def make_engine(variant, d, n, c, kw):
    eng = E.SaeEngine(variant=variant, d_model=d, n_dict=n, max_rows=ROWS, optimizer=c.opt, clip_thresh=c.thresh, weight_decay=c.wd,
                      betas=c.betas, k=8 if variant == "topk" else 0, **kw)
    if variant == "topk":
        eng.set_topk_options(1e12, ROWS)
    return eng


def inject(eng, variant, d, n, g):
    """The gradient into grad_tensor()[:nparams]; the loss scalars behind it are not touched."""
    vec = padded_flat(variant, d, n, g)
    nparams = eng.grad_layout()[0]
    gt = eng.grad_tensor()
    assert vec.size == nparams and gt.numel() >= nparams + 8
    gt[:nparams].copy_(torch.from_numpy(vec))
    torch.cuda.synchronize()


def load_state(eng, variant, d, n, c, p, g, m, v):
    eng.set_params(p)
    eng.set_opt_state(c.t - 1, m, v)
    inject(eng, variant, d, n, g)


@functools.lru_cache(maxsize=4)            # (deterministic: a miss only computes again; the large cases are not kept)
def family(config, case_name):
    _, variant, d, n, _, _ = CONFIGS[config]
    c = BY_NAME[case_name]
    p, g, m, v = R.make_inputs(shapes_of(variant, d, n), c, SEED)
    return c, p, g, m, v


@functools.lru_cache(maxsize=4)            # (deterministic: a miss only computes again; the large cases are not kept)
def reference(config, case_name):
    c, p, g, m, v = family(config, case_name)
    return R.reference_step(p, g, m, v, c)


@functools.lru_cache(maxsize=4)            # (deterministic: a miss only computes again; the large cases are not kept)
def updated(config, case_name):
    """(p', m', v', step, metrics[3]) of one injected update."""
    _, variant, d, n, kw, _ = CONFIGS[config]
    c, p, g, m, v = family(config, case_name)
    eng = make_engine(variant, d, n, c, kw)
    try:
        load_state(eng, variant, d, n, c, p, g, m, v)
        eng.optimizer_step(c.lr, c.scale)
        p1 = eng.get_params()
        step, m1, v1 = eng.get_opt_state()
        total = float(eng.metrics()[3])
    finally:
        eng.close()
    return p1, m1, v1, step, total


WORST = {}          # kernel -> largest |error| / bound seen, for the report at the end


def check(got, ref, label, kernel):
    p1, m1, v1, total = got
    n = sum(a.size for a in ref["p"].values())
    bad, compared = R.count_violations(p1, m1, v1, ref)
    ratios = [R.worst_ratio(x, ref, w) for x, w in ((p1, "p"), (m1, "m"), (v1, "v"))]
    rn = abs(total - ref["total"]) / ref["tol_total"]
    print(f"{label}: largest |error| / bound  p {ratios[0]:.3f}  m {ratios[1]:.3f}  v {ratios[2]:.3f}  norm {rn:.3f}  ({compared} elements)")
    WORST[kernel] = max([WORST.get(kernel, 0.0), rn] + ratios)
    assert compared == 3 * n, "every element of p, m and v is compared"
    assert bad == 0, f"{label}: " + "; ".join(R.report(x, ref, w) for x, w in ((p1, "p"), (m1, "m"), (v1, "v")))
    assert abs(total - ref["total"]) <= ref["tol_total"], f"{label}: metrics[3] = {total!r}, float64 norm {ref['total']!r}, bound {ref['tol_total']:.3g}"


@pytest.mark.parametrize("config,case_name", [(k, c.name) for k, cfg in CONFIGS.items() for c in cfg[5]])
def test_update_is_inside_the_bound_on_every_element(config, case_name):
    kernel = CONFIGS[config][0]
    c = BY_NAME[case_name]
    ref = reference(config, case_name)
    assert (ref["coef"] < 1.0) == c.clipped and (ref["coef"] == 1.0) == (not c.clipped)
    p1, m1, v1, step, total = updated(config, case_name)
    assert step == c.t
    check((p1, m1, v1, total), ref, f"{config} {case_name}", kernel)


def test_parameter_counts_reach_the_grid_stride_loops():
    """The flat update loops above 2 097 152 parameters (2048 blocks x 256 threads x 4), the norm kernel above 1 048 576."""
    for config, want in (("flat_topk_384_3072", 2362752), ("flat_384_3072_flag79", 1182720)):
        _, variant, d, n, _, _ = CONFIGS[config]
        assert padded_flat(variant, d, n, {k: np.zeros(s, np.float32) for k, s in shapes_of(variant, d, n).items()}).size == want
    assert 2362752 > 2097152 > 1182720 > 1048576


@pytest.mark.parametrize("case", BITWISE_CASES, ids=lambda c: c.name)
def test_three_kernels_agree_to_the_bit(case):
    """The same L1 inputs at (384, 256) through the cols kernel, the tiled one (flag 80) and the flat one (flag 79)."""
    outs = [updated(config, case.name) for config in ("cols_384_256", "tiled_384_256_flag80", "flat_384_256_flag79")]
    c, ref = case, reference("cols_384_256", case.name)
    assert c.rectified and c.wd != 0 and ref["coef"] == 1.0 or c.opt == "adam" and ref["coef"] < 1.0
    check(outs[0][:3] + (outs[0][4],), ref, f"cols_384_256 {case.name}", "cols")        # ... and it is the right answer
    for name, other in zip(("flag 80", "flag 79"), outs[1:]):
        for which, a, b in zip("pmv", outs[0][:3], other[:3]):
            for k in a:
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (name, which, k, int((a[k] != b[k]).sum()))
        assert other[3] == outs[0][3] == c.t and other[4] == outs[0][4]


@pytest.mark.parametrize("d,n", [(384, 256), (128, 128)])
@pytest.mark.parametrize("case", (R.KERNEL_CASES[3], R.KERNEL_CASES[0]), ids=lambda c: c.name)
def test_norm_on_load_against_the_reference_that_normalises_between_the_updates(d, n, case):
    """cols kernel: update, eval (the forward that stands for the in-place normalisation), update.  The second update divides the master
    by the first one's column norms while loading.  Its reference starts from the first update's own output (read from a run without
    the eval: get_params there is the un-normalised update, within the plain bound) and normalises the columns in float64."""
    shapes = shapes_of("l1", d, n)
    c1 = case
    c2 = dataclasses.replace(c1, t=c1.t + 1)
    p, g1, m, v = R.make_inputs(shapes, c1, SEED)
    _, g2, _, _ = R.make_inputs(shapes, c2, SEED + 1)
    x = torch.randn(64, d, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    eng = make_engine("l1", d, n, c1, {})
    try:
        load_state(eng, "l1", d, n, c1, p, g1, m, v)
        eng.optimizer_step(c1.lr, c1.scale)
        pa = eng.get_params()                                    # between the update and any forward: un-normalised
        step, ma, va = eng.get_opt_state()
        assert step == c1.t
        check((pa, ma, va, float(eng.metrics()[3])), R.reference_step(p, g1, m, v, c1), f"norm_on_load {d}x{n} {c1.name}, first update", "cols")
        load_state(eng, "l1", d, n, c1, p, g1, m, v)             # again, this time nothing looks at the master in between
        eng.optimizer_step(c1.lr, c1.scale)
        eng.eval(x)
        inject(eng, "l1", d, n, g2)
        eng.optimizer_step(c2.lr, c2.scale)
        p2 = eng.get_params()
        step, m2, v2 = eng.get_opt_state()
        total = float(eng.metrics()[3])
    finally:
        eng.close()
    assert step == c2.t
    nrm = np.linalg.norm(pa["decoder.weight"].astype(np.float64), axis=0)
    assert (np.abs(nrm - 1) > 1e-3).mean() > 0.9, "nearly all columns are far from unit norm: the division shows"
    ref = R.reference_step(pa, g2, ma, va, c2, normalise="decoder.weight", d_p=round_up(d, 128))
    check((p2, m2, v2, total), ref, f"norm_on_load {d}x{n} {c1.name}, second update", "cols")
    bad, _ = R.count_violations(p2, m2, v2, R.reference_step(pa, g2, ma, va, c2))
    assert bad > d * n // 2, f"an update without the division would pass too ({bad} elements differ)"


def _tame(c, shapes, lr):
    """The family's p, g and m with the second moment a steady run would hold (v = m^2: every update is of the order of lr, none is
    thousands of it), at learning rate lr."""
    p, g, m, v = R.make_inputs(shapes, c, SEED)
    v = {k: m[k] * m[k] for k in v}
    return dataclasses.replace(c, lr=lr), p, g, m, v


@pytest.mark.parametrize("variant,d,n,case", [("topk", 256, 512, R.KERNEL_CASES[0]), ("l1", 384, 256, R.KERNEL_CASES[4])],
                         ids=["topk_256_512", "l1_cols_384_256_rectified"])
def test_bf16_copies_that_leave_with_the_update_are_those_of_a_fresh_engine(variant, d, n, case):
    """TopK: optimizer_kernel's OptCast ranges (We_b, Wd_b).  L1 cols: Wb / Wt of the normalised weights.  Engine A evaluates 64 rows
    on the copies its update wrote; engine B is given A's parameters and makes its own (cast pass; colnorm_partial + normalize_cast).
    Same latent bits, same loss scalars."""
    shapes = shapes_of(variant, d, n)
    c, p, g, m, v = _tame(case, shapes, 0.05 if variant == "topk" else 1.0)      # (rect bc2s / bc1 is 0.03 at the rectified step)
    assert variant == "topk" or c.rectified
    x = torch.randn(64, d, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).cuda()
    a = make_engine(variant, d, n, c, {})
    b = make_engine(variant, d, n, c, {})
    try:
        load_state(a, variant, d, n, c, p, g, m, v)
        a.optimizer_step(c.lr, c.scale)
        pa = a.get_params()                                      # (L1: un-normalised, and the folded state is settled by this read)
        for k in pa:                                             # far more than a bf16 ulp (2^-8 relative): a stale copy would show
            if pa[k].ndim == 2:
                moved = np.abs(pa[k] - p[k]) > 2.0 ** -5 * np.abs(p[k])
                assert moved.mean() > 0.5, (k, moved.mean())
        assert all(np.isfinite(w).all() for w in pa.values())
        load_state(a, variant, d, n, c, p, g, m, v)              # the same update again, and this time the forward reads its copies
        a.optimizer_step(c.lr, c.scale)
        a.eval(x)
        lat_a, met_a = a.debug_read(0, 64 * n).copy(), a.metrics().copy()
        b.set_params(pa)
        b.eval(x)
        lat_b, met_b = b.debug_read(0, 64 * n).copy(), b.metrics().copy()
        b.set_params(p)                                          # and the stale copy does show: the initial weights give another latent
        b.eval(x)
        lat_0 = b.debug_read(0, 64 * n).copy()
    finally:
        a.close()
        b.close()
    assert np.isfinite(lat_a).all() and (lat_a != 0).mean() > 0.005
    assert not np.array_equal(lat_0.view(np.uint32), lat_a.view(np.uint32))
    assert np.array_equal(lat_a.view(np.uint32), lat_b.view(np.uint32)), int((lat_a != lat_b).sum())
    assert np.array_equal(met_a[:3].view(np.uint32), met_b[:3].view(np.uint32)), (met_a, met_b)


def test_loss_scalars_are_averaged_by_grad_scale_once():
    d, n = 384, 256
    c = R.KERNEL_CASES[4]
    p, _, _, _ = R.make_inputs(shapes_of("l1", d, n), c, SEED)
    x = torch.randn(ROWS, d, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()
    eng = make_engine("l1", d, n, c, {})
    try:
        eng.set_params(p)
        eng.forward_backward(x)
        before = eng.metrics().copy()
        eng.optimizer_step(c.lr, 0.5)
        once = eng.metrics().copy()
        eng.optimizer_step(c.lr, 0.5)
        twice = eng.metrics().copy()
    finally:
        eng.close()
    assert np.all(before[:3] > 0) and np.isfinite(before).all()
    assert np.array_equal(once[:3], np.float32(0.5) * before[:3]), (before, once)          # a multiply by 0.5 is exact
    assert np.array_equal(twice[:3], once[:3]), (once, twice)


def test_zz_largest_error_to_bound_ratio_per_kernel():
    """The figure DESIGN.md section 2 quotes (run with -s): how much of the derived bound each kernel uses at the worst element of all
    the comparisons above."""
    if set(WORST) != {"cols", "tiled", "flat"}:              # run on its own: take the comparisons first
        for config, cfg in CONFIGS.items():
            for c in cfg[5]:
                test_update_is_inside_the_bound_on_every_element(config, c.name)
    assert set(WORST) == {"cols", "tiled", "flat"}
    for kernel, w in sorted(WORST.items()):
        print(f"largest |error| / bound, {kernel} kernel: {w:.3f}")
        assert w <= 1.0
