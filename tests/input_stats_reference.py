"""Float64 rule and error bounds of the input statistics (sae_input_moments / sae_input_median; freud_amd/csrc/input_stats.h;
freud_amd/input_stats.py).  Shared by tests/test_input_stats_cpu.py (properties of the rule, an fp32 emulation of the kernels'
arithmetic and mutations of the rule, all held to the bounds below) and the GPU tests (which hold the kernels to them).  Nothing here
is a transcription of the kernels: the rule is the one of the module docstring of freud_amd/input_stats.py, evaluated in float64.

THE RULE.  The sample is the first files of a shard directory; file f counts min(length_f, T) frames (T without lengths); N = the
counted frames, x_i the counted rows as float64.
    mean, var = sum (x_i - mean)^2 / N (centred), min, max, mean_sq_norm = sum |x_i|^2 / N, and on the host total_variance = sum_d var,
    sigma = sqrt(total_variance), mean_energy_fraction = |mean|^2 / mean_sq_norm, norm_scale = sqrt(d / mean_sq_norm)
    Weiszfeld, m_0 = mean:  dist_i = |x_i - m_k|,  w_i = 1 / max(dist_i, floor),  floor = max(2^-20 sigma, FLT_MIN),
    m_{k+1} = sum w_i x_i / sum w_i,  J_k = sum dist_i / N  for k = 0 .. I;  shift = |m_I - m_{I-1}| / sigma

THE BOUNDS.  u = 2^-53 and U = 2^-24 are the unit round-offs of one fp64 / fp32 operation; first-order terms are carried and
multiplied by SLACK = 1.001 for the second-order ones.  Sums are bounded for the WORST order: a sum of n terms, each added with one
rounding (fused into its product or not), is within (n - 1) u sum|terms| of the exact sum whatever the order -- so the bounds hold
for the kernels' order (a chain per thread, the waves of a unit, the units ascending) and for any other.

  moments (truth: math.fsum of the float64 terms)
    sum x        the terms are exact:                                   (N - 1) u sum|x|
    mean         one division more:                                     E_mean = (N - 1) u sum|x| / N + u |mean|
    css          sum (x - mean~)^2 with the engine's own mean~ = mean + e, |e| <= E_mean.  For the exact mean sum (x - mean) = 0, so
                 sum (x - mean~)^2 = css + N e^2 exactly; a term is fl(x - mean~)^2 (relative 2 u) fused into its add (N roundings
                 over the sum), and the truth's own terms carry 3 u:    E_css = (N + 5) u css + N E_mean^2
    sum |x|^2    N d terms, every square exact in fp64:                 (N d - 1) u sum |x|^2
    min, max     exact.

  one Weiszfeld step from a given float64 estimate m (the engine's own m_k, read from its path)
    diff_c = fl32(x_c - m_c): the fp64 difference (u) rounded once to fp32:   relative U (+ u)
    diff_c^2:  2 U from diff, U for the product:                              3 U
    s = the fp32 sum of the d squares, all terms >= 0, any order:             3 U + (d - 1) U = (d + 2) U
       (the padding the kernel adds is +0: s + 0 == s, no rounding)
    dist = sqrtf(s): half the relative error, one rounding:                   E_dist = ((d + 2) / 2 + 1) U
    max(dist, floor): exact where dist >= floor (the tests assert that every row is at least 2^-4 sigma >> floor away from every
       iterate; the degenerate sample of identical rows has floor = FLT_MIN, a power of two, and is checked to the bit instead)
    w = 1.f / that: one rounding:                                             delta = ((d + 2) / 2 + 2) U
    With every weight within a relative delta of its exact value, w~_i = w_i (1 + e_i): m~_j - m'_j = sum w_i e_i (x_ij - m'_j) /
    sum w~_i, so the weighted mean moves by at most 2 delta / (1 - delta) times the weighted mean absolute deviation
    MAD_j = sum w_i |x_ij - m'_j| / sum w_i (the factor 2 is the issue's; delta / (1 - delta) would do).  The fp64 sums add
    (N + 2) u 2 sum w_i |x_ij| / sum w_i (numerator, denominator, division):
        E_m[j] = 2 delta / (1 - delta) MAD_j + 2 (N + 2) u sum w_i |x_ij| / sum w_i
    J = sum dist_i / N, every dist within E_dist, N terms in fp64 and a division:
        E_J = (E_dist + (N + 1) u) J

Never compare an I-iteration result with an I-iteration replay: rounding differences would compound through a map whose contraction
nobody has bounded.  check_outputs compares step by step: the engine's own m_k goes into the float64 single step, the result is held
against the engine's m_{k+1}.
"""
import math

import numpy as np

U = 2.0 ** -24
u64 = 2.0 ** -53
SLACK = 1.001
FLT_MIN = float(np.finfo(np.float32).tiny)
CLEAR = 2.0 ** -4          # every row at least CLEAR * sigma away from every iterate: the condition the step bound is derived under


# ---- the rule in float64 --------------------------------------------------------------------------------------------------------
def counted_rows(x, lengths=None):
    """x [n_files, T, d] (any float dtype, the values exact in float64), lengths per file or None -> the counted rows, float64 [N, d],
    in file order."""
    x = np.asarray(x)
    F, T, _d = x.shape
    cnt = [T] * F if lengths is None else [min(int(l), T) for l in lengths]
    assert all(c >= 1 for c in cnt)
    return np.concatenate([x[f, :cnt[f]].astype(np.float64) for f in range(F)], axis=0)


def _fsum_cols(a):
    return np.array([math.fsum(col) for col in np.ascontiguousarray(a.T)], dtype=np.float64)


def moments(rows):
    """The moments of float64 rows [N, d], sums by math.fsum: dict(N, mean, css, var, min, max, sum_sq, sum_abs, mean_sq_norm,
    total_variance, sigma, mean_energy_fraction, norm_scale)."""
    rows = np.asarray(rows, np.float64)
    N, d = rows.shape
    mean = _fsum_cols(rows) / N
    css = _fsum_cols((rows - mean) ** 2)
    sum_sq = math.fsum((rows * rows).ravel())              # (the square of a value that came from fp32 is exact in fp64)
    var = css / N
    tv = math.fsum(var)
    msn = sum_sq / N
    return {"N": N, "mean": mean, "css": css, "var": var, "min": rows.min(0), "max": rows.max(0), "sum_sq": sum_sq,
            "sum_abs": _fsum_cols(np.abs(rows)), "mean_sq_norm": msn, "total_variance": tv, "sigma": math.sqrt(tv),
            "mean_energy_fraction": math.fsum(mean * mean) / msn if msn > 0 else 0.0,
            "norm_scale": math.sqrt(d / msn) if msn > 0 else float("inf")}


def floor_of(sigma):
    return max(2.0 ** -20 * sigma, FLT_MIN)


def distances(rows, m):
    return np.sqrt(((rows - m) ** 2).sum(1))


def step(rows, m, floor):
    """One Weiszfeld step in float64 from the estimate m: (m_next [d], J at m, dist [N], w [N])."""
    dist = distances(rows, np.asarray(m, np.float64))
    w = 1.0 / np.maximum(dist, floor)
    return (w[:, None] * rows).sum(0) / w.sum(), dist.sum() / rows.shape[0], dist, w


def weiszfeld(rows, iterations=32, start=None, floor=None):
    """The whole rule: (path [I + 1, d], objective [I + 1]) from m_0 = the mean (or `start`)."""
    rows = np.asarray(rows, np.float64)
    mo = moments(rows)
    floor = floor_of(mo["sigma"]) if floor is None else floor
    path = [mo["mean"] if start is None else np.asarray(start, np.float64)]
    obj = []
    for _ in range(iterations):
        m, J, _dist, _w = step(rows, path[-1], floor)
        path.append(m)
        obj.append(J)
    obj.append(distances(rows, path[-1]).sum() / rows.shape[0])
    return np.array(path), np.array(obj)


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
def mean_bound(mo):
    return SLACK * ((mo["N"] - 1) * u64 * mo["sum_abs"] / mo["N"] + u64 * np.abs(mo["mean"]))


def css_bound(mo):
    return SLACK * ((mo["N"] + 5) * u64 * mo["css"] + mo["N"] * mean_bound(mo) ** 2)


def sum_sq_bound(mo, d):
    return SLACK * (mo["N"] * d - 1) * u64 * mo["sum_sq"]


def dist_rel(d):
    return ((d + 2) / 2.0 + 1.0) * U


def weight_rel(d):
    return ((d + 2) / 2.0 + 2.0) * U


def step_bound(rows, m_next, w, d):
    """Per coordinate: how far the kernel's m_{k+1} may lie from step()'s."""
    delta = weight_rel(d)
    sw = w.sum()
    mad = (w[:, None] * np.abs(rows - m_next)).sum(0) / sw
    return SLACK * (2 * delta / (1 - delta) * mad + 2 * (rows.shape[0] + 2) * u64 * (w[:, None] * np.abs(rows)).sum(0) / sw)


def objective_bound(J, N, d):
    return SLACK * (dist_rel(d) + (N + 1) * u64) * J


# ---- an implementation's outputs against the rule ----------------------------------------------------------------------------------
def check_outputs(x, lengths, out_moments, path, objective, mo=None, rows=None):
    """Everything the tests assert of (moments [4 d + 2], path [I + 1, d], objective [I + 1]) computed from x [n_files, T, d] and
    lengths: a list of failures, empty when the outputs are inside every bound.  Also asserts the condition on the inputs: no counted
    row within CLEAR sigma of any iterate of the path (unless sigma == 0: identical rows, held to the bit)."""
    rows = counted_rows(x, lengths) if rows is None else rows
    mo = moments(rows) if mo is None else mo
    N, d = rows.shape
    out_moments, path, objective = (np.asarray(a, np.float64) for a in (out_moments, path, objective))
    bad = []

    def hold(name, got, want, bound):
        err = np.abs(np.asarray(got, np.float64) - want)
        if not np.all(err <= bound):            # (a NaN fails)
            worst = np.nanargmax(np.where(np.isnan(err), np.inf, err / np.maximum(bound, 1e-300))) if np.ndim(err) else 0
            bad.append(f"{name}: error {np.ravel(err)[worst]:.3e} > bound {np.ravel(np.broadcast_to(bound, np.shape(err)))[worst]:.3e}")

    if int(out_moments[4 * d + 1]) != N:
        bad.append(f"N: {out_moments[4 * d + 1]} != {N}")
    hold("mean", out_moments[:d], mo["mean"], mean_bound(mo))
    hold("css", out_moments[d:2 * d], mo["css"], css_bound(mo))
    if not (np.array_equal(out_moments[2 * d:3 * d], mo["min"]) and np.array_equal(out_moments[3 * d:4 * d], mo["max"])):
        bad.append("min / max are not exact")
    hold("sum_sq", out_moments[4 * d], mo["sum_sq"], sum_sq_bound(mo, d))
    if not np.array_equal(path[0], out_moments[:d]):
        bad.append("m_0 is not the engine's own mean")
    floor = floor_of(mo["sigma"])
    I = path.shape[0] - 1
    if mo["sigma"] == 0.0:
        if not (np.array_equal(path, np.broadcast_to(rows[0], path.shape)) and np.array_equal(objective, np.zeros(I + 1))):
            bad.append("identical rows: the path is not that row to the bit, or J != 0")
        return bad
    for k in range(I + 1):
        m_next, J, dist, w = step(rows, path[k], floor)
        assert dist.min() >= CLEAR * mo["sigma"], f"iterate {k}: a row lies within 2^-4 sigma: the bound is not meaningful here"
        hold(f"J_{k}", objective[k], J, objective_bound(J, N, d))
        if k < I:
            hold(f"m_{k + 1}", path[k + 1], m_next, step_bound(rows, m_next, w, d))
    return bad


# ---- an fp32 emulation of the kernels' arithmetic, and mutations of the rule --------------------------------------------------------
MUTATIONS = ("inverse_square_weight", "no_square_root", "no_floor", "start_at_zero", "uncentred_variance", "untrimmed_lengths",
             "mean_over_files_T", "m_rounded_to_fp32")


def emulate(x, lengths=None, iterations=8, mutation=None):
    """What the kernels compute, in numpy with their number formats (fp32 differences, squared distance, root and weight; fp64 sums, in
    numpy's own order) -> (moments [4 d + 2], path, objective).  mutation: one of MUTATIONS, a wrong rule."""
    assert mutation is None or mutation in MUTATIONS
    x = np.asarray(x)
    F, T, d = x.shape
    rows = counted_rows(x, None if mutation == "untrimmed_lengths" else lengths)
    N = rows.shape[0]
    mean = rows.sum(0) / (F * T if mutation == "mean_over_files_T" else N)
    if mutation == "uncentred_variance":
        css = (rows * rows).sum(0) - N * mean * mean
    else:
        css = ((rows - mean) ** 2).sum(0)
    out = np.concatenate([mean, css, rows.min(0), rows.max(0), [(rows * rows).sum(), float(N)]])
    sigma = math.sqrt(max(css.sum(), 0.0) / N)
    floor = np.float32(floor_of(sigma))
    path, obj = [np.zeros(d) if mutation == "start_at_zero" else mean.copy()], []
    f32 = np.float32
    for k in range(iterations + 1):
        m = path[-1]
        if mutation == "m_rounded_to_fp32":
            diff = rows.astype(f32) - m.astype(f32)
        else:
            diff = (rows - m).astype(f32)
        s = (diff * diff).sum(1, dtype=f32)
        dist = s if mutation == "no_square_root" else np.sqrt(s)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = dist if mutation == "no_floor" else np.maximum(dist, floor)
            w = (f32(1) / (den * den if mutation == "inverse_square_weight" else den)).astype(np.float64)
            obj.append(dist.astype(np.float64).sum() / N)
            if k < iterations:
                path.append((w[:, None] * rows).sum(0) / w.sum())
    return out, np.array(path), np.array(obj)


# ---- the tests' inputs ------------------------------------------------------------------------------------------------------------
def gaussian_sample(n_files, T, d, seed, dtype=np.float32, offset_dim=True):
    """Gaussian rows with a per-dimension offset; with offset_dim, dimension 1 is shifted by 800 and carries most of the spread
    (std 4 against 0.25), and dimension 3 (d > 3) is shifted by 800 with std 0.25 -- massive activations.  Rounded to `dtype`
    ("bfloat16": float32 values that bf16 holds exactly), so that the sample is exact in the engine's input format."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_files, T, d)) * 0.25 + rng.standard_normal(d) * 0.5
    if offset_dim:
        x[..., 1] = 800.0 + 4.0 * rng.standard_normal((n_files, T))
        if d > 3:
            x[..., 3] += 800.0
    if dtype == "bfloat16":
        b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
        b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16              # round to nearest even
        return b.astype(np.uint32).view(np.float32).reshape(x.shape)
    return x.astype(dtype)
