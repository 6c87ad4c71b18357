"""Float64 rule and per-element error bounds of the decoder-norm constraint of TopK training (sae_set_decoder_constraint;
freud_amd/csrc/dec_norm.h: topk_dec_project_kernel, topk_dec_renorm_kernel).  Shared by tests/test_decoder_constraint_cpu.py (which
holds the rule to the real reference model's two functions, to an fp32 emulation of the kernels and to mutations of the rule) and the
GPU tests (which hold the kernels to it, stage by stage).  Nothing here is a transcription of the kernels: the rule is the reference
model's (topkautoencoder.py:153-175), evaluated in float64.

    project   g_j <- g_j - (g_j . w_j) w_j                        every row j of W_dec[n][d]; no division by |w_j|^2
    update    clip_grad_norm_ of the PROJECTED gradients, then Adam / RAdam: tests/optimizer_reference.py, unchanged
    renorm    w_j <- w_j / (||w_j||_2 + EPS),  EPS = 2^-23         torch.finfo(float32).eps; a zero row stays zero

THE BOUNDS, in the manner of tests/optimizer_reference.py: U = 2^-24 is the unit round-off of one fp32 operation, every operation is
correctly rounded (no fast-math flag), first-order error terms are carried per element and multiplied by SLACK = 1.001 for the
second-order ones.  Sums are bounded for the WORST summation order: a sum of N rounded products is within N U sum|terms| of the exact
sum whatever the order and whether or not a product is fused into its add (N - 1 adds and one product rounding on any path), so the
bounds hold for the kernels' order (a per-lane chain, then a butterfly over the 64 lanes) and for any other.  N = d_p, the padded row:
the zeros of the padding are terms too.

  project   dot = fl(sum g_i w_i):            E_dot = d_p U sum|g_i w_i|
            t_i = fl(dot w_i):                 E_t   = E_dot |w_i| + U |dot w_i|
            g'_i = fl(g_i - t_i):              E_g'  = E_t + U |g'_i|
            absolute: g_i - t_i cancels when the gradient is parallel to the row (a purely parallel row leaves rounding noise of the
            size of the bound and nothing else).
  renorm    ss = fl(sum w_i^2), all terms >= 0:  relative error d_p U; a square below 2^-126 is rounded to a multiple of 2^-149, which
            adds at most d_p 2^-149 to the sum (the test inputs keep that below 2^-60 of it).
            nrm = sqrtf(ss):                   d_p U / 2 + U
            den = fl(nrm + EPS):               one more U (both terms positive; EPS is a power of two, exact in fp32)
            o_i = fl(w_i / den):               one more U:      E_o = ((d_p / 2 + 3) U + d_p 2^-150 / ss) |o_i|  + 2^-150 (o_i may be subnormal)
            A zero row gives exactly 0 / (0 + EPS) = +0: its bound is 0.
  row norm  after the renorm ||w_j|| = n / (n + EPS) (n the norm before it) up to the element errors above:
                | ||w_j|| - 1 |  <=  EPS / (n + EPS) + (d_p / 2 + 3) U SLACK
            -- 2^-23 + 67 U at d_p = 128 for a row that was near unit norm.
"""
import numpy as np

from tests import optimizer_reference as R

U = R.U
SLACK = R.SLACK
EPS = 2.0 ** -23
assert EPS == float(np.finfo(np.float32).eps)


def round_up(v, m):
    return (v + m - 1) // m * m


# ---- the rule in float64 --------------------------------------------------------------------------------------------------------
def project(g, w):
    """remove_gradient_parallel_to_decoder_directions: g [n][d], w [n][d] -> the projected gradient (float64)."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    return g - (g * w).sum(1, keepdims=True) * w


def renorm(w):
    """set_decoder_norm_to_unit_norm: w [n][d] -> w / (||w_j|| + EPS) (float64)."""
    w = np.asarray(w, np.float64)
    return w / (np.sqrt((w * w).sum(1, keepdims=True)) + EPS)


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
def project_bound(g, w, d_p):
    """Per element: how far the fp32 projection (any summation order) may lie from project(g, w)."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    dot = (g * w).sum(1, keepdims=True)
    E_dot = d_p * U * np.abs(g * w).sum(1, keepdims=True)
    E_t = E_dot * np.abs(w) + U * np.abs(dot * w)
    return SLACK * (E_t + U * np.abs(g - dot * w))


def renorm_rel(d_p):
    return (d_p / 2.0 + 3.0) * U


def renorm_bound(w, d_p):
    """Per element: how far the fp32 renorm (any summation order) may lie from renorm(w).  Zero rows: 0."""
    w = np.asarray(w, np.float64)
    ss = (w * w).sum(1, keepdims=True)
    live = ss > 0
    assert (ss[live] > 2.0 ** -90).all(), "a row this small leaves the range the bound was derived for"
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(live, renorm_rel(d_p) + d_p * 2.0 ** -150 / np.where(live, ss, 1.0), 0.0)
    return np.where(live, SLACK * rel * np.abs(renorm(w)) + 2.0 ** -150, 0.0)


def row_norm_bound(w_before, d_p):
    """Per row: the bound on | ||w_j|| - 1 | after the renorm of w_before (rows of zeros: not unit, excluded by the caller)."""
    n = np.sqrt((np.asarray(w_before, np.float64) ** 2).sum(1))
    return EPS / (n + EPS) + SLACK * renorm_rel(d_p)


def violations(got, ref, tol):
    """Boolean array: the element is not finite or further than the bound from the reference.  Nothing is masked."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(got) | ~(np.abs(got - ref) <= tol)


def worst_ratio(got, ref, tol):
    """max |got - ref| / bound (0 / 0 counts as 0; a non-finite element as infinity)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / tol)))


# ---- an fp32 emulation of the two kernels' order ---------------------------------------------------------------------------------
def _lanes(a, d_p):
    """[n][d] -> float32 [n][NV][64][4]: float4 i = q * 64 + lane of the padded row, zeros where the row has none."""
    a = np.asarray(a, np.float32)
    n, d = a.shape
    nv = (d_p + 255) // 256
    buf = np.zeros((n, nv * 256), np.float32)
    buf[:, :d] = a
    return buf.reshape(n, nv, 64, 4)


def _wave_sum(v):
    """The xor butterfly over 64 lanes, float32: v [n][64] -> [n][64] (every lane holds the sum)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(np.float32)
    return v


def _lane_dot(a, b):
    acc = np.zeros(a.shape[:1] + (64,), np.float32)
    for q in range(a.shape[1]):
        for j in range(4):
            acc = (acc + (a[:, q, :, j] * b[:, q, :, j]).astype(np.float32)).astype(np.float32)
    return acc


def emulate_project(g, w, d_p):
    """fp32, lane partial then butterfly, product and subtraction rounded separately -> float32 [n][d]."""
    n, d = np.asarray(g).shape
    gl, wl = _lanes(g, d_p), _lanes(w, d_p)
    dot = _wave_sum(_lane_dot(gl, wl))[:, None, :, None]
    out = (gl - (dot * wl).astype(np.float32)).astype(np.float32)
    return out.reshape(n, -1)[:, :d]


def emulate_renorm(w, d_p):
    """-> (float32 [n][d], its bf16 copy as float32)."""
    n, d = np.asarray(w).shape
    wl = _lanes(w, d_p)
    ss = _wave_sum(_lane_dot(wl, wl))
    den = (np.sqrt(ss).astype(np.float32) + np.float32(EPS)).astype(np.float32)[:, None, :, None]
    out = (wl / den).astype(np.float32).reshape(n, -1)[:, :d]
    return out, bf16_round(out)


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
ZERO_ROW, ZERO_GRAD_ROW, PARALLEL_ROW = 3, 5, 7


def plant_rows(p, g, m, v):
    """The family of tests/optimizer_reference.make_inputs for a TopK shape, with W_dec's rows brought to unit norm perturbed by at most
    1e-3 relative and three planted rows: ZERO_ROW all zero (weights, gradient and both moments: the update leaves it zero),
    ZERO_GRAD_ROW with a zero gradient, PARALLEL_ROW whose gradient is exactly 3 w_j (a multiply by 3 in fp32 of the fp32 row: purely
    parallel up to that rounding).  The parallel row's weights are +-1/sqrt(d) in a fixed sign pattern before the perturbation: what
    the projection leaves of it is rounding noise, multiples of an ulp of 3 w_i, and with no tiny w_i none of it comes near the
    subnormal range that tests/optimizer_reference.py refuses to bound.  On copies; -> (p, g, m, v)."""
    p, g, m, v = ({k: a.copy() for k, a in t.items()} for t in (p, g, m, v))
    W = p["W_dec"].astype(np.float64)
    n = W.shape[0]
    scale = 1.0 + 1e-3 * np.cos(np.arange(n))[:, None]                   # |scale - 1| <= 1e-3, fixed, no generator
    scale[PARALLEL_ROW] = 1.0           # (unit to fp32 rounding: without the division by |w|^2 the rule leaves 3 (1 - |w|^2) w of 3 w)
    W[PARALLEL_ROW] = np.where(np.arange(W.shape[1]) % 3 == 0, -1.0, 1.0)
    W = W / np.sqrt((W * W).sum(1, keepdims=True)) * scale
    p["W_dec"] = R.f32(W)
    p["W_dec"][ZERO_ROW] = 0.0
    g["W_dec"][ZERO_ROW] = 0.0
    m["W_dec"][ZERO_ROW] = 0.0
    v["W_dec"][ZERO_ROW] = 0.0
    g["W_dec"][ZERO_GRAD_ROW] = 0.0
    g["W_dec"][PARALLEL_ROW] = np.float32(3.0) * p["W_dec"][PARALLEL_ROW]
    return p, g, m, v


def lift_small_projections(p, g, c, d_p):
    """tests/optimizer_reference.reference_step refuses a case whose clipped gradient has a non-zero element so small that
    (1 - b2) g'^2 could be subnormal (below 2^-100): its bounds are relative.  The family's own gradients clear that by a factor of 1.3
    only (thresh 1e-3, not clipped), and a projection g_i - (g . w) w_i cancels to something far smaller in a handful of the 10^5
    elements.  This moves those few g_i, on the CPU and by the float64 rule alone, so that the projected value is at least
    3 project_bound + 10^3 x that floor away from zero -- whatever an fp32 projection inside the bound makes of it then clears the floor.
    Rows whose projection is exactly zero (no gradient) stay; PARALLEL_ROW stays as planted: what is left of it is a multiple of an
    ulp of 3 w_i (about 2^-25), no tiny value.  -> g (a copy), the number of elements moved."""
    g = {k: a.copy() for k, a in g.items()}
    W = np.asarray(p["W_dec"], np.float64)
    b2 = c.betas[1]
    rows = np.ones(W.shape[0], bool)
    rows[PARALLEL_ROW] = False
    moved = 0
    for _ in range(20):
        G = g["W_dec"].astype(np.float64)
        proj, tol = project(G, W), project_bound(G, W, d_p)
        coef = R.clip_of(dict(g, W_dec=proj), c)[2]
        floor = 1e3 * np.sqrt(2.0 ** -100 / (1 - b2)) / (c.scale * coef)
        need = 3 * tol + floor
        small = (np.abs(proj) < need) & (tol > 0) & rows[:, None]
        if not small.any():
            return g, moved
        moved += int(small.sum())
        t = (G * W).sum(1, keepdims=True) * W
        g["W_dec"][small] = R.f32(t + np.where(proj < 0, -2.0, 2.0) * need)[small]
    raise AssertionError("the projection could not be kept off zero")

