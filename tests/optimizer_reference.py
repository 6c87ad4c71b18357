"""Float64 reference and per-element error bound for one optimizer update of the engine (sae_optimizer_step: gnorm_partial_kernel, then
optimizer_kernel / optimizer_l1_kernel / optimizer_l1_cols_kernel, which share adam_update4 and the clip coefficient).  Shared by
tests/test_optimizer_cpu.py (which holds the bound to torch's own optimizers, to an fp32 emulation and to twelve mutations of it) and
tests/test_optimizer_gpu.py (which holds the three kernels to it).  Nothing here is an import or a transcription of the kernel: the
reference is torch's documented rule (torch.nn.utils.clip_grad_norm_, torch.optim.Adam, torch.optim.RAdam, single-tensor forms; the
restatement in oracle/sae_oracle.py), evaluated in float64.

The operation, with t the number of the step that is taken (the state holds t - 1 before it):

    total = sqrt(sum (scale g)^2)  over ALL parameters         coef = min(1, thresh / (total + 1e-6))          g' = scale g coef
    RAdam with weight decay:  g' <- g' + wd p                  (not decoupled; Adam is run without weight decay, as the engine does)
    m' = m + (1 - b1)(g' - m)                                  v' = b2 v + (1 - b2) g'^2
    bc1 = 1 - b1^t    bc2 = 1 - b2^t    rho_inf = 2 / (1 - b2) - 1    rho_t = rho_inf - 2 t b2^t / bc2
    Adam:              p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    RAdam, rho_t > 5:  p' = p - lr (m' / bc1) sqrt(bc2) / (sqrt(v') + eps) rect
                       rect = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
    RAdam otherwise:   p' = p - lr m' / bc1
    norm_on_load (L1 weight matrix only):  p <- p / max(||p[:, j]||, 1e-12)  before all of the above

For the betas of the family, (0.9, 0.999) and (0.8, 0.99), rho_t first exceeds 5 at t = 6 and is 5 at no integer t (4.996 / 5.994 and
4.960 / 5.940 at t = 5 / 6): `rho_t >= 5` and `rho_t > 5` never differ, so that mutation does not exist here
(tests/test_optimizer_cpu.py asserts it for t = 1 .. 2000).

THE BOUND.  u = 2^-24 is the unit round-off of one fp32 operation.  Add, subtract, multiply, divide and sqrt are correctly rounded:
the build passes no fast-math flag (tests/test_optimizer_cpu.py checks the Makefile), so divide and sqrt are the correctly rounded
expansions.  No intermediate of the family is subnormal (the smallest, (1 - b2) g'^2, is asserted above 2^-100), so every rounding is
relative.  Each host scalar (lr, scale, thresh, wd, 1 - b1, b2, 1 - b2, bc1, sqrt(bc2), lr / bc1, rect, eps, 1e-6) is a double that is
cast to fp32: one more u wherever it enters.  The errors are carried forward per element as absolute errors E_x (a running error
analysis), first order in u; the result is multiplied by SLACK = 1.001 for the second-order terms (the largest first-order relative
error below is under 40 u = 2.4e-6), and the one division by an inexact denominator uses r / (1 - r) instead of r.

  norm      s_i = fl(g_i scale_f): e_s = u [cast of scale, if not exact] + u [multiply, if scale != 1].  The squares are taken in fp32 (u)
            and summed in double (n 2^-53 for n terms, all non-negative): e_S = 2 e_s + u + n 2^-53.  The sum is cast to fp32 (u) and
            sqrtf'd (halves what came before, adds u):   e_total = (e_S + u) / 2 + u      -- 2 u + n 2^-54 for scale = 1, <= 4 u + ...
  coef      1 exactly when thresh / (total + 1e-6) > 1 (cases closer than 1e-3 to the threshold are refused).  Otherwise the add costs
            u and 1e-6f u of a part of a non-negative sum (2 u), thresh_f u, the divide u:   e_coef = e_total + 4 u   <= 8 u
  g'        e_g = e_s + e_coef + u [multiply by coef, if coef != 1]   <= 11 u: relative.  E_g = e_g |g'|.
            With weight decay gj = fl(g' + fl(wd_f p)):  E_g = e_g |g'| + 2 u wd |p| + wd E_pin + u |gj|, and G = |g'| + wd |p| stands
            for |g'| below (gj may cancel: its error is absolute from here on).
  m'        d = fl(gj - m) errs by E_g + u |gj - m|; fl((1 - b1)_f d) adds 2 u; the final add u |m'|.  With |gj - m| <= G + |m|:
                E_m = (1 - b1)(E_g + 3 u (G + |m|)) + u |m'|         i.e.  c_m u (|m| + G),  c_m <= (1 - b1)(e_g / u + 6) + 1 <= 4.4
            absolute, because gj - m cancels (a quarter of the family has m = g' to within a rounding).
  v'        fl(v b2_f): 2 u;  fl(fl((1 - b2)_f gj) gj): 3 u and the error of gj twice;  the add u:
                E_v = 2 u b2 v + (1 - b2)(2 |gj| E_g + E_g^2) + 3 u (1 - b2) gj^2 + u v'
            -- without weight decay that is relative, c_v u v' with c_v = 4 + 2 e_g / u <= 26.
  sqrt      s = sqrtf(v'):  E_s = min(E_v / sqrt(v'), sqrt(E_v)) + u sqrt(v')
  Adam      den = fl(fl(s / bc2s_f) + eps_f):  E_den = E_s / bc2s + 2 u s / bc2s + u eps + u den;  fl(fl(-step_f m') / den): 3 u:
                E_delta = (lr / bc1) E_m / den + |delta| (3 u + r / (1 - r)),   r = E_den / den
  RAdam     mh = fl(m' / bc1_f): 2 u;  fl(mh lr_f): 2 u.  Not rectified:   E_delta = (lr / bc1) E_m + 4 u |delta|
            Rectified: den = fl(s + eps_f):  E_den = E_s + u eps + u den;  fl(1 / den): u + r;  fl(. bc2s_f): 2 u;  the product with
            fl(mh lr_f): u;  fl(. rect_f): 2 u:
                E_delta = step E_m / den + |delta| (10 u + r / (1 - r)),   step = lr sqrt(bc2) rect / bc1
  p'        E_p = E_pin + E_delta + u |p'|.   In the issue's shape:  u |p'| + c_p u |delta| + step c_m u (|m| + G) / den  with
            c_p = 3 + r / u (Adam), 4 (RAdam), 10 + r / u (rectified), and r / u <= c_v / 2 + 3 = 16 without weight decay.
  norm_on_load   the denominator is sqrtf of an fp32 sum of d_p squares in the kernel's order: a chain of four fused multiply-adds (4
            roundings on the first square), a tree of eight (3), the slabs of 32 rows one after the other (d_p / 32): a square passes
            D = 7 + d_p / 32 roundings, all terms are non-negative, so the sum is within D u; sqrtf halves that and adds u, the divide
            adds u:   E_pin = ((7 + d_p / 32) / 2 + 2) u |p|     -- 11.5 u at d_p = 384, against (d_p / 2 + 3) u = 195 u for an arbitrary
            order.  It goes into E_p directly and, with weight decay, into E_g.
  metrics[3]     the norm: e_total above.

torch's own clip_grad_norm_ accumulates the squares in fp32, in an order that depends on the host, not in double: its norm is held to the
bound of an fp32 sum of n non-negative terms in any order, (n + 3) u, and its elements to the bound above with e_total widened by the
error torch's norm actually has (`norm_extra_u`, in units of u; an input of the update, not part of it).  The kernels get 0."""
import dataclasses
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.001
BETAS = ((0.9, 0.999), (0.8, 0.99))
LR = 1e-3


@dataclasses.dataclass(frozen=True)
class Case:
    """One update of the input family.  `clipped`: the gradient is rescaled so that the norm of scale * g is 20 x thresh (coef < 1) or
    thresh / 4 (coef == 1 exactly)."""
    opt: str            # "adam" or "radam"
    t: int              # the step that is taken
    betas: tuple
    wd: float
    scale: float
    thresh: float
    clipped: bool
    lr: float = LR

    @property
    def eps(self):      # the engine's defaults (RAdam(eps=1e-5), Adam's 1e-8)
        return 1e-5 if self.opt == "radam" else 1e-8

    @property
    def name(self):
        s = {1.0: "1", 0.5: "h", 1.0 / 3.0: "t"}[self.scale]
        return (f"{self.opt}_t{self.t}_b{int(round(self.betas[0] * 10))}_wd{'1' if self.wd else '0'}_s{s}_c{self.thresh:g}_"
                f"{'clip' if self.clipped else 'noclip'}")

    @property
    def rectified(self):
        return self.opt == "radam" and host_scalars(self)["rho_t"] > 5.0


def host_scalars(c, t=None):
    """bc1, bc2, rho_inf, rho_t, rect (0 when not rectified) of step t in float64."""
    t = c.t if t is None else t
    b1, b2 = c.betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * t * b2 ** t / bc2 if bc2 > 0 else float("nan")
    rect = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) if rho_t > 5.0 else 0.0
    return {"bc1": bc1, "bc2": bc2, "rho_inf": rho_inf, "rho_t": rho_t, "rect": rect}


# The cases every kernel sees on the GPU (tests/test_optimizer_gpu.py): Adam, RAdam not rectified, rectified with and without weight
# decay, coef == 1 and coef < 1, all three scales, all three thresholds, both betas, every step of the family.
THIRD = 1.0 / 3.0
KERNEL_CASES = (
    Case("adam", 1000, BETAS[0], 0.0, 0.5, 1.0, True),
    Case("adam", 1, BETAS[1], 0.0, 1.0, 1e-3, False),
    Case("radam", 5, BETAS[0], 0.0, 1.0, 1e6, False),
    Case("radam", 6, BETAS[0], 0.01, THIRD, 1e-3, True),
    Case("radam", 7, BETAS[1], 0.0, 1.0, 1.0, False),
    Case("radam", 1000, BETAS[0], 0.01, 0.5, 1e6, True),
)
# the rectified step with weight decay and coef == 1 on which the three kernels are compared bit for bit, next to KERNEL_CASES[0]
RECTIFIED_WD_UNCLIPPED = Case("radam", 7, BETAS[0], 0.01, 1.0, 1.0, False)
# ... and the rest of what the CPU test vouches for: each optimizer at each step and beta pair, weight decay on both sides of the
# rectification switch, every scale on both sides of the clip (no full cross product: 5 x 2 x 3 x 3 x 2 x 3 = 540 would say no more).
CPU_CASES = KERNEL_CASES + (
    RECTIFIED_WD_UNCLIPPED,
    Case("adam", 5, BETAS[0], 0.0, THIRD, 1.0, False),
    Case("adam", 6, BETAS[1], 0.0, 0.5, 1e6, True),
    Case("adam", 7, BETAS[0], 0.0, 1.0, 1e-3, True),
    Case("adam", 1000, BETAS[0], 0.0, 1.0, 1e6, False),
    Case("radam", 1, BETAS[0], 0.0, 0.5, 1.0, True),
    Case("radam", 1, BETAS[1], 0.01, 1.0, 1e-3, False),
    Case("radam", 5, BETAS[1], 0.01, THIRD, 1.0, True),
    Case("radam", 6, BETAS[1], 0.0, 0.5, 1e6, False),
    Case("radam", 6, BETAS[0], 0.0, 1.0, 1.0, True),
    Case("radam", 7, BETAS[0], 0.01, THIRD, 1e6, False),
    Case("radam", 7, BETAS[1], 0.01, 1.0, 1e-3, True),
    Case("radam", 1000, BETAS[0], 0.0, THIRD, 1.0, False),
)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def flat(arrs):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrs.values()])


def unflat(vec, like):
    out, o = {}, 0
    for k, a in like.items():
        out[k] = vec[o:o + a.size].reshape(a.shape)
        o += a.size
    return out


def clip_of(grads, c):
    """(total, ratio, coef) of clip_grad_norm_ on scale * g in float64."""
    total = math.sqrt(sum(float(((c.scale * np.asarray(g, np.float64)) ** 2).sum()) for g in grads.values()))
    ratio = c.thresh / (total + 1e-6)
    return total, ratio, min(1.0, ratio)


def make_inputs(shapes, c, seed):
    """The input family for `shapes` (name -> shape, in the engine's parameter order; 2-D tensors are weights, 1-D ones biases) and
    case c: float32 dicts p, g, m, v.  By flat index i over all parameters:
      g   random sign, magnitude log-uniform over [1e-9, 1e-1]; exactly 0 where i % 16 == 5; magnitude 10 on the four elements
          [8, 12) of the first tensor; then rescaled so that ||scale g|| is 20 thresh (c.clipped) or thresh / 4
      m   the same distribution, independent; +g' (the clipped, scaled gradient, rounded to fp32) where i % 4 == 2; 0 where i % 64 == 5
      v   log-uniform over [1e-16, 1e-2]; exactly 0 where i % 32 == 5 (g is 0 there too: the denominator is eps, and delta is 0
          where m is 0 as well) and where i % 32 == 25
      p   N(0, 1/d) for a weight [d][n] (L1) or N(0, 1/shape[1]) (TopK's [n][d]), 0.01 N(0, 1) for a bias"""
    rng = np.random.default_rng(seed)
    N = sum(int(np.prod(s)) for s in shapes.values())
    i = np.arange(N)

    def logu(lo, hi):
        return np.exp(rng.uniform(math.log(lo), math.log(hi), N))

    g = np.where(rng.random(N) < 0.5, -1.0, 1.0) * logu(1e-9, 1e-1)
    g[i % 16 == 5] = 0.0
    g[8:12] = np.array([10.0, -10.0, 10.0, 10.0])
    target = c.thresh * (20.0 if c.clipped else 0.25)
    g = f32(g * (target / (c.scale * math.sqrt(float((g ** 2).sum())))))
    like = {k: np.empty(s, np.float32) for k, s in shapes.items()}
    grads = unflat(g, like)
    _, ratio, coef = clip_of(grads, c)
    assert (coef < 1.0) == c.clipped and abs(ratio - 1.0) > 0.5
    m = np.where(rng.random(N) < 0.5, -1.0, 1.0) * logu(1e-9, 1e-1) * (target / 20.0)
    gp = g.astype(np.float64) * c.scale * coef
    m[i % 4 == 2] = gp[i % 4 == 2]
    m[i % 64 == 5] = 0.0
    v = logu(1e-16, 1e-2)
    v[(i % 32 == 5) | (i % 32 == 25)] = 0.0
    p = []
    for s in shapes.values():
        p.append(rng.standard_normal(s) / math.sqrt(s[0] if len(s) == 2 and len(shapes) == 2 else s[-1]) if len(s) == 2
                 else 0.01 * rng.standard_normal(s))
    p = {k: f32(a) for k, a in zip(shapes, p)}
    return p, grads, unflat(f32(m), like), unflat(f32(v), like)


def column_normalise(W):
    """(W / max(||W[:, j]||, 1e-12), the norms) in float64."""
    W = np.asarray(W, np.float64)
    nrm = np.maximum(np.sqrt((W ** 2).sum(0)), 1e-12)
    return W / nrm, nrm


def norm_on_load_u(d_p):
    """The relative error, in units of u, of a weight the cols kernel divides by last step's column norm while loading."""
    return (7 + d_p // 32) / 2.0 + 2.0


def reference_step(params, grads, exp_avg, exp_avg_sq, c, *, normalise=None, d_p=None, norm_extra_u=0.0):
    """One update in float64 and its bound.  The four dicts map a name to an array (any float type; taken as exact); normalise names the
    L1 weight matrix [d][n] that is divided by its column norms first (norm_on_load; d_p: its padded row count).
    -> dict with "p", "m", "v" (name -> float64 array), "tol_p", "tol_m", "tol_v" (the same shapes), "total", "coef", "tol_total"."""
    b1, b2 = c.betas
    h = host_scalars(c)
    bc1, bc2s = h["bc1"], math.sqrt(h["bc2"])
    like = {k: np.asarray(a) for k, a in params.items()}
    p = {k: np.asarray(a, np.float64) for k, a in params.items()}
    E_pin = {k: np.zeros(a.shape) for k, a in p.items()}
    if normalise is not None:
        p[normalise], _ = column_normalise(p[normalise])
        E_pin[normalise] = norm_on_load_u(d_p) * U * np.abs(p[normalise])
    p, E_pin = flat(p), flat(E_pin)
    g, m, v = (flat({k: np.asarray(a, np.float64) for k, a in d.items()}) for d in (grads, exp_avg, exp_avg_sq))
    total, ratio, coef = clip_of(grads, c)
    assert abs(ratio - 1.0) > 1e-3, "a case this close to the clip threshold is not decided by the reference"

    e_s = (0.0 if float(np.float32(c.scale)) == c.scale else U) + (0.0 if c.scale == 1.0 else U)
    e_S = 2 * e_s + U + g.size * 2.0 ** -53
    e_total = (e_S + U) / 2 + U + norm_extra_u * U
    e_coef = 0.0 if coef == 1.0 else e_total + 4 * U
    e_g = e_s + e_coef + (0.0 if coef == 1.0 else U)

    gp = g * c.scale * coef
    nz = np.abs(gp[gp != 0])
    assert nz.size == 0 or (1 - b2) * nz.min() ** 2 > 2.0 ** -100, "an intermediate of this case could be subnormal"
    if c.opt == "radam" and c.wd != 0.0:
        gj = gp + c.wd * p
        G = np.abs(gp) + c.wd * np.abs(p)
        E_g = e_g * np.abs(gp) + 2 * U * c.wd * np.abs(p) + c.wd * E_pin + U * np.abs(gj)
    else:
        gj, G, E_g = gp, np.abs(gp), e_g * np.abs(gp)
    m1 = m + (1 - b1) * (gj - m)
    E_m = (1 - b1) * (E_g + 3 * U * (G + np.abs(m))) + U * np.abs(m1)
    v1 = b2 * v + (1 - b2) * gj * gj
    E_v = 2 * U * b2 * v + (1 - b2) * (2 * np.abs(gj) * E_g + E_g ** 2) + 3 * U * (1 - b2) * gj * gj + U * v1
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        E_s = np.where(s > 0, np.minimum(E_v / np.where(s > 0, s, 1.0), np.sqrt(E_v)), np.sqrt(E_v)) + U * s

    def inv_err(E_den, den):
        r = E_den / den
        assert r.max() < 0.5
        return r / (1 - r)

    if c.opt == "adam":
        den = s / bc2s + c.eps
        E_den = E_s / bc2s + 2 * U * s / bc2s + U * c.eps + U * den
        step = c.lr / bc1
        delta = step * m1 / den
        E_delta = step * E_m / den + np.abs(delta) * (3 * U + inv_err(E_den, den))
    elif h["rho_t"] > 5.0:
        den = s + c.eps
        E_den = E_s + U * c.eps + U * den
        step = c.lr * bc2s * h["rect"] / bc1
        delta = step * m1 / den
        E_delta = step * E_m / den + np.abs(delta) * (10 * U + inv_err(E_den, den))
    else:
        step = c.lr / bc1
        delta = step * m1
        E_delta = step * E_m + 4 * U * np.abs(delta)
    p1 = p - delta
    E_p = E_pin + E_delta + U * np.abs(p1)
    out = {"total": total, "coef": coef, "tol_total": SLACK * e_total * total}
    for key, val in (("p", p1), ("m", m1), ("v", v1), ("tol_p", SLACK * E_p), ("tol_m", SLACK * E_m), ("tol_v", SLACK * E_v)):
        out[key] = unflat(val, like)
    return out


def violations(got, ref, what):
    """Boolean array per name: the element of `got` (p, m or v; name -> array) is not finite or further than the bound from the
    reference.  Every element is compared: nothing is masked."""
    bad = {}
    for k, r in ref[what].items():
        o = np.asarray(got[k], np.float64)
        assert o.shape == r.shape, (k, o.shape, r.shape)
        with np.errstate(invalid="ignore"):
            bad[k] = ~np.isfinite(o) | ~(np.abs(o - r) <= ref["tol_" + what][k])
    return bad


def count_violations(got_p, got_m, got_v, ref):
    """(violating elements, compared elements) over p, m and v."""
    bad = n = 0
    for what, got in (("p", got_p), ("m", got_m), ("v", got_v)):
        for b in violations(got, ref, what).values():
            bad += int(b.sum())
            n += b.size
    return bad, n


def worst_ratio(got, ref, what):
    """max over the elements of |got - reference| / bound (0 / 0 counts as 0)."""
    w = 0.0
    for k, r in ref[what].items():
        o = np.asarray(got[k], np.float64)
        err, tol = np.abs(o - r), ref["tol_" + what][k]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / tol)
        w = max(w, float(np.nanmax(q)) if np.isfinite(o).all() else math.inf)
    return w


def report(got, ref, what):
    """The violating count and the worst element, for an assertion message."""
    bad = violations(got, ref, what)
    lines = []
    for k, b in bad.items():
        if not b.any():
            continue
        o = np.asarray(got[k], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(np.isfinite(o), np.abs(o - ref[what][k]) / ref["tol_" + what][k], np.inf)
        idx = np.unravel_index(np.nanargmax(q), q.shape)
        lines.append(f"{what}[{k}]: {int(b.sum())} of {b.size} elements violate; worst at {tuple(int(x) for x in idx)}: got {o[idx]!r}, "
                     f"reference {ref[what][k][idx]!r}, |difference| / bound = {q[idx]:.3g}")
    return "; ".join(lines) or f"{what}: no element violates"
