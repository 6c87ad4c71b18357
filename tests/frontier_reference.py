"""The float64 rule of the sparsity frontier (include/freud_sae.h, sae_frontier_files) and the bounds its tests hold the engine to.

Operands as the engine holds them: the slots (vals, idx) collect_features returns for the same rows, the bf16-valued operand rows
w_op [n, d], the delivered x (widened to float32 exactly) and the fp32 bias b (b_dec for TopK, None for L1).  The rule, per row,
in float64:

    R_0 = x - b,   R_{s+1} = R_s - v_s w_{i_s},   E_s = sum_i R_s[i]^2,   s = 0 .. K.

The bounds are counted from the kernel's roundings (the convention of tests/decode_reference.py); nothing is measured on the code
under test.  u = 2^-24 is the unit roundoff of fp32.

* elementwise.  r_0 is one rounded subtraction, every slot one rounded fmaf: after s slots s + 1 roundings, each at most u times a
  magnitude that A_s[i] = |x_i| + |b_i| + sum_{t<s} |v_t| |w_{i_t,i}| dominates (to first order; the factor s + 2 instead of s + 1
  pays for the second-order terms):            |r_s[i] - R_s[i]| <= delta_s[i] = (s + 2) u A_s[i].
* per frame.  e_s is a sum of d_p products r^2 added in some order of at most d_p - 1 additions, every operation rounded once:
      |e_s - E_s| <= sum_i (2 |R_s[i]| delta_s[i] + delta_s[i]^2) + d_p 2^-23 E_s                                      = B_s.
  (d_p 2^-23 = 2 d_p u covers the gamma_{d_p} of any summation order applied to the perturbed squares.)
* sse[s].  The kernel adds the e_s of at most FR_UNIT = 32 rows in fp32 -- 8 per wave in order, then the 4 waves: at most 11
  roundings on a partial -- and the partials in float64:
      |sse[s] - sum_frames E_s| <= sum_frames B_s + 11 u (sum_frames E_s + sum_frames B_s) + 2^-40 sum_frames E_s.
* budgets.  A frame is DECIDED at tau if E_0 == 0 (budget 0 whatever the roundings: r_0 is exactly 0) or, for every s,
      |E_s - tau E_0| > B_s + tau B_0 + 2^-23 tau E_0
  (the last term: one ulp of the fp32 product tau * e_0).  Decided frames are compared bin for bin; an undecided frame may land in
  any bin from the first s whose compare CAN hold to the first s whose compare MUST hold.
"""
import numpy as np

U = 2.0 ** -24
FR_UNIT, FR_CHUNK = 32, 32          # freud_amd/csrc/frontier.h
FOLD_ROUNDINGS = FR_UNIT // 4 + 3
MIN_DECIDED = 0.99


def bf16(a):
    """fp32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def round_up(v, m):
    return -(-v // m) * m


class Reference:
    """E [R, K + 1] float64, B [R, K + 1] its per-frame bound, for the R counted rows handed in."""

    def __init__(self, E, B, d_p):
        self.E, self.B, self.d_p = E, B, d_p
        self.K = E.shape[1] - 1

    # -- sse
    def sse(self):
        return self.E.sum(0)

    def sse_bound(self):
        sE, sB = self.E.sum(0), self.B.sum(0)
        return sB + FOLD_ROUNDINGS * U * (sE + sB) + 2.0 ** -40 * sE

    # -- budgets
    def _slack(self, tau):
        tau = float(np.float32(tau))
        lim = tau * self.E[:, :1]
        return lim, self.B + tau * self.B[:, :1] + 2.0 ** -23 * lim

    def decided(self, tau):
        lim, slack = self._slack(tau)
        return (self.E[:, 0] == 0) | (np.abs(self.E - lim) > slack).all(1)

    def budgets(self, tau):
        """(budget of the float64 rule, lowest and highest bin the bounds allow) per row."""
        lim, slack = self._slack(tau)

        def first(hit):
            return np.where(hit.any(1), hit.argmax(1), self.K + 1)
        zero = self.E[:, 0] == 0
        mid, lo, hi = first(self.E <= lim), first(self.E - slack <= lim), first(self.E + slack <= lim)
        return np.where(zero, 0, mid), np.where(zero, 0, lo), np.where(zero, 0, hi)


def reference(vals, idx, w_op, x, b, d_p=None):
    """vals [R, K] float32, idx [R, K] int, w_op [n, d] bf16-valued, x [R, d] float32, b [d] float32 or None -> Reference."""
    vals = np.asarray(vals, np.float32)
    Rn, K = vals.shape
    x = np.asarray(x, np.float32)
    d = x.shape[1]
    d_p = round_up(d, 128) if d_p is None else d_p
    w = np.asarray(w_op, np.float64)
    bb = np.zeros(d) if b is None else np.asarray(b, np.float32).astype(np.float64)
    R = x.astype(np.float64) - bb
    A = np.abs(x.astype(np.float64)) + np.abs(bb)
    E, B = np.empty((Rn, K + 1)), np.empty((Rn, K + 1))
    for s in range(K + 1):
        delta = (s + 2) * U * A
        E[:, s] = (R * R).sum(1)
        B[:, s] = (2 * np.abs(R) * delta + delta * delta).sum(1) + d_p * 2.0 ** -23 * E[:, s]
        if s < K:
            v = vals[:, s].astype(np.float64)[:, None]
            ws = w[np.asarray(idx)[:, s]]
            R = R - v * ws
            A = A + np.abs(v) * np.abs(ws)
    return Reference(E, B, d_p)


def assert_decidable(ref: Reference, taus, ctx=""):
    """The cap: asserted from the reference alone, before anything is compared."""
    for t in taus:
        share = ref.decided(t).mean()
        print(f"{ctx} tau={float(t):g}: decided {share:.4f} of {len(ref.E)} frames")
        assert share >= MIN_DECIDED, (ctx, float(t), share)


def e_violations(e, ref: Reference):
    """bool [R, K + 1]: the per-frame norms outside their bound (a non-finite value is a violation)."""
    e = np.asarray(e, np.float64)
    return ~(np.abs(e - ref.E) <= ref.B)


def budget_violations(got, ref: Reference, tau):
    """bool [R]: a decided frame in another bin than the rule's, or an undecided one outside the bins the bounds allow."""
    mid, lo, hi = ref.budgets(tau)
    got = np.asarray(got)
    dec = ref.decided(tau)
    return np.where(dec, got != mid, (got < lo) | (got > hi))


def check_hist(hist, ref: Reference, tau, ctx=""):
    """A budget histogram [K + 2] against the rule: the decided frames bin for bin, the undecided ones anywhere between their two
    candidate bins -- so every cumulative count lies between the counts of the two extreme assignments."""
    mid, lo, hi = ref.budgets(tau)
    dec = ref.decided(tau)
    nb = ref.K + 2
    hist = np.asarray(hist, np.int64)
    assert hist.shape == (nb,) and hist.sum() == len(mid), (ctx, hist.sum(), len(mid))
    early = np.bincount(np.where(dec, mid, lo), minlength=nb)      # every undecided frame as early as allowed
    late = np.bincount(np.where(dec, mid, hi), minlength=nb)
    cg, ce, cl = np.cumsum(hist), np.cumsum(early), np.cumsum(late)
    assert (cg <= ce).all() and (cg >= cl).all(), (ctx, float(tau), hist.tolist(), early.tolist(), late.tolist())
    if dec.all():
        np.testing.assert_array_equal(hist, early, err_msg=ctx)


def check_sse(sse, ref: Reference, ctx="", factor=1.0):
    sse = np.asarray(sse, np.float64)
    want, bound = ref.sse(), ref.sse_bound()
    err = np.abs(sse - want)
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"{ctx} sse: worst |err| / bound = {err[worst] / max(bound[worst], 1e-300):.3e} at s={worst} "
          f"(err {err[worst]:.3e}, bound {bound[worst]:.3e}, value {want[worst]:.6e})")
    assert np.isfinite(sse).all() and (err <= factor * bound).all(), (ctx, worst, err[worst], bound[worst])


# ---- a float32 emulation of the kernel's rule, with the mistakes the bounds must catch
def emulate(vals, idx, w_op, x, b, taus, *, order=None, sign=-1.0, use_b=True, shift=0, strict=False, against_x=False):
    """(e [R, K + 1] float32, budgets [R, n_tau]) by the rule in float32 -- numpy's own summation order, which the bounds cover.
    order: a permutation of the slots (None: slot order); sign=+1: +v instead of -v; use_b=False: b left out; shift=1: e_s indexed one
    slot off; strict: < instead of <=; against_x: the threshold taken against |x|^2 instead of e_0."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx)
    Rn, K = vals.shape
    x = np.asarray(x, np.float32)
    bb = np.zeros(x.shape[1], np.float32) if (b is None or not use_b) else np.asarray(b, np.float32)
    w = np.asarray(w_op, np.float32)
    r = x - bb
    e = np.empty((Rn, K + 2), np.float32)
    e[:, 0] = (r * r).sum(1, dtype=np.float32)
    for s in range(K):
        t = s if order is None else order[s]
        r = (r + np.float32(sign) * vals[:, t:t + 1] * w[idx[:, t]]).astype(np.float32)
        e[:, s + 1] = (r * r).sum(1, dtype=np.float32)
    e[:, K + 1] = e[:, K]
    e = e[:, shift:shift + K + 1]
    base = (x * x).sum(1, dtype=np.float32) if against_x else e[:, 0]
    buds = np.empty((Rn, len(taus)), np.int64)
    for ti, t in enumerate(taus):
        lim = (np.float32(t) * base).astype(np.float32)[:, None]
        hit = (e < lim) if strict else (e <= lim)
        buds[:, ti] = np.where(hit.any(1), hit.argmax(1), K + 1)
    return e, buds
