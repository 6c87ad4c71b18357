"""The float64 rule of the pursuit frontier (include/freud_sae.h, sae_pursuit_files), the teacher-forced replay of an engine trace and
the bounds the tests hold the engine to.

Operands as the engine holds them: the bf16-valued operand rows w_op [n, d] (float32 holding bf16 values), the delivered x (widened to
float32 exactly) and the fp32 bias b (b_dec for TopK, None for L1).

The float64 rule (greedy64): R_0 = x - b; step s: sc_j = <R_s, w_j> / |w_j|, j* = the FIRST arg-max, stop if sc_j* <= 0,
a = sc_j* / |w_j*| (> 0 then), R_{s+1} = R_s - a w_j*; E_s = |R_s|^2, held after the stop.

The replay (class Replay) rebuilds the residual in float64 from the engine's OWN trace (idx, val): R_{s+1} = R_s - val_s w_{idx_s}.  Every
bound compares the engine with float64 arithmetic on that residual, so errors do not compound through the choices.

The bounds are counted from the kernel's roundings; nothing is measured on the code under test.  u = 2^-24 is the unit roundoff of
fp32, v = 2^-9 that of bf16 (8 significant bits, round to nearest even).  d_p is d rounded up to 128, C = d_p / 64 the columns of a lane.

* drift.  The engine's r_0 is one rounded subtraction, every update one rounded fmaf WITH THE SAME a AND w AS THE REPLAY: after s updates
  s + 1 roundings, each at most u times a magnitude that A_s[i] = |x_i| + |b_i| + sum_{t<s} |a_t| |w_{j_t,i}| dominates (the factor
  s + 2 pays for the second-order terms, as in tests/frontier_reference.py):
      |r_s[i] - R_s[i]| <= delta_s[i] = (s + 2) u A_s[i].
* selection, eta_s.  sc_j(engine) = fl(acc_j * z_j), acc_j the fp32 MFMA accumulation of rho . w_j, rho = bf16(r_s).
    - rho_i = r_s[i] (1 + e), |e| <= v:                       |sum (rho_i - r_i) w_i|   <= v sum |r_i w_i|
    - the drift of r_s against R_s:                           |sum (r_i - R_i) w_i|     <= sum delta_i |w_i|
    - d_p products (exact: bf16 x bf16 fits fp32) accumulated in fp32 in SOME order, every addition rounded (or truncated: twice the
      roundoff), at most d_p additions:                       <= d_p 2^-23 sum |rho_i w_i|
    - z_j = fl(1 / fl(sqrt(q_j))), q_j an fp32 sum of d_p squares (relative error (C + 6) u: the chain and the butterfly), the square
      root halves it and adds u, the division adds u, the product with acc adds u: relative (C / 2 + 6) u on acc_j z_j.
  Divided by |w_j|, with Cauchy-Schwarz (sum |r_i w_i| <= |r| |w|, sum delta_i |w_i| <= |delta| |w|, |sc_j| <= |R_s|) and |r| <=
  |R_s| + |delta_s|, for EVERY j at once:
      |sc_j(engine) - sc_j(float64 on R_s)| <= eta_s = (v + d_p 2^-23 (1 + v) + (C / 2 + 6) u) (1 + 2^-7) (|R_s| + |delta_s|) + |delta_s|
  (the factor 1 + 2^-7 pays for every product of two of the terms).  So the engine's pick is within 2 eta_s of the best float64 score,
  and a row is DECIDED at s when the float64 top-two margin and the top score both exceed 2 eta_s.
* coefficient.  a = fl(dot / q_j): dot the lane chains of C fmaf and the 6 butterfly additions on r_s (relative (C + 6) u on
  sum |r_i w_i|), q_j as above ((C + 6) u), one division (u):
      |a - <R_s, w_j> / |w_j|^2| <= [(C + 7) u sum |R_i w_i| + (1 + (C + 7) u) sum delta_i |w_i|] / |w_j|^2 + (C + 8) u (1 + 2^-7) |a64|.
* e_s against |R_s|^2: the frontier's per-frame bound, sum_i (2 |R_i| delta_i + delta_i^2) + d_p 2^-23 E_s (any summation order).
* fold: SSE[s] adds the e_s of at most 32 consecutive rows in fp32 in row order (31 roundings), the partials in float64:
      |SSE[s] - sum_rows e_s| <= 32 u sum_rows e_s + 2^-40 sum_rows e_s.
"""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -9
FOLD_ROWS = 32                      # freud_amd/csrc/frontier.h: FR_UNIT
MIN_DECIDED = 0.95


def bf16(a):
    """fp32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def round_up(v, m):
    return -(-v // m) * m


def _operands(w_op, x, b):
    w = np.asarray(w_op, np.float64)
    x = np.asarray(x, np.float32)
    bb = np.zeros(x.shape[1]) if b is None else np.asarray(b, np.float32).astype(np.float64)
    return w, x.astype(np.float64), bb


def norms(w):
    """(|w_j|, |w_j|^2) in float64; a zero direction gets norm inf so that its score is 0 and it never wins."""
    q = (w * w).sum(1)
    return np.where(q > 0, np.sqrt(q), np.inf), np.where(q > 0, q, np.inf)


def scores(R, w, wn):
    """sc_j = <R, w_j> / |w_j| for every row of R: float64 [rows, n]."""
    return (R @ w.T) / wn[None, :]


# ---- the float64 rule
def greedy64(w_op, x, b, K):
    """-> (idx int64 [R, K] (-1 after the stop), val float64 [R, K], E float64 [R, K + 1], top float64 [R, K] the best score at every
    step a live row took, margin float64 [R, K] its distance to the second-best score; nan where the row had stopped)."""
    w, X, bb = _operands(w_op, x, b)
    wn, q = norms(w)
    R = X - bb
    Rn = R.shape[0]
    idx = np.full((Rn, K), -1, np.int64)
    val = np.zeros((Rn, K))
    E = np.empty((Rn, K + 1))
    top = np.full((Rn, K), np.nan)
    margin = np.full((Rn, K), np.nan)
    live = np.ones(Rn, bool)
    E[:, 0] = (R * R).sum(1)
    rows = np.arange(Rn)
    for s in range(K):
        sc = scores(R, w, wn)
        j = sc.argmax(1)
        best = sc[rows, j]
        if sc.shape[1] > 1:
            sc2 = sc.copy()
            sc2[rows, j] = -np.inf
            second = sc2.max(1)
        else:
            second = np.full(Rn, -np.inf)
        top[live, s] = best[live]
        margin[live, s] = (best - second)[live]
        live = live & (best > 0)
        a = np.where(live, best / wn[j], 0.0)
        R = R - a[:, None] * w[j]
        idx[live, s] = j[live]
        val[:, s] = a
        E[:, s + 1] = (R * R).sum(1)
    return idx, val, E, top, margin


# ---- the teacher-forced replay of an engine trace
class Replay:
    """Float64 residuals R_s rebuilt from the engine's trace, with everything the bounds need, per counted row and step:
    E [R, K + 1], Eb its bound, eta [R, K], best [R, K] the best float64 score on R_s, at [R, K] the float64 score of the engine's pick
    (nan after the stop), a64 / ab [R, K] the float64 coefficient of the pick and its bound, amin_near [R, K] the smallest
    (a64 - bound) over the candidates within 2 eta of the best (what a stop on the coefficient needs), second [R, K]."""

    def __init__(self, idx, val, w_op, x, b, d_p=None):
        idx = np.asarray(idx, np.int64)
        val32 = np.asarray(val, np.float32)
        w, X, bb = _operands(w_op, x, b)
        Rn, K = idx.shape
        n, d = w.shape
        d_p = round_up(d, 128) if d_p is None else d_p
        C = d_p // 64
        wn, q = norms(w)
        aw = np.abs(w)
        R = X - bb
        A = np.abs(X) + np.abs(bb)
        rows = np.arange(Rn)
        self.K, self.n, self.d_p, self.wn = K, n, d_p, np.where(np.isfinite(wn), wn, 0.0)
        self.idx, self.val = idx, val32
        self.E, self.Eb = np.empty((Rn, K + 1)), np.empty((Rn, K + 1))
        self.eta, self.best, self.second = (np.empty((Rn, K)) for _ in range(3))
        self.at, self.a64, self.ab, self.amin_near = (np.full((Rn, K), np.nan) for _ in range(4))
        sel = V + d_p * 2.0 ** -23 * (1 + V) + (C / 2 + 6) * U
        for s in range(K + 1):
            delta = (s + 2) * U * A
            self.E[:, s] = (R * R).sum(1)
            self.Eb[:, s] = (2 * np.abs(R) * delta + delta * delta).sum(1) + d_p * 2.0 ** -23 * self.E[:, s]
            if s == K:
                break
            dn = np.sqrt((delta * delta).sum(1))
            self.eta[:, s] = sel * (1 + 2.0 ** -7) * (np.sqrt(self.E[:, s]) + dn) + dn
            sc = scores(R, w, wn)
            self.best[:, s] = sc.max(1)
            self.second[:, s] = np.sort(sc, axis=1)[:, -2] if n > 1 else -np.inf
            # the float64 coefficient of EVERY direction and its bound (for the stop on the coefficient)
            S = np.abs(R) @ aw.T
            D = delta @ aw.T
            a_all = (R @ w.T) / q[None, :]
            ab_all = ((C + 7) * U * S + (1 + (C + 7) * U) * D) / q[None, :] + (C + 8) * U * (1 + 2.0 ** -7) * np.abs(a_all)
            near = sc >= (self.best[:, s] - 2 * self.eta[:, s])[:, None]
            self.amin_near[:, s] = np.where(near, a_all - ab_all, np.inf).min(1)
            picked = idx[:, s] >= 0
            j = np.where(picked, idx[:, s], 0)
            self.at[picked, s] = sc[rows, j][picked]
            self.a64[picked, s] = a_all[rows, j][picked]
            self.ab[picked, s] = ab_all[rows, j][picked]
            a = np.where(picked, val32[:, s].astype(np.float64), 0.0)
            wj = w[j] * picked[:, None]
            R = R - a[:, None] * wj
            A = A + np.abs(a)[:, None] * np.abs(wj)

    # -- what the tests assert; each returns the violations as a bool array
    def shape_violations(self):
        """bool [R]: a pick outside [0, n), a pick after a stop, a non-positive or non-finite coefficient on a pick, or a value other
        than +0.0 after the stop."""
        picked = self.idx >= 0
        after_stop = (~picked[:, :-1] & picked[:, 1:]).any(1) if self.K > 1 else np.zeros(len(picked), bool)
        bad_idx = ((self.idx < -1) | (self.idx >= self.n)).any(1)
        bad_val = (picked & ~(self.val > 0)).any(1) | (picked & ~np.isfinite(self.val)).any(1)
        zero_bits = self.val.view(np.uint32) == 0
        return after_stop | bad_idx | bad_val | (~picked & ~zero_bits).any(1)

    def choice_violations(self):
        """bool [R, K]: a pick whose float64 score on the replayed residual is more than 2 eta below the best."""
        picked = self.idx >= 0
        return picked & ~(self.at >= self.best - 2 * self.eta)

    def stop_violations(self):
        """bool [R]: the FIRST stopped step of a row is legitimate only if the best float64 score is <= 2 eta or a candidate within
        2 eta of the best has a float64 coefficient within its bound of <= 0."""
        picked = self.idx >= 0
        stopped = ~picked
        first = np.where(stopped.any(1), stopped.argmax(1), -1)
        rows = np.nonzero(first >= 0)[0]
        bad = np.zeros(len(picked), bool)
        s = first[rows]
        ok = (self.best[rows, s] <= 2 * self.eta[rows, s]) | (self.amin_near[rows, s] <= 0)
        bad[rows] = ~ok
        return bad

    def value_violations(self):
        """bool [R, K]: a coefficient outside its bound of the float64 one on the replayed residual."""
        picked = self.idx >= 0
        return picked & ~(np.abs(self.val.astype(np.float64) - self.a64) <= self.ab)

    def err_violations(self, err):
        """bool [R, K + 1]: a norm outside its bound of the replayed residual's (a stopped row's residual no longer changes, so the
        held norm obeys the same bound), or -- exactly -- a norm that is not HELD bit for bit after the stop."""
        err = np.asarray(err, np.float32)
        out = ~(np.abs(err.astype(np.float64) - self.E) <= self.Eb)
        stopped = self.idx < 0
        out[:, 1:] |= stopped & (err[:, 1:].view(np.uint32) != err[:, :-1].view(np.uint32))
        return out

    def decided(self):
        """bool [R], for the replay of the FLOAT64 rule's own trace (greedy64): the rows on which the rule leaves the engine no choice.
        The engine's residual differs from this one by its drift (inside eta) and by the coefficients it formed itself: with
        |a - a64| <= ab on equal residuals, a residual difference G feeds the next coefficient by at most G / |w| and the next residual by
        that times |w|, so G_0 = 0, G_{s+1} = 2 G_s + ab_s |w_{j_s}|, and a score moves by at most G_s.  A row is decided when it
        picks at every step and top-two margin and top score both exceed 2 (eta_s + G_s) at every step."""
        picked = self.idx >= 0
        G = np.zeros(len(picked))
        ok = picked.all(1)
        for s in range(self.K):
            tol = 2 * (self.eta[:, s] + G)
            ok &= ((self.best[:, s] - self.second[:, s]) > tol) & (self.best[:, s] > tol)
            j = np.where(picked[:, s], self.idx[:, s], 0)
            G = 2 * G + np.where(picked[:, s], np.nan_to_num(self.ab[:, s]) * self.wn[j], 0.0)
        return ok


def fold_bound(err_sum):
    return FOLD_ROWS * U * np.abs(err_sum) + 2.0 ** -40 * np.abs(err_sum)


def derived(idx, err, taus, n, K):
    """The integer fields of the block recomputed from a trace of the counted rows: (budget [n_tau, K + 2], steps [K + 1], picks [n])
    -- the budget by the kernel's own predicate (one fp32 product, one fp32 compare)."""
    idx = np.asarray(idx, np.int64)
    err = np.asarray(err, np.float32)
    steps = np.bincount((idx >= 0).sum(1), minlength=K + 1)
    picks = np.bincount(idx[idx >= 0], minlength=n)
    budget = np.zeros((len(taus), K + 2), np.int64)
    for t, tau in enumerate(taus):
        lim = (np.float32(tau) * err[:, 0]).astype(np.float32)[:, None]
        hit = err <= lim
        budget[t] = np.bincount(np.where(hit.any(1), hit.argmax(1), K + 1), minlength=K + 2)
    return budget, steps, picks


# ---- a float32 / bf16 emulation of the kernel's rule, with the mistakes the checks must catch
def emulate(w_full, n, x, b, K, *, tie_high=False, abs_score=False, no_z=False, no_q=False, no_coef_stop=False, coef_from_bf16=False,
            no_hold=False, pad_eligible=False):
    """(idx int32 [R, K], val float32 [R, K], err float32 [R, K + 1]) by the rule in float32 -- numpy's own summation orders, which the
    bounds cover.  w_full [n_p, d]: the operand rows with the padding rows (zero in the engine; a test plants garbage there), n of them
    eligible.  The keyword switches are the mutations of tests/test_pursuit_cpu.py."""
    w = np.asarray(w_full, np.float32)
    x = np.asarray(x, np.float32)
    bb = np.zeros(x.shape[1], np.float32) if b is None else np.asarray(b, np.float32)
    q = (w * w).sum(1, dtype=np.float32)
    with np.errstate(divide="ignore"):
        z = np.where(q > 0, (np.float32(1) / np.sqrt(q, dtype=np.float32)).astype(np.float32), np.float32(0))
    elig = (np.arange(w.shape[0]) < (w.shape[0] if pad_eligible else n)) & (z > 0)
    Rn = x.shape[0]
    idx = np.full((Rn, K), -1, np.int32)
    val = np.zeros((Rn, K), np.float32)
    err = np.zeros((Rn, K + 1), np.float32)
    for r in range(Rn):
        res = (x[r] - bb).astype(np.float32)
        err[r, 0] = (res * res).sum(dtype=np.float32)
        live = True
        for s in range(K):
            err[r, s + 1] = np.float32(0) if (no_hold and not live) else err[r, s]
            if not live:
                continue
            rho = bf16(res)
            acc = (w * rho[None, :]).sum(1, dtype=np.float32)
            sc = acc if no_z else (acc * z).astype(np.float32)
            key = np.abs(sc) if abs_score else sc
            key = np.where(elig, key, -np.inf)
            if not elig.any():
                live = False
                continue
            best = key.max()
            cand = np.nonzero(key == best)[0]
            j = int(cand[-1] if tie_high else cand[0])
            if not (best > 0):
                live = False
                continue
            src = rho if coef_from_bf16 else res
            dot = (src * w[j]).sum(dtype=np.float32)
            a = np.float32(dot) if no_q else np.float32(dot / q[j])
            if not (a > 0) and not no_coef_stop:
                live = False
                continue
            res = (res - a * w[j]).astype(np.float32)
            idx[r, s], val[r, s] = j, a
            err[r, s + 1] = (res * res).sum(dtype=np.float32)
    return idx, val, err
