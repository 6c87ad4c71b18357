"""A plain numpy / Python-integer restatement of the resampling rule (include/freud_sae.h, sae_resample_*; the C++ arithmetic it is
compared with: freud_amd/csrc/resample_draw.h).  Test code: nothing here imports the product."""
import math
from fractions import Fraction

import numpy as np

U64 = np.uint64
MASK = (1 << 64) - 1
QBITS = 16
DEAD, PAIRS, SKIPPED_DUPLICATE, TOTAL, LMAX_BITS, NCOUNTS = 0, 1, 2, 3, 4, 8


# ---- weights --------------------------------------------------------------------------------------------------------------
def loss_bits(loss):
    return np.ascontiguousarray(loss, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def l_max_bits(loss) -> int:
    b = loss_bits(loss)
    return int(b.max()) if b.size else 0


def frexp_exp(bits: int) -> int:
    """The frexp exponent of the non-negative float32 with these bits (0 for 0), by math.frexp of its exact value."""
    v = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
    return math.frexp(v)[1] if v != 0 and math.isfinite(v) else (0 if v == 0 else 129)


def weight_q(loss, e: int, qbits: int = QBITS):
    """q_i = floor(l_i 2^(qbits - e)): float64 holds l_i 2^k exactly (a float32 significand, an exponent inside its range)."""
    l = loss_bits(loss).view(np.float32).astype(np.float64)
    q = np.floor(np.ldexp(l, qbits - e))
    return np.minimum(q, float((1 << qbits) - 1)).astype(np.uint64)


def weights(loss, e=None, mutation=None):
    e = frexp_exp(l_max_bits(loss)) if e is None else e
    q = weight_q(loss, e)
    if mutation == "w_linear":
        return q
    if mutation == "w_cubed":
        return q * q * q
    if mutation == "uniform_rows":
        return np.ones_like(q)
    return q * q


def prefix(w, carry: int = 0):
    """The inclusive uint64 prefix continued from `carry`."""
    return np.cumsum(w.astype(np.uint64), dtype=np.uint64) + U64(carry)


# ---- the draw -----------------------------------------------------------------------------------------------------------------
def mix(z):
    """splitmix64's finaliser with its increment, on uint64 arrays (the arithmetic wraps)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def rs_hash(seed: int, round: int, r):
    r = np.asarray(r, dtype=np.uint64)
    s = mix(np.array([seed & MASK], dtype=np.uint64)) ^ U64(round & MASK)
    return mix(mix(s) ^ r)


def mix_int(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def rs_hash_int(seed: int, round: int, r: int) -> int:
    return mix_int(mix_int(mix_int(seed & MASK) ^ (round & MASK)) ^ (r & MASK))


def mulhi64(a, b: int):
    """The high 64 bits of a * b for a uint64 array a and an integer b < 2^64, through 32-bit halves."""
    a = np.asarray(a, dtype=np.uint64)
    m32 = U64(0xFFFFFFFF)
    ah, al = a >> U64(32), a & m32
    bh, bl = U64(b >> 32), U64(b & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
        mid = (ll >> U64(32)) + (lh & m32) + (hl & m32)
        return hh + (lh >> U64(32)) + (hl >> U64(32)) + (mid >> U64(32))


def draw_rows(loss, n_draws: int, seed: int, round: int, mutation=None):
    """The rows that draws r = 0 .. n_draws - 1 pick (no owner rule): first i with c_i > t."""
    w = weights(loss, mutation=mutation)
    if mutation == "first_row_dropped":
        w = w.copy()
        w[0] = 0
    c = prefix(w)
    total = int(c[-1])
    r = np.arange(n_draws, dtype=np.uint64)
    h = r if mutation == "unmixed_counter" else rs_hash(seed, round, r)
    if mutation == "low_bits_only":
        h = h & U64(0xFFFFFFFF)
    t = mulhi64(h, total // 2 if mutation == "half_total" else total)
    if mutation == "exclusive_prefix":
        c = c - w
    if mutation == "last_row_dropped":
        t = mulhi64(h, int(c[-2]))
    i = np.searchsorted(c, t, side="right")
    if mutation == "search_plus_one":
        i = i + 1
    if mutation == "search_minus_one":
        i = i - 1
    if mutation == "mirrored_search":
        i = len(c) - 1 - i
    return np.clip(i, 0, len(c) - 1).astype(np.int64)


MUTATIONS = ("w_linear", "w_cubed", "uniform_rows", "search_plus_one", "search_minus_one", "exclusive_prefix", "first_row_dropped",
             "last_row_dropped", "mirrored_search", "unmixed_counter", "half_total", "low_bits_only")


def select(loss, fire, seed: int, round: int):
    """(latents int32, rows int64, counts int64 [NCOUNTS]) of the selection: the owner of a row is the lowest dead rank that drew it
    (np.unique's first occurrence)."""
    loss = np.ascontiguousarray(loss, dtype=np.float32)
    counts = np.zeros(NCOUNTS, dtype=np.int64)
    dead = np.flatnonzero(np.asarray(fire) == 0).astype(np.int32)
    lmax = l_max_bits(loss)
    c = prefix(weights(loss))
    total = int(c[-1])
    counts[DEAD], counts[TOTAL], counts[LMAX_BITS] = dead.size, np.array([total], dtype=np.uint64).view(np.int64)[0], lmax
    if total == 0 or dead.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), counts
    t = mulhi64(rs_hash(seed, round, np.arange(dead.size, dtype=np.uint64)), total)
    rows = np.searchsorted(c, t, side="right").astype(np.int64)
    _u, first = np.unique(rows, return_index=True)
    own = np.sort(first)
    counts[PAIRS], counts[SKIPPED_DUPLICATE] = own.size, dead.size - own.size
    return dead[own], rows[own], counts


# ---- the column ---------------------------------------------------------------------------------------------------------------
def round_f32(v: Fraction) -> np.float32:
    """v rounded to the nearest float32, ties to even."""
    if v == 0:
        return np.float32(0.0)
    sign, a = (-1 if v < 0 else 1), abs(v)
    if a >= (Fraction(2) - Fraction(2) ** -24) * Fraction(2) ** 127:      # at or beyond the midpoint above the largest finite float32
        return np.float32(sign * np.inf)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = a / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(float(sign * n * ulp))


def fma32(a, b, c) -> np.float32:
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))           # (Inf and NaN travel as in any IEEE operation)
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def norm_sq(x) -> np.float32:
    s = np.float32(0.0)
    for xk in np.asarray(x, dtype=np.float32):
        s = fma32(xk, xk, s)
    return s


def column(x, alpha: float):
    """(degenerate, u float32 [d], b float32) of a drawn row, every step one float32 numpy operation (the sum: an exact fma)."""
    x = np.asarray(x, dtype=np.float32)
    s = norm_sq(x)
    if s == 0 or not np.isfinite(s):
        return True, None, None
    nrm = np.sqrt(s, dtype=np.float32)
    u = (x / nrm).astype(np.float32)
    b = -((np.float32(1.0) - np.float32(alpha)) * nrm)
    return False, u, np.float32(b)


def apply_columns(W, b, m1W, m1b, m2W, m2b, latents, x_rows, alpha: float):
    """The state after sae_resample_apply: W [d, n], b [n] and the two moments of each, copies; -> (the six arrays, applied bool [P])."""
    W, b, m1W, m1b, m2W, m2b = (np.array(a, dtype=np.float32, copy=True) for a in (W, b, m1W, m1b, m2W, m2b))
    applied = np.zeros(len(latents), dtype=bool)
    for i, j in enumerate(latents):
        deg, u, bj = column(x_rows[i], alpha)
        if deg:
            continue
        applied[i] = True
        W[:, j], b[j] = u, bj
        m1W[:, j] = m2W[:, j] = 0
        m1b[j] = m2b[j] = 0
    return (W, b, m1W, m1b, m2W, m2b), applied


def chi_square(rows, w):
    """Pearson's statistic of the draw counts against w_i / total over the rows with w_i > 0 -> (statistic, degrees of freedom);
    a draw on a row of weight 0 gives inf."""
    w = np.asarray(w, dtype=np.float64)
    obs = np.bincount(rows, minlength=w.size).astype(np.float64)
    if (obs[w == 0] > 0).any():
        return float("inf"), int((w > 0).sum()) - 1
    nz = w > 0
    exp = obs.sum() * w[nz] / w.sum()
    return float(((obs[nz] - exp) ** 2 / exp).sum()), int(nz.sum()) - 1
