"""The rule and the error bounds of the input covariance (sae_input_cov; freud_amd/csrc/input_cov.h; freud_amd/input_pca.py).  Shared by
tests/test_input_pca_cpu.py (the bounds can fail: mutations of the rule fall outside them on the inputs the GPU tests use) and by the
GPU tests (which hold the kernels to them).  Nothing here is a transcription of the kernels.

THE RULE.  The sample is x [n_files][T][d] (fp32 / fp16 / bf16, every value exact in float64); file f counts its first
cnt_f = clamp(length_f, 1, T) frames (T without lengths); N = the counted frames.  With a float64 centre c [d] (None: zeros) the
operand of a counted frame k, column i is a_ki = double(x_ki) - c_i: ONE float64 subtraction, one rounding.  A frame that is not
counted has no operand (a zero, not 0 - c_i).  S_ij = sum_k a_ki a_kj, [d][d], not divided by N, the lower triangle the mirror of
the upper to the bit.

THE BOUND.  u = 2^-53.  The operands a_ki are float64 numbers that the reference forms with the same single rounding, so both sides
sum the SAME N real products p_k = a_ki a_kj.  The engine adds them with one rounding per term: the product is fused into its add (the
matrix instruction, fma) or rounded once and then added (two roundings for that term, which gamma_N below also covers for the first
term and every other term enters one addition fewer than N).  By the standard result on recursive summation in any order (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5 / section 4.2: each p_k is multiplied by at most N factors
(1 + delta), |delta| <= u)
        |S~_ij - S_ij| <= gamma_N A_ij,     gamma_m = m u / (1 - m u),     A_ij = sum_k |a_ki a_kj|
for the kernels' order (frames ascending in a segment, segments ascending) and for any other.  Zero operands (padding, frames that do
not count) add exact zeros and do not enter N.

The reference's own error.  Where numpy.longdouble has a significand of at least 64 bits (nmant >= 63; u_l = 2^-(nmant + 1)), S and A
are formed in it: a product of two float64 numbers is rounded once (u_l), N terms are added, so |S_ref - S| <= gamma_N(u_l) A and the
computed A_ref >= A (1 - gamma_N(u_l)).  Elsewhere exact rationals give S and A exactly and their rounding to float64 costs
u |S| <= u A.  The comparison itself, fl(S~ - S_ref) in the reference's format, rounds once more (u_l or u of the difference).  So the
test asserts
        |fl(S~_ij - S_ref_ij)| (1 + u_r) <= (gamma_N(u) + e_ref) A_ref_ij / (1 - e_ref),      u_r = u_l or u
with e_ref = gamma_N(u_l) (long double) or u (rationals).  No empirical factor anywhere.

Against sae_input_moments.  With c = the engine's own mean, the moments' centred sum of squares css_i is an fp64 sum of the same N
fused squares a_ki^2 in another order, so it carries the same bound gamma_N A_ii, and
        |S~_ii - css_i| <= 2 gamma_N A_ii
(the difference of two float64 numbers within a factor 2 of each other is exact).

The eigenvalues (freud_amd/input_pca.py: InputCovariance.eigh).  Weyl: the eigenvalues of two symmetric matrices differ by at most
the 2-norm, hence the Frobenius norm, of their difference.  The solver (LAPACK's symmetric driver through numpy.linalg.eigh: d - 2
Householder reflections from each side, then an orthogonal iteration on the tridiagonal form) is backward stable: its eigenvalues are
those of S + E with ||E||_F <= gamma~_{d^2} ||S||_F for every orthogonal stage (Higham, Theorem 19.4 and Lemma 19.3 applied from both
sides); with the tridiagonal stage counted as a third of that form and the constant of gamma~ taken as its usual small integer,
        solver_error(S) = 4 d^2 u ||S||_F.
Two solves are compared (the engine's scatter, the reference's), so the tests allow ||S~ - S_ref||_F + solver_error(S~) +
solver_error(S_ref).
"""
import fractions

import numpy as np

u64 = 2.0 ** -53
LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63
u_ld = 2.0 ** -(np.finfo(LD).nmant + 1)
UNIT = 256                          # frames per unit (freud_amd/csrc/input_stats.h)

MUTATIONS = ("fp32_accumulate", "center_fp32", "uncounted_minus_c", "drop_last_group", "tile_swapped", "unmirrored")


def gamma(m, u=u64):
    return m * u / (1.0 - m * u)


def counts(n_files, T, lengths=None):
    return [T] * n_files if lengths is None else [min(max(int(l), 1), T) for l in lengths]


def operands(x, lengths=None, center=None):
    """The operands of the rule: float64 [N, d], the counted frames in file order."""
    x = np.asarray(x)
    F, T, d = x.shape
    c = np.zeros(d, np.float64) if center is None else np.asarray(center, np.float64)
    cnt = counts(F, T, lengths)
    return np.concatenate([x[f, :cnt[f]].astype(np.float64) - c for f in range(F)], axis=0)


def reference(a):
    """a: the operands, float64 [N, d] -> (S_ref, A_ref, e_ref): the scatter and sum |a_ki a_kj| in the widest format at hand
    (numpy.longdouble, or float64 rounded from exact rationals) and the relative error e_ref of both against A (see above)."""
    a = np.asarray(a, np.float64)
    N, d = a.shape
    if LD_OK:
        al = a.astype(LD)
        S = al.T @ al
        A = np.abs(al).T @ np.abs(al)
        return S, A, gamma(N, u_ld)
    fr = [[fractions.Fraction(float(v)) for v in row] for row in a]
    S, A = np.zeros((d, d)), np.zeros((d, d))
    for i in range(d):
        for j in range(i, d):
            s = sum((r[i] * r[j] for r in fr), fractions.Fraction(0))
            t = sum((abs(r[i] * r[j]) for r in fr), fractions.Fraction(0))
            S[i, j] = S[j, i] = float(s)
            A[i, j] = A[j, i] = float(t)
    return S, A, u64


def bound(N, A_ref, e_ref):
    """The allowance on |S~ - S_ref| per element (see the module docstring)."""
    return (gamma(N) + e_ref) * A_ref / (1.0 - e_ref)


def check(out, x, lengths=None, center=None, ref=None):
    """The engine's (or an emulation's) scatter held to the rule: a list of failures, [] when it passes."""
    out = np.asarray(out)
    bad = []
    d = x.shape[-1]
    if out.shape != (d, d) or out.dtype != np.float64:
        return [f"shape {out.shape} {out.dtype}"]
    if out.tobytes() != np.ascontiguousarray(out.T).tobytes():
        bad.append("mirror: the lower triangle is not the upper one to the bit")
    a = operands(x, lengths, center)
    S, A, e = ref if ref is not None else reference(a)
    u_r = u_ld if LD_OK else u64
    diff = np.abs(out.astype(S.dtype) - S) * (1.0 + u_r)
    lim = bound(a.shape[0], A, e)
    over = np.triu(diff > lim)
    if over.any():
        i, j = (int(v[0]) for v in np.nonzero(over))
        bad.append(f"bound: {int(over.sum())} elements of the upper triangle, first S[{i}][{j}] off by {float(diff[i, j]):.3e} > {float(lim[i, j]):.3e}")
    return bad


def exact_scatter(x, lengths=None, center=None):
    """Integer-valued x and centre: the scatter as an int64 product, exact.  (A large case goes through the float64 product: with
    |a| <= 12 every partial sum is an integer below 2^53 in any order, so that product is exact too, and much faster.)"""
    a = operands(x, lengths, center)
    ai = a.astype(np.int64)
    assert np.array_equal(ai.astype(np.float64), a) and np.abs(ai).max(initial=0) <= 12
    if a.size * a.shape[1] > 10 ** 9:
        return (a.T @ a).astype(np.int64)
    return ai.T @ ai


def check_exact(out, x, lengths=None, center=None):
    out = np.asarray(out)
    want = exact_scatter(x, lengths, center).astype(np.float64)
    bad = []
    if out.shape != want.shape:
        return [f"shape {out.shape}"]
    up = np.triu(np.ones_like(want, dtype=bool))
    if not np.array_equal(out[up], want[up]):
        bad.append(f"exact upper: {int((out != want)[up].sum())} elements differ")
    if not np.array_equal(out[~up], want[~up]):
        bad.append(f"exact lower: {int((out != want)[~up].sum())} elements differ")
    return bad


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------------
FRAME_CASES = {"one": (1, 1, None), "three": (1, 3, None), "units": (3, 300, None), "ragged": (5, 300, [300, 1, 257, 0, 256]),
               "long": (2, 1030, [1030, 1027])}


def integer_sample(n_files, T, d, seed):
    """(x float32 [n_files, T, d] integer-valued in [-8, 8], centre float64 [d] integer-valued in [-4, 4])."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(n_files, T, d)).astype(np.float32), rng.integers(-4, 5, size=d).astype(np.float64)


BOUND_SHAPE = (3, 300, 24)
BOUND_LENGTHS = [300, 123, 258]


def bound_sample(seed=7):
    """fp32 N(0, 1) data with a mean of order 10^3 in two dimensions: [3, 300, 24], for lengths BOUND_LENGTHS."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(BOUND_SHAPE)
    x[:, :, 5] += 1000.0
    x[:, :, 17] -= 2500.0
    return x.astype(np.float32)


def planted_sample(n_files, T, d, rank=3, noise=1e-2, seed=3):
    """Rank-`rank` data (standard deviations 3, 2, 1.5 along fixed orthonormal directions) plus small isotropic noise, float32
    [n_files, T, d]; the seed draws the frames, not the directions."""
    basis = np.linalg.qr(np.random.default_rng(1234).standard_normal((d, rank)))[0].T
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_files * T, rank)) * np.array([3.0, 2.0, 1.5])[:rank]
    x = z @ basis + noise * rng.standard_normal((n_files * T, d))
    return x.reshape(n_files, T, d).astype(np.float32)


# ---- an emulation of the decomposition, and its mutations ---------------------------------------------------------------------------
def emulate(x, lengths=None, center=None, mutation=None, tile=64):
    """The scatter by the engine's decomposition in float64 numpy -- zero operands for frames that do not count, the 256-frame units
    of a file added in ascending order, the tiles on or above the diagonal mirrored -- or one of MUTATIONS of it."""
    assert mutation is None or mutation in MUTATIONS
    x = np.asarray(x)
    F, T, d = x.shape
    c = np.zeros(d, np.float64) if center is None else np.asarray(center, np.float64)
    cnt = counts(F, T, lengths)
    if mutation == "center_fp32":
        full = (x.astype(np.float32) - c.astype(np.float32)).astype(np.float64)
    else:
        full = x.astype(np.float64) - c
    S = np.zeros((d, d), np.float32 if mutation == "fp32_accumulate" else np.float64)
    for f in range(F):
        for r0 in range(0, T, UNIT):
            a = full[f, r0:r0 + UNIT].copy()
            n = min(max(cnt[f] - r0, 0), a.shape[0])
            if mutation == "drop_last_group":
                n -= n % 4
            if mutation == "uncounted_minus_c":
                a[n:] = 0.0 - c
            else:
                a[n:] = 0.0
            if mutation == "fp32_accumulate":
                for k in range(a.shape[0]):
                    S += np.outer(a[k], a[k]).astype(np.float32)
            else:
                S += a.T @ a
    S = S.astype(np.float64)
    out = np.zeros((d, d), np.float64)
    for i0 in range(0, d, tile):
        for j0 in range(i0, d, tile):
            blk = S[i0:i0 + tile, j0:j0 + tile]
            if mutation == "tile_swapped" and j0 > i0 and blk.shape[0] == blk.shape[1]:
                blk = blk.T
            out[i0:i0 + tile, j0:j0 + tile] = np.triu(blk) if i0 == j0 else blk
    if mutation != "unmirrored":
        out = np.triu(out) + np.triu(out, 1).T
    return out


def solver_error(S):
    """The allowance on eigenvalues from numpy.linalg.eigh's own rounding (see the module docstring)."""
    S = np.asarray(S, np.float64)
    return 4.0 * S.shape[0] ** 2 * u64 * float(np.linalg.norm(S))
