"""Float64 reference, per-element error bound and planted inputs for the CSC sparse backward of the TopK engine (csrc/topk_sparse.h:
csc_count / csc_scan_blocks / csc_scan_latents / csc_items / csc_fill / sparse_bwd<NPAIR> / sparse_combine, then the d b_dec kernels of
csrc/topk_kernels.h).  No GPU use.  Shared by tests/test_topk_backward_bound_cpu.py and tests/test_topk_backward_gpu.py.

The operands, exactly what the kernels read -- all bf16 values, widened to float64 here:

    idx[m][q], a[m][q]     a selection pass: its indices and dense[m][idx] (main: k per row; multi-TopK: 4k per row)
    g_p[m][:]              d (decoder output) of pass p, as the bf16 copy the gathers read (main: de_b, multi-TopK: dm_b)
    xs[m][:]               bf16(fl32(x[m]) - b_dec): one fp32 subtraction, one rounding, recomputed on the host
    wd[j][:], we[j][:]     bf16(W_dec[j]), bf16(W_enc[j]) of the fp32 masters

The reference.  L_j = the entries t = (m, p) of latent j over all passes, in any order;
    s_t = g_p[m] . wd[j],   S_t = |g_p[m]| . |wd[j]|,   gate_t = [a_t > 0],   tau_t = 2^-8 |s_t| + d_p 2^-23 S_t

    dW_dec[j][c] = sum_t a_t g_t[c]                     tol = (L_j + 2) 2^-23 sum_t |a_t g_t[c]|
    dW_enc[j][c] = sum_t gate_t s_t xs[m][c]            tol = sum_t tau_t |xs[m][c]| + (L_j + 2) 2^-23 sum_t (|s_t| + tau_t) |xs[m][c]|
    d b_enc[j]   = sum_t gate_t s_t                     tol = sum_t tau_t + L_j 2^-23 sum_t (|s_t| + tau_t) + 2^-8 |ref|
    d b_dec[c]   = sum_m sum_p g_p[m][c] - sum_j dbe_j we[j][c]
                                                        tol = 2^-8 G_c + M_p 2^-23 G_c + sum_j tol_dbe_j |we[j][c]|
                                                              + n_p 2^-23 sum_j |dbe_j we[j][c]|,      G_c = sum_m sum_p |g_p[m][c]|

Where the terms come from (u = 2^-23: one fp32 ulp per addition, which also admits accumulators that do not round to nearest; the
conventions of tests/decode_reference.py):

  * dW_dec: a product of two bf16 values is exact in fp32, so only the additions round.  A sum of L_j terms in ANY association (pairs
    per trip, 256-entry work items, the combine kernel's four waves) errs by at most (L_j - 1) u sum |terms| to first order; + 2 leaves
    room for the additions of the zero-weight filler entries and the second-order terms.
  * da_t = bf16(fp32 dot): the dot of d_p products in any order is within d_p u S_t of s_t (lane partials, then the wave reduction), its
    rounding to bf16 (8 significant bits, round to nearest: half an ulp of 2^-7) within 2^-8 of it: |da_t - s_t| <= tau_t up to the
    product of the two terms, for which d_p u S_t leaves room (a real dot's error is a fraction of d_p u S_t).  A gated entry
    contributes exactly 0; the table charges it tau_t all the same, which only matters on the two zero rows.
  * dW_enc: the products da_t xs[m][c] (bf16 x bf16) are exact again; sum_t |da_t - s_t| |xs| <= sum_t tau_t |xs|, and the additions
    of terms of size <= (|s_t| + tau_t) |xs| cost (L_j + 2) u of their sum.
  * d b_enc: the same with xs = 1, plus the final bf16 rounding of the stored value, 2^-8 |ref| (the value must be ON the bf16 grid:
    checked separately, a missing rounding moves the answer towards the reference).
  * d b_dec: topk_de_kernel adds the UNROUNDED fp32 g, of which the test only sees the bf16 copy: 2^-8 G_c.  The row sum runs in blocks of
    128 rows and a 16-wave tree, so no addition chain is longer than M_p (also with two passes per row: 2 x 128 + 16 + blocks / 16 < M_p
    for every M_p >= 384 and one pass for the smaller ones): M_p u G_c.  The GEMV sum_j dbe_j we[j][c] takes the unrounded fp32 d b_enc,
    which is within tol_dbe_j of the reference's (that bound contains the stored value's rounding, so it covers either copy), and adds
    n_p products in fp32: n_p u sum_j |dbe_j we[j][c]|.

Nothing in a bound is measured on the code under test.  An empty list has tol = 0: its rows must be zero (the GPU test asks for +0.0 to
the bit).  tests/test_topk_backward_bound_cpu.py keeps the bound honest: a float32 emulation of the kernel's arithmetic violates it
nowhere, each per-latent failure mode of the pipeline violates it on the latents it hits.

Planted inputs (make_case): weights and a batch in which chosen latents have prescribed list lengths.  Planted latent p owns an input
column c_p: W_enc[p] = e_{c_p}, every other latent's weight in that column is 0, b_enc[p] = -1, x[m][c_p] = 8 + b_dec[c_p] on p's row
set and b_dec[c_p] elsewhere: pre[m][p] = 7 on the row set (above every random pre-activation, which are N(0, 1)) and relu(-1) = 0 off
it.  A "hot" latent has b_enc = 6 and a zero encoder row: pre = 6 on every row, it fires on every row (list length M).  Rows M - 1 and M // 2 equal b_dec: sae_in = 0, every
pre-activation is relu(b_enc), so the hot latent and -- lowest column first -- the columns 0 .. q - 2 are selected, the latter with
activation exactly 0: list entries that the ReLU gate must silence.  Row sets are laid cyclically over the other rows from the LAST row
down (the ragged last row block gets planted entries first), so no row holds more than ceil(sum lengths / (M - 2)) planted hits, which
must stay <= k - 2.  Everything else is the random recipe of tests/test_topk_gpu.py::_make_case.  For a bf16 batch b_dec is rounded to
bf16 first, so that the two zero rows stay exactly b_dec in the batch's type."""
import numpy as np
import torch

from tests.decode_reference import as_f32, bf16, bits, round_up

U = 2.0 ** -23
R8 = 2.0 ** -8
CSC_ROWS = 128                 # rows per counting block
CSC_CHUNK = 256                # entries per work item of sparse_bwd_kernel
SB_E = 4                       # entries per trip of sparse_bwd_kernel
REQUIRED_LENGTHS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513)      # + M: the hot latent
PLANT_BIAS, HOT_BIAS, PLANT_X = -1.0, 6.0, 8.0
GRADS = ("W_dec", "W_enc", "b_enc", "b_dec")


# ---- planted inputs -------------------------------------------------------------------------------------------------------------
def allowed_lengths(M, lengths=REQUIRED_LENGTHS):
    """The required lengths that fit the M - 2 rows a planted latent can fire on."""
    return tuple(L for L in lengths if L <= M - 2)


def make_weights(d, n, k, planted_at, n_planted, seed, x_dtype="float32"):
    """-> case dict: P (fp32 torch parameters), planted (latents), cols (their private input columns), hot, and the sizes.
    planted_at: the first of n_planted consecutive latents, or the list of the latents themselves."""
    planted = list(range(planted_at, planted_at + n_planted)) if np.isscalar(planted_at) else [int(p) for p in planted_at]
    assert len(planted) == n_planted == len(set(planted)) <= d and min(planted) > k and max(planted) < n
    hot = min(planted) - 1
    g = torch.Generator().manual_seed(seed)
    We = torch.randn(n, d, generator=g) / d ** 0.5
    Wd = We.clone()
    Wd /= Wd.norm(dim=1, keepdim=True) + torch.finfo(torch.float32).eps
    b_dec = 0.01 * torch.randn(d, generator=g)
    if x_dtype == "bfloat16":
        b_dec = b_dec.bfloat16().float()
    cols = np.unique(np.linspace(0, d - 1, n_planted).round().astype(np.int64))
    assert len(cols) == n_planted
    b_enc = torch.zeros(n)
    We[:, cols] = 0
    for p, c in zip(planted, cols):
        We[p] = 0
        We[p, c] = 1.0
        b_enc[p] = PLANT_BIAS
    We[hot] = 0                 # pre[m][hot] = 6 on every row, whatever the row's norm
    b_enc[hot] = HOT_BIAS
    P ={"encoder.weight": We, "encoder.bias": b_enc, "W_dec": Wd, "b_dec": b_dec}
    return {"d": d, "n": n, "k": k, "P": P, "planted": planted, "cols": cols, "hot": hot, "x_dtype": x_dtype}


def make_batch(case, M, lengths, seed):
    """-> batch dict: x [M][d] (torch, the case's dtype), lengths, rows_of (the row set of every planted latent), zero_rows."""
    d, k, cols = case["d"], case["k"], case["cols"]
    assert len(lengths) == len(case["planted"])
    b_dec = case["P"]["b_dec"]
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(M, 48, generator=g)) @ torch.randn(48, d, generator=g) * 0.2
    zero_rows = (M - 1, M // 2)
    allowed = [m for m in range(M - 1, -1, -1) if m not in zero_rows]
    R = len(allowed)
    x[:, cols] = b_dec[cols]
    hits = np.zeros(M, np.int64)
    rows_of, off = [], 0
    for L, c in zip(lengths, cols):
        assert 0 <= L <= R, f"a planted list of {L} entries does not fit {R} rows"
        rows = np.array([allowed[(off + t) % R] for t in range(L)], np.int64)
        off += L
        x[rows, c] = PLANT_X + b_dec[c]
        hits[rows] += 1
        rows_of.append(np.sort(rows))
    assert hits.max(initial=0) <= k - 2, f"{hits.max()} planted hits in one row, k - 2 = {k - 2}"
    for m in zero_rows:
        x[m] = b_dec
    if case["x_dtype"] == "bfloat16":
        x = x.bfloat16()
        assert all(torch.equal(x[m].float(), b_dec) for m in zero_rows)
    return {"M": M, "x": x, "lengths": tuple(int(L) for L in lengths), "rows_of": rows_of, "zero_rows": zero_rows}


def make_case(d, n, k, M, lengths, planted_at, seed, x_dtype="float32"):
    """Weights and one batch: (case, batch)."""
    case = make_weights(d, n, k, planted_at, len(lengths), seed, x_dtype)
    return case, make_batch(case, M, lengths, seed + 1000)


def list_lengths(idx, n):
    """Entries per latent of one index array [M][q], or of a list of them (the passes of one step)."""
    arrs = idx if isinstance(idx, (list, tuple)) else [idx]
    return sum(np.bincount(np.asarray(i, np.int64).ravel(), minlength=n) for i in arrs)


def assert_coverage(case, batch, idx_passes, a_passes, required=None):
    """The planted structure holds on a selection (the oracle's, or the engine's own): a condition on the INPUTS of the backward,
    raised as an AssertionError -- never a skip.  idx_passes / a_passes: one [M][q] array per pass."""
    n, M, planted, hot = case["n"], batch["M"], case["planted"], case["hot"]
    npass = len(idx_passes)
    idx_passes = [np.asarray(i, np.int64) for i in idx_passes]
    a_passes = [np.asarray(a, np.float64) for a in a_passes]
    L = list_lengths(idx_passes, n)
    for p, want, rows in zip(planted, batch["lengths"], batch["rows_of"]):
        assert L[p] == npass * want, f"planted latent {p}: list length {L[p]}, prescribed {npass} x {want}"
        for idx in idx_passes:
            assert np.array_equal(np.flatnonzero((idx == p).any(1)), rows), f"planted latent {p} fires on other rows than its row set"
    assert L[hot] == npass * M, f"hot latent {hot}: list length {L[hot]}, wanted {npass} x {M}"
    need = allowed_lengths(M) if required is None else tuple(required)
    missing = sorted(set(need) - set(batch["lengths"]))
    assert not missing, f"required list lengths not planted: {missing}"
    got = set(int(v) for v in L)
    missing = sorted(v for v in need if npass * v not in got)
    assert not missing, f"required list lengths absent from the selection: {missing} (x {npass} passes)"
    assert any(v % SB_E for v in got), f"no list length that is not a multiple of {SB_E}"
    for idx, a in zip(idx_passes, a_passes):
        q = idx.shape[1]
        for m in batch["zero_rows"]:
            assert int((a[m] == 0).sum()) == q - 1 and int((a[m] > 0).sum()) == 1 and hot in idx[m], \
                f"zero row {m}: wanted the hot latent and {q - 1} entries of activation 0, got activations {sorted(a[m])[-3:]}"
            assert np.array_equal(np.sort(idx[m][a[m] == 0]), np.arange(q - 1)), f"zero row {m}: the zero entries are not columns 0..{q - 2}"
    if M % CSC_ROWS and sum(batch["lengths"]):
        tail = M // CSC_ROWS * CSC_ROWS
        assert any(len(r) and r.max() >= tail for r in batch["rows_of"]), "no planted entry in the ragged last row block"
    return L


# ---- operands and reference --------------------------------------------------------------------------------------------------------
def _is_bf16(a):
    return not (bits(a) & 0xFFFF).any()


def operands(passes, x, b_dec, W_dec, W_enc, g_exact=None):
    """passes: [(idx [M][q], a [M][q], g [M][d])] in the kernel's pass order (multi-TopK first, main last); a and g must be bf16 values.
    x: [M][d] as the engine received it; the fp32 masters b_dec, W_dec, W_enc.  g_exact (emulation only): the unrounded fp32 g per pass."""
    x32 = as_f32(x).reshape(-1, as_f32(x).shape[-1])
    M, d = x32.shape
    ps = []
    for idx, a, g in passes:
        idx, a, g = np.asarray(idx, np.int64), as_f32(a), as_f32(g)
        assert idx.shape == a.shape and idx.shape[0] == M and g.shape == (M, d)
        assert _is_bf16(a) and _is_bf16(g), "operands of the sparse backward are bf16 values"
        assert (a >= 0).all()
        ps.append({"idx": idx, "a": a, "g": g})
    b32 = as_f32(b_dec)
    return {"M": M, "d": d, "n": W_dec.shape[0], "passes": ps, "xs": bf16(x32 - b32[None, :]), "wd": bf16(W_dec), "we": bf16(W_enc),
            "g_exact": [p["g"] for p in ps] if g_exact is None else [as_f32(g) for g in g_exact]}


def reference(ops):
    """-> {"W_dec": (ref, tol) [n][d], "W_enc": (ref, tol) [n][d], "b_enc": (ref, tol) [n], "b_dec": (ref, tol) [d], "L": [n]}, float64.
    Only the latents with a non-empty list enter the matrix products; the others have ref = tol = 0."""
    M, d, n = ops["M"], ops["d"], ops["n"]
    d_p, n_p, M_p = round_up(d, 128), round_up(n, 128), round_up(M, 128)
    L = list_lengths([p["idx"] for p in ops["passes"]], n)
    J = np.flatnonzero(L > 0)
    pos = np.full(n, -1, np.int64)
    pos[J] = np.arange(len(J))
    wd = ops["wd"][J].astype(np.float64)
    we = ops["we"][J].astype(np.float64)
    xs = ops["xs"].astype(np.float64)
    axs = np.abs(xs)
    nJ = len(J)
    r_wd, t_wd = np.zeros((nJ, d)), np.zeros((nJ, d))
    r_we, t_we_tau, t_we_abs = np.zeros((nJ, d)), np.zeros((nJ, d)), np.zeros((nJ, d))
    r_be, t_be_tau, t_be_abs = np.zeros(nJ), np.zeros(nJ), np.zeros(nJ)
    gsum, gabs = np.zeros(d), np.zeros(d)
    rows = np.arange(M)[:, None]
    for p in ops["passes"]:
        g = p["g"].astype(np.float64)
        A = np.zeros((M, nJ))
        sel = np.zeros((M, nJ), bool)
        A[rows, pos[p["idx"]]] = p["a"]
        sel[rows, pos[p["idx"]]] = True
        assert sel.sum() == p["idx"].size, "an index appears twice in one row of a pass"
        s = g @ wd.T
        S = np.abs(g) @ np.abs(wd).T
        tau = np.where(sel, R8 * np.abs(s) + d_p * U * S, 0.0)
        mag = np.where(sel, np.abs(s), 0.0) + tau
        D = np.where(A > 0, s, 0.0)
        r_wd += A.T @ g
        t_wd += A.T @ np.abs(g)
        r_we += D.T @ xs
        t_we_tau += tau.T @ axs
        t_we_abs += mag.T @ axs
        r_be += D.sum(0)
        t_be_tau += tau.sum(0)
        t_be_abs += mag.sum(0)
        gsum += g.sum(0)
        gabs += np.abs(g).sum(0)
    LJ = L[J].astype(np.float64)
    tol_wd = (LJ + 2)[:, None] * U * t_wd
    tol_we = t_we_tau + (LJ + 2)[:, None] * U * t_we_abs
    tol_be = t_be_tau + LJ * U * t_be_abs + R8 * np.abs(r_be)
    ref_bd = gsum - r_be @ we
    tol_bd = R8 * gabs + M_p * U * gabs + tol_be @ np.abs(we) + n_p * U * (np.abs(r_be) @ np.abs(we))

    def full(v):
        out = np.zeros((n,) + v.shape[1:])
        out[J] = v
        return out

    return {"W_dec": (full(r_wd), full(tol_wd)), "W_enc": (full(r_we), full(tol_we)), "b_enc": (full(r_be), full(tol_be)),
            "b_dec": (ref_bd, tol_bd), "L": L}


def off_grid(out):
    """Boolean: the stored float32 is no bf16 value (its low 16 bits are not zero)."""
    return (bits(out) & 0xFFFF) != 0


def violations(name, out, ref, tol):
    """Boolean, shaped like out: not finite, further than tol from ref, or (d b_enc) not a bf16 value."""
    o = np.asarray(as_f32(out), np.float64)
    bad = ~np.isfinite(o) | ~(np.abs(o - ref) <= tol)
    return bad | off_grid(out) if name == "b_enc" else bad


def worst_ratio(out, ref, tol):
    """max |difference| / tol (0 where both are 0, inf for a difference where tol is 0 or for a non-finite element)."""
    o = np.asarray(as_f32(out), np.float64)
    diff = np.abs(o - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(np.isfinite(o), np.where(diff == 0, 0.0, diff / np.maximum(tol, 1e-300)), np.inf)
    return ratio


def report(name, out, ref, tol, L):
    """The violating share and the worst element with its latent, list length and |difference| / tol, for an assertion message."""
    bad = violations(name, out, ref, tol)
    o = np.asarray(as_f32(out), np.float64)
    ratio = worst_ratio(out, ref, tol)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    where = f"column {at[0]}" if name == "b_dec" else f"latent {at[0]} (list length {int(L[at[0]])})" + (f", column {at[1]}" if len(at) > 1 else "")
    grid = f"; {int(off_grid(out).sum())} are no bf16 value" if name == "b_enc" else ""
    return (f"d {name}: {int(bad.sum())} of {bad.size} elements ({bad.mean():.2%}) violate{grid}; worst at {where}: got {o[at]!r}, "
            f"reference {ref[at]!r}, |difference| / tol = {ratio[at]:.3g}")


def bad_latents(ref, grads):
    """{gradient: sorted latents (columns for b_dec) with a violating element}."""
    out = {}
    for name in GRADS:
        bad = violations(name, grads[name], *ref[name])
        out[name] = np.flatnonzero(bad.reshape(bad.shape[0], -1).any(1))
    return out


# ---- float32 emulation of the kernels' arithmetic (and of their failure modes) -----------------------------------------------------
def entries(ops):
    """The CSC view: (j, m, pass, a) of every entry, sorted by latent and, inside a list, in csc_fill's order (row block, pass,
    64-wide index chunk, row); start[j] .. start[j + 1] is latent j's list."""
    js, ms, ps, aa, qs = [], [], [], [], []
    for pi, p in enumerate(ops["passes"]):
        M, q = p["idx"].shape
        js.append(p["idx"].ravel())
        ms.append(np.repeat(np.arange(M), q))
        qs.append(np.tile(np.arange(q), M))
        ps.append(np.full(M * q, pi))
        aa.append(p["a"].ravel())
    j, m, q, ps, a = (np.concatenate(v) for v in (js, ms, qs, ps, aa))
    order = np.lexsort((m, q // 64, ps, m // CSC_ROWS, j))
    start = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=ops["n"]))])
    return {"j": j[order], "m": m[order], "p": ps[order], "a": a[order].astype(np.float32), "start": start}


def _seq_sum(terms):
    """Sequential float32 sum of the rows of terms, CSC_CHUNK rows at a time, the partial sums added afterwards in order."""
    parts = [np.add.accumulate(terms[i:i + CSC_CHUNK], axis=0, dtype=np.float32)[-1] for i in range(0, len(terms), CSC_CHUNK)]
    return np.add.accumulate(np.stack(parts), axis=0, dtype=np.float32)[-1]


MUTATIONS = ("drop_tail", "drop_from_256", "next_row", "drop_ragged_block", "no_gate", "no_round", "stale_empty", "other_pass")


def emulate(ops, *, reverse=False, mutation=None, latent=None, prev=None):
    """The pipeline in float32 numpy -> {"W_dec", "W_enc", "b_enc", "b_dec"}: per entry da = bf16(fp32 dot), gated; the three sums of a
    list accumulated in float32 in list order (reverse: last entry first), 256 entries per partial sum, the partial sums added
    afterwards; d b_enc rounded to bf16; d b_dec from the unrounded g and the unrounded d b_enc.
    mutation: one failure mode of the pipeline --
      drop_tail          the last entry of every list with L % 256 == 1 is lost
      drop_from_256      entries from 256 on are lost (a second work item that is never combined)
      next_row           one entry of list `latent` gathers row m + 1's g
      drop_ragged_block  the entries of the ragged last 128-row block are lost
      no_gate            da is not gated by a > 0
      no_round           d b_enc is stored unrounded
      stale_empty        an empty list's rows keep `prev` (the gradients of a step before)
      other_pass         one entry of list `latent` gathers the other pass's g (two passes)"""
    assert mutation is None or mutation in MUTATIONS
    M, d, n = ops["M"], ops["d"], ops["n"]
    e = entries(ops)
    gs = [p["g"] for p in ops["passes"]]
    wd, we, xs = ops["wd"], ops["we"], ops["xs"]
    out = {"W_dec": np.zeros((n, d), np.float32), "W_enc": np.zeros((n, d), np.float32), "b_enc": np.zeros(n, np.float32)}
    if mutation == "stale_empty":
        out = {key: np.array(prev[key], np.float32) for key in out}
    dbe_exact = np.zeros(n, np.float32)
    for j in np.flatnonzero(np.diff(e["start"])):
        sl = slice(e["start"][j], e["start"][j + 1])
        m, p, a = e["m"][sl], e["p"][sl], e["a"][sl]
        keep = np.ones(len(m), bool)
        if mutation == "drop_tail" and len(m) % CSC_CHUNK == 1:
            keep[-1] = False
        if mutation == "drop_from_256":
            keep[CSC_CHUNK:] = False
        if mutation == "drop_ragged_block":
            keep &= m < M // CSC_ROWS * CSC_ROWS
        m, p, a = m[keep], p[keep], a[keep]
        gm, gp = m.copy(), p.copy()
        if j == latent and mutation == "next_row":
            t = int(np.flatnonzero(m + 1 < M)[len(m) // 2 if len(m) > 2 else 0])
            gm[t] += 1
        if j == latent and mutation == "other_pass":
            gp[len(m) // 2] = len(gs) - 1 - gp[len(m) // 2]
        G = np.empty((len(m), d), np.float32)
        for pi, g in enumerate(gs):
            G[gp == pi] = g[gm[gp == pi]]
        X = xs[m]
        if reverse:
            G, X, a = G[::-1], X[::-1], a[::-1]
        if len(m) == 0:
            out["W_dec"][j], out["W_enc"][j], out["b_enc"][j] = 0, 0, 0
            continue
        da = bf16((G * wd[j][None, :]).sum(1, dtype=np.float32))
        if mutation != "no_gate":
            da = np.where(a > 0, da, np.float32(0))
        out["W_dec"][j] = _seq_sum(a[:, None] * G)
        out["W_enc"][j] = _seq_sum(da[:, None] * X)
        dbe_exact[j] = _seq_sum(da[:, None])[0]
        out["b_enc"][j] = dbe_exact[j] if mutation == "no_round" else bf16(dbe_exact[j:j + 1])[0]
    per_row = np.zeros((M, d), np.float32)
    for g in ops["g_exact"]:
        per_row = per_row + g
    blocks = [np.add.accumulate(per_row[r:r + CSC_ROWS][::-1] if reverse else per_row[r:r + CSC_ROWS], axis=0, dtype=np.float32)[-1]
              for r in range(0, M, CSC_ROWS)]
    gsum = np.add.accumulate(np.stack(blocks[::-1] if reverse else blocks), axis=0, dtype=np.float32)[-1]
    out["b_dec"] = (gsum - dbe_exact[None, :] @ we).reshape(d).astype(np.float32)
    return out


def oracle_operands(case, batch, multi=False):
    """Operands of the backward from the CPU oracle's forward under the engine's tie rule (fp32-defined bf16 matmuls), with the
    unrounded g for the emulation: (ops, idx_passes, a_passes)."""
    from oracle import sae_oracle as O
    P, k, M, d = case["P"], case["k"], batch["M"], case["d"]
    mode, O.MATMUL_MODE = O.MATMUL_MODE, "fp32"
    try:
        f = O.topk_forward(batch["x"].float().reshape(M, 1, d), P["encoder.weight"], P["encoder.bias"], P["W_dec"], P["b_dec"], k,
                           multi_topk=multi, stable_ties=True)
    finally:
        O.MATMUL_MODE = mode
    tv = f["total_variance"]
    exact = [(2.0 * f["e"] / tv).numpy()]
    sel = [(f["top_indices"].numpy(), f["top_acts"].float().numpy())]
    if multi:
        exact.insert(0, (0.25 * f["e_multi"] / tv).numpy())
        sel.insert(0, (f["multi_indices"].numpy(), f["multi_acts"].float().numpy()))
    passes = [(i, a, bf16(g)) for (i, a), g in zip(sel, exact)]
    ops = operands(passes, batch["x"], P["b_dec"].numpy(), P["W_dec"].numpy(), P["encoder.weight"].numpy(), g_exact=exact)
    return ops, [i for i, _ in sel], [a for _, a in sel]
