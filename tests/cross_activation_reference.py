"""The numpy restatement of the cross-activation rule (freud_amd/csrc/cross.h; freud_amd/cross_activation.py), shared by
tests/test_cross_activation_cpu.py and tests/test_cross_activation_gpu.py.  Integers throughout; a score is
(num.astype(f8) / den.astype(f8)).astype(f4), the order numpy.lexsort by (score descending, count descending, partner ascending)."""
import numpy as np

MEASURES = {"jaccard": 0, "cond": 1, "lift": 2, "count": 3}


def file_len(lengths, f, T):
    return T if lengths is None else int(min(max(int(lengths[f]), 1), T))


def cross_table(za, zb, lengths, lag, *, ignore_files=False):
    """za [F, T, n_a], zb [F, T, n_b] of 0/1 -> the table [(n_a + 1), (n_b + 1)] int64 of one lag: X inside, fire_a in the last
    column, fire_b in the last row, n_pairs in the corner.  ignore_files: the WRONG table of one long series (the tests' precondition
    that a file boundary matters); uncounted frames are still on neither side."""
    F, T, n_a = za.shape
    n_b = zb.shape[2]
    za, zb = za.astype(np.int64), zb.astype(np.int64)
    out = np.zeros((n_a + 1, n_b + 1), np.int64)
    if ignore_files:
        keep = np.concatenate([np.arange(T) < file_len(lengths, f, T) for f in range(F)]).astype(np.int64)
        A = np.concatenate([za.reshape(F * T, n_a) * keep[:, None], keep[:, None]], axis=1)
        B = np.concatenate([zb.reshape(F * T, n_b) * keep[:, None], keep[:, None]], axis=1)
        m = F * T - lag
        return A[:m].T @ B[lag:] if m > 0 else out
    for f in range(F):
        n = file_len(lengths, f, T)
        m = n - lag
        if m <= 0:
            continue
        A = np.concatenate([za[f, :m], np.ones((m, 1), np.int64)], axis=1)
        B = np.concatenate([zb[f, lag:n], np.ones((m, 1), np.int64)], axis=1)
        out += A.T @ B
    return out


def split(table):
    """table -> (X [n_a, n_b], fire_a [n_a], fire_b [n_b], n_pairs)"""
    return table[:-1, :-1], table[:-1, -1], table[-1, :-1], int(table[-1, -1])


def scores(table, measure, by_b):
    """[n_a, n_b] fp32 as the rows of side A (by_b = 0) or of side B (by_b = 1; still indexed [i][j]) see them."""
    X, fa, fb, n_pairs = split(np.asarray(table).astype(np.int64))
    x = X.astype(np.float64)
    FA = np.broadcast_to(fa[:, None], X.shape).astype(np.float64)
    FB = np.broadcast_to(fb[None, :], X.shape).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "jaccard":
            s = x / (fa[:, None] + fb[None, :] - X).astype(np.float64)
        elif measure == "cond":
            s = x / (FB if by_b else FA)
        elif measure == "lift":
            s = (x / FA) / (FB / np.float64(n_pairs))
        else:
            s = x
        return s.astype(np.float32)


def ordf(s):
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def reported(table, exclude_diagonal):
    X = split(np.asarray(table))[0]
    live = X > 0
    if exclude_diagonal:
        live = live & ~np.eye(*X.shape, dtype=bool)
    return live


def keys(table, measure, by_b, exclude_diagonal):
    """uint64 [n_a, n_b] (indexed [i][j] in either orientation): ord(score) << 32 | X, 0 where not reported."""
    X = split(np.asarray(table))[0]
    return np.where(reported(table, exclude_diagonal), (ordf(scores(table, measure, by_b)) << np.uint64(32)) | X.astype(np.uint64),
                    np.uint64(0))


def partners(table, measure, K, by_b, exclude_diagonal):
    """The partner tables of one orientation: (partners int64 -1, counts int64 0, scores fp32 NaN) [rows, K]."""
    X = split(np.asarray(table).astype(np.int64))[0]
    S, live = scores(table, measure, by_b), reported(table, exclude_diagonal)
    if by_b:
        X, S, live = X.T, S.T, live.T
    rows = X.shape[0]
    nb = np.full((rows, K), -1, np.int64)
    cn = np.zeros((rows, K), np.int64)
    sc = np.full((rows, K), np.nan, np.float32)
    for i in range(rows):
        j = np.flatnonzero(live[i])
        order = j[np.lexsort((j, -X[i, j], -S[i, j].astype(np.float64)))][:K]
        m = len(order)
        nb[i, :m], cn[i, :m], sc[i, :m] = order, X[i, order], S[i, order]
    return nb, cn, sc


def has_tied_scores(table, measure, by_b, exclude_diagonal):
    S, live = scores(table, measure, by_b), reported(table, exclude_diagonal)
    if by_b:
        S, live = S.T, live.T
    return any(len(np.unique(S[i][live[i]])) < live[i].sum() for i in range(S.shape[0]))
