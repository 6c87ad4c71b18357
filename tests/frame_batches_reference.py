"""What the CPU and GPU tests of frame batches share: freud_amd/csrc/frame_perm.h restated with plain ints and masks, and the
batches an epoch must deliver, in numpy."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
ROUNDS = 4


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_schedule(key):
    return mix((key + GOLD) & M64)


def round_fn(half, r, ks):
    return mix(((half + (r + 1) * GOLD) & M64) ^ ks)


def feistel(ks, b, x):
    wr = b // 2
    wl = b - wr
    L, R = x >> wr, x & ((1 << wr) - 1)
    for r in range(ROUNDS):
        L, R = R, L ^ (round_fn(R, r, ks) & ((1 << wl) - 1))
        wl, wr = wr, wl
    return (L << wr) | R


def feistel_inverse(ks, b, y):
    wr = b // 2
    wl = b - wr
    L, R = y >> wr, y & ((1 << wr) - 1)
    for r in reversed(range(ROUNDS)):
        wl, wr = wr, wl
        L, R = R ^ (round_fn(L, r, ks) & ((1 << wl) - 1)), L
    return (L << wr) | R


def fp_permute(key, N, p, count=None):
    """count: a one-element list that collects the evaluations of the network."""
    ks = key_schedule(key & M64)
    if N <= 2:
        return (p ^ (ks & 1)) if N == 2 else 0
    b = (N - 1).bit_length()
    x = p
    while True:
        x = feistel(ks, b, x)
        if count is not None:
            count[0] += 1
        if x < N:
            return x


def fp_unpermute(key, N, g):
    ks = key_schedule(key & M64)
    if N <= 2:
        return (g ^ (ks & 1)) if N == 2 else 0
    b = (N - 1).bit_length()
    x = g
    while True:
        x = feistel_inverse(ks, b, x)
        if x < N:
            return x


def fp_position(q, rank, world):
    return q * world + rank


def fp_locate(prefix, n_files, T, g):
    """-> (file, t, bad), clamped as the header clamps."""
    if prefix is None:
        f, at = g // T, g % T
    else:
        lo, hi = 0, n_files
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if int(prefix[mid]) <= g:
                lo = mid
            else:
                hi = mid
        f, at = lo, g - int(prefix[lo])
    bad = g < 0 or f < 0 or f >= n_files or at < 0 or at >= T
    return min(max(f, 0), n_files - 1), min(max(at, 0), T - 1), bad


def prefix_of(lengths):
    """The exclusive prefix sum of the trimmed lengths: int64 [n_files + 1]."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def frame_count(n_files, T, lengths=None):
    return n_files * T if lengths is None else int(np.asarray(lengths, dtype=np.int64).sum())


def store_rows(key, N, positions, n_files, T, lengths=None):
    """Positions of the epoch `key` -> the rows of the store's [n_files * T, d] view they hold (int64)."""
    prefix = None if lengths is None else prefix_of(lengths)
    out = np.empty(len(positions), dtype=np.int64)
    for i, p in enumerate(positions):
        f, t, bad = fp_locate(prefix, n_files, T, fp_permute(key, N, int(p)))
        assert not bad
        out[i] = f * T + t
    return out


def epoch_ordinals(key, N, R, rank, world, n_batches, first_batch=0):
    """The counted ordinals of this rank's batches first_batch .. n_batches - 1 of the epoch `key`: int64 [batches, R]."""
    return np.array([[fp_permute(key, N, fp_position(b * R + j, rank, world)) for j in range(R)] for b in range(first_batch, n_batches)],
                    dtype=np.int64).reshape(-1, R)


def ordinals_to_rows(ordinals, n_files, T, lengths=None):
    """Counted ordinals -> rows of the store's [n_files * T, d] view."""
    prefix = None if lengths is None else prefix_of(lengths)
    flat = np.asarray(ordinals, dtype=np.int64).reshape(-1)
    out = np.empty_like(flat)
    for i, g in enumerate(flat):
        f, t, bad = fp_locate(prefix, n_files, T, int(g))
        assert not bad
        out[i] = f * T + t
    return out.reshape(np.shape(ordinals))


def build_batches(shard_rows, T, d, ordinals):
    """shard_rows [n_files, T * d] (any dtype) and rows of its [n_files * T, d] view, int64 [batches, R] -> [batches, R // T, T, d]."""
    frames = np.asarray(shard_rows).reshape(-1, d)
    o = np.asarray(ordinals, dtype=np.int64)
    return frames[o.reshape(-1)].reshape(o.shape[0], o.shape[1] // T, T, d)


def len_loader(N, R, world):
    return (N // world) // R
