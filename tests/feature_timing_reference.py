"""A numpy reference of the feature timing, written differently from the kernels (no walk over the frames, no state): the [L, n]
mask of a file is padded with a zero row on each side, run starts and ends come from np.diff, bridging merges the runs whose gap
is <= g, and durations are binned with searchsorted over closed-form edges rather than through timing_index."""
import numpy as np

ACTIVE, SPAN, RUNS, FILES, LONGEST, CENSORED = range(6)


def closed_form_edges(sub_bits, upto):
    """The lower edges of the bins, ascending, up to the first one above `upto`: 1 .. 2P - 1, then 2^e (1 + m / P) for e >= s + 1."""
    P = 1 << sub_bits
    edges = list(range(1, 2 * P))
    e = sub_bits + 1
    while not edges or edges[-1] <= upto:
        for m in range(P):
            v = (2 ** e) * (P + m) // P          # exact: e >= s + 1
            edges.append(v)
        e += 1
    return np.array(edges, np.int64)


def n_bins(sub_bits, T):
    e = closed_form_edges(sub_bits, T)
    return int(np.searchsorted(e, T, side="right"))


def bins_of(L, sub_bits, T):
    """Bin of every duration in L (>= 1), by value."""
    return np.searchsorted(closed_form_edges(sub_bits, max(T, int(np.max(L, initial=1)))), np.asarray(L, np.int64), side="right") - 1


def file_runs(mask, g):
    """mask bool [L, n] of one file's counted frames -> (latent, first, last) of every run, in latent order then time order, after
    bridging with g; and (latent, gap) of every gap that is left."""
    L, n = mask.shape
    pad = np.zeros((L + 2, n), np.int8)
    pad[1:-1] = mask
    d = np.diff(pad, axis=0)                      # [L + 1, n]: +1 at a start (row = first frame), -1 at row = last frame + 1
    sj, st = np.nonzero((d == 1).T)               # latent-major, time ascending within a latent
    ej, et = np.nonzero((d == -1).T)
    assert np.array_equal(sj, ej)
    first, last = st, et - 1
    if sj.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z, z
    same = sj[1:] == sj[:-1]                      # run i + 1 follows run i in the same latent
    gap = first[1:] - last[:-1] - 1
    merge = same & (gap <= g)                     # run i + 1 continues run i
    head = np.concatenate([[True], ~merge])       # the runs that open a merged group
    tail = np.concatenate([~merge, [True]])
    keep_gap = same & ~merge
    return sj[head], first[head], last[tail], sj[1:][keep_gap], gap[keep_gap]


def timing_reference(masks, sub_bits, g, T):
    """masks: a list of bool [L[f], n] (the counted frames of every file) -> run_hist, gap_hist [n, NB], totals [n, 6], n_frames,
    and a dict of what occurred (for the tests' own assertions about their cases)."""
    n = masks[0].shape[1]
    nb = n_bins(sub_bits, T)
    run_hist, gap_hist = np.zeros((n, nb), np.int64), np.zeros((n, nb), np.int64)
    totals = np.zeros((n, 6), np.int64)
    frames = 0
    seen = {"dur1": 0, "octave": 0, "whole_file": 0, "gaps": 0, "raw_gaps_le_g": 0, "whole_file_by_latent": np.zeros(n, np.int64)}
    P = 1 << sub_bits
    for m in masks:
        m = np.asarray(m, bool)
        L = m.shape[0]
        frames += L
        totals[:, ACTIVE] += m.sum(0)
        rj, first, last, gj, gap = file_runs(m, g)
        if g > 0:
            _, f0, l0, _, gap0 = file_runs(m, 0)
            seen["raw_gaps_le_g"] += int((gap0 <= g).sum())
        dur = last - first + 1
        np.add.at(run_hist, (rj, bins_of(dur, sub_bits, T)), 1)
        np.add.at(gap_hist, (gj, bins_of(gap, sub_bits, T)), 1)
        np.add.at(totals[:, SPAN], rj, dur)
        np.add.at(totals[:, RUNS], rj, 1)
        totals[np.unique(rj), FILES] += 1
        np.maximum.at(totals[:, LONGEST], rj, dur)
        np.add.at(totals[:, CENSORED], rj, ((first == 0) | (last == L - 1)).astype(np.int64))
        seen["dur1"] += int((dur == 1).sum())
        seen["octave"] += int((dur >= 2 * P).sum())
        seen["whole_file"] += int((dur == L).sum())
        np.add.at(seen["whole_file_by_latent"], rj[dur == L], 1)
        seen["gaps"] += int(gap.size)
    return run_hist, gap_hist, totals, frames, seen
