"""Cross-activation: how often latent i of dictionary A and latent j of dictionary B are active a fixed number of frames apart, for
every pair, in one pass over the Whisper-activation shards.  Two questions, one product: do two dictionaries find the same features
as functions of the data (other layers, other widths, an L1 dictionary against a TopK one, an 8x against a 32x -- where decoder
cosines, dictionary_match.py, have nothing to say), and what follows what in time (A = B, lag > 0).

The rule (freud_amd/csrc/cross.h; include/freud_sae.h, sae_cross_*).  A (n_a latents) and B (n_b latents) see the same files.  File f
has len_f counted frames: min(lengths[f], T), or T without `lengths` (file_pass.check_lengths rules).  A latent is active on a frame
iff the value freud_amd.models encode() returns for it has non-zero magnitude bits (a -0.0 and a selected zero of a TopK row are not
active; a multi_topk model uses its k selection).  For a lag l >= 0

    X_l[i][j]   = #{ (f, t) : t + l < len_f, A_i active at (f, t), B_j active at (f, t + l) }
    fire_a_l[i] = #{ (f, t) : t + l < len_f, A_i active at (f, t) }
    fire_b_l[j] = #{ (f, t) : t + l < len_f, B_j active at (f, t + l) }
    n_pairs_l   = sum_f max(len_f - l, 0)

A pair of frames never crosses a file and an uncounted frame is on neither side of a pair.  A negative lag is the same table with A
and B swapped and is not a parameter.  With A = B and l = 0, X is the co-activation table of coactivation.py.  Counts are int32 (a
pass over more than 2^31 - 1 frames is refused); 0 <= lag < 32768, at most 8 distinct lags in one pass.  Scores, one fixed fp64
expression converted once to fp32:

    jaccard   X / (fire_a + fire_b - X)              overlap of the two firing sets
    cond      X / fire_a   (side "a")                P(B_j at t + l | A_i at t)
              X / fire_b   (side "b")                P(A_i at t | B_j at t + l)
    lift      (X / fire_a) / (fire_b / n_pairs)      cond against the partner's base rate: cond alone is led by dense latents
    count     X

A latent's partners are ordered by score descending, then the larger count, then the lower partner index.  Pairs with X == 0 are not
reported; the diagonal i == j is left out only when A and B are one dictionary and l == 0 (at l > 0 it is the latent's persistence).
Empty slots hold partner -1, count 0 and score NaN.  Everything is exact integer arithmetic on the i8 matrix cores: two runs, and
any batch size, give bitwise identical arrays.

    python -m freud_amd.cross_activation --sae A [--sae_b B] [--data_path_b DIR --layer_name_b L] --data_path DIR --layer_name L
                                         [--lags 0,1,2,4] [--n_neighbors K] [--measure M] [--lengths f.npy] [--batch_files B]
                                         [--counts] --out cross.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional

import numpy as np
import torch

from .coactivation import MAX_FRAMES, select_top_rows
from .engine import CROSS_MAX_LAG, CROSS_MAX_LAGS, CROSS_MEASURES, CROSS_SOURCE, CROSS_TARGET, FILE_TOP_MAX
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

RESERVE_BYTES = 4 << 30           # device memory the tables and masks leave free
_FIELDS = ("lags", "n_pairs", "fire_a", "fire_b", "partners_a", "counts_a", "scores_a", "partners_b", "counts_b", "scores_b")


@dataclasses.dataclass
class CrossActivation:
    """Cross-activation of two dictionaries (or of one with itself) over a dataset, per lag (see the module docstring)."""
    lags: np.ndarray                  # int64 [L]
    n_pairs: np.ndarray               # int64 [L]
    fire_a: np.ndarray                # int64 [L, n_a]
    fire_b: np.ndarray                # int64 [L, n_b]
    partners_a: np.ndarray            # int64 [L, n_a, K]: the partners in B of every latent of A, -1 = empty
    counts_a: np.ndarray              # int64 [L, n_a, K], 0 = empty
    scores_a: np.ndarray              # float32 [L, n_a, K], NaN = empty
    partners_b: np.ndarray            # int64 [L, n_b, K]: the partners in A of every latent of B
    counts_b: np.ndarray
    scores_b: np.ndarray
    tables: Optional[np.ndarray] = None   # int32 [L, n_a, n_b] (return_counts) or None
    measure: str = "jaccard"
    same_dictionary: bool = False

    def _lag(self, lag: int) -> int:
        at = np.flatnonzero(self.lags == int(lag))
        if at.size == 0:
            raise KeyError(f"lag {lag} is not one of {self.lags.tolist()}")
        return int(at[0])

    def _side(self, side: str):
        if side not in ("a", "b"):
            raise ValueError(f"side={side!r} is neither 'a' nor 'b'")
        return ((self.partners_a, self.counts_a, self.scores_a, self.fire_a) if side == "a" else
                (self.partners_b, self.counts_b, self.scores_b, self.fire_b))

    def top(self, i: int, lag: int = 0, side: str = "a"):
        """The partners of latent i of `side` at `lag`, best first: [(partner, count, score)]."""
        p, c, s, _ = self._side(side)
        l = self._lag(lag)
        return [(int(a), int(b), float(v)) for a, b, v in zip(p[l, i], c[l, i], s[l, i]) if a >= 0]

    def mutual_best(self, lag: int = 0):
        """The pairs that are each other's first partner at `lag`: [(i in A, j in B, count, score as A sees it)], by ascending i."""
        l = self._lag(lag)
        first = self.partners_a[l, :, 0]
        i = np.flatnonzero(first >= 0)
        i = i[self.partners_b[l, first[i], 0] == i]
        return [(int(a), int(first[a]), int(self.counts_a[l, a, 0]), float(self.scores_a[l, a, 0])) for a in i]

    def coverage(self, lag: int = 0, threshold: float = 0.5, side: str = "a") -> float:
        """The share of the latents of `side` that fire inside the lag's window whose best partner scores at least `threshold`
        (0.0 where none fires) -- the activation counterpart of DictionaryMatch.matched."""
        _p, _c, s, fire = self._side(side)
        l = self._lag(lag)
        firing = fire[l] > 0
        best = s[l, :, 0]
        hit = firing & ~np.isnan(best) & (best >= np.float32(threshold))
        return float(hit.sum() / firing.sum()) if firing.any() else 0.0

    def summary(self) -> dict:
        per_lag = []
        for l, lag in enumerate(self.lags.tolist()):
            best = self.scores_a[l, :, 0]
            best = best[~np.isnan(best)]
            per_lag.append({"lag": lag, "n_pairs": int(self.n_pairs[l]), "pairs_reported": int((self.partners_a[l] >= 0).sum()),
                            "mutual_best": len(self.mutual_best(lag)), "max_score": float(best.max()) if best.size else None})
        return {"n_a": int(self.fire_a.shape[1]), "n_b": int(self.fire_b.shape[1]), "n_neighbors": int(self.partners_a.shape[2]),
                "measure": self.measure, "same_dictionary": bool(self.same_dictionary), "lags": per_lag}

    def to_npz(self, path: str) -> None:
        extra = {} if self.tables is None else {"tables": self.tables}
        np.savez(path, measure=np.array(self.measure), same_dictionary=np.bool_(self.same_dictionary),
                 **{k: getattr(self, k) for k in _FIELDS}, **extra)

    @classmethod
    def from_npz(cls, path: str) -> "CrossActivation":
        with np.load(path) as z:
            return cls(*(z[k] for k in _FIELDS), z["tables"] if "tables" in z.files else None, str(z["measure"]),
                       bool(z["same_dictionary"]))


def check_lags(lags) -> list:
    """The lags of one pass as a list of ints: 1 to CROSS_MAX_LAGS distinct values in [0, CROSS_MAX_LAG)."""
    try:
        out = [int(v) for v in lags]
        whole = all(float(v) == int(v) for v in lags)
    except (TypeError, ValueError):
        raise ValueError(f"lags={lags!r} is not a sequence of integers") from None
    if not whole:
        raise ValueError(f"lags={lags!r} is not a sequence of integers")
    if not 1 <= len(out) <= CROSS_MAX_LAGS:
        raise ValueError(f"{len(out)} lags: one pass takes 1 to {CROSS_MAX_LAGS}")
    for v in out:
        if v < 0 or v >= CROSS_MAX_LAG:
            raise ValueError(f"lag {v} outside [0, {CROSS_MAX_LAG}) (a negative lag is the table of (B, A))")
    if len(set(out)) != len(out):
        raise ValueError(f"lags={out} holds a duplicate")
    return out


def _listing(data_path, layer_name: str, subset_size):
    """(T, the filenames in file order) of a shard directory or a resident store of one, read without a device."""
    from .loader import MemoryMappedActivationsDataset
    from .resident import ResidentActivations
    if isinstance(data_path, ResidentActivations):
        ds = data_path.dataset
        names = list(ds.metadata["filenames"])[:len(data_path) if subset_size is None else int(subset_size)]
    else:
        ds = MemoryMappedActivationsDataset(data_path, layer_name, subset_size)
        names = list(ds.metadata["filenames"])
    return int(ds.tensor_shape[-2]), names


def check_same_files(data_path, layer_name: str, data_path_b, layer_name_b: str, subset_size) -> None:
    """Two shard directories hold the same files, frame for frame: the same number of files, the same T and the same names in the
    same order -- or ValueError, before any device work."""
    (Ta, a), (Tb, b) = _listing(data_path, layer_name, subset_size), _listing(data_path_b, layer_name_b, subset_size)
    if len(a) != len(b):
        raise ValueError(f"the two directories hold {len(a)} and {len(b)} files")
    if Ta != Tb:
        raise ValueError(f"the two directories hold files of T={Ta} and T={Tb} frames")
    for f, (na, nb) in enumerate(zip(a, b)):
        if na != nb:
            raise ValueError(f"file {f} is {na!r} in one directory and {nb!r} in the other: the filename lists must be equal")


def _check_args(sae_a, sae_b, data_path_b, layer_name_b, lags, n_neighbors, measure):
    if is_raw(sae_a) or (sae_b is not None and is_raw(sae_b)):
        raise ValueError("cross-activation needs an SAE on either side (raw-activation mode is not provided)")
    if (data_path_b is None) != (layer_name_b is None):
        raise ValueError("data_path_b and layer_name_b go together")
    if data_path_b is not None and sae_b is None:
        raise ValueError("data_path_b / layer_name_b need sae_b: one dictionary reads one directory")
    n_neighbors = int(n_neighbors)
    if n_neighbors < 1 or n_neighbors > FILE_TOP_MAX:
        raise ValueError(f"n_neighbors={n_neighbors} outside [1, {FILE_TOP_MAX}]")
    if measure not in CROSS_MEASURES:
        raise ValueError(f"measure={measure!r} is not one of {sorted(CROSS_MEASURES)}")
    return check_lags(lags), n_neighbors


def accumulate(fp_a: FilePass, fp_b: Optional[FilePass], own_shards: bool, lags, tables) -> None:
    """The pass itself: tables (zeroed int32 CUDA [L, n_a + 1, n_b + 1]) += every batch of fp_a.  fp_b=None: one dictionary against
    itself, one encode per batch.  own_shards: fp_b walks its own directory in lockstep; otherwise B encodes fp_a's batches."""
    from . import engine as E

    L, T = len(lags), fp_a.T
    n_a = fp_a.eng.n
    n_b = fp_b.eng.n if fp_b is not None else n_a
    rows_max = fp_a.batch_files * T
    dev = fp_a.device
    if fp_b is None:
        masks_a = torch.empty((1 + L) * E.cross_mask_bytes(n_a, rows_max), dtype=torch.int8, device=dev)
        masks_b = None
    else:
        masks_a = torch.empty(E.cross_mask_bytes(n_a, rows_max), dtype=torch.int8, device=dev)
        masks_b = torch.empty(L * E.cross_mask_bytes(n_b, rows_max), dtype=torch.int8, device=dev)
    batches = zip(fp_a, fp_b) if own_shards else ((ba, ba) for ba in fp_a)
    for (xa, file0, nb, lb), (xb, file0_b, nb_b, _lb) in batches:
        if (file0, nb) != (file0_b, nb_b):
            raise RuntimeError(f"the two passes fell out of step at file {file0} / {file0_b}")
        rows = nb * T
        one_a, one_b = E.cross_mask_bytes(n_a, rows), E.cross_mask_bytes(n_b, rows)
        if fp_b is None:
            fp_a.eng.cross_mask_files(xa, masks_a, CROSS_SOURCE | CROSS_TARGET, lags, lb)
            targets = masks_a[one_a:]
        else:
            fp_a.eng.cross_mask_files(xa, masks_a, CROSS_SOURCE, (), lb)
            fp_b.eng.cross_mask_files(xb, masks_b, CROSS_TARGET, lags, lb)
            targets = masks_b
        for l in range(L):
            E.cross_update(masks_a[:one_a], n_a, targets[l * one_b:(l + 1) * one_b], n_b, rows, tables[l])


@keep_rng
def cross_activation(sae_a, data_path, layer_name: str, *, sae_b=None, data_path_b=None, layer_name_b: Optional[str] = None,
                     lags=(0,), n_neighbors: int = 16, measure: str = "jaccard", lengths=None, subset_size: Optional[int] = None,
                     batch_files: Optional[int] = None, return_counts: bool = False) -> CrossActivation:
    """Cross-activation counts of every pair (latent of A, latent of B) at every lag over the files of a shard directory, and every
    latent's n_neighbors best partners on the other side by `measure`, in both orientations.  sae_a / sae_b: a checkpoint path, a
    freud_amd.models SAE or a SaeEngine (bf16 contexts).  sae_b=None: A against itself, one encode per batch.  sae_b alone: two
    dictionaries over the same shards.  With data_path_b / layer_name_b, B reads its own shard directory (another layer, possibly
    another d and dtype) that must hold the same files: the same number, T and filename list.  data_path / data_path_b: a
    directory or a freud_amd.resident.ResidentActivations of it.  return_counts: also the int32 tables [L, n_a, n_b] on the host.
    batch_files: files per engine call (default: the smaller of what file_pass.default_batch_files gives either side)."""
    lags, n_neighbors = _check_args(sae_a, sae_b, data_path_b, layer_name_b, lags, n_neighbors, measure)
    if data_path_b is not None:
        check_same_files(data_path, layer_name, data_path_b, layer_name_b, subset_size)
    # (the counts are int32: FilePass refuses more than MAX_FRAMES frames before it loads the SAE or touches the device)
    common = dict(what="cross-activation", lengths=lengths, subset_size=subset_size, batch_files=batch_files, max_frames=MAX_FRAMES)
    fp_a = FilePass(sae_a, data_path, layer_name, **common)
    fp_b = None
    if sae_b is not None:
        fp_b = FilePass(sae_b, *((data_path_b, layer_name_b) if data_path_b is not None else (data_path, layer_name)), **common)
        if fp_b.device != fp_a.device:
            raise ValueError(f"the two dictionaries live on {fp_a.device} and {fp_b.device}")
        fp_a.batch_files = fp_b.batch_files = min(fp_a.batch_files, fp_b.batch_files)      # lockstep: what both engines take
    n_a = fp_a.eng.n
    n_b = fp_b.eng.n if fp_b is not None else n_a
    L, K, dev = len(lags), n_neighbors, fp_a.device
    from . import engine as E

    with torch.cuda.device(dev):
        rows_max = fp_a.batch_files * fp_a.T
        need = L * (n_a + 1) * (n_b + 1) * 4 + (E.cross_mask_bytes(n_a, rows_max) * (1 if fp_b is not None else 1 + L)
                                                + (E.cross_mask_bytes(n_b, rows_max) * L if fp_b is not None else 0))
        room = int(torch.cuda.mem_get_info(dev)[0]) - RESERVE_BYTES
        if need > room:
            raise ValueError(f"the {L} tables and the masks need {need} bytes, the device has {room} free beyond its reserve of "
                             f"{RESERVE_BYTES} (fewer lags, or fewer files per batch)")
        tables = torch.zeros(L, n_a + 1, n_b + 1, dtype=torch.int32, device=dev)
        accumulate(fp_a, fp_b, data_path_b is not None, lags, tables)
        margins_a = tables[:, :n_a, n_b].to(torch.int64).cpu().numpy()
        margins_b = tables[:, n_a, :n_b].to(torch.int64).cpu().numpy()
        n_pairs = tables[:, n_a, n_b].to(torch.int64).cpu().numpy()
        if 0 in lags:
            fp_a.check_counted(n_pairs[lags.index(0)])
        m = CROSS_MEASURES[measure]
        sides = []
        for by_b, (n_rows, n_cols) in enumerate(((n_a, n_b), (n_b, n_a))):
            per_lag = []
            for l, lag in enumerate(lags):
                excl = int(fp_b is None and lag == 0)
                per_lag.append(select_top_rows(n_rows, n_cols, K, lambda r0, nr, keys, l=l, excl=excl, by_b=by_b:
                                               E.cross_keys(tables[l], n_a, n_b, m, by_b, excl, r0, nr, keys), dev))
            sides.append([np.stack([t[q] for t in per_lag]) for q in range(3)])
        interior = tables[:, :n_a, :n_b].cpu().numpy() if return_counts else None
    return CrossActivation(np.asarray(lags, np.int64), n_pairs, margins_a, margins_b, *sides[0], *sides[1], interior, measure,
                           fp_b is None)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Co-firing of the latents of two dictionaries (or of one with itself) across time lags.")
    add_pass_arguments(ap)
    ap.add_argument("--sae_b", default=None, help="the second dictionary's checkpoint (default: --sae against itself)")
    ap.add_argument("--data_path_b", "--data-path-b", dest="data_path_b", default=None, help="B's own shard directory (the same files)")
    ap.add_argument("--layer_name_b", "--layer-name-b", dest="layer_name_b", default=None)
    ap.add_argument("--lags", default="0", help="comma-separated frame lags, e.g. 0,1,2,4")
    ap.add_argument("--n_neighbors", type=int, default=16)
    ap.add_argument("--measure", default="jaccard", choices=sorted(CROSS_MEASURES))
    ap.add_argument("--counts", action="store_true", help="also store the int32 count tables")
    a = ap.parse_args(argv)
    lags = [int(v) for v in a.lags.split(",")]
    run_pass_cli(a, lambda lengths: cross_activation(a.sae, a.data_path, a.layer_name, sae_b=a.sae_b, data_path_b=a.data_path_b,
                                                     layer_name_b=a.layer_name_b, lags=lags, n_neighbors=a.n_neighbors,
                                                     measure=a.measure, lengths=lengths, batch_files=a.batch_files,
                                                     return_counts=a.counts))


if __name__ == "__main__":
    main()
