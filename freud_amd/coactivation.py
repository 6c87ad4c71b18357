"""Feature co-activation: which latents of a trained dictionary fire on the same frames -- near-duplicates, families, the dense
latent that rides along with everything -- in one pass over the Whisper-activation shards (without it: encode() of every file, a
threshold, and a dense float Z.T @ Z in torch that computes both halves of a symmetric result).

Semantics (include/freud_sae.h, sae_coact_files / sae_coact_neighbor_keys).  Frames count exactly as in the feature statistics: the
first min(L[f], T) frames of file f when `lengths` is given (file_pass.check_lengths rules), all T otherwise.  Latent j is active on
a frame iff the value freud_amd.models encode() returns for it is > 0 (L1: the bf16 latent of the training kernels; TopK: top_acts
scattered at top_indices, the k selection of a multi_topk model; a -0.0 and a selected zero are not active).  C[i][j] is the number
of counted frames on which i and j are both active: symmetric, C[i][i] == fire_count[i] of feature_stats, int32 (a pass over more
than 2^31 - 1 frames is refused).  Neighbour scores for i != j with C[i][j] > 0, one fp64 division converted once to fp32:

    jaccard   C[i][j] / (C[i][i] + C[j][j] - C[i][j])
    cond      C[i][j] / C[i][i]                            P(j active | i active)
    count     C[i][j]

A latent's neighbours are ordered by score descending, then the larger count, then the lower partner index.  A pair that never
co-fires is not reported, nor the latent itself; empty slots hold partner -1, count 0 and score NaN.  Everything is exact integer
arithmetic on the i8 matrix cores: two runs give bitwise identical arrays.

    python -m freud_amd.coactivation --sae CKPT --data_path DIR --layer_name L [--n_neighbors K] [--measure M] [--lengths f.npy]
                                     [--batch_files B] [--counts] --out coact.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional

import numpy as np
import torch

from .engine import COACT_MEASURES, FILE_TOP_MAX, FILE_TOP_POSITIVE
from .feature_search import unord
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

MAX_FRAMES = 2 ** 31 - 1          # int32 counts
KEY_BLOCK = 1 << 25               # keys per neighbour-selection block (256 MiB of 64-bit keys)
_FIELDS = ("fire_count", "neighbors", "counts", "scores")


@dataclasses.dataclass
class CoActivation:
    """Co-activation of an SAE's latents over a dataset (see the module docstring)."""
    n_frames: int
    fire_count: np.ndarray            # int64 [n]: C[i][i]
    neighbors: np.ndarray             # int64 [n, K], -1 = empty
    counts: np.ndarray                # int64 [n, K], 0 = empty
    scores: np.ndarray                # float32 [n, K], NaN = empty
    matrix: Optional[np.ndarray] = None   # int32 [n, n] (return_counts) or None
    measure: str = "jaccard"

    @property
    def n_latents(self) -> int:
        return int(self.fire_count.shape[0])

    def top(self, j: int):
        """The neighbours of latent j, best first: [(partner, count, score)]."""
        return [(int(p), int(c), float(s)) for p, c, s in zip(self.neighbors[j], self.counts[j], self.scores[j]) if p >= 0]

    def summary(self) -> dict:
        has = self.neighbors[:, 0] >= 0
        best = self.scores[:, 0][has]
        return {"n_frames": int(self.n_frames), "n_latents": self.n_latents, "n_neighbors": int(self.neighbors.shape[1]),
                "measure": self.measure, "dead": int((self.fire_count == 0).sum()), "with_neighbors": int(has.sum()),
                "pairs_reported": int((self.neighbors >= 0).sum()), "max_score": float(best.max()) if best.size else None}

    def to_npz(self, path: str) -> None:
        extra = {} if self.matrix is None else {"matrix": self.matrix}
        np.savez(path, n_frames=np.int64(self.n_frames), measure=np.array(self.measure), **{k: getattr(self, k) for k in _FIELDS}, **extra)

    @classmethod
    def from_npz(cls, path: str) -> "CoActivation":
        with np.load(path) as z:
            return cls(int(z["n_frames"]), *(z[k] for k in _FIELDS), z["matrix"] if "matrix" in z.files else None, str(z["measure"]))


def decode_neighbor_table(top_latents: np.ndarray, top_keys: np.ndarray):
    """[n, K] partners (int32, -1 empty) / neighbour keys -> partners int64, counts int64, scores fp32 (NaN where empty)."""
    k = np.ascontiguousarray(top_keys).view(np.uint64)
    partners = top_latents.astype(np.int64)
    empty = partners < 0
    counts = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    counts[empty] = 0
    scores = np.where(empty, np.float32(np.nan), unord((k >> np.uint64(32)).astype(np.uint32))).astype(np.float32)
    return partners, counts, scores


def _check_args(sae, n_neighbors, measure) -> int:
    if is_raw(sae):
        raise ValueError("feature co-activation needs an SAE (raw-activation co-activation is not provided)")
    n_neighbors = int(n_neighbors)
    if n_neighbors < 1 or n_neighbors > FILE_TOP_MAX:
        raise ValueError(f"n_neighbors={n_neighbors} outside [1, {FILE_TOP_MAX}]")
    if measure not in COACT_MEASURES:
        raise ValueError(f"measure={measure!r} is not one of {sorted(COACT_MEASURES)}")
    return n_neighbors


def select_top_rows(n_rows: int, n_cols: int, n_top: int, write_keys, dev, *, flags: int = FILE_TOP_POSITIVE, row_align: int = 1):
    """Per row of a key table [n_rows, n_cols] its n_top best columns: built and selected in row blocks of at most KEY_BLOCK keys,
    one read-back per block.  write_keys(row0, rows, keys) fills keys [rows, n_cols] (int64 CUDA holding the uint64 keys of
    coact.h / labels.h / dict_match.h) -> (partners, counts, scores) as decode_neighbor_table gives them.  flags: those of
    file_top_features (the scores of co-activation and labels are positive; a cosine is signed and passes 0).  row_align: blocks
    begin at multiples of it where KEY_BLOCK leaves room for one (a key writer that works on aligned tiles computes no row twice)."""
    from . import engine as E

    rows = max(1, min(n_rows, KEY_BLOCK // n_cols))
    if row_align > 1 and row_align <= rows < n_rows:
        rows -= rows % row_align
    keys = torch.empty(rows * n_cols, dtype=torch.int64, device=dev)
    lat = torch.empty(rows * n_top, dtype=torch.int32, device=dev)
    out = torch.empty(rows * n_top, dtype=torch.int64, device=dev)
    tl = np.empty((n_rows, n_top), np.int32)
    tk = np.empty((n_rows, n_top), np.int64)
    for r0 in range(0, n_rows, rows):
        nr = min(rows, n_rows - r0)
        write_keys(r0, nr, keys)
        E.file_top_features(keys, nr, n_cols, n_top, flags, lat, out)
        tl[r0:r0 + nr] = lat[:nr * n_top].view(nr, n_top).cpu().numpy()
        tk[r0:r0 + nr] = out[:nr * n_top].view(nr, n_top).cpu().numpy()
    return decode_neighbor_table(tl, tk)


def neighbor_tables(counts, n: int, n_neighbors: int, measure: str):
    """The neighbour tables of a device count table counts [n, n] (int32 CUDA) -> (partners, counts, scores) as
    decode_neighbor_table gives them."""
    from . import engine as E

    return select_top_rows(n, n, n_neighbors, lambda r0, nr, keys: E.coact_neighbor_keys(counts, n, r0, nr, COACT_MEASURES[measure], keys),
                           counts.device)


@keep_rng
def feature_coactivation(sae, data_path: str, layer_name: str, *, n_neighbors: int = 16, measure: str = "jaccard", lengths=None,
                         subset_size: Optional[int] = None, batch_files: Optional[int] = None,
                         return_counts: bool = False) -> CoActivation:
    """Co-activation counts of every pair of latents of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16
    contexts) over the files of a shard directory, and every latent's n_neighbors best partners by `measure`.  return_counts: also
    the full int32 matrix [n, n] on the host.  batch_files: files per engine call (default: file_pass.default_batch_files)."""
    n_neighbors = _check_args(sae, n_neighbors, measure)
    # (the counts are int32: FilePass refuses more than MAX_FRAMES frames before it loads the SAE or touches the device)
    fp = FilePass(sae, data_path, layer_name, what="feature co-activation", lengths=lengths, subset_size=subset_size,
                  batch_files=batch_files, max_frames=MAX_FRAMES)
    n = fp.eng.n
    with torch.cuda.device(fp.device):
        table = torch.zeros(n, n, dtype=torch.int32, device=fp.device)
        for x, _file0, _nb, lb in fp:
            fp.eng.coact_files(x, table, lb)
        fire = torch.diagonal(table).to(torch.int64).cpu().numpy()
        partners, counts, scores = neighbor_tables(table, n, n_neighbors, measure)
        matrix = table.cpu().numpy() if return_counts else None
    return CoActivation(fp.n_frames, fire, partners, counts, scores, matrix, measure)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Which latents of an SAE fire together over a shard directory.")
    add_pass_arguments(ap)
    ap.add_argument("--n_neighbors", type=int, default=16)
    ap.add_argument("--measure", default="jaccard", choices=sorted(COACT_MEASURES))
    ap.add_argument("--counts", action="store_true", help="also store the full int32 count matrix")
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: feature_coactivation(a.sae, a.data_path, a.layer_name, n_neighbors=a.n_neighbors, measure=a.measure,
                                                         lengths=lengths, batch_files=a.batch_files, return_counts=a.counts))


if __name__ == "__main__":
    main()
