"""Dictionary comparison: what a trained dictionary IS, against another one or against itself -- which 32x latents an 8x latent split
into, whether the TopK run found the features of the L1 run, whether two seeds converged (mean max cosine similarity, MMCS), which
latents duplicate each other -- in one GPU pass (without it: torch's normalize(A) @ normalize(B).T and topk, a 6.7 GB fp32 matrix at
n = 40 960 or a hand-written block loop).

Semantics (include/freud_sae.h, sae_dict_pack / sae_dict_sim_keys).  A dictionary is n directions of length d in fp32: the rows of a
TopK model's W_dec [n][d], the columns of an L1 model's tied decoder.weight [d][n]; both are read in place through their strides.
u = w / ||w|| (fp32 sum of squares in one fixed order, IEEE square root and division; a direction of norm 0 stays the zero vector),
S[i][j] = <ua_i, ub_j> on the bf16 MFMA with every unit vector split into hi + lo bf16 parts (error a few 1e-7, not bf16's few
1e-4).  Per direction i of A its n_neighbors directions of B by cosine descending, then the lower index; signed values as they are.
Self mode (b=None): i is not its own neighbour.  Empty slots hold neighbour -1 and cosine NaN.  Two runs give bitwise identical
arrays, whatever the row blocking.

    python -m freud_amd.dictionary_match --a CKPT [--b CKPT] [--n-neighbors K] [--threshold T] [--out FILE.npz]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
from typing import NamedTuple, Optional

import numpy as np
import torch

from .coactivation import select_top_rows
from .engine import DICT_LEFT, DICT_MAX_D, DICT_MAX_N, DICT_RIGHT, FILE_TOP_MAX
from .file_pass import keep_rng

ROW_ALIGN = 256                   # dict_match.h: DM_ROW_ALIGN, the tile edge of the similarity GEMM
_FIELDS = ("neighbors", "cosines", "norms_a", "norms_b")


class Directions(NamedTuple):
    """A dictionary's directions in place: `weights` is an fp32 tensor seen as [n][d] (a view: its strides are the two below)."""
    weights: torch.Tensor
    dir_stride: int
    elem_stride: int

    @property
    def n(self) -> int:
        return int(self.weights.shape[0])

    @property
    def d(self) -> int:
        return int(self.weights.shape[1])


@dataclasses.dataclass
class DictionaryMatch:
    """Nearest decoder directions of B for every direction of A (see the module docstring)."""
    neighbors: np.ndarray             # int32 [n_a, K], -1 = empty
    cosines: np.ndarray               # float32 [n_a, K], NaN = empty
    norms_a: np.ndarray               # float32 [n_a]
    norms_b: np.ndarray               # float32 [n_b]
    self_mode: bool = False

    @property
    def n_a(self) -> int:
        return int(self.norms_a.shape[0])

    @property
    def n_b(self) -> int:
        return int(self.norms_b.shape[0])

    def top(self, i: int):
        """The neighbours of direction i of A, best first: [(index in B, cosine)]."""
        return [(int(j), float(c)) for j, c in zip(self.neighbors[i], self.cosines[i]) if j >= 0]

    def best(self):
        """(index int32 [n_a], cosine fp32 [n_a]) of every direction's nearest neighbour (-1 / NaN where it has none)."""
        return self.neighbors[:, 0], self.cosines[:, 0]

    def mmcs(self) -> float:
        """Mean max cosine similarity: the mean of the rank-0 cosines (NaN when no direction has a neighbour)."""
        c = self.cosines[:, 0]
        c = c[~np.isnan(c)]
        return float(c.astype(np.float64).mean()) if c.size else float("nan")

    def matched(self, threshold: float) -> np.ndarray:
        """bool [n_a]: the direction has a neighbour with cosine >= threshold."""
        c = self.cosines[:, 0]
        return ~np.isnan(c) & (c >= np.float32(threshold))

    def duplicates(self, threshold: float) -> np.ndarray:
        """Self mode: the pairs i < j with cosine >= threshold among the reported neighbours, int64 [pairs, 2] in ascending order
        (a direction with more than n_neighbors such partners shows its n_neighbors nearest)."""
        if not self.self_mode:
            raise ValueError("duplicates() is defined for a dictionary compared with itself (b=None)")
        hit = (self.neighbors >= 0) & (np.nan_to_num(self.cosines, nan=-np.inf) >= np.float32(threshold))
        i, k = np.nonzero(hit)
        j = self.neighbors[i, k].astype(np.int64)
        pairs = np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1).astype(np.int64).reshape(-1, 2)
        return np.unique(pairs, axis=0) if pairs.size else pairs

    def summary(self, threshold: Optional[float] = None) -> dict:
        c = self.cosines[:, 0]
        c = c[~np.isnan(c)]
        out = {"n_a": self.n_a, "n_b": self.n_b, "n_neighbors": int(self.neighbors.shape[1]), "self_mode": bool(self.self_mode),
               "mmcs": self.mmcs() if c.size else None, "min_best": float(c.min()) if c.size else None,
               "median_best": float(np.median(c)) if c.size else None, "max_best": float(c.max()) if c.size else None,
               "zero_norm_a": int((self.norms_a == 0).sum()), "zero_norm_b": int((self.norms_b == 0).sum())}
        if threshold is not None:
            out["threshold"] = float(threshold)
            out["matched"] = int(self.matched(threshold).sum())
            if self.self_mode:
                out["duplicate_pairs"] = int(self.duplicates(threshold).shape[0])
        return out

    def to_npz(self, path: str) -> None:
        np.savez(path, self_mode=np.bool_(self.self_mode), **{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_npz(cls, path: str) -> "DictionaryMatch":
        with np.load(path) as z:
            return cls(*(z[k] for k in _FIELDS), bool(z["self_mode"]))


def _model_directions(model) -> Directions:
    sd = model.state_dict()
    if "W_dec" in sd:                             # TopK: the rows of W_dec [n][d]
        w = sd["W_dec"].to(model.device)
    else:                                         # L1: the columns of the tied decoder.weight [d][n], seen as [n][d] without a copy
        w = sd["decoder.weight"].to(model.device).t()
    return Directions(w, int(w.stride(0)), int(w.stride(1)))


def decoder_directions(obj, device=None) -> Directions:
    """The decoder directions of `obj` -- a freud_amd.models SAE, a checkpoint path (init_sae_from_checkpoint) or an [n][d] tensor /
    ndarray (any strides: pass decoder.weight.T for the L1 layout) -- as an fp32 tensor on the GPU seen as [n][d], with its direction
    and element strides.  Nothing is transposed: an L1 dictionary comes back as a view of its [d][n] weight.  Non-finite weights and
    shapes outside 1 <= n <= 2^24, 1 <= d <= 8192 raise ValueError, for host data before the GPU is touched."""
    if isinstance(obj, Directions):
        return obj
    if isinstance(obj, str):
        from .models import init_sae_from_checkpoint
        obj = init_sae_from_checkpoint(obj, device="cuda" if device is None else device)
    if hasattr(obj, "state_dict") and hasattr(obj, "n_dict_components"):      # a freud_amd.models SAE
        dirs = _model_directions(obj)
        _check_directions(dirs.weights)
        return dirs
    w = _host_checked(obj)
    if not w.is_cuda:
        w = w.to("cuda" if device is None else device)
    if min(w.stride()) < 1:                       # (an expanded or otherwise degenerate view)
        w = w.contiguous()
    return Directions(w, int(w.stride(0)), int(w.stride(1)))


def _host_checked(obj) -> torch.Tensor:
    """An [n][d] tensor / ndarray as an fp32 tensor where it lives, its shape and values checked."""
    w = obj if isinstance(obj, torch.Tensor) else torch.from_numpy(np.asarray(obj))
    w = w.detach()
    if w.dim() != 2:
        raise ValueError(f"a dictionary is an [n][d] array of directions, got shape {tuple(w.shape)}")
    if w.dtype != torch.float32:
        w = w.float()
    _check_directions(w)
    return w


def _check_directions(w: torch.Tensor) -> None:
    n, d = (int(v) for v in w.shape)
    if not (1 <= n <= DICT_MAX_N and 1 <= d <= DICT_MAX_D):
        raise ValueError(f"a dictionary of {n} directions of length {d}: n must be in [1, 2^24] and d in [1, {DICT_MAX_D}]")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("the dictionary holds non-finite weights")


def _check_n_neighbors(n_neighbors) -> int:
    n_neighbors = int(n_neighbors)
    if n_neighbors < 1 or n_neighbors > FILE_TOP_MAX:
        raise ValueError(f"n_neighbors={n_neighbors} outside [1, {FILE_TOP_MAX}]")
    return n_neighbors


def pack_directions(dirs: Directions, side: int):
    """-> (the packed GEMM operand of sae_dict_pack as a uint8 CUDA tensor, norms fp32 [n] on the device)."""
    from . import engine as E

    w = dirs.weights
    packed = torch.empty(E.dict_pack_bytes(dirs.n, dirs.d), dtype=torch.uint8, device=w.device)
    norms = torch.empty(dirs.n, dtype=torch.float32, device=w.device)
    E.dict_pack(w, dirs.n, dirs.d, dirs.dir_stride, dirs.elem_stride, side, packed, norms)
    return packed, norms


@keep_rng
def compare_dictionaries(a, b=None, *, n_neighbors: int = 8) -> DictionaryMatch:
    """For every decoder direction of `a` its n_neighbors nearest directions of `b` by cosine (a, b: whatever decoder_directions
    takes).  b=None compares `a` with itself: a direction is not its own neighbour."""
    from . import engine as E

    n_neighbors = _check_n_neighbors(n_neighbors)
    self_mode = b is None
    # arrays are checked where they live, both before either moves to the GPU
    a, b = (_host_checked(o) if isinstance(o, (torch.Tensor, np.ndarray)) else o for o in (a, b))
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape[1] != b.shape[1]:
        raise ValueError(f"the dictionaries live in different spaces: d={a.shape[1]} and d={b.shape[1]}")
    da = decoder_directions(a)
    dev = da.weights.device
    db = da if self_mode else decoder_directions(b, device=dev)
    if da.d != db.d:
        raise ValueError(f"the dictionaries live in different spaces: d={da.d} and d={db.d}")
    if db.weights.device != dev:
        wb = db.weights.to(dev)
        db = Directions(wb, int(wb.stride(0)), int(wb.stride(1)))
    n_a, n_b, d = da.n, db.n, da.d
    with torch.cuda.device(dev):
        pa, norms_a = pack_directions(da, DICT_LEFT)
        pb, norms_b = pack_directions(db, DICT_RIGHT)
        partners, _counts, cosines = select_top_rows(
            n_a, n_b, n_neighbors, lambda r0, nr, keys: E.dict_sim_keys(pa, n_a, pb, n_b, d, r0, nr, self_mode, keys), dev,
            flags=0, row_align=ROW_ALIGN)
        na, nb = norms_a.cpu().numpy(), norms_b.cpu().numpy()
    return DictionaryMatch(partners.astype(np.int32), cosines, na, nb, self_mode)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Nearest decoder directions between two SAE dictionaries, or within one.")
    ap.add_argument("--a", required=True, help="checkpoint path")
    ap.add_argument("--b", default=None, help="checkpoint path (default: compare --a with itself)")
    ap.add_argument("--n-neighbors", "--n_neighbors", dest="n_neighbors", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=None, help="also count matched directions (and duplicate pairs) at this cosine")
    ap.add_argument("--out", default=None, help="store the tables as .npz")
    a = ap.parse_args(argv)
    m = compare_dictionaries(a.a, a.b, n_neighbors=a.n_neighbors)
    if a.out:
        m.to_npz(a.out)
    print(json.dumps({**({"out": a.out} if a.out else {}), **m.summary(a.threshold)}))


if __name__ == "__main__":
    main()
