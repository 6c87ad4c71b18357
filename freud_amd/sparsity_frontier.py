"""Sparsity frontier: the FVU of a dictionary at EVERY per-frame latent budget, and how many latents each frame needs, in one pass
over the Whisper-activation shards -- the SAE's curve to put beside the PCA curve of freud_amd.input_pca, what a cut of the feature
store to K' slots costs in reconstruction, and a TopK dictionary read below its k.

Semantics (include/freud_sae.h, sae_frontier_files).  Counted frames as in freud_amd.reconstruction.  For a counted frame the slots
(v_s, i_s), s < K, are exactly those freud_amd.collect_features stores for the row (stable descending sort of encode()'s latent), w_j
is the bf16 decoder direction the reconstruction report uses, and

    r_0 = float(x) - b        (b = b_dec for TopK, 0 for L1)
    r_{s+1} = r_s - v_s w_{i_s}                      (fp32 fmaf, in slot order)
    e_s = |r_s|^2,  s = 0 .. K

sse[s] = sum over the frames of e_s is the squared error of the dataset when every frame keeps its s largest latents; fvu_curve()
divides by the reconstruction report's total variance.  The frame's budget at a threshold tau is the smallest s with
e_s <= tau e_0 (K + 1: not within K); budget[t] is its histogram over the frames.  rows_cut / active_cut count what lies beyond
slot K, as CollectReport.rows_dropped / dropped do.  Two runs give bitwise identical arrays; the integer fields do not depend on
batch_files.

    python -m freud_amd.sparsity_frontier --sae CKPT --data_path DIR --layer_name L [--K 64] [--thresholds 0.5,0.1] --out f.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional, Sequence

import numpy as np

from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

MAX_K, MAX_TAU = 256, 8                     # include/freud_sae.h: SAE_FRONTIER_MAX_K, SAE_FRONTIER_MAX_TAU
DEFAULT_THRESHOLDS = (0.5, 0.2, 0.1, 0.05)
DEFAULT_L1_K = 64
_ARRAYS = ("thresholds", "sse", "sum_x", "sum_x_sq", "budget")
_SCALARS = ("K", "n_frames", "rows_cut", "active_cut")


def check_thresholds(thresholds) -> np.ndarray:
    """The thresholds as float32 [n_tau]: at most MAX_TAU, each finite and inside (0, 1) after the rounding to float32."""
    tau = np.asarray(list(thresholds), dtype=np.float64).reshape(-1)
    if tau.size > MAX_TAU:
        raise ValueError(f"{tau.size} thresholds: at most {MAX_TAU}")
    t32 = tau.astype(np.float32)
    if not (np.isfinite(t32) & (t32 > 0) & (t32 < 1)).all():
        raise ValueError(f"thresholds {tau.tolist()} must be finite and inside (0, 1)")
    return t32


def check_K(K, variant: str, n: int, k: int) -> int:
    """K, or the default (a TopK SAE's k, min(n, 64) for L1, both capped at MAX_K), checked against the limits."""
    top = min(MAX_K, int(k) if variant == "topk" else int(n))
    if K is None:
        return top if variant == "topk" else min(top, DEFAULT_L1_K)
    K = int(K)
    if K < 1 or K > top:
        raise ValueError(f"K={K} outside [1, {top}] (min of {'the model k' if variant == 'topk' else 'n_dict'} and {MAX_K})")
    return K


@dataclasses.dataclass
class SparsityFrontier:
    """The frontier of an SAE over a dataset (see the module docstring)."""
    K: int
    thresholds: np.ndarray      # float32 [n_tau]
    n_frames: int
    rows_cut: int
    active_cut: int
    sse: np.ndarray             # float64 [K + 1]
    sum_x: np.ndarray           # float64 [d]
    sum_x_sq: np.ndarray        # float64 [d]
    budget: np.ndarray          # int64 [n_tau, K + 2]

    @property
    def d(self) -> int:
        return int(self.sum_x.shape[0])

    def sse_curve(self) -> np.ndarray:
        """float64 [K + 1]: the summed squared error with a budget of s latents per frame."""
        return self.sse

    def total_variance(self) -> float:
        """ReconstructionReport.total_variance(): the summed squared deviation from the per-dimension mean."""
        return float((self.sum_x_sq - self.sum_x * self.sum_x / max(self.n_frames, 1)).sum())

    def fvu_curve(self) -> np.ndarray:
        tv = self.total_variance()
        return self.sse / tv if tv > 0 else np.full(self.K + 1, np.nan)

    def fvu(self, k: int) -> float:
        k = int(k)
        if not 0 <= k <= self.K:
            raise ValueError(f"k={k} outside [0, {self.K}]")
        return float(self.fvu_curve()[k])

    def marginal(self) -> np.ndarray:
        """float64 [K]: sse[s] - sse[s + 1], what slot s is worth."""
        return self.sse[:-1] - self.sse[1:]

    def budget_for_fvu(self, target: float) -> Optional[int]:
        """The smallest k with a dataset FVU <= target, or None if K latents per frame do not reach it."""
        hit = np.nonzero(self.fvu_curve() <= float(target))[0]
        return int(hit[0]) if hit.size else None

    def _tau_index(self, tau: float) -> int:
        hit = np.nonzero(self.thresholds == np.float32(tau))[0]
        if hit.size == 0:
            raise ValueError(f"tau={tau} is not one of the thresholds {self.thresholds.tolist()}")
        return int(hit[0])

    def frame_budget_hist(self, tau: float) -> np.ndarray:
        """int64 [K + 2]: frames per budget at tau; the last bin (K + 1) holds the frames that K latents do not bring to tau."""
        return self.budget[self._tau_index(tau)]

    def frame_budget_quantile(self, tau: float, q: float) -> int:
        """The smallest budget that at least a share q of the frames stay within; K + 1 means "not within K"."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q={q} outside [0, 1]")
        h = self.frame_budget_hist(tau)
        total = int(h.sum())
        if total == 0:
            return 0
        return int(np.searchsorted(np.cumsum(h), q * total, side="left"))

    def cut_fraction(self) -> float:
        """The share of the counted frames that have active latents beyond slot K."""
        return self.rows_cut / self.n_frames if self.n_frames else 0.0

    def compare_pca(self, cov) -> np.ndarray:
        """float64 [K + 1, 2]: (fvu(k), cov.pca_fvu(k)) -- k latents per frame against the best rank-k linear code (freud_amd.input_pca's
        InputCovariance; ranks above d stay at its last entry)."""
        if int(cov.d) != self.d:
            raise ValueError(f"the covariance has d={cov.d}, the frontier d={self.d}")
        pca = np.asarray(cov.fvu_curve(), dtype=np.float64)
        return np.stack([self.fvu_curve(), pca[np.minimum(np.arange(self.K + 1), self.d)]], axis=1)

    def summary(self) -> dict:
        fvu = self.fvu_curve()
        marks = sorted({0, 1, 2, 4, 8, 16, 32, 64, 128, 256, self.K} & set(range(self.K + 1)))
        return {"n_frames": int(self.n_frames), "K": int(self.K), "d": self.d, "rows_cut": int(self.rows_cut),
                "active_cut": int(self.active_cut), "cut_fraction": self.cut_fraction(),
                "fvu": {str(k): float(fvu[k]) for k in marks},
                "median_budget": {format(float(t), ".6g"): self.frame_budget_quantile(float(t), 0.5) for t in self.thresholds}}

    def to_npz(self, path: str) -> None:
        np.savez(path, **{k: np.int64(getattr(self, k)) for k in _SCALARS}, **{k: getattr(self, k) for k in _ARRAYS})

    @classmethod
    def from_npz(cls, path: str) -> "SparsityFrontier":
        z = np.load(path)
        return cls(**{k: int(z[k]) for k in _SCALARS}, **{k: z[k] for k in _ARRAYS})

    @classmethod
    def from_block(cls, block: np.ndarray, K: int, thresholds: np.ndarray, d: int) -> "SparsityFrontier":
        """The arrays of an sae_frontier_files block (uint8 bytes, engine.frontier_layout)."""
        from .engine import frontier_layout, unpack_block
        n_tau = int(len(thresholds))
        a = unpack_block(block, frontier_layout(n_tau, K, d))
        return cls(K=int(K), thresholds=np.asarray(thresholds, np.float32).copy(), n_frames=int(a["n_frames"][0]),
                   rows_cut=int(a["rows_cut"][0]), active_cut=int(a["active_cut"][0]), sse=a["sse"], sum_x=a["sum_x"],
                   sum_x_sq=a["sum_x_sq"], budget=a["budget"].reshape(n_tau, K + 2))


@keep_rng
def sparsity_frontier(sae, data_path: str, layer_name: str, *, K: Optional[int] = None,
                      thresholds: Sequence[float] = DEFAULT_THRESHOLDS, lengths=None, subset_size: Optional[int] = None,
                      batch_files: Optional[int] = None) -> SparsityFrontier:
    """The sparsity frontier of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a
    shard directory, in one pass.  K: slots per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 256); thresholds: up to 8
    shares of a frame's energy, each inside (0, 1); batch_files: files per engine call."""
    import torch
    from . import engine as E

    if is_raw(sae):
        raise ValueError("a sparsity frontier needs an SAE (raw activations have no latents to budget)")
    tau = check_thresholds(thresholds)
    if K is not None and not 1 <= int(K) <= MAX_K:
        raise ValueError(f"K={K} outside [1, {MAX_K}]")
    if all(hasattr(sae, a) for a in ("variant", "n", "k")):             # an engine: its limits are known before any loading
        check_K(K, sae.variant, sae.n, sae.k)
    fp = FilePass(sae, data_path, layer_name, what="sparsity frontier", lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    K = check_K(K, fp.eng.variant, fp.eng.n, fp.eng.k)
    d = fp.eng.d
    with torch.cuda.device(fp.device):
        block = torch.zeros(E.frontier_layout(tau.size, K, d)["bytes"], dtype=torch.uint8, device=fp.device)
        for x, _file0, _nb, lb in fp:
            fp.eng.frontier_files(x, K, tau, block, lb)
        host = block.cpu().numpy()                                      # the one read-back
    out = SparsityFrontier.from_block(host, K, tau, d)
    fp.check_counted(out.n_frames)
    return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="FVU of an SAE at every per-frame latent budget, and the frames' budgets, over a shard directory.")
    add_pass_arguments(ap)
    ap.add_argument("--K", type=int, default=None, help="slots per frame (default: a TopK SAE's k, min(n, 64) for L1)")
    ap.add_argument("--thresholds", default=",".join(str(t) for t in DEFAULT_THRESHOLDS), help="comma-separated shares of a frame's energy")
    a = ap.parse_args(argv)
    tau = [float(t) for t in a.thresholds.split(",") if t.strip()]
    run_pass_cli(a, lambda lengths: sparsity_frontier(a.sae, a.data_path, a.layer_name, K=a.K, thresholds=tau, lengths=lengths,
                                                      batch_files=a.batch_files))


if __name__ == "__main__":
    main()
