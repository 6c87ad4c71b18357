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

from .engine import FRONTIER_MAX_K as MAX_K, FRONTIER_MAX_TAU as MAX_TAU
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, resolve_sae, run_pass_cli

DEFAULT_THRESHOLDS = (0.5, 0.2, 0.1, 0.05)
DEFAULT_L1_K = 64


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


def curve_marks(v, lowest: int = 1) -> dict:
    """{str(k): v[k]} at k = 0 (from `lowest` on), the powers of two and the last index of v: what the summaries print of a curve."""
    last = len(v) - 1
    return {str(k): float(v[k]) for k in sorted({0, 1, 2, 4, 8, 16, 32, 64, 128, 256, last}) if lowest <= k <= last}


class FrontierCurve:
    """What the three frontier dataclasses (SparsityFrontier, freud_amd.pursuit.PursuitFrontier, freud_amd.refit.RefitFrontier) share:
    the arithmetic on K, thresholds, n_frames, sse, sum_x, sum_x_sq and budget, the .npz form and the reading of an engine block.  It
    declares no field; _PASS names the engine's layout function and pass method, _NAME the object in error texts."""
    _PASS = _NAME = "frontier"

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

    def compare_pca(self, cov) -> np.ndarray:
        """float64 [K + 1, 2]: (fvu(k), cov.pca_fvu(k)) -- k latents per frame against the best rank-k linear code (freud_amd.input_pca's
        InputCovariance; ranks above d stay at its last entry)."""
        if int(cov.d) != self.d:
            raise ValueError(f"the covariance has d={cov.d}, the frontier d={self.d}")
        pca = np.asarray(cov.fvu_curve(), dtype=np.float64)
        return np.stack([self.fvu_curve(), pca[np.minimum(np.arange(self.K + 1), self.d)]], axis=1)

    def _same_frames(self, other, what: str) -> None:
        if int(other.n_frames) != int(self.n_frames):
            raise ValueError(f"the {what} counted {other.n_frames} frames, the {self._NAME} {self.n_frames}")
        if int(other.d) != self.d:
            raise ValueError(f"the {what} has d={other.d}, the {self._NAME} d={self.d}")

    def compare(self, frontier: "SparsityFrontier") -> np.ndarray:
        """float64 [min(K, frontier.K) + 1, 2]: (encoder FVU, this curve's FVU) at every budget, both over THIS object's denominator.
        The frontier must cover the same frames of the same d."""
        self._same_frames(frontier, "frontier")
        m = min(self.K, int(frontier.K)) + 1
        tv = self.total_variance()
        if not tv > 0:
            return np.full((m, 2), np.nan)
        return np.stack([np.asarray(frontier.sse, np.float64)[:m] / tv, self.sse[:m] / tv], axis=1)

    def _fvu_marks(self) -> dict:
        return curve_marks(self.fvu_curve(), 0)

    def _median_budgets(self) -> dict:
        return {format(float(t), ".6g"): self.frame_budget_quantile(float(t), 0.5) for t in self.thresholds}

    # -- the .npz form, by the dataclass's own fields: the int fields as int64, then the float fields as float64, then the arrays
    def save(self, path: str) -> None:
        kinds = _field_kinds(self)
        np.savez(path, **{k: np.int64(getattr(self, k)) for k, t in kinds.items() if t is int},
                 **{k: np.float64(getattr(self, k)) for k, t in kinds.items() if t is float},
                 **{k: getattr(self, k) for k, t in kinds.items() if t is None})

    @classmethod
    def load(cls, path: str):
        z = np.load(path)
        return cls(**{k: z[k] if t is None else t(z[k]) for k, t in _field_kinds(cls).items()})

    to_npz = save
    from_npz = load

    # -- an engine block (uint8 bytes) by its layout: a scalar field from its one element, budget as [n_tau, K + 2]
    @classmethod
    def _layout(cls, n_tau: int, K: int, d: int, n: int) -> dict:
        from . import engine as E
        return getattr(E, cls._PASS + "_layout")(n_tau, K, d, n)

    @classmethod
    def _from_layout(cls, block: np.ndarray, layout: dict, K: int, thresholds):
        from .engine import unpack_block
        a = unpack_block(block, layout)
        vals = {k: a[k] if t is None else t(a[k][0]) for k, t in _field_kinds(cls).items() if k in a}
        vals["budget"] = a["budget"].reshape(len(thresholds), K + 2)
        return cls(K=int(K), thresholds=np.asarray(thresholds, np.float32).copy(), **vals)


def _field_kinds(cls) -> dict:
    """name -> int, float or None (an array) for every field of a frontier dataclass, in declaration order."""
    scalar = {"int": int, int: int, "float": float, float: float}
    return {f.name: scalar.get(f.type) for f in dataclasses.fields(cls)}


@dataclasses.dataclass
class SparsityFrontier(FrontierCurve):
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

    def cut_fraction(self) -> float:
        """The share of the counted frames that have active latents beyond slot K."""
        return self.rows_cut / self.n_frames if self.n_frames else 0.0

    def summary(self) -> dict:
        return {"n_frames": int(self.n_frames), "K": int(self.K), "d": self.d, "rows_cut": int(self.rows_cut),
                "active_cut": int(self.active_cut), "cut_fraction": self.cut_fraction(), "fvu": self._fvu_marks(),
                "median_budget": self._median_budgets()}

    @classmethod
    def _layout(cls, n_tau: int, K: int, d: int, n: int = 0) -> dict:
        from .engine import frontier_layout
        return frontier_layout(n_tau, K, d)

    @classmethod
    def from_block(cls, block: np.ndarray, K: int, thresholds: np.ndarray, d: int) -> "SparsityFrontier":
        """The arrays of an sae_frontier_files block (uint8 bytes, engine.frontier_layout)."""
        return cls._from_layout(block, cls._layout(len(thresholds), K, d), K, thresholds)


def _run_frontier_pass(cls, check_K, max_k: int, sae, data_path: str, layer_name: str, *, what: str, lacks: str, K, thresholds, lengths,
                       subset_size, batch_files):
    """The driver of sparsity_frontier(), pursuit.pursuit_frontier() and refit.refit_frontier(): one pass of SaeEngine.<cls._PASS>_files
    over the files into one zeroed block, read back once as a cls."""
    import torch

    if is_raw(sae):
        raise ValueError(f"a {what} needs an SAE (raw activations have no {lacks})")
    tau = check_thresholds(thresholds)
    if K is not None and not 1 <= int(K) <= max_k:
        raise ValueError(f"K={K} outside [1, {max_k}]")
    if all(hasattr(sae, a) for a in ("variant", "n", "k")):             # an engine: its limits are known before any loading
        check_K(K, sae.variant, sae.n, sae.k)
    fp = FilePass(sae, data_path, layer_name, what=what, lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    K = check_K(K, fp.eng.variant, fp.eng.n, fp.eng.k)
    layout = cls._layout(tau.size, K, fp.eng.d, fp.eng.n)
    run = getattr(fp.eng, cls._PASS + "_files")
    with torch.cuda.device(fp.device):
        block = torch.zeros(layout["bytes"], dtype=torch.uint8, device=fp.device)
        for x, _file0, _nb, lb in fp:
            run(x, K, tau, block, lb)
        host = block.cpu().numpy()                                      # the one read-back
    out = cls._from_layout(host, layout, K, tau)
    fp.check_counted(out.n_frames)
    return out


def encode_rows(sae, x, who: str):
    """The front half of pursuit.pursuit_encode() and refit.refit_encode(): -> (the engine of sae, x as contiguous rows [rows, d], the
    leading shape of x)."""
    model, eng = resolve_sae(sae)
    if model is None and eng is None:
        raise ValueError(f"{who} needs an SAE")
    if not (hasattr(x, "is_cuda") and x.is_cuda and x.dim() >= 1):
        raise ValueError("x must be a CUDA tensor [..., d]")
    lead, d = tuple(x.shape[:-1]), int(x.shape[-1])
    rows = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if rows < 1:
        raise ValueError("x holds no rows")
    if eng is None:
        eng = model._ensure(-(-rows // 256) * 256)
    if eng.d != d:
        raise ValueError(f"the SAE expects d_model={eng.d}, x has d={d}")
    return eng, x.reshape(rows, d).contiguous(), lead


def parse_curve_cli(argv, description: str, k_help: str, npz_options=()):
    """The command line of the three frontier tools: the pass arguments, --K, --thresholds and the tool's own .npz options (flag,
    help).  -> (the parsed arguments, the thresholds as floats)."""
    ap = argparse.ArgumentParser(description=description)
    add_pass_arguments(ap)
    ap.add_argument("--K", type=int, default=None, help=k_help)
    ap.add_argument("--thresholds", default=",".join(str(t) for t in DEFAULT_THRESHOLDS), help="comma-separated shares of a frame's energy")
    for flag, text in npz_options:
        ap.add_argument(flag, default=None, help=text)
    a = ap.parse_args(argv)
    return a, [float(t) for t in a.thresholds.split(",") if t.strip()]


@keep_rng
def sparsity_frontier(sae, data_path: str, layer_name: str, *, K: Optional[int] = None,
                      thresholds: Sequence[float] = DEFAULT_THRESHOLDS, lengths=None, subset_size: Optional[int] = None,
                      batch_files: Optional[int] = None) -> SparsityFrontier:
    """The sparsity frontier of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a
    shard directory, in one pass.  K: slots per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 256); thresholds: up to 8
    shares of a frame's energy, each inside (0, 1); batch_files: files per engine call."""
    return _run_frontier_pass(SparsityFrontier, check_K, MAX_K, sae, data_path, layer_name, what="sparsity frontier",
                              lacks="latents to budget", K=K, thresholds=thresholds, lengths=lengths, subset_size=subset_size,
                              batch_files=batch_files)


def main(argv=None) -> None:
    a, tau = parse_curve_cli(argv, "FVU of an SAE at every per-frame latent budget, and the frames' budgets, over a shard directory.",
                             "slots per frame (default: a TopK SAE's k, min(n, 64) for L1)")
    run_pass_cli(a, lambda lengths: sparsity_frontier(a.sae, a.data_path, a.layer_name, K=a.K, thresholds=tau, lengths=lengths,
                                                      batch_files=a.batch_files))


if __name__ == "__main__":
    main()
