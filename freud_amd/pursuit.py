"""Pursuit frontier: the FVU the DECODER of a dictionary reaches at every per-frame latent budget when each frame is coded greedily
against the decoder directions, without the trained encoder -- non-negative matching pursuit ("inference-time optimisation"), in one
pass over the Whisper-activation shards.  It is the third curve of the evaluation triangle:

    freud_amd.input_pca           InputCovariance.fvu_curve()      the best rank-r LINEAR code
    freud_amd.sparsity_frontier   SparsityFrontier.fvu_curve()     the dictionary read through its OWN ENCODER
    freud_amd.pursuit             PursuitFrontier.fvu_curve()      the dictionary's DECODER alone, coded greedily

compare(frontier) puts the last two side by side over the same denominator; their difference is the amortisation gap: what L1
shrinkage, a TopK encoder whose pre-activations rank the wrong latents, or a dictionary read below its k cost.  usage(),
never_picked() and support_agreement() say which latents a greedy code needs and how often the encoder fires them.

Semantics (include/freud_sae.h, sae_pursuit_files).  Per counted frame, with w_j the bf16 decoder direction the frontier uses:

    r_0 = float(x) - b                      (b = b_dec for TopK, 0 for L1)
    step s: j* = argmax_j <bf16(r_s), w_j> / |w_j|   (the bf16 MFMA product: it only chooses; ties to the lower j)
            stop if the score is <= 0;  a = <r_s, w_j*> / |w_j*|^2 in fp32;  stop if not a > 0
            r_{s+1} = r_s - a w_j*
    e_s = |r_s|^2,  s = 0 .. K;  a stopped frame keeps its e

A latent may be picked again later (the code accumulates), so e_s is the error with AT MOST s distinct latents.  Two runs give
bitwise identical arrays; the integer fields and the trace do not depend on batch_files.

    python -m freud_amd.pursuit --sae CKPT --data_path DIR --layer_name L [--K 64] [--thresholds 0.5,0.1] [--frontier f.npz] --out p.npz
"""
from __future__ import annotations

import dataclasses
import json
from typing import Optional, Sequence

import numpy as np

from .engine import PURSUIT_MAX_K as MAX_K, PURSUIT_MAX_TAU as MAX_TAU
from .file_pass import keep_rng
from .sparsity_frontier import DEFAULT_THRESHOLDS, FrontierCurve, SparsityFrontier, _run_frontier_pass, curve_marks, encode_rows, parse_curve_cli
from .sparsity_frontier import check_K as _frontier_check_K


def check_K(K, variant: str, n: int, k: int) -> int:
    """K, or the default (the sparsity frontier's: a TopK SAE's k, min(n, 64) for L1, capped at MAX_K), inside [1, MAX_K] -- the
    pursuit is not bound by a TopK model's k."""
    if K is None:
        return _frontier_check_K(None, variant, n, k)
    K = int(K)
    if K < 1 or K > MAX_K:
        raise ValueError(f"K={K} outside [1, {MAX_K}]")
    return K


@dataclasses.dataclass
class PursuitFrontier(FrontierCurve):
    """The pursuit frontier of an SAE's decoder over a dataset (see the module docstring)."""
    K: int
    thresholds: np.ndarray      # float32 [n_tau]
    n_frames: int
    sse: np.ndarray             # float64 [K + 1]
    sum_x: np.ndarray           # float64 [d]
    sum_x_sq: np.ndarray        # float64 [d]
    budget: np.ndarray          # int64 [n_tau, K + 2]
    steps: np.ndarray           # int64 [K + 1]: frames by the number of picks they made before they stopped
    picks: np.ndarray           # int64 [n]: how often latent j was picked
    in_support: np.ndarray      # int64 [K]: picks of step s inside the encoder's own active set of the frame

    _PASS = _NAME = "pursuit"

    @property
    def n(self) -> int:
        return int(self.picks.shape[0])

    @property
    def steps_hist(self) -> np.ndarray:
        """int64 [K + 1]: frames by the number of picks they made (K: never stopped)."""
        return self.steps

    def picks_at_step(self) -> np.ndarray:
        """int64 [K]: the picks made at step s -- the frames that made more than s picks."""
        total = int(self.steps.sum())
        return (total - np.cumsum(self.steps)[:-1]).astype(np.int64)

    def usage(self) -> np.ndarray:
        """float64 [n]: picks of latent j per counted frame."""
        return self.picks / max(self.n_frames, 1)

    def support_agreement(self) -> np.ndarray:
        """float64 [K]: the share of step s's picks that the encoder also fires on that frame (nan where no frame reached step s)."""
        made = self.picks_at_step().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(made > 0, self.in_support / made, np.nan)

    def never_picked(self) -> np.ndarray:
        """The latents no frame ever picked, ascending."""
        return np.nonzero(self.picks == 0)[0]

    def amortisation_gap(self, frontier: SparsityFrontier) -> np.ndarray:
        """float64 [min(K, frontier.K) + 1]: encoder FVU - pursuit FVU at every budget (compare(): the two side by side)."""
        c = self.compare(frontier)
        return c[:, 0] - c[:, 1]

    def summary(self) -> dict:
        agree = self.support_agreement()
        made = int(self.picks.sum())
        return {"n_frames": int(self.n_frames), "K": int(self.K), "d": self.d, "n": self.n, "fvu": self._fvu_marks(),
                "median_budget": self._median_budgets(),
                "mean_picks": made / max(self.n_frames, 1), "never_picked": int(self.never_picked().size),
                "support_agreement": float(self.in_support.sum() / made) if made else None,
                "support_agreement_step0": None if np.isnan(agree[0]) else float(agree[0])}

    @classmethod
    def from_block(cls, block: np.ndarray, K: int, thresholds: np.ndarray, d: int, n: int) -> "PursuitFrontier":
        """The arrays of an sae_pursuit_files block (uint8 bytes, engine.pursuit_layout)."""
        return cls._from_layout(block, cls._layout(len(thresholds), K, d, n), K, thresholds)


@keep_rng
def pursuit_frontier(sae, data_path: str, layer_name: str, *, K: Optional[int] = None,
                     thresholds: Sequence[float] = DEFAULT_THRESHOLDS, files: Optional[int] = None, lengths=None,
                     batch_files: Optional[int] = None) -> PursuitFrontier:
    """The pursuit frontier of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a
    shard directory, in one pass.  K: pursuit steps per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 256); thresholds:
    up to 8 shares of a frame's energy, each inside (0, 1); files: the first `files` files only; batch_files: files per engine call."""
    return _run_frontier_pass(PursuitFrontier, check_K, MAX_K, sae, data_path, layer_name, what="pursuit frontier",
                              lacks="dictionary to pursue", K=K, thresholds=thresholds, lengths=lengths, subset_size=files,
                              batch_files=batch_files)


@keep_rng
def pursuit_encode(sae, x, K: int):
    """The pursuit code of every row of x (a CUDA tensor [..., d]) in pick order: (indices int32 [..., K] -- -1 after the stop --,
    values float32 [..., K] -- the coefficients, +0.0 after the stop --, err float32 [..., K + 1] -- the squared error after s picks).
    Indices may repeat: the code of a latent is the sum of its values.  sae: a freud_amd.models SAE or a SaeEngine."""
    import torch
    from . import engine as E

    K = check_K(int(K), "topk", 0, 0)
    eng, xr, lead = encode_rows(sae, x, "pursuit_encode")
    rows, d = xr.shape
    with torch.cuda.device(x.device):
        idx = torch.empty(rows, K, dtype=torch.int32, device=x.device)
        val = torch.empty(rows, K, dtype=torch.float32, device=x.device)
        err = torch.empty(rows, K + 1, dtype=torch.float32, device=x.device)
        block = torch.zeros(E.pursuit_layout(0, K, d, eng.n)["bytes"], dtype=torch.uint8, device=x.device)
        step = int(eng.max_rows)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            eng.pursuit_files(xr[r0:r1].unsqueeze(0), K, [], block, None, trace=(idx[r0:r1], val[r0:r1], err[r0:r1]))
    return idx.reshape(*lead, K), val.reshape(*lead, K), err.reshape(*lead, K + 1)


def main(argv=None) -> None:
    a, tau = parse_curve_cli(argv, "FVU of an SAE's decoder under greedy (matching pursuit) coding at every per-frame latent budget, over a "
                                   "shard directory.", "pursuit steps per frame (default: a TopK SAE's k, min(n, 64) for L1)",
                             [("--frontier", "a sparsity frontier (.npz of freud_amd.sparsity_frontier) over the same files: adds the "
                                             "amortisation gap to the summary")])
    out = pursuit_frontier(a.sae, a.data_path, a.layer_name, K=a.K, thresholds=tau, lengths=np.load(a.lengths) if a.lengths else None,
                           batch_files=a.batch_files)
    if a.out:
        out.save(a.out)
    summary = {"out": a.out, **out.summary()}
    if a.frontier:
        summary["amortisation_gap"] = curve_marks(out.amortisation_gap(SparsityFrontier.from_npz(a.frontier)))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
