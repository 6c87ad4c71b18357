"""Refit frontier: the FVU a dictionary reaches at every per-frame latent budget when each frame keeps the SUPPORT its encoder chose
and the COEFFICIENTS are the least-squares ones on every prefix of that support, in one pass over the Whisper-activation shards.
It is the fourth curve beside

    freud_amd.input_pca           InputCovariance.fvu_curve()      the best rank-r LINEAR code
    freud_amd.sparsity_frontier   SparsityFrontier.fvu_curve()     the dictionary read through its OWN ENCODER
    freud_amd.pursuit             PursuitFrontier.fvu_curve()      the dictionary's DECODER alone, coded greedily

and splits the amortisation gap (encoder - pursuit) into its two defects: decompose(frontier, pursuit) returns per budget

    coefficient_gap = encoder - refit     what shrinkage and cross-talk cost: the encoder's latents with better coefficients
    support_gap     = refit - pursuit     what the encoder's CHOICE of latents costs against a greedy choice

Semantics (include/freud_sae.h, sae_refit_files).  Per counted frame, with the K slots (v_s, i_s) of freud_amd.collect_features and
w_j the bf16 decoder direction the frontier uses: G = W_s W_s^T (bf16 MFMA, fp32 sums), c = W_s r_0, r_0 = float(x) - b, and a
progressive Cholesky factorisation of G gives e_s, the squared error of the least-squares fit on the first s slots, for every s
at once.  A slot whose pivot falls to 2^-10 of its own norm is DEPENDENT (a repeated or numerically redundant direction) and is
skipped.  The coefficients a_s at the full budget are signed; negative ones are counted per latent.  e_final is the error at budget
K computed directly from the residual.  Two runs give bitwise identical arrays; the integer fields do not depend on batch_files.

    python -m freud_amd.refit --sae CKPT --data_path DIR --layer_name L [--K 64] [--thresholds 0.5,0.1] [--frontier f.npz]
                              [--pursuit p.npz] --out r.npz
"""
from __future__ import annotations

import dataclasses
import json
from typing import Optional, Sequence

import numpy as np

from .engine import REFIT_MAX_K as MAX_K, REFIT_MAX_TAU as MAX_TAU, REFIT_RATIO_BINS as RATIO_BINS
from .file_pass import keep_rng
from .sparsity_frontier import DEFAULT_THRESHOLDS, FrontierCurve, SparsityFrontier, _run_frontier_pass, curve_marks, encode_rows, parse_curve_cli
from .sparsity_frontier import check_K as _frontier_check_K


def check_K(K, variant: str, n: int, k: int, given: bool = False) -> int:
    """K, or the default (the sparsity frontier's, capped at MAX_K), checked against the limits: [1, MAX_K], and for the encoder's
    own support K <= k (TopK) or K <= n (L1)."""
    if K is None:
        return min(MAX_K, _frontier_check_K(None, variant, n, k))
    K = int(K)
    top = MAX_K if given else min(MAX_K, int(k) if variant == "topk" else int(n))
    if K < 1 or K > top:
        raise ValueError(f"K={K} outside [1, {top}]")
    return K


def ratio_edges() -> np.ndarray:
    """float64 [33]: the lower edges of the 32 regular shrinkage bins and the upper edge of the last, 2^-4 .. 2^4 (four per octave:
    2^e (1 + q / 4)).  Bins of shrinkage_hist(): 0 negative, 1 zero, 2 below 2^-4, 3 + i regular, 35 at or above 2^4."""
    i = np.arange(33)
    return 2.0 ** (-4 + i // 4) * (1 + (i % 4) / 4)


@dataclasses.dataclass
class RefitFrontier(FrontierCurve):
    """The refit frontier of an SAE over a dataset (see the module docstring)."""
    K: int
    thresholds: np.ndarray      # float32 [n_tau]
    n_frames: int
    sse: np.ndarray             # float64 [K + 1]
    sse_final: float            # the summed e_final
    sum_x: np.ndarray           # float64 [d]
    sum_x_sq: np.ndarray        # float64 [d]
    budget: np.ndarray          # int64 [n_tau, K + 2]
    kept: np.ndarray            # int64 [K + 1]: frames by the number of kept slots
    slots: np.ndarray           # int64 [n]: frames that hold latent j in an active slot
    neg: np.ndarray             # int64 [n]: kept slots of latent j with a negative refit coefficient
    dep: np.ndarray             # int64 [n]: active slots of latent j that were dependent
    ratio: np.ndarray           # int64 [36]: histogram of a_s / v_s over the kept slots (the encoder's support only)
    bad_index: int = 0          # out-of-range indices of a given support

    _PASS = _NAME = "refit"

    @property
    def n(self) -> int:
        return int(self.slots.shape[0])

    def final_fvu(self) -> float:
        """The FVU at budget K from the directly computed residuals (beside fvu(K), which comes from e_0 - sum y^2)."""
        tv = self.total_variance()
        return float(self.sse_final / tv) if tv > 0 else float("nan")

    def kept_hist(self) -> np.ndarray:
        """int64 [K + 1]: frames by the number of slots the refit kept (active and not dependent)."""
        return self.kept

    def dependent_fraction(self):
        """(float64 [n], float): per latent and overall, the share of its active slots that were dependent (nan: never active).
        The denominator counts a latent once per frame; a given support that repeats an index can exceed 1."""
        with np.errstate(invalid="ignore", divide="ignore"):
            per = np.where(self.slots > 0, self.dep / self.slots, np.nan)
        tot = int(self.slots.sum())
        return per, (float(self.dep.sum() / tot) if tot else float("nan"))

    def negative_fraction(self):
        """(float64 [n], float): per latent and overall, the share of its active slots whose refit coefficient is below zero."""
        with np.errstate(invalid="ignore", divide="ignore"):
            per = np.where(self.slots > 0, self.neg / self.slots, np.nan)
        tot = int(self.slots.sum())
        return per, (float(self.neg.sum() / tot) if tot else float("nan"))

    def shrinkage_hist(self) -> np.ndarray:
        """int64 [36]: kept slots by a_s / v_s (ratio_edges() names the bins); all zero for a given support."""
        return self.ratio

    def shrinkage_quantile(self, q: float) -> float:
        """The lower edge of the bin that holds the q-quantile of a_s / v_s: -inf for the negative bin, 0 for the zero and the
        underflow bins, 2^4 for the overflow bin; nan without any kept slot."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q={q} outside [0, 1]")
        total = int(self.ratio.sum())
        if total == 0:
            return float("nan")
        b = int(np.searchsorted(np.cumsum(self.ratio), q * total, side="left"))
        b = min(b, RATIO_BINS - 1)
        if b == 0:
            return float("-inf")
        if b <= 2:
            return 0.0
        return float(ratio_edges()[b - 3])

    def decompose(self, frontier: SparsityFrontier, pursuit) -> dict:
        """The amortisation gap split at every budget s <= min of the three K: {"encoder", "refit", "pursuit": the three FVU curves
        over this object's denominator, "coefficient_gap": encoder - refit, "support_gap": refit - pursuit}."""
        self._same_frames(frontier, "frontier")
        self._same_frames(pursuit, "pursuit")
        m = min(self.K, int(frontier.K), int(pursuit.K)) + 1
        tv = self.total_variance()
        if not tv > 0:
            nan = np.full(m, np.nan)
            return {"encoder": nan, "refit": nan.copy(), "pursuit": nan.copy(), "coefficient_gap": nan.copy(), "support_gap": nan.copy()}
        enc = np.asarray(frontier.sse, np.float64)[:m] / tv
        ref = self.sse[:m] / tv
        pur = np.asarray(pursuit.sse, np.float64)[:m] / tv
        return {"encoder": enc, "refit": ref, "pursuit": pur, "coefficient_gap": enc - ref, "support_gap": ref - pur}

    def summary(self) -> dict:
        kept_total = int((self.kept * np.arange(self.K + 1)).sum())
        return {"n_frames": int(self.n_frames), "K": int(self.K), "d": self.d, "n": self.n, "fvu": self._fvu_marks(),
                "final_fvu": self.final_fvu(), "median_budget": self._median_budgets(),
                "mean_kept": kept_total / max(self.n_frames, 1), "dependent_fraction": self.dependent_fraction()[1],
                "negative_fraction": self.negative_fraction()[1], "median_shrinkage": self.shrinkage_quantile(0.5),
                "bad_index": int(self.bad_index)}

    @classmethod
    def from_block(cls, block: np.ndarray, K: int, thresholds: np.ndarray, d: int, n: int) -> "RefitFrontier":
        """The arrays of an sae_refit_files block (uint8 bytes, engine.refit_layout)."""
        return cls._from_layout(block, cls._layout(len(thresholds), K, d, n), K, thresholds)


@keep_rng
def refit_frontier(sae, data_path: str, layer_name: str, *, K: Optional[int] = None,
                   thresholds: Sequence[float] = DEFAULT_THRESHOLDS, files: Optional[int] = None, lengths=None,
                   batch_files: Optional[int] = None) -> RefitFrontier:
    """The refit frontier of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a
    shard directory, in one pass.  K: slots per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 128); thresholds: up to 8
    shares of a frame's energy, each inside (0, 1); files: the first `files` files only; batch_files: files per engine call."""
    return _run_frontier_pass(RefitFrontier, check_K, MAX_K, sae, data_path, layer_name, what="refit frontier",
                              lacks="support to refit", K=K, thresholds=thresholds, lengths=lengths, subset_size=files,
                              batch_files=batch_files)


@keep_rng
def refit_encode(sae, x, K: Optional[int] = None, support=None):
    """The least-squares code of every row of x (a CUDA tensor [..., d]) on its support: (indices int32 [..., K] -- -1 on an empty
    slot --, coef float32 [..., K] -- the signed coefficients, +0.0 on a slot that is empty or dependent --, err float32 [..., K + 1]
    -- the squared error of the fit on the first s slots).  support: None -- the K largest latents of the SAE's own encoder, in the
    order of freud_amd.collect_features -- or an integer CUDA tensor [..., K] of latent indices (-1: empty), e.g. the picks of
    freud_amd.pursuit.pursuit_encode: pursuit with a final orthogonal projection.  sae: a freud_amd.models SAE or a SaeEngine."""
    import torch
    from . import engine as E

    eng, xr, lead = encode_rows(sae, x, "refit_encode")
    rows, d = xr.shape
    sup = None
    if support is not None:
        if tuple(support.shape[:-1]) != lead:
            raise ValueError(f"support {tuple(support.shape)} does not match x {tuple(x.shape)}")
        K = check_K(int(support.shape[-1]) if K is None else K, eng.variant, eng.n, eng.k, given=True)
        if int(support.shape[-1]) != K:
            raise ValueError(f"support has {int(support.shape[-1])} slots per row, K={K}")
        sup = support.to(device=x.device, dtype=torch.int32).reshape(rows, K).contiguous()
    else:
        K = check_K(K, eng.variant, eng.n, eng.k)
    with torch.cuda.device(x.device):
        coef = torch.empty(rows, K, dtype=torch.float32, device=x.device)
        err = torch.empty(rows, K + 1, dtype=torch.float32, device=x.device)
        idx = sup if sup is not None else torch.empty(rows, K, dtype=torch.int32, device=x.device)
        block = torch.zeros(E.refit_layout(0, K, d, eng.n)["bytes"], dtype=torch.uint8, device=x.device)
        step = int(eng.max_rows)
        for r0 in range(0, rows, step):
            r1 = min(rows, r0 + step)
            xb = xr[r0:r1].unsqueeze(0)
            eng.refit_files(xb, K, [], block, None, support=None if sup is None else sup[r0:r1], trace={"coef": coef[r0:r1], "err": err[r0:r1]})
            if sup is None:
                # the encoder's own slots, as the refit read them: the same collect on the same rows
                val = torch.empty(r1 - r0, K, dtype=torch.float32, device=x.device)
                st = torch.zeros(8, dtype=torch.int64, device=x.device)
                eng.collect_files(xb, K, val, idx[r0:r1], st)
                idx[r0:r1] = torch.where(val != 0, idx[r0:r1], torch.full_like(idx[r0:r1], -1))
    return idx.reshape(*lead, K), coef.reshape(*lead, K), err.reshape(*lead, K + 1)


def main(argv=None) -> None:
    a, tau = parse_curve_cli(argv, "FVU of an SAE at every per-frame latent budget with least-squares coefficients on the encoder's own "
                                   "support, over a shard directory.",
                             "slots per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 128)",
                             [("--frontier", "a sparsity frontier (.npz of freud_amd.sparsity_frontier) over the same files: adds the "
                                             "coefficient gap to the summary"),
                              ("--pursuit", "a pursuit frontier (.npz of freud_amd.pursuit) over the same files: with --frontier, adds the "
                                            "support gap")])
    out = refit_frontier(a.sae, a.data_path, a.layer_name, K=a.K, thresholds=tau, lengths=np.load(a.lengths) if a.lengths else None,
                         batch_files=a.batch_files)
    if a.out:
        out.save(a.out)
    summary = {"out": a.out, **out.summary()}
    if a.frontier and a.pursuit:
        from .pursuit import PursuitFrontier
        dec = out.decompose(SparsityFrontier.from_npz(a.frontier), PursuitFrontier.load(a.pursuit))
        summary["coefficient_gap"] = curve_marks(dec["coefficient_gap"])
        summary["support_gap"] = curve_marks(dec["support_gap"])
    elif a.frontier:
        cmp_ = out.compare(SparsityFrontier.from_npz(a.frontier))
        summary["coefficient_gap"] = curve_marks(cmp_[:, 0] - cmp_[:, 1])
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
