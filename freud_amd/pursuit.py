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

import argparse
import dataclasses
import json
from typing import Optional, Sequence

import numpy as np

from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng
from .sparsity_frontier import DEFAULT_THRESHOLDS, SparsityFrontier, check_thresholds
from .sparsity_frontier import check_K as _frontier_check_K

MAX_K, MAX_TAU = 256, 8                     # include/freud_sae.h: SAE_PURSUIT_MAX_K, SAE_PURSUIT_MAX_TAU
_ARRAYS = ("thresholds", "sse", "sum_x", "sum_x_sq", "budget", "steps", "picks", "in_support")
_SCALARS = ("K", "n_frames")


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
class PursuitFrontier:
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

    @property
    def d(self) -> int:
        return int(self.sum_x.shape[0])

    @property
    def n(self) -> int:
        return int(self.picks.shape[0])

    # -- the curve: SparsityFrontier's arithmetic on the same fields
    sse_curve = SparsityFrontier.sse_curve
    total_variance = SparsityFrontier.total_variance
    fvu_curve = SparsityFrontier.fvu_curve
    fvu = SparsityFrontier.fvu
    marginal = SparsityFrontier.marginal
    budget_for_fvu = SparsityFrontier.budget_for_fvu
    _tau_index = SparsityFrontier._tau_index
    frame_budget_hist = SparsityFrontier.frame_budget_hist
    frame_budget_quantile = SparsityFrontier.frame_budget_quantile
    compare_pca = SparsityFrontier.compare_pca

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

    def compare(self, frontier: SparsityFrontier) -> np.ndarray:
        """float64 [min(K, frontier.K) + 1, 2]: (encoder FVU, pursuit FVU) at every budget, both over THIS object's denominator.  The
        frontier must cover the same frames of the same d."""
        if int(frontier.n_frames) != int(self.n_frames):
            raise ValueError(f"the frontier counted {frontier.n_frames} frames, the pursuit {self.n_frames}")
        if int(frontier.d) != self.d:
            raise ValueError(f"the frontier has d={frontier.d}, the pursuit d={self.d}")
        m = min(self.K, int(frontier.K)) + 1
        tv = self.total_variance()
        if not tv > 0:
            return np.full((m, 2), np.nan)
        return np.stack([np.asarray(frontier.sse, np.float64)[:m] / tv, self.sse[:m] / tv], axis=1)

    def amortisation_gap(self, frontier: SparsityFrontier) -> np.ndarray:
        """float64 [min(K, frontier.K) + 1]: encoder FVU - pursuit FVU at every budget."""
        c = self.compare(frontier)
        return c[:, 0] - c[:, 1]

    def summary(self) -> dict:
        fvu = self.fvu_curve()
        marks = sorted({0, 1, 2, 4, 8, 16, 32, 64, 128, 256, self.K} & set(range(self.K + 1)))
        agree = self.support_agreement()
        made = int(self.picks.sum())
        return {"n_frames": int(self.n_frames), "K": int(self.K), "d": self.d, "n": self.n,
                "fvu": {str(k): float(fvu[k]) for k in marks},
                "median_budget": {format(float(t), ".6g"): self.frame_budget_quantile(float(t), 0.5) for t in self.thresholds},
                "mean_picks": made / max(self.n_frames, 1), "never_picked": int(self.never_picked().size),
                "support_agreement": float(self.in_support.sum() / made) if made else None,
                "support_agreement_step0": None if np.isnan(agree[0]) else float(agree[0])}

    def save(self, path: str) -> None:
        np.savez(path, **{k: np.int64(getattr(self, k)) for k in _SCALARS}, **{k: getattr(self, k) for k in _ARRAYS})

    @classmethod
    def load(cls, path: str) -> "PursuitFrontier":
        z = np.load(path)
        return cls(**{k: int(z[k]) for k in _SCALARS}, **{k: z[k] for k in _ARRAYS})

    to_npz = save
    from_npz = load

    @classmethod
    def from_block(cls, block: np.ndarray, K: int, thresholds: np.ndarray, d: int, n: int) -> "PursuitFrontier":
        """The arrays of an sae_pursuit_files block (uint8 bytes, engine.pursuit_layout)."""
        from .engine import pursuit_layout, unpack_block
        n_tau = int(len(thresholds))
        a = unpack_block(block, pursuit_layout(n_tau, K, d, n))
        return cls(K=int(K), thresholds=np.asarray(thresholds, np.float32).copy(), n_frames=int(a["n_frames"][0]), sse=a["sse"],
                   sum_x=a["sum_x"], sum_x_sq=a["sum_x_sq"], budget=a["budget"].reshape(n_tau, K + 2), steps=a["steps"],
                   picks=a["picks"], in_support=a["in_support"])


@keep_rng
def pursuit_frontier(sae, data_path: str, layer_name: str, *, K: Optional[int] = None,
                     thresholds: Sequence[float] = DEFAULT_THRESHOLDS, files: Optional[int] = None, lengths=None,
                     batch_files: Optional[int] = None) -> PursuitFrontier:
    """The pursuit frontier of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a
    shard directory, in one pass.  K: pursuit steps per frame (default: a TopK SAE's k, min(n, 64) for L1; at most 256); thresholds:
    up to 8 shares of a frame's energy, each inside (0, 1); files: the first `files` files only; batch_files: files per engine call."""
    import torch
    from . import engine as E

    if is_raw(sae):
        raise ValueError("a pursuit frontier needs an SAE (raw activations have no dictionary to pursue)")
    tau = check_thresholds(thresholds)
    if K is not None:
        check_K(K, "topk", 0, 0)
    fp = FilePass(sae, data_path, layer_name, what="pursuit frontier", lengths=lengths, subset_size=files, batch_files=batch_files)
    K = check_K(K, fp.eng.variant, fp.eng.n, fp.eng.k)
    d, n = fp.eng.d, fp.eng.n
    with torch.cuda.device(fp.device):
        block = torch.zeros(E.pursuit_layout(tau.size, K, d, n)["bytes"], dtype=torch.uint8, device=fp.device)
        for x, _file0, _nb, lb in fp:
            fp.eng.pursuit_files(x, K, tau, block, lb)
        host = block.cpu().numpy()                                      # the one read-back
    out = PursuitFrontier.from_block(host, K, tau, d, n)
    fp.check_counted(out.n_frames)
    return out


@keep_rng
def pursuit_encode(sae, x, K: int):
    """The pursuit code of every row of x (a CUDA tensor [..., d]) in pick order: (indices int32 [..., K] -- -1 after the stop --,
    values float32 [..., K] -- the coefficients, +0.0 after the stop --, err float32 [..., K + 1] -- the squared error after s picks).
    Indices may repeat: the code of a latent is the sum of its values.  sae: a freud_amd.models SAE or a SaeEngine."""
    import torch
    from . import engine as E
    from .file_pass import resolve_sae

    K = check_K(int(K), "topk", 0, 0)
    model, eng = resolve_sae(sae)
    if model is None and eng is None:
        raise ValueError("pursuit_encode needs an SAE")
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
    xr = x.reshape(rows, d).contiguous()
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
    ap = argparse.ArgumentParser(description="FVU of an SAE's decoder under greedy (matching pursuit) coding at every per-frame latent "
                                             "budget, over a shard directory.")
    add_pass_arguments(ap)
    ap.add_argument("--K", type=int, default=None, help="pursuit steps per frame (default: a TopK SAE's k, min(n, 64) for L1)")
    ap.add_argument("--thresholds", default=",".join(str(t) for t in DEFAULT_THRESHOLDS), help="comma-separated shares of a frame's energy")
    ap.add_argument("--frontier", default=None, help="a sparsity frontier (.npz of freud_amd.sparsity_frontier) over the same files: adds "
                                                     "the amortisation gap to the summary")
    a = ap.parse_args(argv)
    tau = [float(t) for t in a.thresholds.split(",") if t.strip()]
    out = pursuit_frontier(a.sae, a.data_path, a.layer_name, K=a.K, thresholds=tau, lengths=np.load(a.lengths) if a.lengths else None,
                           batch_files=a.batch_files)
    if a.out:
        out.save(a.out)
    summary = {"out": a.out, **out.summary()}
    if a.frontier:
        cmp_ = out.compare(SparsityFrontier.from_npz(a.frontier))
        marks = [k for k in (1, 2, 4, 8, 16, 32, 64, 128, 256, cmp_.shape[0] - 1) if k < cmp_.shape[0]]
        summary["amortisation_gap"] = {str(k): float(cmp_[k, 0] - cmp_[k, 1]) for k in sorted(set(marks))}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
