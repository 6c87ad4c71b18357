"""Feature statistics: how sparse a trained dictionary is on real data, and which latents are dead, rare or dense -- in one pass over
the Whisper-activation shards, without collecting the SAE activations (the reference's route: collect_activations.py with
sae_model, a dense fp32 [1500, n] row per file, then a reduction in torch).

Semantics (include/freud_sae.h, sae_stats_files).  Over the files of a shard directory, the first min(L[f], T) frames of file f
count when `lengths` is given (file_pass.check_lengths rules), all T frames otherwise.  Per frame and latent j, a_j is exactly
the value freud_amd.models encode() returns: the bf16 L1 latent of the training kernels, or for TopK the scatter of top_acts at
top_indices (0 elsewhere).  a_j is active iff a_j > 0 (a bf16 -0.0 is not).  Per latent: fire_count (frames where active),
act_sum / act_sq_sum (sums of a_j and a_j^2, float64), act_max (float32, 0 if never active); per frame the number of active
latents, as l0_hist[i] = frames with exactly i active.  l0_hist.sum() == n_frames and sum_i i l0_hist[i] == fire_count.sum().
Two runs over the same data give bitwise identical arrays.

    python -m freud_amd.feature_stats --sae CKPT --data_path DIR --layer_name L [--lengths f.npy] [--batch_files B] --out stats.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional

import numpy as np
import torch

from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

_FIELDS = ("fire_count", "act_sum", "act_sq_sum", "act_max", "l0_hist")


@dataclasses.dataclass
class FeatureStats:
    """Dataset statistics of an SAE's latents (see the module docstring)."""
    n_frames: int
    fire_count: np.ndarray      # int64 [n]
    act_sum: np.ndarray         # float64 [n]
    act_sq_sum: np.ndarray      # float64 [n]
    act_max: np.ndarray         # float32 [n]
    l0_hist: np.ndarray         # int64 [n + 1]

    @property
    def n_latents(self) -> int:
        return int(self.fire_count.shape[0])

    def frequency(self) -> np.ndarray:
        """Fraction of counted frames on which each latent is active (float64 [n])."""
        return self.fire_count / max(self.n_frames, 1)

    def mean_when_active(self) -> np.ndarray:
        """Mean of a_j over the frames where latent j is active; NaN where it never is."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.fire_count > 0, self.act_sum / self.fire_count, np.nan)

    def dead(self) -> np.ndarray:
        """Latents never active on the data (bool [n])."""
        return self.fire_count == 0

    def l0_mean(self) -> float:
        """Mean number of active latents per frame."""
        if self.n_frames == 0:
            return float("nan")
        return float((np.arange(self.l0_hist.shape[0], dtype=np.float64) * self.l0_hist).sum() / self.n_frames)

    def density_histogram(self, bins=50):
        """The feature-density histogram: np.histogram of log10(frequency) over the latents that are active at least once ->
        (counts, edges, n_dead); dead latents (log10 0 = -inf) are counted apart."""
        f = self.frequency()
        alive = self.fire_count > 0
        counts, edges = np.histogram(np.log10(f[alive]), bins=bins)
        return counts, edges, int((~alive).sum())

    def summary(self) -> dict:
        return {"n_frames": int(self.n_frames), "n_latents": self.n_latents, "l0_mean": self.l0_mean(),
                "dead": int(self.dead().sum()), "dense_over_10pct": int((self.frequency() > 0.1).sum())}

    def to_npz(self, path: str) -> None:
        np.savez(path, n_frames=np.int64(self.n_frames), **{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_npz(cls, path: str) -> "FeatureStats":
        z = np.load(path)
        return cls(int(z["n_frames"]), *(z[k] for k in _FIELDS))

    @classmethod
    def from_block(cls, block: np.ndarray, n: int) -> "FeatureStats":
        """The arrays of an sae_stats_files block (uint8 bytes, engine.stats_layout)."""
        from .engine import stats_layout, unpack_block
        a = unpack_block(block, stats_layout(n))
        return cls(int(a["n_frames"][0]), *(a[k] for k in _FIELDS))


@keep_rng
def feature_stats(sae, data_path: str, layer_name: str, *, lengths=None, subset_size: Optional[int] = None,
                  batch_files: Optional[int] = None, unfused: bool = False) -> FeatureStats:
    """Statistics of every latent of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files
    of a shard directory, in one pass.  batch_files: files per engine call (default: file_pass.default_batch_files, which
    picks the fused L1 path where it can); unfused: force the stored-latent L1 path (tests, benchmarks)."""
    from . import engine as E

    if is_raw(sae):
        raise ValueError("feature statistics need an SAE (raw-activation statistics are not provided)")
    fp = FilePass(sae, data_path, layer_name, what="feature statistics", lengths=lengths, subset_size=subset_size,
                  batch_files=batch_files)
    n = fp.eng.n
    with torch.cuda.device(fp.device):
        block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device=fp.device)
        for x, _file0, _nb, lb in fp:
            fp.eng.stats_files(x, block, lb, unfused=unfused)
        host = block.cpu().numpy()                  # the one read-back
    return FeatureStats.from_block(host, n)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Per-latent firing rates and the L0 histogram of an SAE over a shard directory.")
    add_pass_arguments(ap)
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: feature_stats(a.sae, a.data_path, a.layer_name, lengths=lengths, batch_files=a.batch_files))


if __name__ == "__main__":
    main()
