"""Reconstruction report: how well a trained dictionary reconstructs real data, where it fails, and which latents carry the
reconstruction -- in one pass over the Whisper-activation shards.

Semantics (include/freud_sae.h, sae_recon_files).  Over the files of a shard directory, the first min(L[f], T) frames of file f
count when `lengths` is given (file_pass.check_lengths rules), all T frames otherwise.  a is the value freud_amd.models encode()
returns (the bf16 L1 latent, or the TopK k selection), x_hat the decode of exactly that latent -- models.decode(encode(x).latent)
for L1, the sparse fp32 decode with b_dec for TopK -- and r = float(x) - x_hat in fp32.  An element of x equal to -1 is data: the
ignored_index of the reference's mse_loss is not applied.

Both decoders are linear in the latent, so zeroing latent j changes a frame's squared error by 2 a_j (r . w_j) + a_j^2 |w_j|^2
(w_j: its decoder direction).  The pass keeps, per latent, attr_sum = sum a_j (r . w_j), act_sq_sum = sum a_j^2 and dec_norm_sq =
|w_j|^2; per model dimension sum_x, sum_x_sq and sum_r_sq; per file file_sse = sum r^2 and file_energy = sum x^2.  From those:

    ablation_j = 2 attr_sum_j + act_sq_sum_j dec_norm_sq_j     the squared error latent j is worth (first order in the decoder:
                                                               the frame is not re-encoded)
    rescale_j  = 1 + attr_sum_j / (act_sq_sum_j dec_norm_sq_j)  the least-squares gain of latent j, everything else held fixed --
                                                               the shrinkage diagnostic of an L1 dictionary (above 1)
    fvu        = sum r^2 / sum_i (sum_x_sq_i - sum_x_i^2 / n_frames)

Two runs over the same data give bitwise identical arrays.

    python -m freud_amd.reconstruction --sae CKPT --data_path DIR --layer_name L [--lengths f.npy] [--batch_files B] --out report.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import List, Optional

import numpy as np
import torch

from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

_FIELDS = ("attr_sum", "act_sq_sum", "dec_norm_sq", "sum_x", "sum_x_sq", "sum_r_sq", "file_sse", "file_energy")


@dataclasses.dataclass
class ReconstructionReport:
    """Reconstruction quality of an SAE over a dataset (see the module docstring)."""
    n_frames: int
    attr_sum: np.ndarray        # float64 [n]
    act_sq_sum: np.ndarray      # float64 [n]
    dec_norm_sq: np.ndarray     # float32 [n]
    sum_x: np.ndarray           # float64 [d]
    sum_x_sq: np.ndarray        # float64 [d]
    sum_r_sq: np.ndarray        # float64 [d]
    file_sse: np.ndarray        # float64 [n_files]
    file_energy: np.ndarray     # float64 [n_files]
    filenames: List[str] = dataclasses.field(default_factory=list)

    @property
    def n_latents(self) -> int:
        return int(self.attr_sum.shape[0])

    def sse(self) -> float:
        """Sum of squared residuals over the counted frames."""
        return float(self.sum_r_sq.sum())

    def variance_by_dim(self) -> np.ndarray:
        """Per model dimension the sum of squared deviations from its mean over the counted frames (float64 [d])."""
        return self.sum_x_sq - self.sum_x * self.sum_x / max(self.n_frames, 1)

    def total_variance(self) -> float:
        return float(self.variance_by_dim().sum())

    def fvu(self) -> float:
        """Fraction of variance unexplained over the whole dataset."""
        tv = self.total_variance()
        return self.sse() / tv if tv > 0 else float("nan")

    def fvu_by_dim(self) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum_r_sq / self.variance_by_dim()

    def file_nmse(self) -> np.ndarray:
        """Per file: squared error over energy (float64 [n_files]); NaN for a file without energy."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.file_energy > 0, self.file_sse / self.file_energy, np.nan)

    def worst_files(self, n: int = 10):
        """The n files the dictionary explains worst: [(file index, filename or None, nmse)], worst first."""
        nm = self.file_nmse()
        order = np.argsort(-np.nan_to_num(nm, nan=-np.inf), kind="stable")[:n]
        return [(int(i), self.filenames[i] if i < len(self.filenames) else None, float(nm[i])) for i in order]

    def ablation(self) -> np.ndarray:
        """Per latent the increase of the summed squared error when it is zeroed (float64 [n])."""
        return 2.0 * self.attr_sum + self.act_sq_sum * self.dec_norm_sq.astype(np.float64)

    def ablation_share(self) -> np.ndarray:
        return self.ablation() / self.sse()

    def rescale(self) -> np.ndarray:
        """Per latent the least-squares gain with everything else held fixed; NaN for latents that never fire."""
        q = self.act_sq_sum * self.dec_norm_sq.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(q > 0, 1.0 + self.attr_sum / q, np.nan)

    def top_latents(self, n: int = 10, by: str = "ablation"):
        """The n latents with the largest `by` ("ablation", "ablation_share" or "rescale"): [(latent, value)], largest first;
        latents whose value is NaN come last."""
        if by not in ("ablation", "ablation_share", "rescale"):
            raise ValueError(f"by={by!r} must be 'ablation', 'ablation_share' or 'rescale'")
        v = getattr(self, by)()
        order = np.argsort(-np.nan_to_num(v, nan=-np.inf), kind="stable")[:n]
        return [(int(j), float(v[j])) for j in order]

    def summary(self) -> dict:
        ab = self.ablation()
        return {"n_frames": int(self.n_frames), "n_latents": self.n_latents, "n_files": int(self.file_sse.shape[0]), "sse": self.sse(),
                "fvu": self.fvu(), "worst_file_nmse": float(np.nanmax(self.file_nmse())) if self.file_sse.size else float("nan"),
                "top_latent": int(np.argmax(ab)) if ab.size else -1,
                "median_rescale": float(np.nanmedian(self.rescale())) if (self.act_sq_sum > 0).any() else float("nan")}

    def to_npz(self, path: str) -> None:
        np.savez(path, n_frames=np.int64(self.n_frames), filenames=np.asarray(self.filenames, dtype=np.str_),
                 **{k: getattr(self, k) for k in _FIELDS})

    @classmethod
    def from_npz(cls, path: str) -> "ReconstructionReport":
        z = np.load(path)
        return cls(int(z["n_frames"]), *(z[k] for k in _FIELDS), filenames=[str(s) for s in z["filenames"]])

    @classmethod
    def from_block(cls, block: np.ndarray, n: int, d: int, file_out: np.ndarray, filenames=()) -> "ReconstructionReport":
        """The arrays of an sae_recon_files block (uint8 bytes, engine.recon_layout) and the per-file rows [n_files][2]."""
        from .engine import recon_layout, unpack_block
        a = unpack_block(block, recon_layout(n, d))
        fo = np.asarray(file_out, dtype=np.float64).reshape(-1, 2)
        # (_FIELDS' last two are the per-file columns)
        return cls(int(a["n_frames"][0]), *(a[k] for k in _FIELDS[:-2]), fo[:, 0].copy(), fo[:, 1].copy(), list(filenames))


@keep_rng
def reconstruction_report(sae, data_path: str, layer_name: str, *, lengths=None, subset_size: Optional[int] = None,
                          batch_files: Optional[int] = None, unfused: bool = False) -> ReconstructionReport:
    """The reconstruction report of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files
    of a shard directory, in one pass.  batch_files: files per engine call (default: file_pass.default_batch_files); unfused:
    SAE_RECON_UNFUSED (keeps the L1 attribution GEMM off the streaming kernel)."""
    from . import engine as E

    if is_raw(sae):
        raise ValueError("a reconstruction report needs an SAE (there is nothing to reconstruct raw activations with)")
    fp = FilePass(sae, data_path, layer_name, what="reconstruction report", lengths=lengths, subset_size=subset_size,
                  batch_files=batch_files)
    n, d = fp.eng.n, fp.eng.d
    with torch.cuda.device(fp.device):
        block = torch.zeros(E.recon_layout(n, d)["bytes"], dtype=torch.uint8, device=fp.device)
        file_out = torch.zeros(fp.n_total, 2, dtype=torch.float64, device=fp.device)
        for x, file0, nb, lb in fp:
            fp.eng.recon_files(x, block, file_out[file0:file0 + nb], lb, unfused=unfused)
        host, files = block.cpu().numpy(), file_out.cpu().numpy()       # the one read-back
    return ReconstructionReport.from_block(host, n, d, files, fp.filenames)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="FVU, per-file error and per-latent ablation effect of an SAE over a shard directory.")
    add_pass_arguments(ap)
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: reconstruction_report(a.sae, a.data_path, a.layer_name, lengths=lengths, batch_files=a.batch_files))


if __name__ == "__main__":
    main()
