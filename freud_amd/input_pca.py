"""Input covariance and the PCA baseline: the centred scatter S = sum_k (x_k - c)(x_k - c)^T of the first files of a shard directory,
float64, deterministic, in one resident GPU pass -- and on top of it, in host float64, the spectrum, the FVU of the best linear
reconstruction of every rank (the number to put next to a dictionary's FVU), the effective dimension and the held-out form.  Without
it: a torch script that materialises a [frames, d] float64 copy of the sample and gives run-dependent bits.

The rule (include/freud_sae.h, sae_input_cov; written out in float64 in tests/input_cov_reference.py).  The sample is the one of
freud_amd/input_stats.py: the first `files` files in file order, a file counts min(length, T) frames with `lengths`, else T; N = the
counted frames.  a_ki = double(x_ki) - c_i (one rounding), S_ij = sum_k a_ki a_kj accumulated in float64, not divided by N; the lower
triangle is the mirror of the upper to the bit.  c is the engine's own mean (sae_input_moments) for center="mean", zeros for "zero",
or the caller's vector.  Two runs give the same bytes, whatever the device's size.

    python -m freud_amd.input_pca --data-path DIR --layer-name NAME [--files N] [--lengths L.npy] [--center mean|zero] [--out S.npz]
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional, Tuple

import numpy as np

from .file_pass import add_pass_arguments, keep_rng, run_pass_cli
from .input_stats import DEFAULT_BUDGET, DEFAULT_FILES, load_resident_sample

TILE, UNIT, TARGET_GROUPS = 64, 256, 2048         # freud_amd/csrc/input_cov_plan.h: ICV_TILE, ICV_UNIT, ICV_TARGET_GROUPS
_ARRAYS = ("center", "mean", "scatter")
_SCALARS = ("n_files", "n_frames", "d")
SUMMARY_RANKS = (8, 16, 32, 64, 128)


def cov_plan(n_files: int, T: int, d: int) -> dict:
    """The decomposition of freud_amd/csrc/input_cov_plan.h (icv_plan) restated for the host: what the budget check needs before a
    device or the library is there.  {"tile", "tiles", "segments", "units_per_segment", "workspace_bytes"}."""
    ntd = -(-int(d) // TILE)
    tiles = ntd * (ntd + 1) // 2
    units = int(n_files) * -(-int(T) // UNIT)
    want = max(1, min(TARGET_GROUPS // tiles, units))
    ups = -(-units // want)
    segments = -(-units // ups)
    return {"tile": TILE, "tiles": tiles, "segments": segments, "units_per_segment": ups, "workspace_bytes": segments * tiles * TILE * TILE * 8}


def cov_extra_bytes(n_files: int, T: int, d: int) -> int:
    """What input_covariance holds on the device beside the sample: the scatter, the moments' block and the larger workspace."""
    units = int(n_files) * -(-int(T) // UNIT)
    stats_ws = 64 + -(-(4 * d + 2) * 8 // 64) * 64 + units * max(4 * d, d + 2) * 8      # (sae_input_stats_workspace_bytes)
    return d * d * 8 + (4 * d + 2) * 8 + max(cov_plan(n_files, T, d)["workspace_bytes"], stats_ws)


@dataclasses.dataclass(eq=False)
class InputCovariance:
    """The scatter of one sample about `center`, and what follows from it (see the module docstring)."""
    n_files: int
    n_frames: int
    d: int
    center: np.ndarray                # float64 [d]: the c of the rule
    mean: np.ndarray                  # float64 [d]: the sample's mean (sae_input_moments), whatever the centre
    scatter: np.ndarray               # float64 [d, d]: S, not divided by n_frames
    _eig: Optional[Tuple[np.ndarray, np.ndarray]] = dataclasses.field(default=None, repr=False, compare=False)

    def __eq__(self, other) -> bool:
        """The same counts and the same bytes in center, mean and scatter."""
        if not isinstance(other, InputCovariance):
            return NotImplemented
        return all(getattr(self, k) == getattr(other, k) for k in _SCALARS) and all(
            np.asarray(getattr(self, k)).tobytes() == np.asarray(getattr(other, k)).tobytes() for k in _ARRAYS)

    __hash__ = None

    @property
    def covariance(self) -> np.ndarray:
        return self.scatter / self.n_frames

    @property
    def centered_on_mean(self) -> bool:
        return bool(np.array_equal(self.center, self.mean))

    def eigh(self) -> Tuple[np.ndarray, np.ndarray]:
        """(eigenvalues [d] of the scatter, descending, those below zero by rounding clamped to zero; components [d, d] by rows,
        components[i] the unit direction of eigenvalues[i]).  Cached."""
        if self._eig is None:
            w, v = np.linalg.eigh(self.scatter)
            self._eig = (np.maximum(w[::-1], 0.0), np.ascontiguousarray(v[:, ::-1].T))
        return self._eig

    @property
    def eigenvalues(self) -> np.ndarray:
        return self.eigh()[0]

    @property
    def components(self) -> np.ndarray:
        return self.eigh()[1]

    def fvu_curve(self) -> np.ndarray:
        """float64 [d + 1]: entry r is the fraction of variance that the best rank-r linear reconstruction about `center` leaves,
        1 - sum_{i < r} lambda_i / trace(scatter), from 1 at r = 0 to 0 at r = d.  With center="mean" the denominator
        trace(scatter) = sum_k |x_k - mean|^2 is the one ReconstructionReport.fvu() divides by over the same frames: the two numbers
        compare directly.  About another centre the curve is defined about that centre."""
        lam = self.eigenvalues
        total = float(np.trace(self.scatter))
        if not total > 0.0:
            return np.zeros(self.d + 1)
        kept = np.concatenate([[0.0], np.cumsum(lam)]) / total
        return np.clip(1.0 - kept, 0.0, 1.0)

    def pca_fvu(self, r: int) -> float:
        """The FVU of rank-r PCA about `center` (see fvu_curve), 0 <= r <= d."""
        r = int(r)
        if not 0 <= r <= self.d:
            raise ValueError(f"r={r} outside [0, {self.d}]")
        return float(self.fvu_curve()[r])

    def rank_for_fvu(self, target: float) -> int:
        """The smallest r with pca_fvu(r) <= target."""
        hit = np.nonzero(self.fvu_curve() <= float(target))[0]
        if hit.size == 0:
            raise ValueError(f"no rank reaches an FVU of {target}")
        return int(hit[0])

    @property
    def participation_ratio(self) -> float:
        """(sum lambda)^2 / sum lambda^2: the effective dimension (d for an isotropic sample, 1 for a line)."""
        lam = self.eigenvalues
        s2 = float((lam * lam).sum())
        return float(lam.sum()) ** 2 / s2 if s2 > 0 else 0.0

    def heldout_fvu(self, other: "InputCovariance", r: int) -> float:
        """The FVU on `other`'s sample of the projection onto THIS sample's top r components about this sample's centre:
        1 - trace(V_r other.scatter V_r^T) / trace(other.scatter).  `other` must have been computed with center=self.center."""
        if other.d != self.d:
            raise ValueError(f"the other sample has d={other.d}, this one d={self.d}")
        if not np.array_equal(other.center, self.center):
            raise ValueError("heldout_fvu needs the other sample's scatter about THIS sample's centre: compute it with center=self.center")
        r = int(r)
        if not 0 <= r <= self.d:
            raise ValueError(f"r={r} outside [0, {self.d}]")
        total = float(np.trace(other.scatter))
        if not total > 0.0:
            return 0.0
        V = self.components[:r]
        return float(1.0 - np.einsum("ri,ij,rj->", V, other.scatter, V) / total)

    def summary(self) -> dict:
        lam = self.eigenvalues
        about = "mean" if self.centered_on_mean else ("zero" if not self.center.any() else "given")
        return {"n_files": self.n_files, "n_frames": self.n_frames, "d": self.d, "center": about,
                "fvu_about": "the sample mean: comparable with a reconstruction report's FVU" if about == "mean"
                else f"the {about} centre, not the mean: not comparable with a reconstruction report's FVU",
                "trace": float(np.trace(self.scatter)), "total_variance": float(np.trace(self.scatter)) / self.n_frames,
                "top_eigenvalue": float(lam[0]) / self.n_frames, "participation_ratio": self.participation_ratio,
                "pca_fvu": {str(r): self.pca_fvu(r) for r in SUMMARY_RANKS if r <= self.d}}

    def save(self, path: str) -> None:
        with open(path, "wb") as fh:       # (a file object: numpy appends no ".npz" to the name)
            np.savez(fh, **{k: getattr(self, k) for k in _ARRAYS}, **{k: np.asarray(getattr(self, k)) for k in _SCALARS})

    to_npz = save                          # (the name file_pass.run_pass_cli stores a result by)

    @classmethod
    def load(cls, path: str) -> "InputCovariance":
        with np.load(path) as z:
            kw = {k: z[k] for k in _ARRAYS}
            kw.update({k: int(z[k]) for k in _SCALARS})
        return cls(**kw)


def check_center(center, d: Optional[int] = None):
    """center -> "mean", "zero" or a float64 array [d]; anything else is refused."""
    if isinstance(center, str):
        if center not in ("mean", "zero"):
            raise ValueError(f'center={center!r}: "mean", "zero" or a float64 array [d]')
        return center
    c = np.asarray(center)
    if c.ndim != 1 or not np.issubdtype(c.dtype, np.floating) or (d is not None and c.shape[0] != d):
        raise ValueError(f"center must be \"mean\", \"zero\" or a float array [{'d' if d is None else d}], got {c.dtype} {c.shape}")
    if not np.isfinite(c).all():
        raise ValueError("center must be finite")
    return np.ascontiguousarray(c, dtype=np.float64)


def check_input_pca_args(files, center, device_budget_bytes=DEFAULT_BUDGET):
    """The argument rules that need neither the shards nor a device -> the checked centre."""
    if int(files) < 1:
        raise ValueError(f"files={files} must be >= 1")
    if int(device_budget_bytes) < 1:
        raise ValueError(f"device_budget_bytes={device_budget_bytes} must be >= 1")
    return check_center(center)


def sample_covariance(x, lengths=None, center="mean"):
    """The engine's part, on a sample already resident: x [n_files, T, d] CUDA (fp32 / fp16 / bf16), lengths an int32 CUDA tensor
    [n_files] or None, center "mean" | "zero" | float64 numpy [d] -> (moments float64 [4 d + 2] (sae_input_moments), center float64
    [d], scatter float64 [d, d]) as numpy.  No read-back between the two calls: the mean stays on the device."""
    import torch
    from . import engine as E

    B, T, d = (int(v) for v in x.shape)
    center = check_center(center, d)
    with torch.cuda.device(x.device):
        ws = torch.empty(max(E.input_stats_workspace_bytes(B, T, d), E.input_cov_workspace_bytes(B, T, d)), dtype=torch.uint8, device=x.device)
        mom = torch.empty(4 * d + 2, dtype=torch.float64, device=x.device)
        out = torch.empty((d, d), dtype=torch.float64, device=x.device)
        E.input_moments(x, mom, ws, lengths)
        if isinstance(center, str):
            c = mom[:d].contiguous() if center == "mean" else None
        else:
            c = torch.from_numpy(center).to(x.device)
        E.input_cov(x, out, ws, c, lengths)
        moments = mom.cpu().numpy()
        cen = np.zeros(d, np.float64) if c is None else c.cpu().numpy()
        return moments, cen, out.cpu().numpy()


@keep_rng
def input_covariance(data_path: str, layer_name: str, *, files: int = DEFAULT_FILES, lengths=None, center="mean",
                     device_budget_bytes: int = DEFAULT_BUDGET) -> InputCovariance:
    """The scatter of the first `files` files of a shard directory (fewer where it holds fewer) about `center`: "mean" (the sample's
    own), "zero" (the raw second moment) or a float64 array [d].  The sample is the one input_statistics takes, loaded once and kept
    in device memory; sample, output and workspace over device_budget_bytes are refused before the device is touched.  The caller's
    global torch RNG is left as it was."""
    import torch

    center = check_input_pca_args(files, center, device_budget_bytes)
    fp, sample, lens = load_resident_sample(data_path, layer_name, files, lengths, device_budget_bytes, "input covariance", cov_extra_bytes)
    with torch.cuda.device(fp.device):
        moments, cen, scatter = sample_covariance(sample, lens, center)
    d = fp.d
    N = int(moments[4 * d + 1])
    fp.check_counted(N)
    return InputCovariance(n_files=fp.n_total, n_frames=N, d=d, center=cen, mean=moments[:d].copy(), scatter=scatter)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Input covariance and the PCA baseline of the first files of a shard directory.")
    add_pass_arguments(ap, sae=False, out_required=False)
    ap.add_argument("--files", type=int, default=DEFAULT_FILES)
    ap.add_argument("--center", choices=("mean", "zero"), default="mean")
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: input_covariance(a.data_path, a.layer_name, files=a.files, lengths=lengths, center=a.center))


if __name__ == "__main__":
    main()
