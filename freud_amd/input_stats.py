"""Input statistics: what the activations look like before a dictionary exists -- the per-dimension mean, variance and extremes, the
norm scale, the share of the energy that sits in the mean, and the geometric median (the b_dec every TopK recipe starts from:
Bricken et al. 2023) -- of the first files of a shard directory, in one resident GPU pass (without it: a torch script that
materialises [frames, d] temporaries several times per Weiszfeld iteration).

The rule (include/freud_sae.h, sae_input_moments / sae_input_median; written out in float64 in tests/input_stats_reference.py).  The
sample is the first `files` files in file order; a file counts min(length, T) frames with `lengths`, else T; N = the counted frames.
    mean, var = sum (x - mean)^2 / N (centred: a second sweep, not E[x^2] - mean^2), min, max (exact), mean_sq_norm = sum |x|^2 / N
    total_variance = sum_d var, sigma = sqrt(total_variance), mean_energy_fraction = |mean|^2 / mean_sq_norm,
    norm_scale = sqrt(d / mean_sq_norm)
    geometric median: Weiszfeld from m_0 = mean with a fixed iteration count: dist_i = |x_i - m_k|, w_i = 1 / max(dist_i, floor),
    floor = max(2^-20 sigma, FLT_MIN), m_{k+1} = sum w_i x_i / sum w_i, J_k = sum dist_i / N for k = 0 .. I
There is no convergence test on the device: read `shift` = |m_I - m_{I-1}| / sigma and the objective trace.  Two runs give the same
bytes, whatever the device's size.

    python -m freud_amd.input_stats --data-path DIR --layer-name NAME [--files N] [--iterations I] [--lengths L.npy] [--out S.npz]
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional

import numpy as np

from .file_pass import FilePass, add_pass_arguments, keep_rng, run_pass_cli

MAX_D, MAX_ITERATIONS = 2048, 1024                # include/freud_sae.h: SAE_INPUT_MAX_D, SAE_INPUT_MAX_ITERATIONS
FLT_MIN = float(np.finfo(np.float32).tiny)
DEFAULT_FILES, DEFAULT_ITERATIONS, DEFAULT_BUDGET = 256, 32, 8 << 30
_ARRAYS = ("mean", "var", "min", "max", "geometric_median", "geometric_median64", "objective")
_SCALARS = ("n_files", "n_frames", "d", "mean_sq_norm", "total_variance", "mean_energy_fraction", "norm_scale", "shift")


@dataclasses.dataclass
class InputStats:
    """The statistics of one sample (see the module docstring)."""
    n_files: int
    n_frames: int
    d: int
    mean: np.ndarray                  # float64 [d]
    var: np.ndarray                   # float64 [d]
    min: np.ndarray                   # float32 [d]
    max: np.ndarray                   # float32 [d]
    mean_sq_norm: float
    total_variance: float
    mean_energy_fraction: float
    norm_scale: float
    geometric_median: np.ndarray      # float32 [d]: the value an initialisation uses
    geometric_median64: np.ndarray    # float64 [d]
    objective: np.ndarray             # float64 [iterations + 1]: J_0 .. J_I
    shift: float                      # |m_I - m_{I-1}| / sigma (0 where sigma is 0)

    def top_dims(self, n: int = 8) -> np.ndarray:
        """The n dimensions with the largest |mean| / sqrt(var), largest first: the massive activations (a constant dimension with
        a non-zero mean ranks first)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.abs(self.mean) / np.sqrt(self.var)
        z = np.where(np.isnan(z), 0.0, z)
        return np.argsort(-z, kind="stable")[:max(0, int(n))].astype(np.int64)

    def summary(self) -> dict:
        top = self.top_dims(4)
        return {"n_files": self.n_files, "n_frames": self.n_frames, "d": self.d, "mean_sq_norm": self.mean_sq_norm,
                "total_variance": self.total_variance, "mean_energy_fraction": self.mean_energy_fraction, "norm_scale": self.norm_scale,
                "mean_norm": float(np.linalg.norm(self.mean)), "median_norm": float(np.linalg.norm(self.geometric_median64)),
                "objective_first": float(self.objective[0]), "objective_last": float(self.objective[-1]), "shift": self.shift,
                "iterations": int(self.objective.shape[0]) - 1, "top_dims": [int(i) for i in top]}

    def save(self, path: str) -> None:
        with open(path, "wb") as fh:       # (a file object: numpy appends no ".npz" to the name)
            np.savez(fh, **{k: getattr(self, k) for k in _ARRAYS},
                     **{k: np.asarray(getattr(self, k)) for k in _SCALARS})

    to_npz = save                          # (the name file_pass.run_pass_cli stores a result by)

    @classmethod
    def load(cls, path: str) -> "InputStats":
        with np.load(path) as z:
            kw = {k: z[k] for k in _ARRAYS}
            kw.update({k: (int(z[k]) if k in ("n_files", "n_frames", "d") else float(z[k])) for k in _SCALARS})
        return cls(**kw)


def check_input_stats_args(files, iterations, device_budget_bytes=DEFAULT_BUDGET) -> None:
    """The argument rules that need neither the shards nor a device."""
    if int(files) < 1:
        raise ValueError(f"files={files} must be >= 1")
    if not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"iterations={iterations} outside [1, {MAX_ITERATIONS}]")
    if int(device_budget_bytes) < 1:
        raise ValueError(f"device_budget_bytes={device_budget_bytes} must be >= 1")


def check_budget(n_files: int, T: int, d: int, itemsize: int, device_budget_bytes: int, extra_bytes: int = 0) -> None:
    """A resident sample of n_files x T x d elements (and extra_bytes of outputs and workspace beside it) must fit the budget; the
    refusal names the largest `files` that does."""
    per_file = int(T) * int(d) * int(itemsize)
    if int(n_files) * per_file + int(extra_bytes) > int(device_budget_bytes):
        fits = max(0, int(device_budget_bytes) - int(extra_bytes)) // per_file
        hint = f"files={fits} is the most that fits" if fits >= 1 else "not even one file fits"
        beside = f" beside {int(extra_bytes)} bytes of output and workspace" if extra_bytes else ""
        raise ValueError(f"a resident sample of {n_files} files x {T} frames x d={d} ({itemsize} bytes each) takes "
                         f"{int(n_files) * per_file} bytes{beside}, over device_budget_bytes={int(device_budget_bytes)}: {hint}")


def derive(n_files: int, d: int, moments: np.ndarray, path: np.ndarray, objective: np.ndarray) -> InputStats:
    """InputStats from the engine's output blocks: moments float64 [4 d + 2] (include/freud_sae.h: sae_input_moments), the path
    [iterations + 1, d] and the objective trace; the derived scalars are float64 host arithmetic."""
    moments = np.asarray(moments, dtype=np.float64)
    N = int(moments[4 * d + 1])
    mean, var = moments[:d].copy(), moments[d:2 * d] / N
    mean_sq_norm = float(moments[4 * d]) / N
    total_variance = float(var.sum())
    sigma = float(np.sqrt(total_variance))
    step = float(np.linalg.norm(path[-1] - path[-2]))
    return InputStats(
        n_files=int(n_files), n_frames=N, d=int(d), mean=mean, var=var, min=moments[2 * d:3 * d].astype(np.float32),
        max=moments[3 * d:4 * d].astype(np.float32), mean_sq_norm=mean_sq_norm, total_variance=total_variance,
        mean_energy_fraction=float(mean @ mean) / mean_sq_norm if mean_sq_norm > 0 else 0.0,
        norm_scale=float(np.sqrt(d / mean_sq_norm)) if mean_sq_norm > 0 else float("inf"),
        geometric_median=path[-1].astype(np.float32), geometric_median64=path[-1].copy(), objective=np.asarray(objective).copy(),
        shift=step / sigma if sigma > 0 else 0.0)


def weiszfeld_floor(sigma: float) -> float:
    """The floor of the weights' denominators: max(2^-20 sigma, FLT_MIN)."""
    return max(2.0 ** -20 * float(sigma), FLT_MIN)


def sample_statistics(x, lengths=None, iterations: int = DEFAULT_ITERATIONS):
    """The engine's part, on a sample already resident: x [n_files, T, d] CUDA (fp32 / fp16 / bf16), lengths an int32 CUDA tensor
    [n_files] or None -> (moments float64 [4 d + 2], path float64 [iterations + 1, d], objective float64 [iterations + 1]) as numpy.
    One read-back between the two calls: the floor comes from the moments' sigma."""
    import torch
    from . import engine as E

    B, T, d = (int(v) for v in x.shape)
    with torch.cuda.device(x.device):
        ws = torch.empty(E.input_stats_workspace_bytes(B, T, d), dtype=torch.uint8, device=x.device)
        mom = torch.empty(4 * d + 2, dtype=torch.float64, device=x.device)
        E.input_moments(x, mom, ws, lengths)
        moments = mom.cpu().numpy()
        sigma = float(np.sqrt((moments[d:2 * d] / moments[4 * d + 1]).sum()))
        path = torch.empty((iterations + 1, d), dtype=torch.float64, device=x.device)
        obj = torch.empty(iterations + 1, dtype=torch.float64, device=x.device)
        E.input_median(x, mom[:d], weiszfeld_floor(sigma), iterations, path, obj, ws, lengths)
        return moments, path.cpu().numpy(), obj.cpu().numpy()


def load_resident_sample(data_path: str, layer_name: str, files: int, lengths, device_budget_bytes: int, what: str, extra_bytes=None):
    """The first `files` files of a shard directory, loaded once into device memory -> (the FilePass, x [n_files, T, d] on its device
    in the shards' dtype, the trimmed lengths as an int32 tensor there or None).  Every refusal that needs no device -- an empty
    directory, d > MAX_D, a sample (plus extra_bytes(n_files, T, d), where given) over the budget, the lengths' rules -- comes before
    the device is touched."""
    import torch
    from .loader import MemoryMappedActivationsDataset

    ds = MemoryMappedActivationsDataset(data_path, layer_name, int(files))
    if len(ds) == 0:
        raise ValueError(f"{data_path}: no files")
    T, d = int(ds.tensor_shape[-2]), int(ds.tensor_shape[-1])
    if d > MAX_D:
        raise ValueError(f"the shards hold d={d}; the {what} serve{'' if what.endswith('s') else 's'} d <= {MAX_D}")
    check_budget(len(ds), T, d, ds.mmap.dtype.itemsize, device_budget_bytes, extra_bytes(len(ds), T, d) if extra_bytes else 0)
    fp = FilePass(None, data_path, layer_name, what=what, lengths=lengths, subset_size=int(files), max_frames=2 ** 31 - 1)
    with torch.cuda.device(fp.device):
        sample = None
        for x, file0, nb, _lb in fp:
            if sample is None:
                sample = torch.empty((fp.n_total, fp.T, fp.d), dtype=x.dtype, device=fp.device)
            sample[file0:file0 + nb].copy_(x)
        lens = torch.from_numpy(fp._lens).to(fp.device) if fp._lens is not None else None
    return fp, sample, lens


@keep_rng
def input_statistics(data_path: str, layer_name: str, *, files: int = DEFAULT_FILES, lengths=None, iterations: int = DEFAULT_ITERATIONS,
                     device_budget_bytes: int = DEFAULT_BUDGET) -> InputStats:
    """The statistics of the first `files` files of a shard directory (fewer where it holds fewer).  lengths: frames per file for
    those files.  The sample is loaded once and stays in device memory: one over device_budget_bytes is refused before the device is
    touched.  The caller's global torch RNG is left as it was."""
    import torch

    check_input_stats_args(files, iterations, device_budget_bytes)
    fp, sample, lens = load_resident_sample(data_path, layer_name, files, lengths, device_budget_bytes, "input statistics")
    with torch.cuda.device(fp.device):
        moments, path, objective = sample_statistics(sample, lens, int(iterations))
    stats = derive(fp.n_total, fp.d, moments, path, objective)
    fp.check_counted(stats.n_frames)
    return stats


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Input statistics and the geometric median of the first files of a shard directory.")
    add_pass_arguments(ap, sae=False, out_required=False)
    ap.add_argument("--files", type=int, default=DEFAULT_FILES)
    ap.add_argument("--iterations", type=int, default=DEFAULT_ITERATIONS)
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: input_statistics(a.data_path, a.layer_name, files=a.files, lengths=lengths, iterations=a.iterations))


if __name__ == "__main__":
    main()
