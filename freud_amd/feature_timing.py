"""Feature timing: for how long every latent of a trained dictionary fires -- the distribution of its run lengths, of the gaps between
its runs and of its onsets -- in one pass over the Whisper-activation shards.  A frame is a 20 ms step of a 30 s window; a phoneme
detector fires in bursts of 2-6 frames, a word or prosody feature for tens of frames, a speaker or channel feature for the whole
file, and a latent that flickers on and off is usually noise.  The reference reaches such statements by looking at one activation
trace at a time in its GUI; every other pass of this package treats the frames of a file as an unordered bag.

Semantics (include/freud_sae.h, sae_timing_files; freud_amd/csrc/timing_bins.h).  Frames count exactly as in the feature statistics:
the first min(L[f], T) frames of file f when `lengths` is given (file_pass.check_lengths rules), all T otherwise.  A frame is active
iff the bf16 magnitude bits of the value freud_amd.models encode() returns (a multi_topk model uses its k selection) exceed those of
`threshold`; threshold = 0 is the rule of the statistics (a -0.0 and a selected zero of a TopK row are inactive).  With the active
frames t1 < t2 < ... of a latent within one file's counted frames and a bridge g (0..15):

    run        neighbours a < b belong to the same run iff b - a - 1 <= g; runs never cross a file boundary
    duration   last - first + 1, bridged frames included
    gap        b - a - 1 between two consecutive runs of one file (> g); the silence before the first and after the last run is none
    censored   the run starts on frame 0 or ends on the last counted frame of its file: its duration is a lower bound

Durations and gaps L >= 1 are binned exactly on small integers and logarithmically above, in integers: with s = sub_bits, P = 2^s,
idx = L if L < 2P else sh P + (L >> sh), sh = floor(log2 L) - s; bin = idx - 1; NB = idx(T).  s = 2: 1..7 frames have a bin each
(20-140 ms), then four bins per octave; T = 1500 gives 37 bins.  run_hist[j, b] and gap_hist[j, b] count runs and gaps, totals[j] is
(ACTIVE frames, SPAN = the summed durations, RUNS, FILES with at least one run, the LONGEST run, CENSORED runs).  Every count is an
integer sum (LONGEST an integer maximum): two runs give bitwise identical arrays, whatever batch_files.

Out of scope: a fused GEMM epilogue (runs cross the row tiles), runs across files, raw (no-SAE) activations, fp8 contexts,
value-weighted statistics such as the peak or the area of a run, a split by label, and a list of the individual segments (the
feature index already gives positions).

    python -m freud_amd.feature_timing --sae CKPT --data_path DIR --layer_name L [--sub_bits S] [--bridge G] [--threshold V]
                                       [--lengths f.npy] [--batch_files B] --out timing.npz
"""
from __future__ import annotations

import argparse
import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from .engine import (TIMING_ACTIVE, TIMING_CENSORED, TIMING_FILES, TIMING_LONGEST, TIMING_MAX_BRIDGE, TIMING_NTOTALS, TIMING_RUNS, TIMING_SPAN,
                     check_sub_bits, timing_nbins)
from .activation_hist import quantile_bounds
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

_ARRAYS = ("run_hist", "gap_hist", "totals")


def threshold_bits(threshold) -> int:
    """The bf16 bit pattern of `threshold`: a finite, non-negative float that IS a bf16 value (nothing is rounded); ValueError
    otherwise."""
    try:
        v = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold={threshold!r} is not a number") from None
    if not math.isfinite(v) or v < 0:
        raise ValueError(f"threshold={v} must be finite and non-negative")
    f32 = np.array([v], np.float64).astype(np.float32)
    bits = int(f32.view(np.uint32)[0])
    if float(f32[0]) != v or (bits & 0xFFFF):
        raise ValueError(f"threshold={v!r} is not a bf16 value (it would have to be rounded)")
    return (bits >> 16) & 0x7FFF


def _check_args(sae, sub_bits, bridge, threshold) -> Tuple[int, int, int]:
    sub_bits, bridge = check_sub_bits(sub_bits), int(bridge)
    if bridge < 0 or bridge > TIMING_MAX_BRIDGE:
        raise ValueError(f"bridge={bridge} outside [0, {TIMING_MAX_BRIDGE}]")
    thr = threshold_bits(threshold)
    if is_raw(sae):
        raise ValueError("feature timing needs an SAE (the timing of raw activations is not provided)")
    return sub_bits, bridge, thr


def lower_edges(sub_bits: int, n_bins: int) -> np.ndarray:
    """int64 [n_bins + 1]: entry b is the smallest duration of bin b, the last one the first duration past the last bin."""
    P = 1 << int(sub_bits)
    idx = np.arange(1, int(n_bins) + 2, dtype=np.int64)
    return np.where(idx < 2 * P, idx, (P + idx % P) << np.maximum(idx // P - 1, 0))


@dataclasses.dataclass
class FeatureTiming:
    """Run-length and gap histograms of an SAE's latents over a dataset (see the module docstring)."""
    n_frames: int
    n_files: int
    T: int
    spec: Tuple[int, int, int]                   # (sub_bits, bridge, threshold_bits)
    run_hist: np.ndarray                         # int64 [n, NB]
    gap_hist: np.ndarray                         # int64 [n, NB]
    totals: np.ndarray                           # int64 [n, 6]: ACTIVE, SPAN, RUNS, FILES, LONGEST, CENSORED

    @property
    def n_latents(self) -> int:
        return int(self.run_hist.shape[0])

    @property
    def n_bins(self) -> int:
        return int(self.run_hist.shape[1])

    @property
    def sub_bits(self) -> int:
        return int(self.spec[0])

    @property
    def bridge(self) -> int:
        return int(self.spec[1])

    @property
    def threshold(self) -> float:
        return float(np.array([int(self.spec[2]) << 16], np.uint32).view(np.float32)[0])

    @property
    def n_runs(self) -> np.ndarray:
        return self.totals[:, TIMING_RUNS]

    def edges(self) -> np.ndarray:
        """int64 [NB + 1] frames: edges()[b] is the smallest duration (or gap) of bin b, the last entry one past the last bin."""
        return lower_edges(self.sub_bits, self.n_bins)

    def bin_bounds(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi) int64 [NB]: bin b holds the durations lo[b] <= L < hi[b] (hi - lo = 1 for the exact bins)."""
        e = self.edges()
        return e[:-1], e[1:]

    def _ratio(self, num: np.ndarray, den: np.ndarray) -> np.ndarray:
        den = den.astype(np.float64)
        return np.where(den > 0, num.astype(np.float64) / np.where(den > 0, den, 1.0), np.nan)

    def mean_duration(self) -> np.ndarray:
        """float64 [n] frames: SPAN / RUNS (NaN without a run); censored runs enter with their observed length."""
        return self._ratio(self.totals[:, TIMING_SPAN], self.totals[:, TIMING_RUNS])

    def duty(self) -> np.ndarray:
        """float64 [n]: ACTIVE / n_frames, the share of the counted frames on which the latent is active."""
        return self.totals[:, TIMING_ACTIVE].astype(np.float64) / max(1, int(self.n_frames))

    def persistence(self) -> np.ndarray:
        """float64 [n]: 1 - RUNS / ACTIVE at bridge = 0, the share of a latent's active frames that are followed by an active frame
        (up to file ends); 0 for a latent that only flickers, near 1 for one that stays on.  NaN for a dead latent."""
        if self.bridge != 0:
            raise ValueError(f"persistence is defined at bridge = 0, this pass ran with bridge = {self.bridge}")
        return 1.0 - self._ratio(self.totals[:, TIMING_RUNS], self.totals[:, TIMING_ACTIVE])

    def censored_fraction(self) -> np.ndarray:
        """float64 [n]: CENSORED / RUNS, the share of the runs whose duration is only a lower bound."""
        return self._ratio(self.totals[:, TIMING_CENSORED], self.totals[:, TIMING_RUNS])

    def quantile(self, q: float, which: str = "run") -> Tuple[np.ndarray, np.ndarray]:
        """Per latent the bounds (lo, hi), float64 [n] frames, of the bin that holds the q-th order statistic (inverted-CDF rank: the
        max(1, ceil(q N))-th smallest of N) of its run durations (which="run") or gaps ("gap"): lo <= L < hi.  NaN where there is
        nothing to rank."""
        if which not in ("run", "gap"):
            raise ValueError(f"which={which!r} is neither 'run' nor 'gap'")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q={q} outside [0, 1]")
        return quantile_bounds((self.run_hist if which == "run" else self.gap_hist).astype(np.int64), q, *self.bin_bounds())

    @staticmethod
    def seconds(frames, frame_ms: float = 20.0):
        """Frames -> seconds (Whisper's encoder: 20 ms per frame)."""
        return np.asarray(frames, np.float64) * (float(frame_ms) / 1000.0)

    def top_latents(self, by: str = "mean_duration", n_top: int = 10, min_runs: int = 1) -> np.ndarray:
        """int64 [<= n_top]: the latents with at least min_runs runs, by descending mean_duration | longest | runs | persistence; ties
        go to the lower index."""
        if by == "mean_duration":
            key = self.mean_duration()
        elif by == "longest":
            key = self.totals[:, TIMING_LONGEST].astype(np.float64)
        elif by == "runs":
            key = self.totals[:, TIMING_RUNS].astype(np.float64)
        elif by == "persistence":
            key = self.persistence()
        else:
            raise ValueError(f"by={by!r} is none of 'mean_duration', 'longest', 'runs', 'persistence'")
        if int(n_top) < 0:
            raise ValueError(f"n_top={n_top} must be >= 0")
        keep = np.flatnonzero((self.totals[:, TIMING_RUNS] >= int(min_runs)) & ~np.isnan(key))
        order = np.argsort(-key[keep], kind="stable")              # stable: equal keys stay in index order
        return keep[order][: int(n_top)].astype(np.int64)

    def summary(self) -> dict:
        t = self.totals
        runs, active = int(t[:, TIMING_RUNS].sum()), int(t[:, TIMING_ACTIVE].sum())
        lo, hi = self.quantile(0.5)
        live = t[:, TIMING_RUNS] > 0
        return {"n_frames": int(self.n_frames), "n_files": int(self.n_files), "n_latents": self.n_latents, "T": int(self.T),
                "n_bins": self.n_bins, "sub_bits": self.sub_bits, "bridge": self.bridge, "threshold": self.threshold,
                "dead": int((~live).sum()), "runs": runs, "active_frames": active, "gaps": int(self.gap_hist.sum()),
                "censored_runs": int(t[:, TIMING_CENSORED].sum()), "longest_run": int(t[:, TIMING_LONGEST].max()) if t.size else 0,
                "single_frame_runs": int(self.run_hist[:, 0].sum()),
                "whole_file_latents": int((t[:, TIMING_LONGEST] >= self.T).sum()),
                "mean_duration": float(t[:, TIMING_SPAN].sum() / runs) if runs else None,
                "median_duration_lo": float(np.nanmedian(lo)) if live.any() else None,
                "median_duration_hi": float(np.nanmedian(hi)) if live.any() else None}

    def check(self) -> None:
        """The invariants of the pass, per latent (RuntimeError names the first one that fails)."""
        t = self.totals
        runs, files, active, span = t[:, TIMING_RUNS], t[:, TIMING_FILES], t[:, TIMING_ACTIVE], t[:, TIMING_SPAN]
        bad = None
        if not (self.run_hist.sum(1) == runs).all():
            bad = "sum(run_hist) != RUNS"
        elif not (self.gap_hist.sum(1) == runs - files).all():
            bad = "sum(gap_hist) != RUNS - FILES"
        elif not ((span == active).all() if self.bridge == 0 else (span >= active).all()):
            bad = "SPAN != ACTIVE at bridge = 0" if self.bridge == 0 else "SPAN < ACTIVE"
        elif not (t[:, TIMING_LONGEST] <= self.T).all():
            bad = "LONGEST > T"
        if bad:
            raise RuntimeError(f"the timing arrays are inconsistent: {bad}")

    def to_npz(self, path: str) -> None:
        np.savez(path, n_frames=np.int64(self.n_frames), n_files=np.int64(self.n_files), T=np.int64(self.T),
                 spec=np.asarray(self.spec, np.int64), **{k: getattr(self, k) for k in _ARRAYS})

    @classmethod
    def from_npz(cls, path: str) -> "FeatureTiming":
        with np.load(path) as z:
            return cls(int(z["n_frames"]), int(z["n_files"]), int(z["T"]), tuple(int(v) for v in z["spec"]), *(z[k] for k in _ARRAYS))


@keep_rng
def feature_timing(sae, data_path: str, layer_name: str, *, sub_bits: int = 2, bridge: int = 0, threshold: float = 0.0, lengths=None,
                   subset_size: Optional[int] = None, batch_files: Optional[int] = None) -> FeatureTiming:
    """Run-length and gap histograms of every latent of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16
    contexts) over the files of a shard directory.  threshold: a finite, non-negative bf16 value (it is not rounded).  batch_files:
    files per engine call (default: file_pass.default_batch_files); the result does not depend on it."""
    sub_bits, bridge, thr = _check_args(sae, sub_bits, bridge, threshold)
    fp = FilePass(sae, data_path, layer_name, what="feature timing", lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    n, T = fp.eng.n, fp.T
    nb = timing_nbins(sub_bits, T)
    with torch.cuda.device(fp.device):
        run_hist = torch.zeros(n, nb, dtype=torch.int64, device=fp.device)
        gap_hist = torch.zeros_like(run_hist)
        totals = torch.zeros(n, TIMING_NTOTALS, dtype=torch.int64, device=fp.device)
        n_frames = torch.zeros(1, dtype=torch.int64, device=fp.device)
        for x, _file0, _nbf, lb in fp:
            fp.eng.timing_files(x, sub_bits, bridge, thr, run_hist, gap_hist, totals, n_frames, lb)
        counted = int(n_frames.item())
        res = FeatureTiming(fp.n_frames, fp.n_total, T, (sub_bits, bridge, thr), run_hist.cpu().numpy(), gap_hist.cpu().numpy(),
                            totals.cpu().numpy())
    fp.check_counted(counted)
    res.check()
    return res


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Run-length and gap histograms of every latent of an SAE over a shard directory.")
    add_pass_arguments(ap)
    ap.add_argument("--sub_bits", type=int, default=2)
    ap.add_argument("--bridge", type=int, default=0, help="inactive frames a run may span (0..15)")
    ap.add_argument("--threshold", type=float, default=0.0, help="a frame is active above this bf16 value")
    a = ap.parse_args(argv)
    run_pass_cli(a, lambda lengths: feature_timing(a.sae, a.data_path, a.layer_name, sub_bits=a.sub_bits, bridge=a.bridge,
                                                   threshold=a.threshold, lengths=lengths, batch_files=a.batch_files))


if __name__ == "__main__":
    main()
