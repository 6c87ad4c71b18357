"""Activation histograms: how strongly every latent of a trained dictionary fires -- the distribution of its value over the frames, of
every file's maximum, and (for a few chosen latents) of its value on the frames of each label -- in one pass over the
Whisper-activation shards.  The reference shows such distributions one feature at a time: the GUI's "Histogram of Max Activation
Values per File" (gui/src/ActivationSearchTab.js over top_activations(..., return_max_per_file=True), one pass over the data per
feature looked at) and src/scripts/plot_polysemantic.py (one feature on the frames of six phoneme classes).

Semantics (include/freud_sae.h, sae_hist_files; freud_amd/csrc/hist_bins.h).  Frames count exactly as in the feature statistics: the
first min(L[f], T) frames of file f when `lengths` is given (file_pass.check_lengths rules), all T otherwise.  The value binned is the
one freud_amd.models encode() returns (a multi_topk model uses its k selection), on its own bf16 bit pattern: with lo_exp = L,
octaves = O, sub_bits = s, P = 2^s and NB = O P + 3,

    bin 0        the value is 0 (inactive; a -0.0 and a selected zero of a TopK row as well)
    bin 1        underflow, 0 < a < 2^L
    bin 2 + i    edges()[i] <= a < edges()[i + 1], edges()[i] = 2^(L + i // P) (1 + (i % P) / P), 0 <= i < O P
    bin NB - 1   overflow, a >= 2^(L + O)

Every edge is a bf16 value, so no comparison rounds: the counts are exact integers and two runs give bitwise identical arrays.
frame_hist[j, b] counts frames, file_max_hist[j, b] counts files by the bin of their maximum over their counted frames (a file on
which the latent never fires: bin 0) -- files_in_range() reads off it how many files a min_val / max_val band of the feature
search keeps, for every latent at once.  With label_latents (at most 64) and labels under the rules of freud_amd.feature_labels,
label_hist[s, l, b] counts the counted frames that carry label l and on which latent label_latents[s] falls in bin b; row C is the
"any" row (frame_hist of that latent) and label_count[l] the counted frames that carry l.

Out of scope: raw (no-SAE) activations, fp8 contexts, per-label float sums or means, histograms of pre-activations.

    python -m freud_amd.activation_hist --sae CKPT --data_path DIR --layer_name L [--lo_exp L] [--octaves O] [--sub_bits S]
                                        [--lengths f.npy] [--batch_files B] [--label_latents 1,5,9 (--file_labels f.npy |
                                        --frame_labels f.npy) [--class_names names.json]] --out hist.npz
"""
from __future__ import annotations

import argparse
import dataclasses
import json
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import feature_labels as FL
from .engine import HIST_MAX_SEL, hist_nbins
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

_ARRAYS = ("frame_hist", "file_max_hist", "label_hist", "label_latents", "label_count")


def _prev_bf16(v: np.ndarray) -> np.ndarray:
    """The largest bf16 value below each positive bf16 value of v (float32; +inf -> the largest finite one), as float64."""
    bits = (np.asarray(v, np.float32).view(np.uint32) >> 16) - 1
    return (bits << 16).astype(np.uint32).view(np.float32).astype(np.float64)


def quantile_bounds(h: np.ndarray, q: float, lo_b: np.ndarray, hi_b: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Per row of the histograms h (int64 [n, NB]) the bounds (lo_b[b], hi_b[b]), float64 [n], of the bin b that holds the q-th order
    statistic by the inverted-CDF rank -- the max(1, ceil(q N))-th smallest of the row's N values: the first bin whose cumulative
    count reaches the rank.  NaN where N = 0."""
    total = h.sum(1)
    rank = np.maximum(1, np.ceil(q * total.astype(np.float64)).astype(np.int64))
    b = (np.cumsum(h, 1) < rank[:, None]).sum(1)
    ok = total > 0
    b = np.where(ok, b, 0)
    return np.where(ok, lo_b[b].astype(np.float64), np.nan), np.where(ok, hi_b[b].astype(np.float64), np.nan)


@dataclasses.dataclass
class ActivationHistograms:
    """Value histograms of an SAE's latents over a dataset (see the module docstring)."""
    n_frames: int
    n_files: int
    spec: Tuple[int, int, int]                   # (lo_exp, octaves, sub_bits)
    frame_hist: np.ndarray                       # int64 [n, NB]
    file_max_hist: np.ndarray                    # int64 [n, NB]
    label_hist: Optional[np.ndarray] = None      # int64 [n_sel, C + 1, NB] or None
    label_latents: Optional[np.ndarray] = None   # int64 [n_sel]
    label_count: Optional[np.ndarray] = None     # int64 [C + 1]: counted frames that carry the label; entry C = n_frames
    class_names: Optional[List[str]] = None

    @property
    def n_latents(self) -> int:
        return int(self.frame_hist.shape[0])

    @property
    def n_bins(self) -> int:
        return int(self.frame_hist.shape[1])

    def edges(self) -> np.ndarray:
        """float64 [O P + 1]: edges()[i] is the lower edge of bin 2 + i, the last one the lower edge of the overflow bin."""
        lo_exp, octaves, sub_bits = self.spec
        P = 1 << sub_bits
        i = np.arange(octaves * P + 1)
        return np.ldexp(1.0 + (i % P) / P, lo_exp + i // P)

    def bin_bounds(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lo, hi) float64 [NB]: bin b holds the values lo[b] <= a < hi[b] (bin 0: only 0; bin 1: 0 < a < hi[1]; overflow: hi = inf)."""
        e = self.edges()
        return np.concatenate([[0.0, 0.0], e]), np.concatenate([[0.0], e, [np.inf]])

    def quantile(self, q: float, which: str = "frame", active_only: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """Per latent the bounds (lo, hi), float64 [n], of the bin that holds the q-th order statistic (inverted-CDF rank: the
        max(1, ceil(q N))-th smallest of N) of its value on the counted frames (which="frame") or of the files' maxima ("file");
        active_only: over the non-zero values only.  The statistic v satisfies lo <= v < hi (0 < v < hi in the underflow bin, lo = hi
        = 0 in bin 0).  NaN where there is nothing to rank."""
        if which not in ("frame", "file"):
            raise ValueError(f"which={which!r} is neither 'frame' nor 'file'")
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"q={q} outside [0, 1]")
        h = (self.frame_hist if which == "frame" else self.file_max_hist).astype(np.int64)
        if active_only:
            h = h.copy()
            h[:, 0] = 0
        return quantile_bounds(h, q, *self.bin_bounds())

    def files_in_range(self, min_val: Optional[float] = None, max_val: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Per latent the number of files whose maximum m passes the feature search's filter min_val <= m <= max_val (None: no
        bound), as a bracket (at_least, at_most), int64 [n]: the files of the bins that lie inside the band, and of those that
        touch it.  The two are equal when min_val is a bin's lower edge (or 0) and max_val the largest bf16 value of a bin."""
        lo_b, hi_b = self.bin_bounds()
        e32 = self.edges().astype(np.float32)                         # (2^128 -> inf: the overflow bin then holds only Inf / NaN)
        lo = lo_b.copy()
        lo[1] = float(np.uint32(1 << 16).view(np.float32))            # the smallest positive bf16
        lo[-1] = float(e32[-1])
        top = np.concatenate([[0.0], _prev_bf16(e32), [np.inf]])      # the largest value of each bin
        mn = -np.inf if min_val is None else float(min_val)
        mx = np.inf if max_val is None else float(max_val)
        inside = (lo >= mn) & (top <= mx)
        touch = (top >= mn) & (lo <= mx)
        return self.file_max_hist[:, inside].sum(1).astype(np.int64), self.file_max_hist[:, touch].sum(1).astype(np.int64)

    def label_id(self, label: Union[int, str, None]) -> int:
        """Row of label_hist for a label id, a class name, or None / "any" (all counted frames)."""
        C = int(self.label_count.shape[0]) - 1
        if label is None or label == "any":
            return C
        if isinstance(label, str):
            if self.class_names is None or label not in self.class_names:
                raise KeyError(f"no class named {label!r}")
            return self.class_names.index(label)
        if not 0 <= int(label) <= C:
            raise KeyError(f"label {label} outside [0, {C}]")
        return int(label)

    def label_distribution(self, latent: int, label: Union[int, str, None]) -> np.ndarray:
        """int64 [NB]: the frame histogram of `latent` (one of label_latents) on the frames that carry `label`."""
        if self.label_hist is None:
            raise ValueError("the pass was run without label_latents")
        at = np.flatnonzero(self.label_latents == int(latent))
        if at.size == 0:
            raise KeyError(f"latent {latent} is not one of label_latents {self.label_latents.tolist()}")
        return self.label_hist[int(at[0]), self.label_id(label)]

    def summary(self) -> dict:
        active = self.frame_hist[:, 1:].sum(1)
        lo, hi = self.quantile(0.5)
        return {"n_frames": int(self.n_frames), "n_files": int(self.n_files), "n_latents": self.n_latents, "n_bins": self.n_bins,
                "lo_exp": int(self.spec[0]), "octaves": int(self.spec[1]), "sub_bits": int(self.spec[2]),
                "dead": int((active == 0).sum()), "active_values": int(active.sum()),
                "underflow": int(self.frame_hist[:, 1].sum()), "overflow": int(self.frame_hist[:, -1].sum()),
                "median_active_lo": float(np.nanmedian(lo)) if np.isfinite(lo).any() else None,
                "median_active_hi": float(np.nanmedian(hi)) if np.isfinite(lo).any() else None,
                "label_latents": None if self.label_latents is None else self.label_latents.tolist()}

    def to_npz(self, path: str) -> None:
        extra = {k: getattr(self, k) for k in _ARRAYS if getattr(self, k) is not None}
        if self.class_names is not None:
            extra["class_names"] = np.array(self.class_names, dtype=str)
        np.savez(path, n_frames=np.int64(self.n_frames), n_files=np.int64(self.n_files), spec=np.asarray(self.spec, np.int64), **extra)

    @classmethod
    def from_npz(cls, path: str) -> "ActivationHistograms":
        with np.load(path) as z:
            names = [str(s) for s in z["class_names"]] if "class_names" in z.files else None
            return cls(int(z["n_frames"]), int(z["n_files"]), tuple(int(v) for v in z["spec"]),
                       *(z[k] if k in z.files else None for k in _ARRAYS), names)


def _check_label_latents(label_latents) -> Optional[np.ndarray]:
    if label_latents is None:
        return None
    a = np.asarray(label_latents)
    if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("label_latents must be a non-empty list of integer latent indices")
    if a.size > HIST_MAX_SEL:
        raise ValueError(f"{a.size} label_latents > {HIST_MAX_SEL}")
    if int(a.min()) < 0:
        raise ValueError(f"label_latents holds the index {int(a.min())} < 0")
    return a.astype(np.int64)


@keep_rng
def activation_histograms(sae, data_path: str, layer_name: str, *, lo_exp: int = -12, octaves: int = 24, sub_bits: int = 2, lengths=None,
                          subset_size: Optional[int] = None, batch_files: Optional[int] = None, label_latents=None, file_labels=None,
                          frame_labels=None, n_classes: Optional[int] = None, class_names=None) -> ActivationHistograms:
    """Value histograms of every latent of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the
    files of a shard directory.  label_latents: up to 64 latent indices whose frame histogram is also split by label; then exactly
    one of file_labels and frame_labels, with n_classes and class_names, as in freud_amd.feature_labels.  batch_files: files per engine
    call (default: file_pass.default_batch_files); the result does not depend on it."""
    spec = (int(lo_exp), int(octaves), int(sub_bits))
    nb = hist_nbins(spec)
    sel = _check_label_latents(label_latents)
    has_labels = file_labels is not None or frame_labels is not None
    if sel is not None and not has_labels:
        raise ValueError("label_latents need file_labels or frame_labels")
    if sel is None and has_labels:
        raise ValueError("file_labels / frame_labels need label_latents (the latents whose histogram is split by label)")
    if is_raw(sae):
        raise ValueError("activation histograms need an SAE (histograms of raw activations are not provided)")
    labels, per_file, C = None, False, 0
    if sel is not None:
        labels, per_file, C, _ = FL._check_args(sae, data_path, layer_name, subset_size, file_labels, frame_labels, n_classes, class_names,
                                                1, "f1")
    fp = FilePass(sae, data_path, layer_name, what="activation histograms", lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    n, T = fp.eng.n, fp.T
    if sel is not None and int(sel.max()) >= n:
        raise ValueError(f"label_latents holds the index {int(sel.max())} >= n_dict={n}")
    with torch.cuda.device(fp.device):
        frame_hist = torch.zeros(n, nb, dtype=torch.int64, device=fp.device)
        file_max_hist = torch.zeros_like(frame_hist)
        n_frames = torch.zeros(1, dtype=torch.int64, device=fp.device)
        sel_dev = lhist = lcount = None
        if sel is not None:
            sel_dev = torch.from_numpy(sel.astype(np.int32)).to(fp.device)
            lhist = torch.zeros(sel.size, C + 1, nb, dtype=torch.int64, device=fp.device)
            lcount = torch.zeros(C + 1, dtype=torch.int64, device=fp.device)
        for x, file0, nbf, lb in fp:
            lab = FL.batch_labels(labels, per_file, file0, nbf, T, fp.device) if sel is not None else None
            fp.eng.hist_files(x, spec, frame_hist, file_max_hist, n_frames, lb, lab, C, sel_dev, lhist, lcount)
        counted = int(n_frames.item())
        res = ActivationHistograms(fp.n_frames, fp.n_total, spec, frame_hist.cpu().numpy(), file_max_hist.cpu().numpy(),
                                   None if sel is None else lhist.cpu().numpy(), sel, None if sel is None else lcount.cpu().numpy(),
                                   None if class_names is None else [str(s) for s in class_names])
    fp.check_counted(counted)
    return res


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Value histograms of every latent of an SAE over a shard directory.")
    add_pass_arguments(ap)
    ap.add_argument("--lo_exp", type=int, default=-12)
    ap.add_argument("--octaves", type=int, default=24)
    ap.add_argument("--sub_bits", type=int, default=2)
    ap.add_argument("--label_latents", default=None, help="comma-separated latent indices whose histogram is split by label")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--file_labels", default=None, help=".npy of int class ids [n_files] or [n_files, S] (-1 = none)")
    g.add_argument("--frame_labels", default=None, help=".npy of int class ids [n_files, T] or [n_files, T, S] (-1 = none)")
    ap.add_argument("--class_names", default=None, help=".json list of the class names")
    a = ap.parse_args(argv)
    names = None
    if a.class_names:
        with open(a.class_names) as f:
            names = json.load(f)
    run_pass_cli(a, lambda lengths: activation_histograms(
        a.sae, a.data_path, a.layer_name, lo_exp=a.lo_exp, octaves=a.octaves, sub_bits=a.sub_bits, lengths=lengths,
        batch_files=a.batch_files, label_latents=[int(v) for v in a.label_latents.split(",")] if a.label_latents else None,
        file_labels=np.load(a.file_labels, mmap_mode="r") if a.file_labels else None,
        frame_labels=np.load(a.frame_labels, mmap_mode="r") if a.frame_labels else None, class_names=names))


if __name__ == "__main__":
    main()
