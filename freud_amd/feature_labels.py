"""Feature labels: which latents of a trained dictionary detect which labels of the data -- an ESC-50 class per file, a speaker, the
phoneme of every 20 ms frame -- and what a latent detects, with precision and recall, in one pass over the Whisper-activation
shards (without it: encode() of every file, a threshold, and a dense float onehot.T @ mask in torch).

Semantics (include/freud_sae.h, sae_label_files / sae_label_keys).  Frames count exactly as in the feature statistics and the
co-activation: the first min(L[f], T) frames of file f when `lengths` is given (file_pass.check_lengths rules), all T otherwise.
Latent j is active on a frame iff the value freud_amd.models encode() returns for it is > 0 (a -0.0 and a selected zero of a TopK
row are not active; a multi_topk model uses its k selection).  Every frame carries up to S distinct class ids in [0, C) in S slots,
-1 = an empty slot; 1 <= S <= 16, 1 <= C <= 4096.  A[l][j] is the number of counted frames that carry label l and on which latent j
is active, label_count[l] the number of counted frames that carry l, fire_count[j] the number on which j is active (the fire_count
of feature_stats, the diagonal of the co-activation table); int32 counts (a pass over more than 2^31 - 1 frames is refused).
Scores for A[l][j] > 0, one fp64 division converted once to fp32:

    f1          2 A / (fire_count[j] + label_count[l])
    precision   A / fire_count[j]                          P(l | j active)
    recall      A / label_count[l]                         P(j active | l)
    count       A

Two answers: per label its best latents, per latent its best labels, both ordered by score descending, then the larger count, then
the lower index.  A pair that never meets is not reported; empty slots hold -1, count 0 and score NaN.  Everything is exact integer
arithmetic on the i8 matrix cores: two runs give bitwise identical arrays.

Out of scope: per-label activation sums or means (floats; counts only here -- the DISTRIBUTION of a latent's value per label, in
exact integer bins, is freud_amd.activation_hist's label_latents), labels for raw (no-SAE) activations, and deriving
the labels from file names or alignments (the caller's job).

    python -m freud_amd.feature_labels --sae CKPT --data_path DIR --layer_name L (--file_labels f.npy | --frame_labels f.npy)
                                       [--class_names names.json] [--n_top K] [--measure M] [--lengths f.npy] [--batch_files B]
                                       [--counts] --out labels.npz
"""
from __future__ import annotations

import argparse
import dataclasses
import json
from typing import List, Optional, Union

import numpy as np
import torch

from . import coactivation as CO
from . import engine as E
from .engine import FILE_TOP_MAX, LABEL_MAX_CLASSES, LABEL_MAX_SLOTS, LABEL_MEASURES
from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

MAX_FRAMES = 2 ** 31 - 1          # int32 counts
_SCAN_ELEMS = 1 << 24             # label ids checked per slice of a (possibly memory-mapped) label array
_FIELDS = ("label_count", "fire_count", "label_latents", "label_counts", "label_scores", "latent_labels", "latent_counts",
           "latent_scores")


@dataclasses.dataclass
class FeatureLabels:
    """Label association of an SAE's latents over a dataset (see the module docstring)."""
    n_frames: int
    label_count: np.ndarray           # int64 [C]: counted frames that carry the label
    fire_count: np.ndarray            # int64 [n]: counted frames on which the latent is active
    label_latents: np.ndarray         # int64 [C, K]: a label's best latents, -1 = empty
    label_counts: np.ndarray          # int64 [C, K], 0 = empty
    label_scores: np.ndarray          # float32 [C, K], NaN = empty
    latent_labels: np.ndarray         # int64 [n, min(K, C)]: a latent's best labels, -1 = empty
    latent_counts: np.ndarray         # int64 [n, min(K, C)]
    latent_scores: np.ndarray         # float32 [n, min(K, C)]
    matrix: Optional[np.ndarray] = None   # int32 [C, n] (return_counts) or None
    measure: str = "f1"
    class_names: Optional[List[str]] = None

    @property
    def n_classes(self) -> int:
        return int(self.label_count.shape[0])

    @property
    def n_latents(self) -> int:
        return int(self.fire_count.shape[0])

    def label_id(self, label: Union[int, str]) -> int:
        if isinstance(label, str):
            if self.class_names is None or label not in self.class_names:
                raise KeyError(f"no class named {label!r}")
            return self.class_names.index(label)
        return int(label)

    def top_latents(self, label: Union[int, str]):
        """The best latents of a label (id or name), best first: [(latent, count, score)]."""
        l = self.label_id(label)
        return [(int(p), int(c), float(s)) for p, c, s in zip(self.label_latents[l], self.label_counts[l], self.label_scores[l]) if p >= 0]

    def top_labels(self, latent: int):
        """The best labels of a latent, best first: [(label id, count, score)]."""
        j = int(latent)
        return [(int(p), int(c), float(s)) for p, c, s in zip(self.latent_labels[j], self.latent_counts[j], self.latent_scores[j]) if p >= 0]

    def summary(self) -> dict:
        has = self.label_latents[:, 0] >= 0
        best = self.label_scores[:, 0][has]
        return {"n_frames": int(self.n_frames), "n_classes": self.n_classes, "n_latents": self.n_latents,
                "n_top": int(self.label_latents.shape[1]), "measure": self.measure, "labels_seen": int((self.label_count > 0).sum()),
                "labels_with_latents": int(has.sum()), "latents_with_labels": int((self.latent_labels[:, 0] >= 0).sum()),
                "dead": int((self.fire_count == 0).sum()), "max_score": float(best.max()) if best.size else None}

    def to_npz(self, path: str) -> None:
        extra = {} if self.matrix is None else {"matrix": self.matrix}
        if self.class_names is not None:
            extra["class_names"] = np.array(self.class_names, dtype=str)
        np.savez(path, n_frames=np.int64(self.n_frames), measure=np.array(self.measure), **{k: getattr(self, k) for k in _FIELDS}, **extra)

    @classmethod
    def from_npz(cls, path: str) -> "FeatureLabels":
        with np.load(path) as z:
            names = [str(s) for s in z["class_names"]] if "class_names" in z.files else None
            return cls(int(z["n_frames"]), *(z[k] for k in _FIELDS), z["matrix"] if "matrix" in z.files else None, str(z["measure"]), names)


def _scan_ids(a: np.ndarray):
    """(min id, max id) of a label array [..., S] and a ValueError for a frame whose slots repeat an id; read in slices of its first axis."""
    lo, hi = 0, -1
    step = max(1, _SCAN_ELEMS // max(1, int(np.prod(a.shape[1:]))))
    for i in range(0, a.shape[0], step):
        blk = np.asarray(a[i:i + step])
        if blk.size == 0:
            continue
        lo, hi = min(lo, int(blk.min())), max(hi, int(blk.max()))
        if blk.shape[-1] > 1:
            srt = np.sort(blk, axis=-1)
            dup = (srt[..., 1:] == srt[..., :-1]) & (srt[..., 1:] >= 0)
            if dup.any():
                at = tuple(int(v) + (i if k == 0 else 0) for k, v in enumerate(np.argwhere(dup.any(-1))[0]))
                raise ValueError(f"duplicate label ids within the slots of one frame (at {at})")
    return lo, hi


def _check_args(sae, data_path, layer_name, subset_size, file_labels, frame_labels, n_classes, class_names, n_top, measure):
    """Every argument rule that needs no SAE and no device -> (labels as [n_files, S] or [n_files, T, S], per_file, n_classes, n_top)."""
    from .loader import MemoryMappedActivationsDataset

    if is_raw(sae):
        raise ValueError("feature labels need an SAE (labels for raw activations are not provided)")
    n_top = int(n_top)
    if n_top < 1 or n_top > FILE_TOP_MAX:
        raise ValueError(f"n_top={n_top} outside [1, {FILE_TOP_MAX}]")
    if measure not in LABEL_MEASURES:
        raise ValueError(f"measure={measure!r} is not one of {sorted(LABEL_MEASURES)}")
    if (file_labels is None) == (frame_labels is None):
        raise ValueError("give exactly one of file_labels and frame_labels")
    per_file = file_labels is not None
    a = file_labels if per_file else frame_labels
    name = "file_labels" if per_file else "frame_labels"
    if not isinstance(a, np.ndarray):
        a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be integers, got {a.dtype}")
    ds = MemoryMappedActivationsDataset(data_path, layer_name, subset_size)
    n_files, T = len(ds), int(ds.tensor_shape[-2])
    base = (n_files,) if per_file else (n_files, T)
    if a.ndim not in (len(base), len(base) + 1) or tuple(a.shape[:len(base)]) != base:
        want = "[n_files] or [n_files, S]" if per_file else "[n_files, T] or [n_files, T, S]"
        raise ValueError(f"{name} must be {want} with n_files={n_files}" + ("" if per_file else f", T={T}") + f", got shape {a.shape}")
    if a.ndim == len(base):
        a = a.reshape(*base, 1)
    S = int(a.shape[-1])
    if S < 1 or S > LABEL_MAX_SLOTS:
        raise ValueError(f"{S} label slots outside [1, {LABEL_MAX_SLOTS}]")
    lo, hi = _scan_ids(a)
    if lo < -1:
        raise ValueError(f"{name} holds the id {lo}: ids are >= 0, or -1 for an empty slot")
    n_classes = hi + 1 if n_classes is None else int(n_classes)
    if n_classes < 1 or n_classes > LABEL_MAX_CLASSES:
        raise ValueError(f"n_classes={n_classes} outside [1, {LABEL_MAX_CLASSES}]")
    if hi >= n_classes:
        raise ValueError(f"{name} holds the id {hi} >= n_classes={n_classes}")
    if class_names is not None and len(class_names) != n_classes:
        raise ValueError(f"{len(class_names)} class_names for n_classes={n_classes}")
    return a, per_file, n_classes, n_top


def batch_labels(labels: np.ndarray, per_file: bool, file0: int, nb: int, T: int, device) -> torch.Tensor:
    """The labels of files [file0, file0 + nb) as the engine takes them: contiguous int32 [nb, T, S] on `device`, per-file labels
    expanded to every frame of their file (`labels`, `per_file`: what _check_args returns)."""
    S = int(labels.shape[-1])
    lab = torch.from_numpy(np.ascontiguousarray(labels[file0:file0 + nb], dtype=np.int32)).to(device)
    if per_file:
        lab = lab.reshape(nb, 1, S).expand(nb, T, S)
    return lab.reshape(nb, T, S).contiguous()


@keep_rng
def feature_labels(sae, data_path: str, layer_name: str, *, file_labels=None, frame_labels=None, n_classes: Optional[int] = None,
                   class_names=None, n_top: int = 16, measure: str = "f1", lengths=None, subset_size: Optional[int] = None,
                   batch_files: Optional[int] = None, return_counts: bool = False) -> FeatureLabels:
    """Label counts of every (label, latent) of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over
    the files of a shard directory, every label's n_top best latents and every latent's min(n_top, C) best labels by `measure`.
    Exactly one of file_labels (int [n_files] or [n_files, S]: the labels of all frames of a file) and frame_labels (int
    [n_files, T] or [n_files, T, S]); both may be np.memmap and reach the device one batch at a time.  n_classes: default max id
    + 1.  class_names: C names, kept in the result.  return_counts: also the int32 matrix [C, n] on the host.  batch_files: files
    per engine call (default: file_pass.default_batch_files)."""
    labels, per_file, C, n_top = _check_args(sae, data_path, layer_name, subset_size, file_labels, frame_labels, n_classes, class_names,
                                             n_top, measure)
    # (the counts are int32: FilePass refuses more than MAX_FRAMES frames before it loads the SAE or touches the device)
    fp = FilePass(sae, data_path, layer_name, what="feature labels", lengths=lengths, subset_size=subset_size, batch_files=batch_files,
                  max_frames=MAX_FRAMES)
    n, T = fp.eng.n, fp.T
    m = LABEL_MEASURES[measure]
    with torch.cuda.device(fp.device):
        table = torch.zeros(C + 1, n, dtype=torch.int32, device=fp.device)
        lcount = torch.zeros(C + 1, dtype=torch.int64, device=fp.device)
        for x, file0, nb, lb in fp:
            fp.eng.label_files(x, batch_labels(labels, per_file, file0, nb, T, fp.device), C, table, lcount, lb)
        by_label = CO.select_top_rows(C, n, n_top, lambda r0, nr, keys: E.label_keys(table, lcount, C, n, m, False, r0, nr, keys), fp.device)
        by_latent = CO.select_top_rows(n, C, min(n_top, C), lambda r0, nr, keys: E.label_keys(table, lcount, C, n, m, True, r0, nr, keys),
                                       fp.device)
        counts = lcount.cpu().numpy()
        fire = table[C].to(torch.int64).cpu().numpy()
        matrix = table[:C].cpu().numpy() if return_counts else None
    fp.check_counted(counts[C])
    return FeatureLabels(fp.n_frames, counts[:C].copy(), fire, *by_label, *by_latent, matrix, measure,
                         None if class_names is None else [str(s) for s in class_names])


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Which latents of an SAE detect which labels over a shard directory.")
    add_pass_arguments(ap)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--file_labels", default=None, help=".npy of int class ids [n_files] or [n_files, S] (-1 = none)")
    g.add_argument("--frame_labels", default=None, help=".npy of int class ids [n_files, T] or [n_files, T, S] (-1 = none)")
    ap.add_argument("--class_names", default=None, help=".json list of the class names")
    ap.add_argument("--n_top", type=int, default=16)
    ap.add_argument("--measure", default="f1", choices=sorted(LABEL_MEASURES))
    ap.add_argument("--counts", action="store_true", help="also store the int32 count matrix [C, n]")
    a = ap.parse_args(argv)
    names = None
    if a.class_names:
        with open(a.class_names) as f:
            names = json.load(f)
    run_pass_cli(a, lambda lengths: feature_labels(a.sae, a.data_path, a.layer_name,
                                                   file_labels=np.load(a.file_labels, mmap_mode="r") if a.file_labels else None,
                                                   frame_labels=np.load(a.frame_labels, mmap_mode="r") if a.frame_labels else None,
                                                   class_names=names, n_top=a.n_top, measure=a.measure, lengths=lengths,
                                                   batch_files=a.batch_files, return_counts=a.counts))


if __name__ == "__main__":
    main()
