"""Feature search: for EVERY latent at once, the answer of the reference's `top_activations` (src/utils/activations.py:61-132,
served to the GUI by gui_server.py:91-99) -- the top-N files by the maximum of the latent's (trimmed) series, with that maximum
and its time.

The reference needs the SAE activations collected to disk first (collect_activations.py with sae_model: a dense fp32 [1500, n]
row per file for L1) and then makes one full pass over that dataset PER LATENT.  Here one pass over the Whisper-activation shards
does all latents: the engine encodes a batch of files with the training kernels and keeps only per-(file, latent) maxima (the
L1 latent is never written: include/freud_sae.h, sae_search_files), merges them into a per-latent top-N table on the device
(sae_search_merge) and the host reads the table back once at the end.

Semantics are the reference's, including its quirks: the trim to int(duration / TIMESTEP_S) frames (here: `lengths`, since
durations come from audio files that this project does not decode), the first maximal frame, the filter
min_val <= value <= max_val, the stable order (value descending, file ascending; a file that ties the N-th is dropped), and in
absolute_magnitude mode the signed value at argmax |a| filtered, |value| ranked, but the time of the SIGNED argmax returned
(activations.py:106-121).

    python -m freud_amd.feature_search --sae CKPT|none --data_path DIR --layer_name L --n_files N [--absolute]
        [--min_val V] [--max_val V] [--lengths file.npy] --out atlas.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import List, Optional, Sequence

import numpy as np
import torch

from .file_pass import FilePass, add_pass_arguments, check_lengths, default_batch_files, keep_rng, resolve_sae    # noqa: F401 (re-exported)

TIMESTEP_S = 30 / 1500          # src/utils/constants.py:17


@dataclasses.dataclass
class FeatureAtlas:
    """values / file_idx / frames / times: [n_latents, n_files]; empty slots have file_idx -1, frame -1, value and time NaN.
    max_per_file: [len(max_per_file_features), number of files] (the signed value in abs mode), or None."""
    values: np.ndarray
    file_idx: np.ndarray
    frames: np.ndarray
    times: np.ndarray
    filenames: List[str]
    max_per_file: Optional[np.ndarray] = None
    max_per_file_features: Optional[np.ndarray] = None

    def top(self, feature_idx: int):
        """[(filename, value, time)] of one latent, best first (the reference's pq without the series)."""
        out = []
        for v, f, t in zip(self.values[feature_idx], self.file_idx[feature_idx], self.times[feature_idx]):
            if f < 0:
                break
            out.append((self.filenames[int(f)], float(v), float(t)))
        return out

    def to_npz(self, path: str) -> None:
        arrays = dict(values=self.values, file_idx=self.file_idx, frames=self.frames, times=self.times,
                      filenames=np.array(self.filenames, dtype=str))
        if self.max_per_file is not None:
            arrays["max_per_file"] = self.max_per_file
            arrays["max_per_file_features"] = self.max_per_file_features
        np.savez(path, **arrays)


def unord(o: np.ndarray) -> np.ndarray:
    """Inverse of search_keys.h's order-preserving float map (uint32 -> float32)."""
    o = np.asarray(o, dtype=np.uint32)
    u = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return u.view(np.float32)


def decode_table(top_keys: np.ndarray, top_frames: np.ndarray):
    """[N, n] rank keys / frames of sae_search_merge -> values [n, N] fp32, file indices [n, N] int64 (-1 empty), frames, times."""
    r = np.ascontiguousarray(top_keys).view(np.uint64)
    empty = r == 0
    values = unord((r >> np.uint64(32)).astype(np.uint32))
    files = (np.uint64(0xFFFFFFFF) - (r & np.uint64(0xFFFFFFFF))).astype(np.int64)
    frames = top_frames.astype(np.int64)
    values = np.where(empty, np.float32(np.nan), values).astype(np.float32)
    files[empty] = -1
    frames[empty] = -1
    times = np.array([[f * TIMESTEP_S if f >= 0 else float("nan") for f in row] for row in frames.T.tolist()], dtype=np.float64)
    return values.T.copy(), files.T.copy(), frames.T.copy(), times


@keep_rng
def search_features(sae, data_path: str, layer_name: str, n_files: int, *, absolute_magnitude: bool = False,
                    min_val: Optional[float] = None, max_val: Optional[float] = None, lengths=None,
                    subset_size: Optional[int] = None, batch_files: Optional[int] = None,
                    max_per_file_features: Optional[Sequence[int]] = None) -> FeatureAtlas:
    """top_activations for every latent of `sae` (None: every column of the activations themselves) in one pass.
    batch_files: files per engine call (default: default_batch_files)."""
    from . import engine as E

    n_files = int(n_files)
    if n_files < 1 or n_files > E.SEARCH_MAX_TOP:
        raise ValueError(f"n_files={n_files} outside [1, {E.SEARCH_MAX_TOP}]")
    fp = FilePass(sae, data_path, layer_name, what="feature search", lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    eng, dev, n_total = fp.eng, fp.device, fp.n_total
    raw = eng is None
    ncols = fp.d if raw else eng.n
    flags = (E.SEARCH_ABS if absolute_magnitude else 0) | (E.SEARCH_MIN if min_val is not None else 0) | \
            (E.SEARCH_MAX if max_val is not None else 0)
    feats = None
    if max_per_file_features is not None:
        feats = np.asarray(list(max_per_file_features), dtype=np.int64)
        if feats.size == 0 or feats.min() < 0 or feats.max() >= ncols:
            raise ValueError(f"max_per_file_features must be latent indices in [0, {ncols})")

    with torch.cuda.device(dev):
        keys = torch.empty(fp.batch_files * ncols, dtype=torch.int64, device=dev)
        aux = torch.empty(fp.batch_files * ncols, dtype=torch.int64, device=dev) if (raw and absolute_magnitude) else None
        top_keys = torch.zeros(n_files * ncols, dtype=torch.int64, device=dev)
        top_frames = torch.zeros(n_files * ncols, dtype=torch.int32, device=dev)
        feats_dev = torch.from_numpy(feats.astype(np.int32)).to(dev) if feats is not None else None
        per_file = torch.zeros(len(feats), n_total, dtype=torch.float32, device=dev) if feats is not None else None
        for x, file0, nb, lb in fp:
            if raw:
                E.search_raw_files(x, keys, aux, lb, absolute=absolute_magnitude)
            else:
                eng.search_files(x, keys, lb)
            E.search_merge(keys, aux, nb, ncols, file0, n_files, flags, 0.0 if min_val is None else float(min_val),
                           0.0 if max_val is None else float(max_val), top_keys, top_frames)
            if feats is not None:
                E.search_file_values(keys, aux, nb, ncols, flags, feats_dev, file0, per_file)
        tk = top_keys.view(n_files, ncols).cpu().numpy()          # the one read-back
        tf = top_frames.view(n_files, ncols).cpu().numpy()
        pf = per_file.cpu().numpy() if per_file is not None else None
    values, files, frames, times = decode_table(tk, tf)
    return FeatureAtlas(values, files, frames, times, fp.filenames, pf, feats)


def _series(sae_model, eng, x: torch.Tensor, feature_idx) -> torch.Tensor:
    """The latent's series over one file's rows [T, d] -- encode() of freud_amd.models (or x's own column in raw mode).
    feature_idx: one index -> [T]; a sequence of indices -> [T, len] from ONE encode() (file_features.py)."""
    many = not isinstance(feature_idx, (int, np.integer))
    if many:
        feature_idx = [int(j) for j in feature_idx]
    if sae_model is None and eng is None:
        return x[:, feature_idx].float().cpu()
    if sae_model is None:
        raise TypeError("top_activations needs a freud_amd.models SAE (or None) to re-encode the winning files")
    if sae_model._variant == "l1":
        return sae_model.encode(x).latent[:, feature_idx].float().cpu()
    enc = sae_model.encode(x)                       # activation_tensor_from_indexed (activations.py:41-58)

    def column(j):
        dense = torch.zeros(x.shape[0], dtype=torch.float32, device=enc.top_acts.device)
        hit = enc.top_indices == j
        dense += (enc.top_acts.float() * hit).sum(dim=1)
        return dense.cpu()

    if not many:
        return column(feature_idx)
    return torch.stack([column(j) for j in feature_idx], dim=1) if feature_idx else torch.zeros(x.shape[0], 0)


@keep_rng
def top_activations(sae, data_path: str, layer_name: str, feature_idx: int, n_files: int, max_val: Optional[float],
                    min_val: Optional[float], absolute_magnitude: bool, return_max_per_file: bool, lengths=None):
    """activations.py:61-132 with the reference's return shape: ([(audio_file, trimmed series, value, time)], max_per_file or None).
    The series are re-encoded for the winning files only."""
    from .loader import MemoryMappedActivationsDataset, require_directory
    require_directory(data_path)                # (the winners' series are read from the files below)
    model, eng = resolve_sae(sae)
    atlas = search_features(model if model is not None else eng, data_path, layer_name, n_files, absolute_magnitude=absolute_magnitude,
                            min_val=min_val, max_val=max_val, lengths=lengths,
                            max_per_file_features=[feature_idx] if return_max_per_file else None)
    ds = MemoryMappedActivationsDataset(data_path, layer_name)
    T = int(ds.tensor_shape[-2])
    lens = check_lengths(lengths, len(ds), T)
    dev = model.device if model is not None else torch.device("cuda", torch.cuda.current_device())
    pq = []
    for value, t, f in zip(atlas.values[feature_idx], atlas.times[feature_idx], atlas.file_idx[feature_idx]):
        if f < 0:
            break
        x, fname = ds[int(f)]
        L = T if lens is None else int(lens[int(f)])
        series = _series(model, eng, x.to(dev), feature_idx)[:L]
        pq.append((fname, series, float(value), float(t)))
    mpf = [float(v) for v in atlas.max_per_file[0]] if return_max_per_file else None
    return pq, mpf


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Top-N files of every latent in one pass (the reference's top_activations).")
    add_pass_arguments(ap, "checkpoint path, or 'none' for the activations' own columns")
    ap.add_argument("--n_files", type=int, required=True)
    ap.add_argument("--absolute", action="store_true")
    ap.add_argument("--min_val", type=float, default=None)
    ap.add_argument("--max_val", type=float, default=None)
    a = ap.parse_args(argv)
    lengths = np.load(a.lengths) if a.lengths else None
    atlas = search_features(None if a.sae.lower() == "none" else a.sae, a.data_path, a.layer_name, a.n_files,
                            absolute_magnitude=a.absolute, min_val=a.min_val, max_val=a.max_val, lengths=lengths,
                            batch_files=a.batch_files)
    atlas.to_npz(a.out)
    print(f"{a.out}: {atlas.values.shape[0]} latents x top {atlas.values.shape[1]} over {len(atlas.filenames)} files")


if __name__ == "__main__":
    main()
