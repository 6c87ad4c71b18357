"""File features: for EVERY file at once, the answer of the reference's `top_activations_for_audio` (src/utils/activations.py:135-209,
served to the GUI as /top_features) -- the top-N latents that describe a file, with their maxima and times.  It is the
transpose of the feature search's FeatureAtlas (feature_search.py: latent -> files).

The reference answers for one uploaded file at a time, with a Python loop over the frames that sorts a growing list once per
frame.  Here one pass over the Whisper-activation shards does all files: per batch the engine leaves one 64-bit key per
(file, latent) -- the maximum of the trimmed series and its first frame (sae_search_files; the L1 latent is never written) -- and
one more kernel selects each file's top N across its latents (include/freud_sae.h, sae_file_top_features) straight into the rows of
a device table that the host reads back once at the end.

Semantics.  A latent's value in a file is the maximum of its trimmed series, its frame the first frame of that maximum.  A
file's answer is ordered by value descending, then the earlier frame (the reference's stable sort over the frames in order), then
the lower latent index (the reference leaves that last case to torch.topk's order within a frame).  One deliberate difference, for
SAEs only: latents whose value is not > 0 are not reported -- the reference pads a short answer with zero-valued latents that
torch.topk picks among ties.  Raw mode (no SAE) reports signed values as they are.  Unused slots hold latent -1, frame -1 and NaN.

    python -m freud_amd.file_features --sae CKPT|none --data_path DIR --layer_name L --n_top N [--lengths f.npy]
        [--batch_files B] --out file_features.npz
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import List, Optional, Union

import numpy as np
import torch

from .feature_search import TIMESTEP_S, _series, unord
from .engine import FILE_TOP_MAX
from .file_pass import FilePass, add_pass_arguments, keep_rng, resolve_sae


@dataclasses.dataclass
class FileFeatures:
    """latents / values / frames / times: [n_files, n_top], best first; empty slots have latent -1, frame -1, value and time NaN."""
    latents: np.ndarray
    values: np.ndarray
    frames: np.ndarray
    times: np.ndarray
    filenames: List[str]

    def top(self, file: Union[int, str]):
        """[(latent, value, time)] of one file (an index or a file name), best first."""
        f = self.filenames.index(file) if isinstance(file, str) else int(file)
        out = []
        for j, v, t in zip(self.latents[f], self.values[f], self.times[f]):
            if j < 0:
                break
            out.append((int(j), float(v), float(t)))
        return out

    def to_npz(self, path: str) -> None:
        np.savez(path, latents=self.latents, values=self.values, frames=self.frames, times=self.times,
                 filenames=np.array(self.filenames, dtype=str))

    @classmethod
    def from_npz(cls, path: str) -> "FileFeatures":
        with np.load(path) as z:
            return cls(z["latents"], z["values"], z["frames"], z["times"], [str(s) for s in z["filenames"]])


def decode_file_table(top_latents: np.ndarray, top_keys: np.ndarray):
    """[F, N] latents (int32, -1 empty) / file keys of sae_file_top_features -> latents int64, values fp32, frames int64, times."""
    k = np.ascontiguousarray(top_keys).view(np.uint64)
    latents = top_latents.astype(np.int64)
    empty = latents < 0
    values = unord((k >> np.uint64(32)).astype(np.uint32))
    values = np.where(empty, np.float32(np.nan), values).astype(np.float32)
    frames = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
    frames[empty] = -1
    times = np.where(empty, np.nan, frames.astype(np.float64) * TIMESTEP_S)
    return latents, values, frames, times


def _check_n_top(n_top) -> int:
    n_top = int(n_top)
    if n_top < 1 or n_top > FILE_TOP_MAX:
        raise ValueError(f"n_top={n_top} outside [1, {FILE_TOP_MAX}]")
    return n_top


@keep_rng
def file_features(sae, data_path: str, layer_name: str, n_top: int, *, lengths=None, subset_size: Optional[int] = None,
                  batch_files: Optional[int] = None) -> FileFeatures:
    """The top n_top latents of `sae` (None: the columns of the activations themselves) for every file, in one pass.
    batch_files: files per engine call (default: file_pass.default_batch_files)."""
    from . import engine as E

    n_top = _check_n_top(n_top)
    fp = FilePass(sae, data_path, layer_name, what="file features", lengths=lengths, subset_size=subset_size, batch_files=batch_files)
    eng, dev, n_total = fp.eng, fp.device, fp.n_total
    raw = eng is None
    ncols = fp.d if raw else eng.n
    flags = 0 if raw else E.FILE_TOP_POSITIVE
    with torch.cuda.device(dev):
        keys = torch.empty(fp.batch_files * ncols, dtype=torch.int64, device=dev)
        top_latents = torch.full((n_total, n_top), -1, dtype=torch.int32, device=dev)
        top_keys = torch.zeros(n_total, n_top, dtype=torch.int64, device=dev)
        for x, file0, nb, lb in fp:
            if raw:
                E.search_raw_files(x, keys, None, lb)
            else:
                eng.search_files(x, keys, lb)
            E.file_top_features(keys, nb, ncols, n_top, flags, top_latents[file0:file0 + nb], top_keys[file0:file0 + nb])
        tl = top_latents.cpu().numpy()                            # the one read-back
        tk = top_keys.cpu().numpy()
    return FileFeatures(*decode_file_table(tl, tk), fp.filenames)


@keep_rng
def top_activations_for_file(sae, x, top_n: int, length: Optional[int] = None):
    """activations.py:135-209 with the reference's return shape, for one file's Whisper activations x [T, d] (a tensor or an array;
    this project does not run Whisper): (activation_indexes best first, max_activations: their trimmed series, fp32 CPU [L]).
    length: the file's frames (the reference's activation_length_from_audio_array), capped at T; default T."""
    from . import engine as E

    top_n = _check_n_top(top_n)
    x = torch.as_tensor(x)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        x = x.float()
    if x.dim() == 3 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 2:
        raise ValueError(f"x must be one file's activations [T, d], got {tuple(x.shape)}")
    T = int(x.shape[0])
    L = T if length is None else int(length)
    if L < 1:
        raise ValueError(f"length={L} must be >= 1: an empty series has no maximum")
    L = min(L, T)
    model, eng = resolve_sae(sae)
    if eng is not None:
        raise TypeError("top_activations_for_file needs a freud_amd.models SAE (or None) to return the series")
    if model is not None and model.activation_size != int(x.shape[1]):
        raise ValueError(f"the SAE expects d_model={model.activation_size}, x holds d={int(x.shape[1])}")
    if not torch.cuda.is_available():
        raise RuntimeError("the file features run on the GPU (HIP engine); there is no CPU path")
    dev = model.device if model is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        x = x.to(dev).contiguous()
        lb = torch.tensor([L], dtype=torch.int32, device=dev)
        if model is None:
            ncols, flags = int(x.shape[1]), 0
            keys = torch.empty(ncols, dtype=torch.int64, device=dev)
            E.search_raw_files(x[None], keys, None, lb)
        else:
            ncols, flags = model.n_dict_components, E.FILE_TOP_POSITIVE
            keys = torch.empty(ncols, dtype=torch.int64, device=dev)
            model._ensure(-(-T // 256) * 256).search_files(x[None], keys, lb)
        top_latents = torch.empty(top_n, dtype=torch.int32, device=dev)
        top_keys = torch.empty(top_n, dtype=torch.int64, device=dev)
        E.file_top_features(keys, 1, ncols, top_n, flags, top_latents, top_keys)
        latents, values, _frames, _times = decode_file_table(top_latents.cpu().numpy()[None], top_keys.cpu().numpy()[None])
        indexes = [int(j) for j in latents[0] if j >= 0]
        series = _series(model, None, x, indexes)[:L]            # one encode() of the file, then a column gather
    max_activations = []
    for r, (j, v) in enumerate(zip(indexes, values[0])):
        act = series[:, r].contiguous()
        # the reference's sanity check (activations.py:204-206), kept as a real check
        if float(act.max()) != float(v):
            raise RuntimeError(f"Max activation at index {j} is {float(act.max())} but expected {float(v)}")
        max_activations.append(act)
    return indexes, max_activations


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Top-N latents of every file in one pass (the reference's top_activations_for_audio).")
    add_pass_arguments(ap, "checkpoint path, or 'none' for the activations' own columns")
    ap.add_argument("--n_top", type=int, required=True)
    a = ap.parse_args(argv)
    lengths = np.load(a.lengths) if a.lengths else None
    ff = file_features(None if a.sae.lower() == "none" else a.sae, a.data_path, a.layer_name, a.n_top, lengths=lengths,
                       batch_files=a.batch_files)
    ff.to_npz(a.out)
    print(f"{a.out}: {ff.latents.shape[0]} files x top {ff.latents.shape[1]}, {int((ff.latents >= 0).sum())} latents reported")


if __name__ == "__main__":
    main()
