"""Feature collection: the SAE features of a dataset written as the reference's indexed feature shards, in one GPU pass over the
cached layer activations.  The reference does this with collect_activations.py and `sae_model` set: it runs Whisper on the audio
again, encodes, and appends <layer>_activation_values.npy + <layer>_feature_indices.npy + <layer>_metadata.json, which its
MemoryMappedActivationsDataset reads back as activation_type == "indexed" and gui_server.py searches.  Here the layer activations
are already on disk: collection is one encode per row and a per-row select, no Whisper, no audio.

Semantics (include/freud_sae.h, sae_collect_files; freud_amd/csrc/collect.h).  All T frames of every file are stored (the reference
collects untrimmed and trims at search time).  With a the latent row exactly as freud_amd.models encode() returns it (TopK: the
scatter of the k selection), a row's K slots are numpy.argsort(-a, kind="stable")[:K]: value descending, equal values by the lower
column.  Slots are sorted, so the first K' slots of a row are its top K' and a store can be truncated by prefix; a row with fewer
than K positive latents is padded with zero-valued latents in increasing column order (stored as +0.0), so the indices of a row are
always distinct, which the reference's activation_tensor_from_indexed needs.  TopK: K defaults to the model's k and the store is
the selection itself, canonically ordered.  L1: K has no default -- the L0 histogram of freud_amd.feature_stats says how many
latents a row fires -- and the report says what, if anything, was cut: the store equals the latent iff `dropped` is 0.

Files, in the reference's format: <out>/<layer>_activation_values.npy (float32 [n_files, T * K]), <out>/<layer>_feature_indices.npy
(int64, or int32 with index_dtype="int32"; the reference's reader takes either), <out>/<layer>_metadata.json with the reference's
keys tensor_shape = [T, K], activation_shape = [T, n_dict], filenames, and one more key, "freud_amd", that the reference ignores:
the variant, K, "sorted": true, the index dtype and the eight statistics.  They are written under temporary names and renamed at
the end, metadata last: an interrupted run leaves nothing that loads as a store.  layout="tensor" (L1 only) writes the reference's
own dense form instead, <layer>_tensors.npy as float32 [n_files, T * n_dict].

Refused before the GPU is touched: an out_folder that is data_path; an out_folder that already holds <layer>_tensors.npy when an
indexed store is asked for (the reference's loader would prefer it and never see the store); an out_folder that already holds a
store unless overwrite is set.

Out of scope: raw (no-SAE) collection -- that is the shards themselves; fp8 contexts; trimming by audio length; compressed values.

    python -m freud_amd.collect_features --config configs/features/NAME.json [--k K] [--index-dtype int64|int32]
                                         [--layout indexed|tensor] [--overwrite]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
from typing import Iterable, List, Optional, Tuple

import numpy as np

from .engine import COLLECT_MAX_K, _alias

STAT_NAMES = ("rows", "stored", "dropped", "rows_dropped", "max_active", "largest_dropped_bits", "reserved6", "reserved7")
_INDEX_DTYPES = {"int64": np.int64, "int32": np.int32}
_PARTIAL = ".partial"


def store_paths(folder: str, layer_name: str) -> dict:
    return {"values": os.path.join(folder, f"{layer_name}_activation_values.npy"),
            "indices": os.path.join(folder, f"{layer_name}_feature_indices.npy"),
            "tensors": os.path.join(folder, f"{layer_name}_tensors.npy"),
            "metadata": os.path.join(folder, f"{layer_name}_metadata.json")}


def bf16_bits_to_float(bits: int) -> float:
    return float(np.array([int(bits) << 16], dtype=np.uint32).view(np.float32)[0])


@dataclasses.dataclass
class CollectReport:
    """What a collection wrote and what it cut (see the module docstring)."""
    variant: str
    layout: str
    n_files: int
    T: int
    K: int
    n_dict: int
    index_dtype: str
    rows: int                    # rows collected
    stored: int                  # active latents stored
    dropped: int                 # active latents beyond slot K
    rows_dropped: int            # rows that dropped at least one
    max_active: int              # the largest number of active latents in a row
    largest_dropped: float       # the largest dropped value (0.0 if none)
    complete: bool               # nothing was dropped: the store equals the latent
    paths: dict
    bytes_written: int

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self))


def check_out_folder(data_path: str, out_folder: str, layer_name: str, layout: str, overwrite: bool) -> None:
    """The refusals of a collection; no file is touched."""
    from .loader import require_directory
    require_directory(data_path)                              # (the guard below compares the two folders)
    if os.path.realpath(out_folder) == os.path.realpath(data_path):
        raise ValueError(f"out_folder {out_folder!r} is the shard directory itself: its {layer_name}_metadata.json would be replaced")
    p = store_paths(out_folder, layer_name)
    if layout == "indexed" and os.path.exists(p["tensors"]):
        raise ValueError(f"{p['tensors']} exists: a reader prefers it and would never see the indexed store (remove it or choose another out_folder)")
    held = [p[k] for k in ("values", "indices", "tensors", "metadata") if os.path.exists(p[k])]
    if held and not overwrite:
        raise ValueError(f"{out_folder!r} already holds {', '.join(os.path.basename(h) for h in held)} (overwrite=True replaces them)")


class StoreWriter:
    """The files of one collection.  write() fills the rows of a batch of files; finish() renames the data files into place and
    writes the metadata last.  Until then nothing under out_folder loads as a store.  A folder that already holds a store or a
    <layer>_tensors.npy is refused unless overwrite is set; then they are removed, metadata first, before the first byte is written."""

    def __init__(self, out_folder: str, layer_name: str, filenames: List[str], T: int, K: int, n_dict: int, *, variant: str,
                 index_dtype: str = "int64", layout: str = "indexed", overwrite: bool = False):
        from numpy.lib.format import open_memmap

        if layout not in ("indexed", "tensor"):
            raise ValueError(f"layout={layout!r} is neither 'indexed' nor 'tensor'")
        if index_dtype not in _INDEX_DTYPES:
            raise ValueError(f"index_dtype={index_dtype!r} is neither 'int64' nor 'int32'")
        self.folder, self.layer_name, self.filenames = out_folder, layer_name, [str(f) for f in filenames]
        self.T, self.K, self.n_dict, self.variant, self.index_dtype, self.layout = int(T), int(K), int(n_dict), variant, index_dtype, layout
        self.paths = store_paths(out_folder, layer_name)
        held = [os.path.basename(self.paths[k]) for k in ("metadata", "values", "indices", "tensors") if os.path.exists(self.paths[k])]
        if held and not overwrite:
            raise ValueError(f"{out_folder!r} already holds {', '.join(held)} (overwrite=True removes them)")
        os.makedirs(out_folder, exist_ok=True)
        for key in ("metadata", "values", "indices", "tensors"):      # metadata first: what is left never loads
            for path in (self.paths[key], self.paths[key] + _PARTIAL):
                if os.path.exists(path):
                    os.unlink(path)
        n_files = len(self.filenames)
        self._maps = {}
        if layout == "indexed":
            self._maps["values"] = open_memmap(self.paths["values"] + _PARTIAL, mode="w+", dtype=np.float32, shape=(n_files, self.T * self.K),
                                               version=(1, 0))
            self._maps["indices"] = open_memmap(self.paths["indices"] + _PARTIAL, mode="w+", dtype=_INDEX_DTYPES[index_dtype],
                                                shape=(n_files, self.T * self.K), version=(1, 0))
        else:
            self._maps["tensors"] = open_memmap(self.paths["tensors"] + _PARTIAL, mode="w+", dtype=np.float32,
                                                shape=(n_files, self.T * self.n_dict), version=(1, 0))
        self._written = 0

    def write(self, file0: int, values: np.ndarray, indices: Optional[np.ndarray] = None) -> None:
        nb = int(values.shape[0])
        if self.layout == "indexed":
            self._maps["values"][file0:file0 + nb] = values.reshape(nb, -1)
            self._maps["indices"][file0:file0 + nb] = indices.reshape(nb, -1)
        else:
            self._maps["tensors"][file0:file0 + nb] = values.reshape(nb, -1)
        self._written += nb

    def abort(self) -> None:
        maps, self._maps = self._maps, {}
        for key, m in maps.items():
            del m
            if os.path.exists(self.paths[key] + _PARTIAL):
                os.unlink(self.paths[key] + _PARTIAL)

    def finish(self, stats: np.ndarray) -> int:
        """Flush, rename, write the metadata; returns the bytes written."""
        if self._written != len(self.filenames):
            raise RuntimeError(f"{self._written} of {len(self.filenames)} files were written")
        total = 0
        maps, self._maps = self._maps, {}
        for key, m in maps.items():
            m.flush()
            del m
        for key in maps:
            os.replace(self.paths[key] + _PARTIAL, self.paths[key])
            total += os.path.getsize(self.paths[key])
        stats = [int(v) for v in stats]
        width = self.K if self.layout == "indexed" else self.n_dict
        meta = {"tensor_shape": [self.T, width], "activation_shape": [self.T, self.n_dict], "filenames": self.filenames,
                "freud_amd": {"variant": self.variant, "layout": self.layout, "K": self.K, "sorted": True, "index_dtype": self.index_dtype,
                              "stats": dict(zip(STAT_NAMES, stats))}}
        with open(self.paths["metadata"] + _PARTIAL, "w") as f:
            json.dump(meta, f)
        os.replace(self.paths["metadata"] + _PARTIAL, self.paths["metadata"])
        return total + os.path.getsize(self.paths["metadata"])


def write_store(batches: Iterable[Tuple[int, np.ndarray, Optional[np.ndarray]]], writer: StoreWriter, stats_of) -> CollectReport:
    """Drain `batches` -- (file0, values [nb, T, K] or [nb, T, n], indices or None) in file order, from the device source below or
    any other -- into the writer; stats_of() gives the eight statistics once the batches are through.  A failure removes the
    partial files and leaves no store."""
    try:
        for file0, values, indices in batches:
            writer.write(file0, values, indices)
        stats = np.asarray(stats_of(), dtype=np.int64)
        nbytes = writer.finish(stats)
    except BaseException:
        writer.abort()
        raise
    p = writer.paths
    paths = ({"values": p["values"], "indices": p["indices"]} if writer.layout == "indexed" else {"tensors": p["tensors"]})
    paths["metadata"] = p["metadata"]
    return CollectReport(writer.variant, writer.layout, len(writer.filenames), writer.T, writer.K, writer.n_dict, writer.index_dtype,
                         int(stats[0]), int(stats[1]), int(stats[2]), int(stats[3]), int(stats[4]), bf16_bits_to_float(stats[5]),
                         int(stats[2]) == 0, paths, int(nbytes))


def _device_batches(fp, K: int, index_dtype: str, stats):
    """The device source of an indexed store: per batch one engine call into one of two device buffer pairs, then its copy to one of
    two pinned host pairs on a copy stream.  The copy of batch b runs under the kernels of batch b + 1 and the caller's file write of
    batch b - 1: a batch is handed out only after the next one is enqueued."""
    import torch

    dev, T, B = fp.device, fp.T, fp.batch_files
    tdt = torch.int32 if index_dtype == "int32" else torch.int64
    vd = [torch.empty(B, T, K, dtype=torch.float32, device=dev) for _ in range(2)]
    xd = [torch.empty(B, T, K, dtype=tdt, device=dev) for _ in range(2)]
    vh = [torch.empty(B, T, K, dtype=torch.float32).pin_memory() for _ in range(2)]
    xh = [torch.empty(B, T, K, dtype=tdt).pin_memory() for _ in range(2)]
    copy_stream = torch.cuda.Stream(device=dev)
    pending = None
    for b, (x, file0, nb, _lens) in enumerate(fp):
        s = b & 1
        fp.eng.collect_files(x, K, vd[s][:nb], xd[s][:nb], stats)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            vh[s][:nb].copy_(vd[s][:nb], non_blocking=True)
            xh[s][:nb].copy_(xd[s][:nb], non_blocking=True)
            done = torch.cuda.Event()
            done.record(copy_stream)
        if pending is not None:
            p_file0, p_nb, p_s, p_done = pending
            p_done.synchronize()
            yield p_file0, vh[p_s][:p_nb].numpy(), xh[p_s][:p_nb].numpy()
        pending = (file0, nb, s, done)
    if pending is not None:
        p_file0, p_nb, p_s, p_done = pending
        p_done.synchronize()
        yield p_file0, vh[p_s][:p_nb].numpy(), xh[p_s][:p_nb].numpy()


def _latent_batches(fp):
    """The dense source (layout="tensor", L1): the stored latent of the eval forward, widened to float32."""
    import torch

    n = fp.eng.n
    for x, file0, nb, _lens in fp:
        fp.eng.eval(x.reshape(nb * fp.T, fp.d))
        ptr, ld = fp.eng.latent_buffer()
        lat = _alias(ptr, (nb * fp.T, ld), "<i2", fp.device).view(torch.bfloat16)[:, :n]
        yield file0, lat.float().reshape(nb, fp.T, n).cpu().numpy(), None


def collect_features(sae, data_path: str, layer_name: str, out_folder: str, *, k: Optional[int] = None, index_dtype: str = "int64",
                     layout: str = "indexed", subset_size: Optional[int] = None, batch_files: Optional[int] = None,
                     overwrite: bool = False) -> CollectReport:
    """Write the features of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) over the files of a shard
    directory to out_folder (module docstring).  k: slots per row -- TopK: at most and by default the model's k; L1: required, at
    most min(n_dict, 1024).  batch_files: files per engine call (default: file_pass.default_batch_files); the files written do not
    depend on it."""
    import torch
    from .file_pass import FilePass, is_raw, keep_rng

    if is_raw(sae):
        raise ValueError("feature collection needs an SAE: the raw activations are the shards themselves")
    if layout not in ("indexed", "tensor"):
        raise ValueError(f"layout={layout!r} is neither 'indexed' nor 'tensor'")
    if index_dtype not in _INDEX_DTYPES:
        raise ValueError(f"index_dtype={index_dtype!r} is neither 'int64' nor 'int32'")
    if k is not None and int(k) < 1:
        raise ValueError(f"k={k} must be >= 1")
    check_out_folder(data_path, out_folder, layer_name, layout, overwrite)

    @keep_rng
    def run() -> CollectReport:
        fp = FilePass(sae, data_path, layer_name, what="feature collection", subset_size=subset_size, batch_files=batch_files)
        eng = fp.eng
        n, variant = eng.n, eng.variant
        if layout == "tensor":
            if variant != "l1":
                raise ValueError("layout='tensor' is the reference's dense L1 form; a TopK store is indexed")
            K = n
        elif variant == "topk":
            K = int(eng.k) if k is None else int(k)
            if K > int(eng.k):
                raise ValueError(f"k={K} > the model's k={eng.k}: a TopK row holds k latents")
        else:
            if k is None:
                raise ValueError("an L1 store needs k, the slots per row: the L0 histogram of freud_amd.feature_stats (l0_hist) says how "
                                 "many latents a row fires; the report's `dropped` says what a k cut")
            K = int(k)
            if K > min(n, COLLECT_MAX_K):
                raise ValueError(f"k={K} > min(n_dict={n}, {COLLECT_MAX_K})")
        writer = StoreWriter(out_folder, layer_name, fp.filenames, fp.T, K, n, variant=variant, index_dtype=index_dtype, layout=layout,
                             overwrite=overwrite)
        with torch.cuda.device(fp.device):
            stats = torch.zeros(8, dtype=torch.int64, device=fp.device)
            if layout == "tensor":
                return write_store(_latent_batches(fp), writer, lambda: np.zeros(8, np.int64))
            return write_store(_device_batches(fp, K, index_dtype, stats), writer, lambda: stats.cpu().numpy())

    return run()


class FeatureShards:
    """Reader of an indexed store: memmaps of both files, the metadata, and per-file / per-latent views."""

    def __init__(self, data_path: str, layer_name: str):
        p = store_paths(data_path, layer_name)
        with open(p["metadata"]) as f:
            self.metadata = json.load(f)
        self.values = np.load(p["values"], mmap_mode="r")
        self.indices = np.load(p["indices"], mmap_mode="r")
        self.T, self.K = (int(v) for v in self.metadata["tensor_shape"])
        self.n_dict = int(self.metadata["activation_shape"][-1])
        self.filenames = list(self.metadata["filenames"])
        self.info = self.metadata.get("freud_amd")
        if self.values.shape != self.indices.shape or self.values.shape != (len(self.filenames), self.T * self.K):
            raise ValueError(f"{data_path}: values {self.values.shape} / indices {self.indices.shape} do not match the metadata")

    def __len__(self) -> int:
        return len(self.filenames)

    def rows(self, file: int) -> Tuple[np.ndarray, np.ndarray]:
        """(values [T, K] float32, indices [T, K]) of one file."""
        return self.values[file].reshape(self.T, self.K), self.indices[file].reshape(self.T, self.K)

    def dense(self, file: int) -> np.ndarray:
        """float32 [T, n_dict]: the stored slots of one file scattered (the latent itself when nothing was dropped)."""
        v, i = self.rows(file)
        out = np.zeros((self.T, self.n_dict), np.float32)
        np.put_along_axis(out, np.asarray(i, dtype=np.int64), np.asarray(v), axis=1)
        return out

    def series(self, latent: int, files=None) -> np.ndarray:
        """float32 [files, T]: the value of one latent on every frame -- the reference's activation_tensor_from_indexed, vectorised
        (the indices of a row are distinct, so at most one slot matches)."""
        sel = np.arange(len(self)) if files is None else np.atleast_1d(np.asarray(files, dtype=np.int64))
        out = np.zeros((sel.size, self.T), np.float32)
        for o, f in enumerate(sel):
            v, i = self.rows(int(f))
            out[o] = np.where(i == int(latent), v, np.float32(0)).sum(axis=1, dtype=np.float32)
        return out


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Write the SAE features of a shard directory in the reference's indexed form.")
    ap.add_argument("--config", required=True, help="the reference's configs/features/*.json: sae_model, layer_name, data_path (a "
                    "shard directory here), out_folder, batch_size, collect_max; whisper_model, device, dl_max_workers are ignored")
    ap.add_argument("--k", type=int, default=None, help="slots per row (TopK: default the model's k; L1: required)")
    ap.add_argument("--index-dtype", dest="index_dtype", choices=sorted(_INDEX_DTYPES), default="int64")
    ap.add_argument("--layout", choices=["indexed", "tensor"], default="indexed")
    ap.add_argument("--overwrite", action="store_true")
    a = ap.parse_args(argv)
    with open(a.config) as f:
        cfg = json.load(f)
    known = {"sae_model", "layer_name", "data_path", "out_folder", "batch_size", "collect_max", "whisper_model", "device", "dl_max_workers"}
    unknown = sorted(set(cfg) - known)
    if unknown:
        raise SystemExit(f"{a.config}: unknown keys {unknown}")
    for key in ("sae_model", "layer_name", "data_path", "out_folder"):
        if not cfg.get(key):
            raise SystemExit(f"{a.config}: {key} is required")
    rep = collect_features(cfg["sae_model"], cfg["data_path"], cfg["layer_name"], cfg["out_folder"], k=a.k, index_dtype=a.index_dtype,
                           layout=a.layout, subset_size=cfg.get("collect_max"), batch_files=cfg.get("batch_size"), overwrite=a.overwrite)
    print(rep.to_json())


if __name__ == "__main__":
    main()
