"""Feature index: the latent-major postings of an indexed feature store (freud_amd.collect_features, or the reference's
collect_activations.py with sae_model set), built in one GPU pass and kept next to the store.

The store is row-major: per file [T, K] values and [T, K] latent indices.  The question asked of it is per latent -- which files
fire latent j, where and how strongly, inside this value band -- and the reference answers it by scanning every slot of every
file for each query (src/utils/activations.py:41-58, activation_tensor_from_indexed, under top_activations :95-101).  The index is
the transpose of the store: for every latent the list of (position, value) of the slots that fire it, position = file * T +
frame, ascending.  A query then reads one list: no SAE, no Whisper activations, no GPU.

Files, in the store's folder (written under temporary names and renamed at the end, the metadata last):
  <layer>_postings_starts.npy     int64 [n_dict + 1]: list j is [starts[j], starts[j + 1])
  <layer>_postings_positions.npy  uint32 [nnz]
  <layer>_postings_values.npy     float32 [nnz]: the stored bits
  <layer>_postings.json           n_files, T, K, n_dict, nnz, the store's index dtype, the build statistics and the fingerprint of
                                  the store (byte sizes of both store files, a hash of the filenames): a stale index is refused.
A slot is posted iff its value is not +-0.0 and its index lies in [0, n_dict); +0.0 padding and a TopK slot whose ReLU output is 0
contribute nothing to a series.  A store with n_files * T >= 2^32 is refused.  The indices of a row must be distinct (the
reference's .nonzero().item() raises where they are not): a store that repeats one fails the build.

The build (include/freud_sae.h, sae_findex_*; freud_amd/csrc/findex.h) is a stable counting sort by latent: sweep 1 counts, the
prefix sum gives the list starts, sweep 2 fills -- once per latent range when the lists do not fit the device budget.  The files
written depend neither on batch_files nor on the number of ranges.

    python -m freud_amd.feature_index build --data_path DIR --layer_name L [--overwrite]
    python -m freud_amd.feature_index top --data_path DIR --layer_name L --feature J --n_files N [--min_val V] [--max_val V]
                                          [--absolute] [--lengths file.npy]
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
from typing import List, Optional, Tuple

import numpy as np

from .collect_features import store_paths
from .file_pass import check_lengths

TIMESTEP_S = 30 / 1500          # src/utils/constants.py:17
_PARTIAL = ".partial"
_KEYS = ("metadata", "starts", "positions", "values")      # metadata first: what is left never loads
MAX_POSITIONS = 1 << 32
FORMAT_VERSION = 1


def index_paths(folder: str, layer_name: str) -> dict:
    return {"starts": os.path.join(folder, f"{layer_name}_postings_starts.npy"),
            "positions": os.path.join(folder, f"{layer_name}_postings_positions.npy"),
            "values": os.path.join(folder, f"{layer_name}_postings_values.npy"),
            "metadata": os.path.join(folder, f"{layer_name}_postings.json")}


def store_fingerprint(folder: str, layer_name: str, filenames: List[str]) -> dict:
    """What ties an index to its store: the byte sizes of both store files and a hash of the indexed filenames."""
    p = store_paths(folder, layer_name)
    h = hashlib.sha256(json.dumps([str(f) for f in filenames]).encode()).hexdigest()
    return {"values_bytes": os.path.getsize(p["values"]), "indices_bytes": os.path.getsize(p["indices"]), "filenames_sha256": h}


def check_positions(n_files: int, T: int) -> None:
    """A position is a uint32: refused from the shape alone."""
    if int(n_files) * int(T) >= MAX_POSITIONS:
        raise ValueError(f"n_files * T = {int(n_files)} * {int(T)} = {int(n_files) * int(T)} >= 2^32: a position does not fit a uint32 "
                         "(index a subset_size of the files)")


@dataclasses.dataclass
class FeatureIndexReport:
    """What a build wrote."""
    n_files: int
    T: int
    K: int
    n_dict: int
    index_dtype: str
    slots: int                   # slots of the store seen
    nnz: int                     # slots posted
    zero_slots: int              # +-0.0 slots skipped
    out_of_range: int            # non-zero slots whose index is outside [0, n_dict): counted, not posted
    longest_list: int
    longest_latent: int          # the lowest latent with the longest list
    empty_lists: int
    sweeps: int                  # passes over the store: 1 count + one fill per latent range
    ranges: List[Tuple[int, int]]
    paths: dict
    bytes_written: int

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self))


def plan_ranges(starts: np.ndarray, budget_bytes: int, workspace_bytes_per_latent: int) -> List[Tuple[int, int]]:
    """Contiguous latent ranges whose lists (8 bytes a slot) plus workspace fit budget_bytes each, as few as a greedy walk gives.
    A range holds fewer than 2^32 - 1 slots (32-bit places on the device)."""
    starts = np.asarray(starts, dtype=np.int64)
    n = starts.size - 1
    per = int(workspace_bytes_per_latent)
    cost = starts * 8 + np.arange(n + 1, dtype=np.int64) * per          # cost(j0, j1) = cost[j1] - cost[j0]: monotone in j1
    out, j0 = [], 0
    while j0 < n:
        j1 = int(np.searchsorted(cost, cost[j0] + int(budget_bytes), side="right")) - 1
        j1 = min(j1, int(np.searchsorted(starts, starts[j0] + (MAX_POSITIONS - 2), side="right")) - 1, n)
        if j1 <= j0:
            need = int(cost[j0 + 1] - cost[j0])
            raise ValueError(f"device_budget_bytes={int(budget_bytes)} does not hold the list of latent {j0} "
                             f"({int(starts[j0 + 1] - starts[j0])} slots, {need} bytes with its workspace)")
        out.append((j0, j1))
        j0 = j1
    return out


def index_metadata(n_files: int, T: int, K: int, n_dict: int, index_dtype: str, starts: np.ndarray, stats: dict, n_ranges: int,
                   fingerprint: dict) -> dict:
    """The contents of <layer>_postings.json; stats: slots, zero_slots, out_of_range."""
    counts = np.diff(np.asarray(starts, dtype=np.int64))
    longest_latent = int(np.argmax(counts)) if counts.size else 0
    build = {"slots": int(stats["slots"]), "zero_slots": int(stats["zero_slots"]), "out_of_range": int(stats["out_of_range"]),
             "longest_list": int(counts[longest_latent]) if counts.size else 0, "longest_latent": longest_latent,
             "empty_lists": int((counts == 0).sum()), "sweeps": 1 + int(n_ranges), "ranges": int(n_ranges)}
    return {"format": FORMAT_VERSION, "n_files": int(n_files), "T": int(T), "K": int(K), "n_dict": int(n_dict), "nnz": int(starts[-1]),
            "index_dtype": index_dtype, "build": build, "fingerprint": fingerprint}


class IndexWriter:
    """The files of one build; nothing under the folder loads as an index until finish()."""

    def __init__(self, folder: str, layer_name: str, overwrite: bool):
        self.paths = index_paths(folder, layer_name)
        held = [os.path.basename(self.paths[k]) for k in _KEYS if os.path.exists(self.paths[k])]
        if held and not overwrite:
            raise ValueError(f"{folder!r} already holds {', '.join(held)} (overwrite=True replaces them)")
        self._maps = {}
        self._overwrite = overwrite

    def open(self, starts: np.ndarray) -> None:
        from numpy.lib.format import open_memmap
        for key in _KEYS:
            for path in (self.paths[key], self.paths[key] + _PARTIAL):
                if os.path.exists(path):
                    os.unlink(path)
        nnz = int(starts[-1])
        with open(self.paths["starts"] + _PARTIAL, "wb") as f:
            np.save(f, np.asarray(starts, dtype=np.int64))
        if nnz == 0:                    # (an empty file cannot be mapped)
            for key, dt in (("positions", np.uint32), ("values", np.float32)):
                with open(self.paths[key] + _PARTIAL, "wb") as f:
                    np.save(f, np.zeros(0, dt))
            return
        self._maps["positions"] = open_memmap(self.paths["positions"] + _PARTIAL, mode="w+", dtype=np.uint32, shape=(nnz,), version=(1, 0))
        self._maps["values"] = open_memmap(self.paths["values"] + _PARTIAL, mode="w+", dtype=np.float32, shape=(nnz,), version=(1, 0))

    def write(self, s0: int, positions: np.ndarray, values: np.ndarray) -> None:
        if positions.size == 0:
            return
        self._maps["positions"][s0:s0 + positions.size] = positions
        self._maps["values"][s0:s0 + values.size] = values

    def abort(self) -> None:
        self._maps = {}
        for key in _KEYS:
            if os.path.exists(self.paths[key] + _PARTIAL):
                os.unlink(self.paths[key] + _PARTIAL)

    def finish(self, meta: dict) -> int:
        maps, self._maps = self._maps, {}
        for m in maps.values():
            m.flush()
        del maps
        total = 0
        for key in ("starts", "positions", "values"):
            os.replace(self.paths[key] + _PARTIAL, self.paths[key])
            total += os.path.getsize(self.paths[key])
        with open(self.paths["metadata"] + _PARTIAL, "w") as f:
            json.dump(meta, f)
        os.replace(self.paths["metadata"] + _PARTIAL, self.paths["metadata"])
        return total + os.path.getsize(self.paths["metadata"])


def _store_batches(shards, n_files: int, batch_files: int, dev):
    """The store's files in batches, host -> device through two pinned buffer pairs and a copy stream: the copy of batch b + 1 runs
    under the kernels of batch b.  Yields (values [rows, K], indices [rows, K], file0, nb) on the device, ordered on the current
    stream; a buffer pair is reused only after the kernels that read it (enqueued by the consumer before it asks for the next batch)
    have finished."""
    import torch

    T, K, B = shards.T, shards.K, int(batch_files)
    tdt = torch.int32 if shards.indices.dtype == np.int32 else torch.int64
    vh = [torch.empty(B, T * K, dtype=torch.float32).pin_memory() for _ in range(2)]
    xh = [torch.empty(B, T * K, dtype=tdt).pin_memory() for _ in range(2)]
    vd = [torch.empty(B, T * K, dtype=torch.float32, device=dev) for _ in range(2)]
    xd = [torch.empty(B, T * K, dtype=tdt, device=dev) for _ in range(2)]
    copy_stream = torch.cuda.Stream(device=dev)
    used = [None, None]                 # per pair: the event behind the kernels that read it last
    main = torch.cuda.current_stream(dev)

    def stage(b):
        s, f0 = b & 1, b * B
        nb = min(B, n_files - f0)
        if used[s] is not None:
            used[s].synchronize()       # (also: the pinned pair's last copy is long done)
        vh[s][:nb].numpy()[...] = shards.values[f0:f0 + nb]
        xh[s][:nb].numpy()[...] = shards.indices[f0:f0 + nb]
        with torch.cuda.stream(copy_stream):
            vd[s][:nb].copy_(vh[s][:nb], non_blocking=True)
            xd[s][:nb].copy_(xh[s][:nb], non_blocking=True)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return s, f0, nb, done

    nbatches = (n_files + B - 1) // B
    nxt = stage(0)
    for b in range(nbatches):
        s, f0, nb, done = nxt
        main.wait_event(done)
        yield vd[s][:nb].view(nb * T, K), xd[s][:nb].view(nb * T, K), f0, nb
        ev = torch.cuda.Event()
        ev.record(main)
        used[s] = ev
        if b + 1 < nbatches:
            nxt = stage(b + 1)          # the host copy and the upload of batch b + 1 run under the kernels of batch b
    torch.cuda.synchronize(dev)


def default_batch_files(T: int, K: int, index_bytes: int, n_files: int) -> int:
    """Files per batch: about 64 MiB of store per buffer pair."""
    return max(1, min(int(n_files), (64 << 20) // max(1, T * K * (4 + index_bytes))))


def build_feature_index(data_path: str, layer_name: str, *, subset_size: Optional[int] = None, batch_files: Optional[int] = None,
                        device_budget_bytes: Optional[int] = None, overwrite: bool = False, device=None) -> FeatureIndexReport:
    """Build the index of the store in data_path (module docstring).  subset_size: index the first files only.  batch_files: files per
    device batch.  device_budget_bytes: what the lists of one latent range (8 bytes a slot) plus the kernels' workspace may take on
    the device (default: half of the free device memory); more ranges mean more fill sweeps, never other files."""
    import torch
    from . import engine
    from .collect_features import FeatureShards

    shards = FeatureShards(data_path, layer_name)
    n_files = len(shards) if subset_size is None else min(len(shards), int(subset_size))
    if n_files < 1:
        raise ValueError(f"{data_path}: no files to index")
    T, K, n = shards.T, shards.K, shards.n_dict
    check_positions(n_files, T)
    if K > engine.COLLECT_MAX_K:
        raise ValueError(f"K={K} > {engine.COLLECT_MAX_K}")
    if shards.indices.dtype not in (np.int32, np.int64) or shards.values.dtype != np.float32:
        raise ValueError(f"the store holds {shards.values.dtype} values and {shards.indices.dtype} indices; float32 and int32 / int64 are indexed")
    if not torch.cuda.is_available():
        raise RuntimeError("the feature index is built on the GPU (there is no CPU fallback); reading it needs none")
    index_dtype = str(shards.indices.dtype)
    filenames = shards.filenames[:n_files]
    fingerprint = store_fingerprint(data_path, layer_name, filenames)
    writer = IndexWriter(data_path, layer_name, overwrite)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    B = default_batch_files(T, K, shards.indices.dtype.itemsize, n_files) if batch_files is None else max(1, min(int(batch_files), n_files))
    max_rows = B * T

    try:
        with torch.cuda.device(dev):
            totals = torch.zeros(n, dtype=torch.int64, device=dev)
            stats = torch.zeros(engine.FINDEX_NSTATS, dtype=torch.int64, device=dev)
            err = torch.zeros(2, dtype=torch.int64, device=dev)
            for v, x, _f0, _nb in _store_batches(shards, n_files, B, dev):                      # sweep 1
                engine.findex_count(v, x, n, totals, stats)
            starts_dev = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(totals, 0, out=starts_dev[1:])
            starts = starts_dev.cpu().numpy()
            st = dict(zip(engine.FINDEX_STAT_NAMES, (int(s) for s in stats.cpu().numpy())))
            nnz = int(starts[-1])
            if nnz != st["posted"] or st["slots"] != n_files * T * K:
                raise RuntimeError(f"count sweep: {nnz} slots in the lists, {st['posted']} posted, {st['slots']} of {n_files * T * K} seen")
            per_latent = engine.findex_workspace_bytes(max_rows, 1)
            if device_budget_bytes is None:
                device_budget_bytes = torch.cuda.mem_get_info(dev)[0] // 2
            ranges = plan_ranges(starts, int(device_budget_bytes), per_latent)
            writer.open(starts)
            cursor = starts_dev[:-1].clone()
            cap = max(1, max(int(starts[j1] - starts[j0]) for j0, j1 in ranges))
            pos_dev = torch.empty(cap, dtype=torch.int32, device=dev)
            val_dev = torch.empty(cap, dtype=torch.float32, device=dev)
            work = torch.empty(max(1, max(engine.findex_workspace_bytes(max_rows, j1 - j0) for j0, j1 in ranges)), dtype=torch.uint8, device=dev)
            for j0, j1 in ranges:                                                               # sweep 2, once per range
                base, cnt = int(starts[j0]), int(starts[j1] - starts[j0])
                if cnt == 0:
                    continue
                for v, x, f0, _nb in _store_batches(shards, n_files, B, dev):
                    engine.findex_fill(v, x, n, j0, j1, f0 * T, cursor, base, pos_dev, val_dev, work, err)
                engine.findex_verify(starts_dev, j0, j1, base, pos_dev, n_files * T, err)
                bad, over = (int(e) for e in err.cpu().numpy())
                if over or not torch.equal(cursor[j0:j1], starts_dev[j0 + 1:j1 + 1]):
                    raise RuntimeError("fill sweep: the lists do not end where the count sweep said (did the store change during the build?)")
                if bad:
                    raise ValueError(f"the store has duplicate indices in a row ({bad} slots of the latents [{j0}, {j1}) are out of order)")
                writer.write(base, pos_dev[:cnt].cpu().numpy().view(np.uint32), val_dev[:cnt].cpu().numpy())
        meta = index_metadata(n_files, T, K, n, index_dtype, starts, st, len(ranges), fingerprint)
        build = meta["build"]
        nbytes = writer.finish(meta)
    except BaseException:
        writer.abort()
        raise
    return FeatureIndexReport(n_files, T, K, n, index_dtype, st["slots"], nnz, st["zero_slots"], st["out_of_range"], build["longest_list"],
                              build["longest_latent"], build["empty_lists"], 1 + len(ranges), [tuple(r) for r in ranges], dict(writer.paths), int(nbytes))


class FeatureIndex:
    """Reader of the index; numpy only (no GPU, no engine library).  A stale index -- one whose store has other file sizes or other
    filenames than the store it was built from -- is refused."""

    def __init__(self, data_path: str, layer_name: str):
        p = index_paths(data_path, layer_name)
        with open(p["metadata"]) as f:
            self.metadata = json.load(f)
        m = self.metadata
        self.n_files, self.T, self.K, self.n_dict, self.nnz = (int(m[k]) for k in ("n_files", "T", "K", "n_dict", "nnz"))
        check_positions(self.n_files, self.T)
        with open(store_paths(data_path, layer_name)["metadata"]) as f:
            self.filenames = [str(v) for v in json.load(f)["filenames"]][:self.n_files]
        now = store_fingerprint(data_path, layer_name, self.filenames)
        if len(self.filenames) != self.n_files or now != m["fingerprint"]:
            raise ValueError(f"{p['metadata']} is stale: it was built from a store with {m['fingerprint']}, the store now has {now} "
                             "(rebuild with overwrite=True)")
        self.starts = np.load(p["starts"])
        mode = "r" if self.nnz else None
        self.positions = np.load(p["positions"], mmap_mode=mode)
        self.values = np.load(p["values"], mmap_mode=mode)
        if (self.starts.shape != (self.n_dict + 1,) or int(self.starts[-1]) != self.nnz or self.positions.shape != (self.nnz,)
                or self.values.shape != (self.nnz,) or self.positions.dtype != np.uint32 or self.values.dtype != np.float32):
            raise ValueError(f"{data_path}: the postings files do not match {p['metadata']}")

    def __len__(self) -> int:
        return self.n_files

    @property
    def counts(self) -> np.ndarray:
        return np.diff(self.starts)

    def postings(self, latent: int) -> Tuple[np.ndarray, np.ndarray]:
        """(positions uint32, values float32) of one latent: memmap views, positions ascending."""
        j = int(latent)
        if not 0 <= j < self.n_dict:
            raise IndexError(f"latent {j} outside [0, {self.n_dict})")
        s, e = int(self.starts[j]), int(self.starts[j + 1])
        return self.positions[s:e], self.values[s:e]

    def series(self, latent: int, files=None) -> np.ndarray:
        """float32 [files, T]: the value of one latent on every frame; bit-equal to FeatureShards.series."""
        p, v = self.postings(latent)
        if files is None:
            dense = np.zeros(self.n_files * self.T, np.float32)
            dense[np.asarray(p, dtype=np.int64)] = v
            return dense.reshape(self.n_files, self.T)
        sel = np.atleast_1d(np.asarray(files, dtype=np.int64))
        out = np.zeros((sel.size, self.T), np.float32)
        for o, f in enumerate(sel):
            f = int(f) + self.n_files if int(f) < 0 else int(f)
            if not 0 <= f < self.n_files:
                raise IndexError(f"file {int(f)} outside [0, {self.n_files})")
            a, b = np.searchsorted(p, [f * self.T, (f + 1) * self.T])
            out[o, np.asarray(p[a:b], dtype=np.int64) - f * self.T] = v[a:b]
        return out

    def _kept(self, latent: int, lengths):
        p, v = self.postings(latent)
        p, v = np.asarray(p, dtype=np.int64), np.asarray(v)
        file, frame = p // self.T, p % self.T
        L = check_lengths(lengths, self.n_files, self.T)
        L = np.full(self.n_files, self.T, np.int64) if L is None else L.astype(np.int64)
        keep = frame < L[file]
        return file[keep], frame[keep], v[keep], L

    def file_max(self, latent: int, lengths=None, absolute_magnitude: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(values float32 [n_files], frames int64 [n_files]): the reference's rule on the dense (trimmed) series -- the first maximal
        frame; absolute_magnitude: the signed value at the first argmax |a|.  A frame without a posting is 0.0, so a file with no kept
        posting has 0.0 at frame 0, and a file whose kept values are all negative has 0.0 at its first frame without a posting."""
        file, frame, v, L = self._kept(latent, lengths)
        vals, frames = np.zeros(self.n_files, np.float32), np.zeros(self.n_files, np.int64)
        if file.size == 0:
            return vals, frames
        first = np.flatnonzero(np.r_[True, file[1:] != file[:-1]])
        cnt = np.diff(np.r_[first, file.size])
        key = np.abs(v) if absolute_magnitude else v
        gmax = np.maximum.reduceat(key, first)
        at = np.minimum.reduceat(np.where(key == np.repeat(gmax, cnt), np.arange(file.size), file.size), first)
        at = np.minimum(at, file.size - 1)                       # (a NaN group has no equal element)
        g = file[first]
        vals[g], frames[g] = v[at], frame[at]
        if not absolute_magnitude:
            for i in np.flatnonzero(~(gmax > 0)):                # kept values all negative: an unposted frame, 0.0, is the maximum
                f = int(g[i])
                if cnt[i] >= L[f]:
                    continue                                     # every kept frame is posted: the negative maximum stands
                fr = frame[first[i]:first[i] + cnt[i]]
                gap = np.flatnonzero(fr != np.arange(cnt[i]))
                vals[f], frames[f] = np.float32(0), int(gap[0]) if gap.size else int(cnt[i])
        return vals, frames

    def top_activations(self, latent: int, n_files: int, max_val: Optional[float] = None, min_val: Optional[float] = None,
                        absolute_magnitude: bool = False, return_max_per_file: bool = False, lengths=None):
        """The reference's top_activations (src/utils/activations.py:61-132) for one latent, from its list alone: (pq, max_per_file)
        with pq = [(filename, trimmed series, max value, max time)], value descending then file ascending, filtered by
        min_val <= signed value <= max_val; absolute_magnitude ranks |value| and, as the reference does, reports the time of the
        SIGNED argmax (freud_amd/feature_search.py).  max_per_file (signed values, every file) or None."""
        L = check_lengths(lengths, self.n_files, self.T)
        signed, sframes = self.file_max(latent, lengths, False)
        if absolute_magnitude:
            value, _ = self.file_max(latent, lengths, True)
            rank = np.abs(value)
        else:
            value, rank = signed, signed
        allow = np.ones(self.n_files, bool)
        if max_val is not None:
            allow &= ~(value > max_val)
        if min_val is not None:
            allow &= ~(value < min_val)
        cand = np.flatnonzero(allow)
        order = cand[np.argsort(-rank[cand].astype(np.float64), kind="stable")][:max(int(n_files), 0)]
        pq = []
        if order.size:
            ser = self.series(latent, order)
            for o, f in enumerate(order):
                n = self.T if L is None else int(L[f])
                pq.append((self.filenames[int(f)], ser[o, :n].copy(), float(rank[f]), int(sframes[f]) * TIMESTEP_S))
        return pq, ([float(x) for x in value] if return_max_per_file else None)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Build or query the latent-major postings index of an indexed feature store.")
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="build the index on the GPU")
    q = sub.add_parser("top", help="the reference's top_activations for one latent, from the index")
    for sp in (b, q):
        sp.add_argument("--data_path", required=True, help="the store's folder")
        sp.add_argument("--layer_name", required=True)
    b.add_argument("--subset_size", type=int, default=None)
    b.add_argument("--batch_files", type=int, default=None)
    b.add_argument("--device_budget_bytes", type=int, default=None)
    b.add_argument("--overwrite", action="store_true")
    q.add_argument("--feature", type=int, required=True)
    q.add_argument("--n_files", type=int, required=True)
    q.add_argument("--min_val", type=float, default=None)
    q.add_argument("--max_val", type=float, default=None)
    q.add_argument("--absolute", action="store_true")
    q.add_argument("--lengths", default=None, help=".npy of frames per file")
    a = ap.parse_args(argv)
    if a.cmd == "build":
        rep = build_feature_index(a.data_path, a.layer_name, subset_size=a.subset_size, batch_files=a.batch_files,
                                  device_budget_bytes=a.device_budget_bytes, overwrite=a.overwrite)
        print(rep.to_json())
        return
    ix = FeatureIndex(a.data_path, a.layer_name)
    lengths = None if a.lengths is None else np.load(a.lengths)
    pq, _ = ix.top_activations(a.feature, a.n_files, a.max_val, a.min_val, a.absolute, False, lengths)
    print(json.dumps([{"file": f, "value": v, "time": t, "frames": int(s.size)} for f, s, v, t in pq]))


if __name__ == "__main__":
    main()
