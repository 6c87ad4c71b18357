"""HBM-resident training data: a shard directory uploaded ONCE, every batch drawn on the device.

The host link bounds a real training run (the loader-fed step takes about twice the bare step at d = 384), and
every epoch sends the same bytes over it again.  A [1500, 384] file is 1.15 MB in bf16: datasets of that kind fit beside the engine
many times over.  For them

* ResidentActivations reads the shard directory once, in file order, through the streaming loader (native delivery, no shuffle) into
  one device tensor [n_files, T*d] -- in the shard's own dtype ("native": reference semantics bit for bit), or with fp32 shards
  converted on the device by the rule of the loader's host conversion ("bfloat16": include/freud_sae.h, sae_store_convert);
* ResidentActivationDataLoader is MemoryMappedActivationDataLoader with the batches assembled by one gather kernel per batch
  (sae_store_gather) instead of copies over the link: the same epoch_batches() -- so the same RNG draws, rank slices, drop_last and
  skip_next -- the same (x [B, T, d], filenames) batches bit for bit, into a ring of `depth` device buffers;
* FilePass (file_pass.py) takes a native store in place of the directory and yields zero-copy slices of it.

An index list is validated on the host (check_indices) before it is uploaded; the kernel clamps and counts all the same, and the
count is read once per epoch.  The store does not fit: ResidentOverflow, before anything is allocated.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import numpy as np

from .file_pass import keep_rng
from .loader import MemoryMappedActivationDataLoader, MemoryMappedActivationsDataset

DTYPES = ("native", "bfloat16")
RESERVE_BYTES = 4 << 30           # left free beside the store when max_gb is not given: the engine, the rings, the passes' scratch
UPLOAD_BATCH_BYTES = 64 << 20     # the upload walks the directory in batches of about this size
DEFAULT_OVERLAP = False           # measured (tools/bench_resident.py, profiles/resident_bench.json): the gather
                                  # on the compute stream, in front of its step, is faster than on a stream of its own


class ResidentOverflow(RuntimeError):
    """The store does not fit the device memory it may take."""


def check_dtype(dtype: str) -> str:
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be 'native' or 'bfloat16', got {dtype!r}")
    return dtype


def check_indices(batches: Sequence[Sequence[int]], n_files: int) -> np.ndarray:
    """The file indices of an epoch's batches, one after another, as int32 -- after the check that every one lies in [0, n_files)."""
    flat = np.fromiter((i for b in batches for i in b), dtype=np.int64)
    if flat.size and (int(flat.min()) < 0 or int(flat.max()) >= n_files):
        raise ValueError(f"file indices [{int(flat.min())}, {int(flat.max())}] leave the store's [0, {n_files})")
    return flat.astype(np.int32)


def parse_resident_data(spec) -> Optional[dict]:
    """The optional train() key "resident_data" -> None (absent or false) or {"dtype": None | name, "max_gb", "on_overflow"};
    ValueError for a form it does not take.  dtype None: what the streaming loader would deliver."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict) or set(spec) - {"dtype", "max_gb", "on_overflow"}:
        raise ValueError(f"\"resident_data\" is true, false or an object of dtype, max_gb, on_overflow; got {spec!r}")
    dtype, max_gb, on_overflow = spec.get("dtype"), spec.get("max_gb"), spec.get("on_overflow", "error")
    if dtype is not None and dtype not in DTYPES:
        raise ValueError(f"\"resident_data\": dtype is \"native\" or \"bfloat16\"; got {dtype!r}")
    if max_gb is not None and (isinstance(max_gb, bool) or not isinstance(max_gb, (int, float)) or not max_gb > 0):
        raise ValueError(f"\"resident_data\": max_gb is a positive number of GiB; got {max_gb!r}")
    if on_overflow not in ("error", "stream"):
        raise ValueError(f"\"resident_data\": on_overflow is \"error\" or \"stream\"; got {on_overflow!r}")
    return {"dtype": dtype, "max_gb": max_gb, "on_overflow": on_overflow}


def _deliver(deliver_dtype: Optional[str]) -> str:
    """None -> what the streaming loader delivers by default (FREUD_LOADER_DELIVER, else native)."""
    return check_dtype(deliver_dtype if deliver_dtype is not None else os.environ.get("FREUD_LOADER_DELIVER", "native"))


class ResidentActivations:
    """A shard directory in device memory.  `dtype` follows the loader's deliver_dtype: "bfloat16" converts fp32 shards on the device
    (2-byte shards stay as they are), "native" keeps the shard's dtype.  max_gb: the most the store may take (GiB; default: the free
    device memory less RESERVE_BYTES) -- more is a ResidentOverflow that names both numbers, raised before anything is allocated.

    Attributes: data [n_files, T*d] on `device`, metadata, tensor_shape, activation_shape, filenames, nbytes, dataset (the host side:
    MemoryMappedActivationsDataset), native (whether data holds the shard's own values), upload_seconds."""

    def __init__(self, data_path: str, layer_name: str, *, device="cuda", dtype: str = "native", subset_size: Optional[int] = None,
                 max_gb: Optional[float] = None):
        check_dtype(dtype)
        if max_gb is not None and not max_gb > 0:
            raise ValueError(f"max_gb={max_gb!r} must be positive")
        ds = MemoryMappedActivationsDataset(data_path, layer_name, subset_size)
        n_files = len(ds)
        if n_files == 0:
            raise ValueError(f"{data_path}: no files")
        import torch
        if not torch.cuda.is_available() or torch.device(device).type != "cuda":
            raise RuntimeError("the resident store lives in HBM and is read by HIP kernels; there is no CPU path")
        import time
        from . import engine
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        T, d = int(ds.tensor_shape[-2]), int(ds.tensor_shape[-1])
        row = T * d
        src_dtype = torch.from_numpy(np.empty(0, dtype=ds.mmap.dtype)).dtype
        convert = dtype == "bfloat16" and ds.mmap.dtype == np.float32
        store_dtype = torch.bfloat16 if convert else src_dtype
        es = torch.empty(0, dtype=store_dtype).element_size()
        need = n_files * row * es
        budget = int(max_gb * (1 << 30)) if max_gb is not None else int(torch.cuda.mem_get_info(dev)[0]) - RESERVE_BYTES
        if need > budget:
            raise ResidentOverflow(f"the store of {n_files} files x {row} values needs {need} bytes ({need / 2 ** 30:.3f} GiB); "
                                   f"it may take {budget} bytes ({budget / 2 ** 30:.3f} GiB)"
                                   + ("" if max_gb is not None else f" -- the free device memory less {RESERVE_BYTES >> 30} GiB"))
        self.dataset, self.device, self.dtype, self.native = ds, dev, dtype, not convert
        self.data_path, self.layer_name = data_path, layer_name
        self.metadata, self.tensor_shape, self.activation_shape = ds.metadata, list(ds.tensor_shape), ds.activation_shape
        self.filenames = list(ds.metadata["filenames"])
        t0 = time.time()
        with torch.cuda.device(dev):
            self.data = torch.empty((n_files, row), dtype=store_dtype, device=dev)
            keep_rng(self._upload)(engine, subset_size, max(1, min(n_files, UPLOAD_BATCH_BYTES // max(1, row * ds.mmap.dtype.itemsize))))
            torch.cuda.current_stream(dev).synchronize()
        self.upload_seconds = time.time() - t0
        self.nbytes = need

    def _upload(self, engine, subset_size, batch_files: int) -> None:
        loader = MemoryMappedActivationDataLoader(self.data_path, self.layer_name, batch_files, subset_size=subset_size,
                                                  dl_kwargs={"shuffle": False, "drop_last": False}, device=self.device,
                                                  deliver_dtype="native")
        file0 = 0
        for x, _names in loader:
            nb = int(x.shape[0])
            dst = self.data[file0:file0 + nb]
            if self.native:
                dst.copy_(x.reshape(nb, -1))
            else:
                engine.store_convert(x.reshape(-1), dst.reshape(-1))
            file0 += nb
        if file0 != len(self):
            raise RuntimeError(f"the loader delivered {file0} of {len(self)} files")

    def __len__(self) -> int:
        return len(self.filenames)


class ResidentActivationDataLoader(MemoryMappedActivationDataLoader):
    """MemoryMappedActivationDataLoader over a resident store: the same constructor arguments, attributes and iteration contract
    (module docstring).  data_path may be a ResidentActivations (then subset_size, deliver_dtype and max_gb are not used).  Needs a
    GPU.  overlap: the gathers run on a stream of their own, ordered against the compute stream by events both ways exactly as the
    streaming loader orders its copies (True), or on the compute stream itself (False)."""

    def __init__(self, data_path, layer_name: str, batch_size: int, dl_max_workers: int = 0, subset_size: Optional[int] = None,
                 dl_kwargs: Optional[dict] = None, *, device="cuda", rank: int = 0, world_size: int = 1, depth: int = 3,
                 deliver_dtype: Optional[str] = None, max_gb: Optional[float] = None, overlap: bool = DEFAULT_OVERLAP):
        # (not the parent's constructor: it registers -- pins -- the shard file for the copies this loader never makes)
        dl_kwargs = dict(dl_kwargs or {})
        if isinstance(data_path, ResidentActivations):
            self.store = data_path
        else:
            self.store = ResidentActivations(data_path, layer_name, device=device, dtype=_deliver(deliver_dtype), subset_size=subset_size,
                                             max_gb=max_gb)
        self._dataset = self.dataset = self.store.dataset
        self.batch_size = batch_size
        self.shuffle, self.drop_last = bool(dl_kwargs.get("shuffle", False)), bool(dl_kwargs.get("drop_last", False))
        self.activation_shape, self.activation_type = self._dataset.activation_shape, self._dataset.activation_type
        self.dataset_length = len(self._dataset)
        self.device = self.store.device
        self.rank, self.world_size, self.depth = rank, world_size, max(2, depth)
        self.dl_max_workers = dl_max_workers
        self.overlap = bool(overlap)
        self.skip_next = 0
        self._registered = None
        self._ring = None           # (buffers, the compute-stream event after each one's last reader); one live iterator owns it
        self._ring_busy = False
        self._stream = None
        self._err = None

    def __iter__(self):
        import torch
        from . import engine
        batches = self.epoch_batches()
        if self.skip_next:
            batches = batches[self.skip_next:]
            self.skip_next = 0
        if not batches:
            return
        store, dev, depth = self.store, self.device, self.depth
        T, d = int(store.tensor_shape[-2]), int(store.tensor_shape[-1])
        names = store.filenames
        flat = check_indices(batches, len(store))        # the check; the kernel's clamp and count are the second line
        shared = not self._ring_busy
        new_ring = lambda: ([torch.empty((self.batch_size, T * d), dtype=store.data.dtype, device=dev) for _ in range(depth)], [None] * depth)
        if shared:
            if self._ring is None:
                self._ring = new_ring()
            self._ring_busy = True
        ring, consumed = self._ring if shared else new_ring()
        try:
            if self._err is None:
                self._err = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.overlap and self._stream is None:
                self._stream = torch.cuda.Stream(device=dev)
            err, side = self._err, self._stream if self.overlap else None
            idx_dev = torch.from_numpy(flat).to(dev)     # the epoch's indices: one upload
            if side is not None:
                uploaded = torch.cuda.Event()
                uploaded.record(torch.cuda.current_stream(dev))
                side.wait_event(uploaded)
            at = 0
            for bi, idxs in enumerate(batches):
                slot, nb = bi % depth, len(idxs)
                compute = torch.cuda.current_stream(dev)
                if side is not None and consumed[slot] is not None:
                    side.wait_event(consumed[slot])
                engine.store_gather(store.data, idx_dev[at:at + nb], ring[slot], err, stream=side if side is not None else compute)
                if side is not None:
                    landed = torch.cuda.Event()
                    landed.record(side)
                    compute.wait_event(landed)
                at += nb
                yield ring[slot][:nb].view(nb, T, d), [names[i] for i in idxs]
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                consumed[slot] = ev
            if side is not None:
                side.synchronize()
            bad = int(err.item())                        # once per epoch
            if bad:
                err.zero_()
                raise RuntimeError(f"{bad} batch rows of this epoch asked for files outside the store's [0, {len(store)}): "
                                   "they were clamped into it, the batches are not the epoch's")
        finally:
            if shared:
                self._ring_busy = False
