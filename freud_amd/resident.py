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
* ResidentFrameDataLoader draws FRAMES instead of files: an epoch is a keyed permutation of every counted frame, evaluated inside
  the gather kernel (sae_store_gather_frames; csrc/frame_perm.h), a batch is the next batch_size * T of them, and with lengths the
  padding of every file is left out -- the train() key "frame_batches" (parse_frame_batches);
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
        from . import engine
        batches = self.epoch_batches()
        if self.skip_next:
            batches = batches[self.skip_next:]
            self.skip_next = 0
        if not batches:
            return
        import torch
        store = self.store
        T, d = int(store.tensor_shape[-2]), int(store.tensor_shape[-1])
        names = store.filenames
        flat = check_indices(batches, len(store))        # the check; the kernel's clamp and count are the second line

        def jobs(dev):
            idx_dev = torch.from_numpy(flat).to(dev)     # the epoch's indices: one upload
            at = 0
            for idxs in batches:
                nb, idx = len(idxs), idx_dev[at:at + len(idxs)]
                at += nb
                yield (lambda buf, err, stream, idx=idx: engine.store_gather(store.data, idx, buf, err, stream=stream),
                       lambda buf, nb=nb, idxs=idxs: (buf[:nb].view(nb, T, d), [names[i] for i in idxs]))

        yield from self._ring_epoch(jobs, lambda bad: f"{bad} batch rows of this epoch asked for files outside the store's [0, {len(store)}): "
                                                      "they were clamped into it, the batches are not the epoch's")

    def _ring_epoch(self, jobs, complaint):
        """One epoch through the ring of `depth` buffers [batch_size, T * d].  jobs(dev) -- called once, after the ring exists and
        before the first gather, on the compute stream -- yields per batch (launch(buffer, err, stream), deliver(buffer) -> what
        the loader yields).  With overlap the launches run on the side stream, ordered against the compute stream by events both
        ways: a buffer is not overwritten before the compute stream has passed its last reader, and not read before its gather
        landed.  The error word is read once, after the last batch; a count is complaint(count) as a RuntimeError."""
        import torch
        store, dev, depth = self.store, self.device, self.depth
        T, d = int(store.tensor_shape[-2]), int(store.tensor_shape[-1])
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
            todo = jobs(dev)
            first = next(todo)                           # (the generator's setup -- the uploads -- runs here)
            if side is not None:
                uploaded = torch.cuda.Event()
                uploaded.record(torch.cuda.current_stream(dev))
                side.wait_event(uploaded)
            import itertools
            for bi, (launch, deliver) in enumerate(itertools.chain([first], todo)):
                slot = bi % depth
                compute = torch.cuda.current_stream(dev)
                if side is not None and consumed[slot] is not None:
                    side.wait_event(consumed[slot])
                launch(ring[slot], err, side if side is not None else compute)
                if side is not None:
                    landed = torch.cuda.Event()
                    landed.record(side)
                    compute.wait_event(landed)
                yield deliver(ring[slot])
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                consumed[slot] = ev
            if side is not None:
                side.synchronize()
            bad = int(err.item())                        # once per epoch
            if bad:
                err.zero_()
                raise RuntimeError(complaint(bad))
        finally:
            if shared:
                self._ring_busy = False


def parse_frame_batches(spec, resident: Optional[dict] = None) -> Optional[dict]:
    """The optional train() key "frame_batches" -> None (absent or false) or {"lengths": None | path}; `resident` is what
    parse_resident_data made of the config's "resident_data".  ValueError for a form it does not take, for the key without a
    resident store and for a store that may fall back to streaming.  Needs no device."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict) or set(spec) - {"lengths"}:
        raise ValueError(f"\"frame_batches\" is true, false or an object of lengths; got {spec!r}")
    lengths = spec.get("lengths")
    if lengths is not None and not isinstance(lengths, (str, os.PathLike)):
        raise ValueError(f"\"frame_batches\": lengths is the path of a .npy file of frames per file; got {lengths!r}")
    if resident is None:
        raise ValueError("\"frame_batches\" draws its frames from the resident store: the config needs \"resident_data\" too")
    if resident["on_overflow"] == "stream":
        raise ValueError("\"frame_batches\" with \"resident_data\": {\"on_overflow\": \"stream\"}: the streaming loader has no frame "
                         "batches to fall back to")
    return {"lengths": None if lengths is None else os.fspath(lengths)}


def load_frame_lengths(path: str, data_path: str, layer_name: str) -> np.ndarray:
    """The lengths file of "frame_batches" (.npy, int frames per file in file order) held to the shard directory by
    file_pass.check_lengths; every failure is a ValueError that names the key.  Needs no device."""
    from .file_pass import check_lengths
    try:
        raw = np.load(path, allow_pickle=False)
    except Exception as e:          # noqa: BLE001 -- whatever numpy makes of a file that is no array
        raise ValueError(f"\"frame_batches\": lengths file {path!r} does not load: {e}") from e
    ds = MemoryMappedActivationsDataset(data_path, layer_name)
    try:
        return check_lengths(raw, len(ds), int(ds.tensor_shape[-2]))
    except ValueError as e:
        raise ValueError(f"\"frame_batches\": lengths file {path!r}: {e}") from e


class ResidentFrameDataLoader(ResidentActivationDataLoader):
    """Frame batches over a resident store: an epoch is a pseudo-random permutation of every COUNTED frame of the dataset and a batch
    is the next batch_size * T of them -- all T frames of every file, or with lengths (frames per file, in file order; what
    file_pass.check_lengths takes) only each file's first lengths[f], so that padding never reaches a batch.  The permutation is
    computed, not stored: position p of the epoch holds frame fp_permute(key, N, p) (freud_amd/csrc/frame_perm.h), evaluated inside
    the gather kernel (sae_store_gather_frames), one call per batch.

    Iteration yields (x [batch_size, T, d], []): the shape the engine, max_rows and set_topk_options(..., T) expect, and no
    filenames, because the frames of a batch share none.  The T axis carries no meaning here -- TopK's x.mean(0) is then a mean over
    batch_size unrelated frames per slot.  len(loader) = (N // world_size) // (batch_size * T) batches; the frames beyond the last
    full batch are not seen in that epoch, and they are other frames in the next one, since the key changes.  An epoch without a
    single batch is a ValueError here.  Rank r of W reads the positions r, r + W, ...: with the same seed and RNG history every rank
    draws the same key and the ranks' frames are disjoint.

    __iter__ makes exactly one draw from torch's global RNG -- the epoch's key, kept as epoch_key -- so train()'s resume works
    unchanged: skip_next = s starts at batch s of the same permutation and reads nothing of the batches before it.  The ring, the
    overlap switch, the event ordering and the once-per-epoch error word are ResidentActivationDataLoader's.  data_path may be a
    ResidentActivations (of either dtype).  Needs a GPU."""

    def __init__(self, data_path, layer_name: str, batch_size: int, dl_max_workers: int = 0, subset_size: Optional[int] = None, *,
                 lengths=None, device="cuda", rank: int = 0, world_size: int = 1, depth: int = 3, deliver_dtype: Optional[str] = None,
                 max_gb: Optional[float] = None, overlap: bool = DEFAULT_OVERLAP):
        from .file_pass import check_lengths
        if not (isinstance(batch_size, int) and batch_size >= 1 and 0 <= rank < world_size):
            raise ValueError(f"batch_size={batch_size!r}, rank={rank!r}, world_size={world_size!r}")
        ds = data_path.dataset if isinstance(data_path, ResidentActivations) else MemoryMappedActivationsDataset(data_path, layer_name, subset_size)
        n_files, T = len(ds), int(ds.tensor_shape[-2])
        trimmed = check_lengths(lengths, n_files, T)       # (before any device work)
        N = n_files * T if trimmed is None else int(trimmed.astype(np.int64).sum())
        R = batch_size * T
        if (N // world_size) // R < 1:
            raise ValueError(f"an epoch holds no batch: N = {N} counted frames over world_size = {world_size} ranks are fewer than one "
                             f"batch of R = batch_size * T = {R} frames")
        super().__init__(data_path, layer_name, batch_size, dl_max_workers, subset_size, {"shuffle": True, "drop_last": True}, device=device,
                         rank=rank, world_size=world_size, depth=depth, deliver_dtype=deliver_dtype, max_gb=max_gb, overlap=overlap)
        self.n_frames, self.rows_per_batch, self.lengths = N, R, trimmed
        self.epoch_key = None
        self._prefix = None
        if trimmed is not None:
            import torch
            prefix = np.concatenate([[0], np.cumsum(trimmed.astype(np.int64))]).astype(np.int64)
            self._prefix = torch.from_numpy(prefix).to(self.device)     # once per loader

    def __len__(self) -> int:
        return (self.n_frames // self.world_size) // self.rows_per_batch

    def epoch_batches(self):
        raise TypeError("a frame loader's batches hold frames, not files: there is no list of file indices")

    def __iter__(self):
        import torch
        from . import engine
        key = int(torch.empty((), dtype=torch.int64).random_().item())      # the epoch's key: the one draw
        self.epoch_key = key
        first, self.skip_next = self.skip_next, 0
        n = len(self)
        if first >= n:
            return
        store, R, W, rank, N, prefix = self.store, self.rows_per_batch, self.world_size, self.rank, self.n_frames, self._prefix
        T, d, B = int(store.tensor_shape[-2]), int(store.tensor_shape[-1]), self.batch_size

        def jobs(_dev):
            for b in range(first, n):
                yield (lambda buf, err, stream, b=b: engine.store_gather_frames(store.data, T, prefix, N, key, b * R * W + rank, W,
                                                                                buf.view(B * T, d), err, stream=stream),
                       lambda buf: (buf.view(B, T, d), []))

        yield from self._ring_epoch(jobs, lambda bad: f"{bad} frames of this epoch lay outside the store by the length prefix: they were "
                                                      "clamped into it, the batches are not the epoch's")
