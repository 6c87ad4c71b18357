"""One GPU pass over a shard directory in batches of files: what the feature search (feature_search.py) and the feature statistics
(feature_stats.py) share.  Both encode batches of files with the training kernels and keep a reduction instead of the latent; this
module owns the argument rules, the choice of the batch size, the walk over the shard loader and the front and tail of the passes'
command lines.  It imports without torch (the feature index's reader takes check_lengths from here): torch is imported where a pass
runs."""
from __future__ import annotations

import functools
import json
from typing import Optional

import numpy as np


def check_lengths(lengths, n_total: int, T: int) -> Optional[np.ndarray]:
    """Trim lengths (frames per file, in file order) -> int32 capped at T; a length below 1 is an error (the reference fails on
    max() of an empty series)."""
    if lengths is None:
        return None
    a = np.asarray(lengths)
    if a.ndim != 1 or a.shape[0] != n_total:
        raise ValueError(f"lengths must hold one entry per file ({n_total}), got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"lengths must be integers, got {a.dtype}")
    if a.size and int(a.min()) < 1:
        raise ValueError(f"lengths must be >= 1 (file {int(np.argmin(a))} has {int(a.min())}): an empty series has no maximum")
    return np.minimum(a.astype(np.int64), T).astype(np.int32)


def is_raw(sae) -> bool:
    """Whether `sae` asks for raw mode: None, or the command lines' "none"."""
    return sae is None or (isinstance(sae, str) and sae.lower() == "none")


def resolve_sae(sae):
    """None (raw mode) | checkpoint path | freud_amd.models instance | SaeEngine -> (model or None, engine or None)."""
    if is_raw(sae):
        return None, None
    if isinstance(sae, str):
        from .models import init_sae_from_checkpoint
        sae = init_sae_from_checkpoint(sae)
    from .engine import SaeEngine
    if isinstance(sae, SaeEngine):
        return None, sae
    if not hasattr(sae, "_ensure"):
        raise TypeError(f"sae must be None, a checkpoint path, a freud_amd.models SAE or a SaeEngine, got {type(sae).__name__}")
    return sae, None


def default_batch_files(T: int, n: Optional[int], n_total: int) -> int:
    """Files per batch when the caller gives none: 16, or for an L1 / TopK SAE the fewest files at which the encoder GEMM has the
    2048 output tiles of 256 x 256 that its streaming form (gemm256s.h: gemm_launch.h gemm_streams, 4 x G2_PERSIST_STATIC) needs, so
    that an L1 pass takes the fused epilogue (n = 3072, T = 1500: 30 files; n = 40 960: 16).  Dictionaries whose padded size is
    no multiple of 256 never stream; above 512 files the batch stays at 16 (n < 1024) and the latent is stored and reduced."""
    B = 16
    if n is not None:
        n_p = -(-n // 128) * 128
        if n_p % 256 == 0:
            need = -(-2048 // (n_p // 256))                  # 256-row blocks of the batch
            b_min = ((need - 1) * 256) // T + 1              # round_up(B T, 256) / 256 >= need
            if b_min <= 512:
                B = max(B, b_min)
    return max(1, min(B, n_total))


def keep_rng(fn):
    """A pass must not disturb the caller's global torch RNG: the loader's epoch_batches() draws the DataLoader base seed, and
    building a model from a checkpoint runs the reference modules' random initialisations before the weights are loaded."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        import torch
        state = torch.get_rng_state()
        try:
            return fn(*a, **k)
        finally:
            torch.set_rng_state(state)
    return wrapped


class FilePass:
    """The set-up of one pass, then its batches.  `sae`: see resolve_sae (None: raw mode, no engine); `what` is the noun of the
    error messages ("feature search", "feature statistics").  `max_frames`: a pass over more than this many frames (files x T) is
    refused.  Every check that needs no device comes before the one that does.  `data_path`: the shard directory, or a
    freud_amd.resident.ResidentActivations of it in the shards' own dtype -- then the batches are zero-copy slices of the store and
    nothing crosses the host link.

    Attributes: model, eng (None in raw mode), device, T, d, n_total, n_frames (the frames that count: the trimmed lengths, or
    files x T), batch_files, filenames.  Iterating yields
    (x [nb, T, d] on `device` in the shards' dtype, file0, nb, lengths[file0:file0 + nb] on `device` or None) in file order."""

    def __init__(self, sae, data_path: str, layer_name: str, *, what: str, lengths=None, subset_size: Optional[int] = None,
                 batch_files: Optional[int] = None, max_frames: Optional[int] = None):
        import torch
        from .loader import MemoryMappedActivationsDataset

        if batch_files is not None and int(batch_files) < 1:
            raise ValueError(f"batch_files={batch_files} must be >= 1")
        from .resident import ResidentActivations
        store = data_path if isinstance(data_path, ResidentActivations) else None
        if store is not None:
            # a resident store in place of the directory: its first subset_size files, as zero-copy slices (__iter__)
            if store.layer_name != layer_name:
                raise ValueError(f"the store holds layer {store.layer_name!r}, the {what} asks for {layer_name!r}")
            if not store.native:
                raise ValueError(f"the {what} reads the shards' own values: the store holds them converted to {store.data.dtype}")
            if subset_size is not None and not 0 <= int(subset_size) <= len(store):
                raise ValueError(f"subset_size={subset_size} outside the store's {len(store)} files")
            ds = store.dataset
            n_total = len(store) if subset_size is None else int(subset_size)
        else:
            ds = MemoryMappedActivationsDataset(data_path, layer_name, subset_size)
            n_total = len(ds)
        if n_total == 0:
            raise ValueError(f"{data_path}: no files")
        T, d = int(ds.tensor_shape[-2]), int(ds.tensor_shape[-1])
        if max_frames is not None and n_total * T > max_frames:
            raise ValueError(f"{n_total} files x {T} frames exceed the {max_frames} frames of one {what} pass")
        self._lens = check_lengths(lengths, n_total, T)
        self.n_frames = int(self._lens.sum(dtype=np.int64)) if self._lens is not None else n_total * T
        model, eng = resolve_sae(sae)
        runs = f"the {what} run{'' if what.endswith('s') else 's'}"

        def bf16_only(e):
            if e.precision != "bf16":
                raise ValueError(f"{runs} in bf16 contexts only")

        n = None
        if eng is not None or model is not None:
            sae_d, n = (eng.d, eng.n) if eng is not None else (model.activation_size, model.n_dict_components)
            if sae_d != d:
                raise ValueError(f"the SAE expects d_model={sae_d}, the shards hold d={d}")
        if eng is not None:
            bf16_only(eng)
        if not torch.cuda.is_available():
            raise RuntimeError(f"{runs} on the GPU (HIP engine); there is no CPU path")
        B = int(batch_files) if batch_files is not None else default_batch_files(T, n, n_total)
        B = min(B, n_total)
        if model is not None:
            eng = model._ensure(-(-B * T // 256) * 256)     # (row room for an even number of 128-row blocks: the fused epilogue's GEMM)
            bf16_only(eng)
            dev = model.device
        elif eng is not None:
            dev = torch.device("cuda", eng.device_id)
            if B * T > eng.max_rows:
                B = max(1, eng.max_rows // T)
                if B * T > eng.max_rows:
                    raise ValueError(f"one file of {T} rows exceeds the engine's max_rows={eng.max_rows}")
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.model, self.eng, self.device = model, eng, dev
        self.T, self.d, self.n_total, self.batch_files = T, d, n_total, B
        self.filenames = list(ds.metadata["filenames"])[:n_total]
        if store is not None and store.device.index != (dev.index if dev.index is not None else torch.cuda.current_device()):
            raise ValueError(f"the store lives on {store.device}, the {what} runs on {dev}")
        self._store = store
        self._loader_args = (data_path, layer_name, subset_size)

    def check_counted(self, counted: int) -> None:
        """The frames the engine counted on the device must be the frames of the pass."""
        if int(counted) != self.n_frames:
            raise RuntimeError(f"the engine counted {int(counted)} frames, the pass holds {self.n_frames}")

    def __iter__(self):
        import torch
        from .loader import MemoryMappedActivationDataLoader

        data_path, layer_name, subset_size = self._loader_args
        lens_dev = torch.from_numpy(self._lens).to(self.device) if self._lens is not None else None
        if self._store is not None:
            for file0 in range(0, self.n_total, self.batch_files):
                nb = min(self.batch_files, self.n_total - file0)
                yield (self._store.data[file0:file0 + nb].view(nb, self.T, self.d), file0, nb,
                       lens_dev[file0:file0 + nb] if lens_dev is not None else None)
            return
        # (native delivery whatever FREUD_LOADER_DELIVER says, no shuffle: raw mode sees x unrounded, an SAE what encode() of the
        # shard rows sees)
        loader = MemoryMappedActivationDataLoader(data_path, layer_name, self.batch_files, subset_size=subset_size,
                                                  dl_kwargs={"shuffle": False, "drop_last": False}, device=self.device,
                                                  deliver_dtype="native")
        file0 = 0
        for x, _names in loader:
            nb = int(x.shape[0])
            yield x, file0, nb, (lens_dev[file0:file0 + nb] if lens_dev is not None else None)
            file0 += nb
        if file0 != self.n_total:
            raise RuntimeError(f"the loader delivered {file0} of {self.n_total} files")


def add_pass_arguments(ap, sae_help: str = "checkpoint path", *, sae: bool = True, out_required: bool = True) -> None:
    """The arguments that every pass's command line takes (--data-path and --layer-name are also spelled with an underscore).
    sae=False: a pass without a dictionary takes neither --sae nor --batch_files; out_required=False: --out is optional."""
    if sae:
        ap.add_argument("--sae", required=True, help=sae_help)
    ap.add_argument("--data_path", "--data-path", dest="data_path", required=True)
    ap.add_argument("--layer_name", "--layer-name", dest="layer_name", required=True)
    ap.add_argument("--lengths", default=None, help=".npy of int frames per file (file order); default: the full T")
    if sae:
        ap.add_argument("--batch_files", type=int, default=None)
    ap.add_argument("--out", required=out_required, default=None)


def run_pass_cli(a, run) -> None:
    """The tail of a pass's command line over its parsed arguments: result = run(the --lengths array or None), stored as a.out
    (where one is given), and one JSON line of its summary()."""
    result = run(np.load(a.lengths) if a.lengths else None)
    if a.out:
        result.to_npz(a.out)
    print(json.dumps({"out": a.out, **result.summary()}))
