"""GPU: the HBM-resident store (freud_amd/resident.py over include/freud_sae.h's sae_store_convert / sae_store_gather).

* the conversion on the value table of tests/resident_cases.py, bit-equal to the host library, on the vector path, its scalar tail
  and the unaligned path;
* the gather against torch's own store[idx], byte for byte, at the edges of the piece, on the 16-, 4- and 2-byte paths, into strided
  and misaligned destinations; a bad index is clamped and counted; a store beyond 2^31 elements;
* ResidentActivationDataLoader yields the batches of MemoryMappedActivationDataLoader, bit for bit;
* train() with "resident_data" writes the checkpoints of the streaming run; the overflow rules;
* FilePass over a store returns the bytes of the path-based pass."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd.loader import MemoryMappedActivationDataLoader, write_shards
from tests import resident_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- convert ----------------------------------------------------------------------------------------------------------------
def _convert(u32: np.ndarray, off: int) -> np.ndarray:
    """u32 through sae_store_convert with source and destination `off` elements into their (aligned) allocations."""
    n = u32.size
    src = torch.zeros(n + off + 8, dtype=torch.int32, device=DEV)
    src[off:off + n] = torch.from_numpy(np.array(u32.view(np.int32))).to(DEV)
    dst = torch.full((n + off + 16,), 0x1234, dtype=torch.int16, device=DEV)
    E.store_convert(src[off:off + n].view(torch.float32), dst[off:off + n].view(torch.bfloat16))
    out = dst.cpu().numpy().view(np.uint16)
    assert np.all(out[:off] == 0x1234) and np.all(out[off + n:] == 0x1234), "the conversion wrote outside its n values"
    return out[off:off + n]


@pytest.mark.parametrize("off", [0, 1])
def test_convert_whole_table(off):
    got, want, table = _convert(RC.convert_table(), off), RC.convert_expected(), RC.convert_table()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(table[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048 + 11])
def test_convert_lengths(n, off):
    """The table's tail (NaN rows of the grid, the neighbours of -1.0, the specials): whole groups of 8, the scalar tail, both."""
    table, want = RC.convert_table(), RC.convert_expected()
    np.testing.assert_array_equal(_convert(np.ascontiguousarray(table[-n:]), off), want[-n:])
    lo = 6 * 0xBF7F                                      # ... and the grid rows around 0xBF80
    np.testing.assert_array_equal(_convert(np.ascontiguousarray(table[lo:lo + n]), off), want[lo:lo + n])


# ---- gather -----------------------------------------------------------------------------------------------------------------
P = None


def _piece():
    global P
    if P is None:
        P = E.store_piece_bytes()
    return P


def _store(n_files, row_bytes, dtype, seed=0):
    es = torch.empty(0, dtype=dtype).element_size()
    assert row_bytes % es == 0
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(-2 ** 15, 2 ** 15, (n_files, row_bytes // 2), dtype=torch.int16, generator=g)
    return raw.view(dtype).to(DEV)


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def _gather(store, idx, out):
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    E.store_gather(store, torch.tensor(idx, dtype=torch.int32, device=DEV), out, err)
    return int(err.item())


ROWS = ["30", "P-16", "P", "P+16", "2P+2"]


def _row_bytes(name):
    p = _piece()
    return {"30": 30, "P-16": p - 16, "P": p, "P+16": p + 16, "2P+2": 2 * p + 2}[name]


# (an fp32 row is a multiple of 4 bytes: 30 and 2 P + 2 exist for 2-byte stores only)
@pytest.mark.parametrize("row,dtype", [(r, torch.int16) for r in ROWS] + [(r, torch.float16) for r in ROWS]
                         + [(r, torch.float32) for r in ("P-16", "P", "P+16")], ids=lambda v: v if isinstance(v, str) else str(v)[6:])
def test_gather_shapes(row, dtype):
    rb = _row_bytes(row)
    store = _store(7, rb, dtype)
    idx = [6, 5, 4, 3, 2, 1, 0, 3, 3, 0, 6]              # reversed, repeated
    want = _bytes(store.view(torch.int16)[torch.tensor(idx, device=DEV)])
    out = torch.zeros((len(idx), store.shape[1]), dtype=dtype, device=DEV)
    assert _gather(store, idx, out) == 0
    np.testing.assert_array_equal(_bytes(out), want)
    # nb = 1, into a buffer of more rows: the others stay
    out = torch.zeros((3, store.shape[1]), dtype=dtype, device=DEV)
    assert _gather(store, [4], out) == 0
    np.testing.assert_array_equal(_bytes(out[:1]), _bytes(store[4:5]))
    assert not _bytes(out[1:]).any()


@pytest.mark.parametrize("pad", [8, 2, 1], ids=["stride16", "stride4", "stride2"])
@pytest.mark.parametrize("row", ROWS)
def test_gather_into_a_strided_destination(row, pad):
    """A destination stride larger than the row (pad int16 elements more): the padding stays; the stride decides the path."""
    rb = _row_bytes(row)
    store = _store(5, rb, torch.int16, seed=1)
    idx = [4, 0, 2, 2]
    big = torch.full((len(idx), rb // 2 + pad), 0x5A5A, dtype=torch.int16, device=DEV)
    assert _gather(store, idx, big[:, :rb // 2]) == 0
    np.testing.assert_array_equal(_bytes(big[:, :rb // 2]), _bytes(store[torch.tensor(idx, device=DEV)]))
    assert bool((big[:, rb // 2:] == 0x5A5A).all())


@pytest.mark.parametrize("row", ROWS)
def test_gather_into_a_destination_two_bytes_off(row):
    rb = _row_bytes(row)
    store = _store(5, rb, torch.int16, seed=2)
    idx, n = [1, 4, 0], rb // 2
    flat = torch.full((3 * n + 9,), 0x5A5A, dtype=torch.int16, device=DEV)
    assert _gather(store, idx, flat[1:1 + 3 * n].view(3, n)) == 0
    np.testing.assert_array_equal(_bytes(flat[1:1 + 3 * n].view(3, n)), _bytes(store[torch.tensor(idx, device=DEV)]))
    assert int(flat[0]) == 0x5A5A and bool((flat[1 + 3 * n:] == 0x5A5A).all())
    # ... and a store that starts two bytes off
    sflat = torch.arange(5 * n + 1, dtype=torch.int16, device=DEV)
    s2 = sflat[1:].view(5, n)
    out = torch.zeros((3, n), dtype=torch.int16, device=DEV)
    assert _gather(s2, idx, out) == 0
    np.testing.assert_array_equal(_bytes(out), _bytes(s2[torch.tensor(idx, device=DEV)]))


def test_a_bad_index_is_clamped_and_counted():
    store = _store(5, _row_bytes("P+16"), torch.int16, seed=3)
    out = torch.zeros((5, store.shape[1]), dtype=torch.int16, device=DEV)
    assert _gather(store, [-1, 5, 2 ** 31 - 1, 2, -2 ** 31], out) == 4
    np.testing.assert_array_equal(_bytes(out), _bytes(store[torch.tensor([0, 4, 4, 2, 0], device=DEV)]))


def test_gather_argument_refusals():
    store = _store(3, 64, torch.int16)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    for bad_out in (torch.zeros((1, 32), dtype=torch.int16, device=DEV), torch.zeros((2, 31), dtype=torch.int16, device=DEV),
                    torch.zeros((2, 32), dtype=torch.float16, device=DEV), torch.zeros((2, 64), dtype=torch.int16, device=DEV)[:, ::2]):
        with pytest.raises(E.EngineError, match="out must be"):
            E.store_gather(store, idx, bad_out, err)
    with pytest.raises(E.EngineError, match="idx must be"):
        E.store_gather(store, idx.long(), torch.zeros((2, 32), dtype=torch.int16, device=DEV), err)
    odd = torch.zeros((3, 5), dtype=torch.uint8, device=DEV)
    with pytest.raises(E.EngineError, match="multiples of 2 bytes"):
        E.store_gather(odd, idx, torch.zeros((2, 5), dtype=torch.uint8, device=DEV), err)


def test_gather_from_a_store_beyond_2_31_elements():
    """2^31 int16 elements and three rows more, allocated and not filled: one file near the end is written and gathered -- its offset
    does not fit 32 bits in elements, let alone in bytes."""
    row, n_files = 1024, (1 << 21) + 3
    free, _total = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip("needs 6 GB of free device memory")
    store = torch.empty((n_files, row), dtype=torch.int16, device=DEV)
    assert store.numel() > 2 ** 31
    f = n_files - 2
    store[f] = torch.arange(row, dtype=torch.int16, device=DEV) * 3 + 1
    out = torch.zeros((2, row), dtype=torch.int16, device=DEV)
    assert _gather(store, [f, f], out) == 0
    want = (np.arange(row, dtype=np.int16) * 3 + 1)
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([want, want]))
    del store


# ---- loader -----------------------------------------------------------------------------------------------------------------
N_FILES, T, D = 23, 5, 384


@pytest.fixture(scope="module")
def shard_dirs(tmp_path_factory):
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((N_FILES, T * D)).astype(np.float32)
    rows[3, :7] = [-1.0, np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(-2)), np.nan, np.inf, 0.0, -0.0]
    out = {}
    for name, dt in (("f32", np.float32), ("f16", np.float16)):
        p = str(tmp_path_factory.mktemp("resident_" + name))
        write_shards(p, "L", rows.astype(dt), [T, D])
        out[name] = p
    return out


def _epochs(loader, n=2, skip=0):
    loader.skip_next = skip
    out = []
    for _ in range(n):
        for x, names in loader:
            out.append((x.clone().cpu(), list(names)))
    return out


@pytest.mark.parametrize("overlap", [True, False], ids=["side", "inline"])
@pytest.mark.parametrize("shards,deliver", [("f32", "native"), ("f32", "bfloat16"), ("f16", "native")])
def test_loader_yields_the_streaming_loaders_batches(shard_dirs, shards, deliver, overlap):
    from freud_amd.resident import ResidentActivationDataLoader, ResidentActivations
    path = shard_dirs[shards]
    store = ResidentActivations(path, "L", device=DEV, dtype=deliver)
    assert store.tensor_shape == [T, D] and len(store.filenames) == N_FILES and store.metadata["tensor_shape"] == [T, D]
    want_dtype = {"f32": torch.float32, "f16": torch.float16}[shards] if deliver == "native" else \
        (torch.bfloat16 if shards == "f32" else torch.float16)
    assert store.data.dtype == want_dtype and store.nbytes == N_FILES * T * D * store.data.element_size() == store.data.numel() * store.data.element_size()
    kw = {"shuffle": True, "drop_last": True}
    for rank, world, skip, batch in ((0, 1, 0, 4), (1, 2, 0, 3), (0, 1, 2, 4)):
        torch.manual_seed(7)
        ref = MemoryMappedActivationDataLoader(path, "L", batch, 0, None, kw, device=DEV, rank=rank, world_size=world, deliver_dtype=deliver)
        want = _epochs(ref, skip=skip)
        state_after = torch.get_rng_state()
        torch.manual_seed(7)
        dl = ResidentActivationDataLoader(store, "L", batch, 0, None, kw, rank=rank, world_size=world, overlap=overlap)
        assert len(dl) == len(ref) and dl.activation_shape == ref.activation_shape and dl.dataset_length == ref.dataset_length
        assert dl.dataset.tensor_shape == ref.dataset.tensor_shape
        got = _epochs(dl, skip=skip)
        assert torch.equal(torch.get_rng_state(), state_after)           # the same draws
        assert len(got) == len(want) == 2 * len(ref) - skip and len(want) > 0
        for (xg, ng), (xw, nw) in zip(got, want):
            assert ng == nw and xg.dtype == xw.dtype and xg.shape == xw.shape
            np.testing.assert_array_equal(_bytes(xg), _bytes(xw))


def test_loader_from_a_path_follows_the_delivery_default(shard_dirs, monkeypatch):
    from freud_amd.resident import ResidentActivationDataLoader
    monkeypatch.setenv("FREUD_LOADER_DELIVER", "bfloat16")
    state = torch.get_rng_state()
    dl = ResidentActivationDataLoader(shard_dirs["f32"], "L", 4, 0, 10, {"shuffle": False}, device=DEV)
    assert torch.equal(torch.get_rng_state(), state)                     # the upload leaves the global RNG alone
    assert dl.store.data.dtype == torch.bfloat16 and len(dl.store) == 10 and not dl.store.native
    ref = MemoryMappedActivationDataLoader(shard_dirs["f32"], "L", 4, 0, 10, {"shuffle": False}, device=DEV)
    for (xg, ng), (xw, nw) in zip(_epochs(dl, 1), _epochs(ref, 1)):
        assert ng == nw
        np.testing.assert_array_equal(_bytes(xg), _bytes(xw))


# ---- train() ----------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _train(tmp_path_factory, golden_dir, fixture, extra=None, deliver=None):
    """One train() run on a golden fixture -> its last checkpoint (a streaming run is shared by the tests that compare with it)."""
    from freud_amd.train_sae import train
    key = (fixture, deliver) if extra is None else None
    if key in _RUNS:
        return _RUNS[key]
    z = np.load(os.path.join(golden_dir, f"{fixture}.npz"))
    meta = json.loads(str(z["meta"]))
    tmp = str(tmp_path_factory.mktemp("resident_train"))
    folder = os.path.join(tmp, "train")
    write_shards(folder, meta["layer"], z["shard"], [meta["T"], meta["d"]], [f"/data/audio/file_{i:04d}.flac" for i in range(meta["n_files"])])
    cfg = copy.deepcopy(meta["config"])
    cfg.update(train_folder=folder, val_folder=folder, run_dir=os.path.join(tmp, "run"), device="cuda", **(extra or {}))
    old = os.environ.pop("FREUD_LOADER_DELIVER", None)
    try:
        if deliver is not None:
            os.environ["FREUD_LOADER_DELIVER"] = deliver
        train(**cfg)
    finally:
        os.environ.pop("FREUD_LOADER_DELIVER", None)
        if old is not None:
            os.environ["FREUD_LOADER_DELIVER"] = old
    ck_dir = os.path.join(cfg["run_dir"], "checkpoints")
    last = max((f for f in os.listdir(ck_dir) if f.startswith("step")), key=lambda f: int(f[4:-4]))
    ck = torch.load(os.path.join(ck_dir, last), map_location="cpu", weights_only=True)
    if key is not None:
        _RUNS[key] = ck
    return ck


def _same(a, b, where="ck"):
    """Parameters, moments and step of two checkpoints: byte-equal."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b)), where
    else:
        assert a == b, where


def _same_run(a, b):
    assert a["step"] == b["step"] and a["step"] > 0
    _same(a["model"], b["model"], "model")
    _same(a["optimizer"], b["optimizer"], "optimizer")


@pytest.mark.parametrize("dtype", ["native", "bfloat16"])
@pytest.mark.parametrize("fixture", ["trainloop_l1", "trainloop_topk"])
def test_resident_training_writes_the_streaming_runs_checkpoint(tmp_path_factory, golden_dir, fixture, dtype):
    streaming = _train(tmp_path_factory, golden_dir, fixture, deliver=None if dtype == "native" else "bfloat16")
    key = True if dtype == "native" else {"dtype": "bfloat16"}
    resident = _train(tmp_path_factory, golden_dir, fixture, extra={"resident_data": key})
    _same_run(resident, streaming)
    assert resident["hparams"]["resident_data"] == key and "resident_data" not in streaming["hparams"]


def test_overflow(tmp_path_factory, golden_dir, shard_dirs, capsys):
    from freud_amd.resident import ResidentActivations, ResidentOverflow
    need = N_FILES * T * D * 4
    with pytest.raises(ResidentOverflow, match=rf"needs {need} bytes .* may take {need - 1} bytes"):
        ResidentActivations(shard_dirs["f32"], "L", device=DEV, max_gb=(need - 1) / 2 ** 30)
    assert ResidentActivations(shard_dirs["f32"], "L", device=DEV, max_gb=need / 2 ** 30).nbytes == need
    with pytest.raises(ResidentOverflow):
        _train(tmp_path_factory, golden_dir, "trainloop_l1", extra={"resident_data": {"max_gb": 1e-9}})
    capsys.readouterr()
    fell_back = _train(tmp_path_factory, golden_dir, "trainloop_l1", extra={"resident_data": {"max_gb": 1e-9, "on_overflow": "stream"}})
    assert "streaming the shards instead" in capsys.readouterr().out
    _same_run(fell_back, _train(tmp_path_factory, golden_dir, "trainloop_l1"))


# ---- FilePass ---------------------------------------------------------------------------------------------------------------
def _npz_bytes(result, path):
    result.to_npz(path)
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_file_pass_over_a_store(shard_dirs, tmp_path):
    from freud_amd.config import TopKAutoEncoderConfig
    from freud_amd.feature_stats import feature_stats
    from freud_amd.models import TopKAutoEncoder
    from freud_amd.reconstruction import reconstruction_report
    from freud_amd.resident import ResidentActivations
    torch.manual_seed(3)
    sae = TopKAutoEncoder(D, TopKAutoEncoderConfig(n_dict_components=512, k=8), max_rows=1536)
    path = shard_dirs["f16"]
    store = ResidentActivations(path, "L", device=DEV)
    lens = np.arange(N_FILES) % T + 1
    for fn, kw in ((feature_stats, {}), (reconstruction_report, {}), (feature_stats, {"subset_size": 9})):
        sub = kw.get("subset_size", N_FILES)
        a = _npz_bytes(fn(sae, path, "L", lengths=lens[:sub], batch_files=4, **kw), str(tmp_path / "a.npz"))
        b = _npz_bytes(fn(sae, store, "L", lengths=lens[:sub], batch_files=4, **kw), str(tmp_path / "b.npz"))
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (fn.__name__, k)
    # the passes promise native values: a converted store is refused, and so is a pass that reads the files itself
    with pytest.raises(ValueError, match="shards' own values"):
        feature_stats(sae, ResidentActivations(shard_dirs["f32"], "L", device=DEV, dtype="bfloat16"), "L")
    from freud_amd.feature_search import top_activations
    with pytest.raises(TypeError, match="data_path must be the path of a shard directory"):
        top_activations(sae, store, "L", 0, 3, None, None, False, False)
