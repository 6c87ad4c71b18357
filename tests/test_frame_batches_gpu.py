"""GPU: frame batches (freud_amd/resident.py, ResidentFrameDataLoader, over include/freud_sae.h's sae_store_gather_frames).

* the kernel against store.view(n T, d)[rows] with the rows of tests/frame_batches_reference.py, byte for byte: frames of 2 bytes to
  more than a workgroup's span, on the 16-, 4- and 2-byte paths, trimmed and untrimmed, strided positions, padded and misaligned
  destinations, no ordinals, no rows; every refusal leaves the error word and the destination alone; a malformed prefix is clamped
  and counted; a store beyond 2^32 bytes;
* the loader: every rank's batches are the reference's, the ranks' frames are distinct and never padding, one RNG draw per epoch,
  skip_next, both overlap settings, three shard / delivery dtypes;
* train() with "frame_batches": reproducible, not the file-batch run, recorded, resumable mid-epoch to the byte, refused when the
  key changes; a recording engine sees the reference's batches."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd.loader import write_shards
from tests import frame_batches_reference as REF

pytestmark = pytest.mark.gpu
DEV = "cuda"

N_FILES, T = 7, 12
LENGTHS = [12, 1, 5, 12, 3, 7, 9]
SPAN_BYTES = 1024 * 16                                   # what one workgroup moves at the widest unit (frame_perm.h: FP_SPAN_UNITS)
FRAME_BYTES = (2, 10, 24, 32, 48, 768, 1536, 5120, SPAN_BYTES + 16)
KEY = 0x9F3A5C7E12B4D680


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def _store(frame_bytes, seed=0, n_files=N_FILES, rows_per_file=T):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 15, 2 ** 15, (n_files, rows_per_file * frame_bytes // 2), dtype=torch.int16, generator=g).to(DEV)


def _prefix(lengths):
    return None if lengths is None else torch.from_numpy(REF.prefix_of(lengths)).to(DEV)


def _want_rows(lengths, pos0, stride, rows, key=KEY, n_files=N_FILES, rows_per_file=T):
    N = REF.frame_count(n_files, rows_per_file, lengths)
    return REF.store_rows(key, N, [pos0 + j * stride for j in range(rows)], n_files, rows_per_file, lengths)


def _row_counts(N, pos0, stride):
    most = (N - 1 - pos0) // stride + 1
    return sorted({min(r, most) for r in (1, 3, 64, 257)})


@pytest.mark.parametrize("lengths", [None, LENGTHS], ids=["untrimmed", "trimmed"])
@pytest.mark.parametrize("frame_bytes", FRAME_BYTES)
def test_gathered_frames_are_the_references(frame_bytes, lengths):
    store, d = _store(frame_bytes), frame_bytes // 2
    frames = store.view(N_FILES * T, d)
    N = REF.frame_count(N_FILES, T, lengths)
    assert N == (84 if lengths is None else 49)
    prefix = _prefix(lengths)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pos0, stride in ((0, 1), (1, 2), (3, 4)):
        for rows in _row_counts(N, pos0, stride):
            want = _want_rows(lengths, pos0, stride, rows)
            out = torch.full((rows + 1, d), 0x5A5A, dtype=torch.int16, device=DEV)
            ordinals = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
            E.store_gather_frames(store, T, prefix, N, KEY, pos0, stride, out[:rows], err, ordinals=ordinals)
            got_rows = ordinals.cpu().numpy()
            np.testing.assert_array_equal(got_rows, want)
            np.testing.assert_array_equal(_bytes(out[:rows]), _bytes(frames[ordinals]))
            assert bool((out[rows] == 0x5A5A).all()), "the gather wrote past its rows"
            if stride == 1 and rows == N:
                assert np.array_equal(np.sort(got_rows), np.sort(REF.ordinals_to_rows(np.arange(N), N_FILES, T, lengths)))
    assert int(err.item()) == 0


@pytest.mark.parametrize("frame_bytes", FRAME_BYTES)
def test_padded_and_misaligned_destinations_no_ordinals_no_rows(frame_bytes):
    store, d = _store(frame_bytes, seed=1), frame_bytes // 2
    frames = store.view(N_FILES * T, d)
    prefix, N, rows = _prefix(LENGTHS), 49, 23
    want = torch.from_numpy(_want_rows(LENGTHS, 2, 2, rows)).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pad in (8, 2, 1):                                # a destination stride 16, 4, 2 bytes beyond the frame: the padding stays
        big = torch.full((rows, d + pad), 0x5A5A, dtype=torch.int16, device=DEV)
        E.store_gather_frames(store, T, prefix, N, KEY, 2, 2, big[:, :d], err)
        np.testing.assert_array_equal(_bytes(big[:, :d]), _bytes(frames[want]))
        assert bool((big[:, d:] == 0x5A5A).all())
    flat = torch.full((rows * d + 9,), 0x5A5A, dtype=torch.int16, device=DEV)       # a destination two bytes off
    E.store_gather_frames(store, T, prefix, N, KEY, 2, 2, flat[1:1 + rows * d].view(rows, d), err)
    np.testing.assert_array_equal(_bytes(flat[1:1 + rows * d]), _bytes(frames[want]))
    assert int(flat[0]) == 0x5A5A and bool((flat[1 + rows * d:] == 0x5A5A).all())
    sflat = torch.randint(-2 ** 15, 2 ** 15, (N_FILES * T * d + 1,), dtype=torch.int16).to(DEV)      # a store two bytes off
    s2 = sflat[1:].view(N_FILES, T * d)
    out = torch.zeros((rows, d), dtype=torch.int16, device=DEV)
    E.store_gather_frames(s2, T, prefix, N, KEY, 2, 2, out, err)
    np.testing.assert_array_equal(_bytes(out), _bytes(s2.view(-1, d)[want]))
    none = torch.full((4, d), 0x5A5A, dtype=torch.int16, device=DEV)                 # rows = 0: a no-op that succeeds
    E.store_gather_frames(store, T, prefix, N, KEY, 0, 1, none[:0], err)
    E.store_gather_frames(store, T, prefix, N, KEY, N + 5, 0, none[:0], err)
    assert bool((none == 0x5A5A).all()) and int(err.item()) == 0


def _raw(store, rows_per_file, frame_bytes, prefix, n_frames, pos0, stride, rows, out, out_stride, err, n_files=None, store_ptr=None,
         out_ptr=None):
    return E.load().sae_store_gather_frames(C.c_void_p(store_ptr if store_ptr is not None else store.data_ptr()),
                                            store.shape[0] if n_files is None else n_files, rows_per_file, frame_bytes,
                                            None if prefix is None else C.c_void_p(prefix.data_ptr()), n_frames, KEY, pos0, stride, rows,
                                            C.c_void_p(out_ptr if out_ptr is not None else out.data_ptr()), out_stride,
                                            None, C.c_void_p(err.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_refusals_leave_the_error_word_and_the_destination_alone():
    fb = 32
    store = _store(fb, seed=2)
    out = torch.full((8, fb // 2), 0x5A5A, dtype=torch.int16, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    prefix = _prefix(LENGTHS)
    ok = dict(store=store, rows_per_file=T, frame_bytes=fb, prefix=None, n_frames=84, pos0=0, stride=1, rows=8, out=out, out_stride=fb, err=err)
    refused = {
        "rows < 0": dict(rows=-1),
        "the last position is N": dict(pos0=77),
        "the last position leaves N by the stride": dict(pos0=3, stride=12),
        "pos0 < 0": dict(pos0=-1),
        "pos0 = N": dict(pos0=84, rows=1),
        "stride 0": dict(stride=0),
        "the last position overflows 64 bits": dict(stride=2 ** 62, rows=8),
        "N beyond the store": dict(n_frames=85),
        "N beyond the trimmed store's room": dict(prefix=prefix, n_frames=85),
        "N = 0": dict(n_frames=0, rows=0),
        "N < 0": dict(n_frames=-3),
        "no files": dict(n_files=0),
        "an odd store address": dict(store_ptr=store.data_ptr() + 1),
        "an odd destination address": dict(out_ptr=out.data_ptr() + 1),
        "an odd frame": dict(frame_bytes=31, out_stride=32),
        "an odd destination stride": dict(out_stride=33),
        "a destination stride below the frame": dict(out_stride=30),
    }
    for name, change in refused.items():
        assert _raw(**{**ok, **change}) != 0, name
        assert name and E.load().sae_last_error()
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and bool((out == 0x5A5A).all())
    assert _raw(**ok) == 0 and _raw(**{**ok, "rows": 0, "pos0": 99}) == 0
    np.testing.assert_array_equal(_bytes(out), _bytes(store.view(-1, fb // 2)[torch.from_numpy(_want_rows(None, 0, 1, 8)).to(DEV)]))
    # the binding's own checks
    for bad_out in (torch.zeros((2, 15), dtype=torch.int16, device=DEV), torch.zeros((2, 16), dtype=torch.float16, device=DEV),
                    torch.zeros((2, 32), dtype=torch.int16, device=DEV)[:, ::2], torch.zeros((2, 16), dtype=torch.int16)):
        with pytest.raises(E.EngineError, match="out must be"):
            E.store_gather_frames(store, T, None, 84, KEY, 0, 1, bad_out, err)
    good = torch.zeros((2, 16), dtype=torch.int16, device=DEV)
    with pytest.raises(E.EngineError, match="store must be"):
        E.store_gather_frames(store, 5, None, 84, KEY, 0, 1, good, err)
    with pytest.raises(E.EngineError, match="prefix must be"):
        E.store_gather_frames(store, T, prefix[:-1], 49, KEY, 0, 1, good, err)
    with pytest.raises(E.EngineError, match="prefix must be"):
        E.store_gather_frames(store, T, prefix.int(), 49, KEY, 0, 1, good, err)
    with pytest.raises(E.EngineError, match="ordinals must be"):
        E.store_gather_frames(store, T, None, 84, KEY, 0, 1, good, err, ordinals=torch.zeros(3, dtype=torch.int64, device=DEV))


def test_a_malformed_prefix_is_clamped_and_counted():
    fb = 48
    store, d = _store(fb, seed=3), fb // 2
    bad_prefix = torch.tensor([0, 30, 31, 36, 48, 51, 58, 84], dtype=torch.int64, device=DEV)      # file 0 claims 30 frames of its 12
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros((84, d), dtype=torch.int16, device=DEV)
    ordinals = torch.zeros(84, dtype=torch.int64, device=DEV)
    E.store_gather_frames(store, T, bad_prefix, 84, KEY, 0, 1, out, err, ordinals=ordinals)
    rows = ordinals.cpu().numpy()
    assert int(err.item()) == 18 + 14 and rows.min() >= 0 and rows.max() < N_FILES * T       # t in [12, 30) of file 0; [12, 26) of file 6
    np.testing.assert_array_equal(_bytes(out), _bytes(store.view(-1, d)[ordinals]))


def test_padding_never_reaches_a_launch():
    fb, sentinel = 24, 0x7F7F
    d = fb // 2
    store = torch.randint(-2 ** 14, 2 ** 14, (N_FILES, T, d), dtype=torch.int16).to(DEV)
    for f, n in enumerate(LENGTHS):
        store[f, n:] = sentinel
    store = store.view(N_FILES, T * d)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for key in (1, 2):
        out = torch.zeros((49, d), dtype=torch.int16, device=DEV)
        E.store_gather_frames(store, T, _prefix(LENGTHS), 49, key, 0, 1, out, err)
        assert not bool((out == sentinel).any())
        assert np.array_equal(np.sort(_bytes(out).view(np.int16).reshape(49, d), axis=0),
                              np.sort(_bytes(store.view(-1, d)[(store.view(-1, d) != sentinel).all(1)]).view(np.int16).reshape(49, d), axis=0))


def test_a_store_beyond_2_32_bytes():
    """2^33 bytes and three files more, allocated and not filled: the frames a 64-row launch reads are planted and gathered -- the
    byte offsets of about half of them do not fit 32 bits."""
    d, rpf, n_files = 512, 8, (1 << 20) + 3
    store = torch.empty((n_files, rpf * d), dtype=torch.int16, device=DEV)
    assert store.numel() * 2 > 2 ** 32
    N = n_files * rpf
    want = REF.store_rows(KEY, N, [5 + 3 * j for j in range(64)], n_files, rpf)
    assert (want * d * 2 >= 2 ** 32).sum() > 8 and len(set(want.tolist())) == 64
    planted = torch.randint(-2 ** 15, 2 ** 15, (64, d), dtype=torch.int16).to(DEV)
    rows = torch.from_numpy(want).to(DEV)
    store.view(-1, d)[rows] = planted
    out = torch.zeros((64, d), dtype=torch.int16, device=DEV)
    ordinals = torch.zeros(64, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    E.store_gather_frames(store, rpf, None, N, KEY, 5, 3, out, err, ordinals=ordinals)
    np.testing.assert_array_equal(ordinals.cpu().numpy(), want)
    np.testing.assert_array_equal(_bytes(out), _bytes(planted))
    assert int(err.item()) == 0
    del store


# ---- loader -----------------------------------------------------------------------------------------------------------------
LN_FILES, LT, LD, LB = 9, 6, 24, 2
L_LENGTHS = [6, 1, 5, 6, 3, 2, 6, 4, 6]
PAD = 1024.0                                             # exact in fp32, fp16 and bf16; no N(0, 1) draw equals it


@pytest.fixture(scope="module")
def shard_dirs(tmp_path_factory):
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((LN_FILES, LT, LD)).astype(np.float32)
    for f, n in enumerate(L_LENGTHS):
        rows[f, n:] = PAD
    rows = rows.reshape(LN_FILES, LT * LD)
    out = {}
    for name, dt in (("f32", np.float32), ("f16", np.float16)):
        p = str(tmp_path_factory.mktemp("frames_" + name))
        write_shards(p, "L", rows.astype(dt), [LT, LD])
        out[name] = p
    return out


def _epochs(loader, n=2, skip=0):
    """-> [(key, [batch, ...])] of n epochs."""
    loader.skip_next = skip
    out = []
    for _ in range(n):
        got = []
        for x, names in loader:
            assert names == [] and tuple(x.shape) == (LB, LT, LD)
            got.append(x.clone().cpu())
        out.append((loader.epoch_key, got))
    return out


@pytest.mark.parametrize("overlap", [True, False], ids=["side", "inline"])
@pytest.mark.parametrize("shards,deliver", [("f32", "native"), ("f32", "bfloat16"), ("f16", "native")])
@pytest.mark.parametrize("lengths", [None, L_LENGTHS], ids=["untrimmed", "trimmed"])
def test_loader_delivers_the_references_batches(shard_dirs, shards, deliver, overlap, lengths):
    from freud_amd.resident import ResidentActivations, ResidentFrameDataLoader
    store = ResidentActivations(shard_dirs[shards], "L", device=DEV, dtype=deliver)
    host = store.data.cpu().view(torch.int16 if store.data.element_size() == 2 else torch.int32).numpy()
    N, R = REF.frame_count(LN_FILES, LT, lengths), LB * LT
    pad = torch.tensor(PAD, dtype=store.data.dtype)
    np_lengths = None if lengths is None else np.array(lengths)
    seen = {}
    for rank, world, skip in ((0, 1, 0), (0, 2, 0), (1, 2, 0), (0, 1, 2)):
        dl = ResidentFrameDataLoader(store, "L", LB, lengths=np_lengths, rank=rank, world_size=world, overlap=overlap)
        n = len(dl)
        assert n == REF.len_loader(N, R, world) and n >= 1 and dl.n_frames == N
        torch.manual_seed(7)
        keys = [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(2)]      # the draws, made by hand
        state_after = torch.get_rng_state()
        torch.manual_seed(7)
        got = _epochs(dl, skip=skip)
        assert torch.equal(torch.get_rng_state(), state_after), "an epoch is exactly one draw"
        assert [k for k, _ in got] == keys and keys[0] != keys[1]
        for e, (key, batches) in enumerate(got):
            first = skip if e == 0 else 0
            assert len(batches) == n - first
            ordinals = REF.epoch_ordinals(key, N, R, rank, world, n, first_batch=first)
            assert ordinals.min() >= 0 and ordinals.max() < N
            rows = REF.ordinals_to_rows(ordinals, LN_FILES, LT, lengths)
            want = REF.build_batches(host, LT, LD, rows)
            for b, x in enumerate(batches):
                assert x.dtype == store.data.dtype
                np.testing.assert_array_equal(_bytes(x), want[b].reshape(-1).view(np.uint8))
                if lengths is not None:
                    assert not bool((x == pad).any()), "padding in a batch"
            seen[(world, rank, skip, e)] = ordinals
        assert not torch.equal(got[0][1][-1], got[1][1][-1]), "two epochs deliver the same last batch"
    # the ranks of a world: distinct frames, world * len * R of them
    for e in (0, 1):
        both = np.concatenate([seen[(2, 0, 0, e)].reshape(-1), seen[(2, 1, 0, e)].reshape(-1)])
        assert both.size == 2 * REF.len_loader(N, R, 2) * R == np.unique(both).size
        one = seen[(1, 0, 0, e)].reshape(-1)
        assert one.size == REF.len_loader(N, R, 1) * R == np.unique(one).size
    # skip_next = 2 is the epoch without its two leading batches
    np.testing.assert_array_equal(seen[(1, 0, 2, 0)], seen[(1, 0, 0, 0)][2:])
    np.testing.assert_array_equal(seen[(1, 0, 2, 1)], seen[(1, 0, 0, 1)])


def test_same_seed_same_bytes_and_a_loader_built_from_a_path(shard_dirs):
    from freud_amd.resident import ResidentFrameDataLoader
    runs = []
    for _ in range(2):
        state = torch.get_rng_state()
        dl = ResidentFrameDataLoader(shard_dirs["f16"], "L", LB, lengths=np.array(L_LENGTHS), device=DEV)
        assert torch.equal(torch.get_rng_state(), state)                 # the upload leaves the global RNG alone
        assert dl.dataset.tensor_shape == [LT, LD] and dl.store.data.dtype == torch.float16
        torch.manual_seed(11)
        runs.append(_epochs(dl))
    for (ka, a), (kb, b) in zip(*runs):
        assert ka == kb and len(a) == len(b) == 3
        for x, y in zip(a, b):
            np.testing.assert_array_equal(_bytes(x), _bytes(y))
    with pytest.raises(TypeError, match="frames, not files"):
        dl.epoch_batches()


# ---- train() ----------------------------------------------------------------------------------------------------------------
def _fixture(golden_dir, fixture):
    z = np.load(os.path.join(golden_dir, f"{fixture}.npz"))
    return z, json.loads(str(z["meta"]))


def _train(tmp_path_factory, golden_dir, fixture, extra, lengths=None, engine_factory=None):
    """One train() run on a golden fixture -> (its run directory, {step: checkpoint})."""
    from freud_amd.train_sae import train
    z, meta = _fixture(golden_dir, fixture)
    tmp = str(tmp_path_factory.mktemp("frames_train"))
    folder = os.path.join(tmp, "train")
    write_shards(folder, meta["layer"], z["shard"], [meta["T"], meta["d"]], [f"/data/audio/file_{i:04d}.flac" for i in range(meta["n_files"])])
    cfg = copy.deepcopy(meta["config"])
    cfg.update(train_folder=folder, val_folder=folder, run_dir=os.path.join(tmp, "run"), device="cuda", **extra)
    if lengths is not None:
        np.save(os.path.join(tmp, "lengths.npy"), np.asarray(lengths))
        cfg["frame_batches"] = {"lengths": os.path.join(tmp, "lengths.npy")}
    old = os.environ.pop("FREUD_LOADER_DELIVER", None)
    try:
        train(**cfg, **({} if engine_factory is None else {"engine_factory": engine_factory}))
    finally:
        if old is not None:
            os.environ["FREUD_LOADER_DELIVER"] = old
    return cfg["run_dir"], _checkpoints(cfg["run_dir"])


def _checkpoints(run_dir):
    ck_dir = os.path.join(run_dir, "checkpoints")
    return {int(f[4:-4]): torch.load(os.path.join(ck_dir, f), map_location="cpu", weights_only=True)
            for f in os.listdir(ck_dir) if f.startswith("step")}


def _same(a, b, where="ck"):
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


_RUNS = {}
FRAMES = {"resident_data": True, "frame_batches": True}


def _shared(tmp_path_factory, golden_dir, fixture, kind):
    """The frame-batch run ("frames") and the file-batch run ("files") of a fixture, made once for the tests that compare with them."""
    if (fixture, kind) not in _RUNS:
        _RUNS[(fixture, kind)] = _train(tmp_path_factory, golden_dir, fixture, FRAMES if kind == "frames" else {"resident_data": True})
    return _RUNS[(fixture, kind)]


def _resume_cfg(golden_dir, fixture, run_dir, checkpoints, into):
    _z, meta = _fixture(golden_dir, fixture)
    cfg = copy.deepcopy(meta["config"])
    hp = checkpoints[4]["hparams"]
    cfg.update(train_folder=hp["train_folder"], val_folder=hp["val_folder"], device="cuda", **FRAMES, run_dir=os.path.join(run_dir, into),
               start_checkpoint=os.path.join(run_dir, "checkpoints", "step4.pth"))
    return cfg, meta


@pytest.mark.parametrize("fixture", ["trainloop_l1", "trainloop_topk"])
def test_training_is_reproducible_recorded_and_not_the_file_run(tmp_path_factory, golden_dir, fixture):
    _run_a, a = _shared(tmp_path_factory, golden_dir, fixture, "frames")
    _run_b, b = _train(tmp_path_factory, golden_dir, fixture, FRAMES)
    _run_f, files = _shared(tmp_path_factory, golden_dir, fixture, "files")
    last = max(a)
    assert last == 7 and sorted(a) == sorted(b) and 4 in a
    for s in a:
        _same_run(a[s], b[s])
    assert a[last]["hparams"]["frame_batches"] is True and "frame_batches" not in files[last]["hparams"]
    assert not all(np.array_equal(_bytes(a[last]["model"][k]), _bytes(files[last]["model"][k])) for k in a[last]["model"])


@pytest.mark.parametrize("fixture", ["trainloop_l1", "trainloop_topk"])
def test_a_run_resumed_mid_epoch_ends_as_the_uninterrupted_run(tmp_path_factory, golden_dir, fixture):
    from freud_amd.train_sae import train
    run_a, a = _shared(tmp_path_factory, golden_dir, fixture, "frames")
    last = max(a)
    cfg, _meta = _resume_cfg(golden_dir, fixture, run_a, a, "resumed")
    side = torch.load(os.path.join(run_a, "resume", "step4.pth"), map_location="cpu", weights_only=True)
    assert int(side["epoch_batches_done"]) == 1          # 3 batches an epoch: step 4 is the second epoch's first
    train(**cfg)
    resumed = _checkpoints(cfg["run_dir"])
    assert max(resumed) == last == 7
    _same_run(resumed[last], a[last])
    ends = [torch.load(os.path.join(r, "resume", f"step{last}.pth"), map_location="cpu", weights_only=True) for r in (run_a, cfg["run_dir"])]
    assert ends[0]["step"] == ends[1]["step"] == last and ends[0]["epoch_batches_done"] == ends[1]["epoch_batches_done"]
    assert torch.equal(ends[0]["epoch_rng_state"], ends[1]["epoch_rng_state"])
    if fixture == "trainloop_topk":
        assert torch.equal(ends[0]["num_frames_since_fired"], ends[1]["num_frames_since_fired"])


def test_resuming_with_another_form_of_the_key_is_refused(tmp_path_factory, golden_dir):
    from freud_amd.train_sae import train
    fixture = "trainloop_l1"
    run_a, a = _shared(tmp_path_factory, golden_dir, fixture, "frames")
    run_f, _files = _shared(tmp_path_factory, golden_dir, fixture, "files")
    cfg, meta = _resume_cfg(golden_dir, fixture, run_a, a, "refused")
    np.save(os.path.join(run_a, "lengths.npy"), np.full(meta["n_files"], meta["T"]))
    for other in ({"frame_batches": None}, {"frame_batches": {"lengths": os.path.join(run_a, "lengths.npy")}},
                  {"start_checkpoint": os.path.join(run_f, "checkpoints", "step4.pth")}):
        with pytest.raises(ValueError, match="frame_batches"):
            train(**{**cfg, **other})


@pytest.mark.parametrize("lengths", [None, [12, 1, 5, 12, 3, 7, 9, 12, 12, 11]], ids=["untrimmed", "trimmed"])
def test_a_recording_engine_sees_the_references_batches(tmp_path_factory, golden_dir, monkeypatch, lengths):
    from tests.fake_engine import OracleEngine
    z, meta = _fixture(golden_dir, "trainloop_l1")
    n_files, T_, d, B = meta["n_files"], meta["T"], meta["d"], meta["config"]["batch_size"]
    seen, calls = [], []

    class Recording(OracleEngine):
        def step(self, x, lr, stream=None):
            seen.append(x.detach().cpu().numpy().copy())
            super().step(x, lr)

    real = E.store_gather_frames

    def audited(store, T, prefix, n_frames, key, pos0, pos_stride, out, err, ordinals=None, stream=None):
        calls.append((int(key), int(n_frames), int(pos0), int(pos_stride), prefix is not None))
        return real(store, T, prefix, n_frames, key, pos0, pos_stride, out, err, ordinals=ordinals, stream=stream)
    monkeypatch.setattr(E, "store_gather_frames", audited)
    extra = {"resident_data": True} if lengths is not None else {"resident_data": True, "frame_batches": True}
    _train(tmp_path_factory, golden_dir, "trainloop_l1", extra, lengths=lengths, engine_factory=lambda **kw: Recording(**kw))
    N, R = REF.frame_count(n_files, T_, lengths), B * T_
    per_epoch = REF.len_loader(N, R, 1)
    assert len(seen) == len(calls) == meta["config"]["steps"] and per_epoch == (3 if lengths is None else 2)
    assert len({c[0] for c in calls}) == -(-len(calls) // per_epoch), "one key per epoch"
    for i, ((key, n_frames, pos0, stride, trimmed), x) in enumerate(zip(calls, seen)):
        b = i % per_epoch
        assert (n_frames, pos0, stride, trimmed) == (N, b * R, 1, lengths is not None) and key == calls[i - b][0]
        rows = REF.ordinals_to_rows(REF.epoch_ordinals(key, N, R, 0, 1, b + 1, first_batch=b), n_files, T_, lengths)
        want = REF.build_batches(z["shard"], T_, d, rows)[0]
        assert x.shape == want.shape == (B, T_, d) and x.dtype == want.dtype
        np.testing.assert_array_equal(x.view(np.uint8), want.view(np.uint8))
