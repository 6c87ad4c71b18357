"""CPU: frame batches without a device.

* freud_amd/csrc/frame_perm.h compiled for the HOST (g++ -Wall -Werror) into a table-driven program: fp_permute is an exact bijection
  of [0, N) on every N that can be enumerated, with at most 2^bit_length(N - 1) evaluations of the network over all positions;
  fp_unpermute inverts it at sizes that cannot; tests/frame_batches_reference.py restates all of it; the image mixes over keys
  (chi-square at significance 1e-6); fp_locate is numpy.searchsorted; the block decomposition covers every byte of every frame of a
  launch exactly once; seven mutations of the header each fail one of these checks;
* the handling of the "frame_batches" key and of a lengths array of the wrong size, all before any device call; the symbol in
  EXPORTED_SYMBOLS; exactly one translation unit builds the kernel."""
import os
import subprocess

import numpy as np
import pytest

from tests import frame_batches_reference as REF
from tests.build_units import assert_one_unit_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "freud_amd", "csrc", "frame_perm.h")

SMALL_N = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097, 65537)
LARGE_N = (2 ** 31 + 11, 3 * 10 ** 8, 2 ** 33 + 5, 2 ** 62 - 1)
KEYS = (0, 2 ** 64 - 1, 0x0123456789ABCDEF)
# chi-square quantiles at significance 1e-6 (scipy.stats.chi2.isf(1e-6, dof)): a sound permutation fails once in a million runs of
# the -- deterministic -- test, i.e. the bound is not tuned to what this code gives
CHI2_49_P1EM6 = 111.136
CHI2_63_P1EM6 = 131.370
MIX_KEYS = 4096

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "frame_perm.h"

static uint64_t u64(const char* s) { return strtoull(s, NULL, 10); }

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "all")) {            // all KEY N: "evals", then the image of every position
    const uint64_t key = u64(argv[2]), N = u64(argv[3]);
    uint64_t evals = 0;
    std::vector<uint64_t> img(N);
    for (uint64_t p = 0; p < N; ++p) img[p] = fp_permute_counted(key, N, p, &evals);
    printf("%llu\n", (unsigned long long)evals);
    for (uint64_t p = 0; p < N; ++p) printf("%llu\n", (unsigned long long)img[p]);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "some")) {           // some KEY N < positions: "image position-of-image image-of-unpermute"
    const uint64_t key = u64(argv[2]), N = u64(argv[3]);
    unsigned long long p;
    while (scanf("%llu", &p) == 1) {
      const uint64_t g = fp_permute(key, N, p);
      printf("%llu %llu %llu\n", (unsigned long long)g, (unsigned long long)fp_unpermute(key, N, g),
             (unsigned long long)fp_permute(key, N, fp_unpermute(key, N, p)));
    }
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "keys")) {           // keys N P COUNT: the images of P and P + 1 under the keys 0 .. COUNT - 1
    const uint64_t N = u64(argv[2]), p = u64(argv[3]), count = u64(argv[4]);
    for (uint64_t k = 0; k < count; ++k)
      printf("%llu %llu\n", (unsigned long long)fp_permute(k, N, p), (unsigned long long)fp_permute(k, N, p + 1));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "pos")) {
    printf("%llu\n", (unsigned long long)fp_position(u64(argv[2]), u64(argv[3]), u64(argv[4])));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "locate")) {         // locate PREFIX_FILE|- N_FILES T < ordinals: "file t bad row"
    const int64_t n_files = atoll(argv[3]), T = atoll(argv[4]);
    std::vector<int64_t> prefix;
    if (strcmp(argv[2], "-")) {
      FILE* f = fopen(argv[2], "rb");
      if (!f) return 2;
      prefix.resize(n_files + 1);
      if (fread(prefix.data(), 8, n_files + 1, f) != (size_t)(n_files + 1)) return 3;
      fclose(f);
    }
    long long g;
    while (scanf("%lld", &g) == 1) {
      int64_t file, t;
      const bool bad = fp_locate(prefix.empty() ? nullptr : prefix.data(), n_files, T, g, &file, &t);
      printf("%lld %lld %d %lld\n", (long long)file, (long long)t, (int)bad, (long long)fp_store_row(file, T, t));
    }
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "cover")) {          // cover FRAME_BYTES WIDTH ROWS OUT: the plan; to OUT, int64 per unit
    const int64_t fb = atoll(argv[2]), rows = atoll(argv[4]);   // of every workgroup: row * FRAME_BYTES + byte in the frame
    const int width = atoi(argv[3]);
    const fp_plan p = fp_plan_of(fb, width, rows);
    printf("%lld %lld %lld %lld %lld %lld %d %d\n", (long long)p.upf, (long long)p.pieces, (long long)p.rows_per_block, (long long)p.blocks,
           (long long)FP_SPAN_UNITS, (long long)FP_MAX_ROWS, FP_THREADS, FP_UNROLL);
    FILE* out = fopen(argv[5], "wb");
    if (!out) return 2;
    for (int64_t w = 0; w < p.blocks; ++w) {
      int64_t row0, unit0;
      int nrows, n;
      fp_block_span(p, rows, w, &row0, &nrows, &unit0, &n);
      if (nrows < 1 || n < 1 || nrows > FP_MAX_ROWS || (int64_t)nrows * n > FP_SPAN_UNITS) return 4;
      for (uint32_t e = 0; e < (uint32_t)nrows * (uint32_t)n; ++e) {
        uint32_t r, c;
        fp_unit_of(e, (uint32_t)n, &r, &c);
        if (r >= (uint32_t)nrows || c >= (uint32_t)n) return 5;
        const int64_t at = (row0 + r) * fb + (unit0 + c) * width;
        fwrite(&at, 8, 1, out);
      }
    }
    fclose(out);
    return 0;
  }
  return 1;
}
"""


def _compile(folder, header_text=None):
    """The program over the header as it is, or over `header_text` in its place."""
    src = folder / "frames.cpp"
    src.write_text(_SRC)
    include = os.path.join(ROOT, "freud_amd", "csrc")
    if header_text is not None:
        (folder / "frame_perm.h").write_text(header_text)
        include = str(folder)
    exe = folder / "frames"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{include}", str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("frames"))


def _run(prog, *args, stdin=None):
    out = subprocess.run([prog, *map(str, args)], check=True, capture_output=True, text=True, input=stdin).stdout
    return [[int(v) for v in l.split()] for l in out.splitlines()]


def _positions(N, count=3000):
    rng = np.random.default_rng(N % (2 ** 32))
    some = {0, 1, N - 1, N - 2, N // 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 31, N - 2 ** 32}
    some |= {int(v) for v in rng.integers(0, N, size=count, dtype=np.uint64)}
    return sorted(p for p in some if 0 <= p < N)


# ---- the checks; the mutation tests run them again on mutated headers
def check_exhaustive(prog, ns=SMALL_N, python_too=True):
    for N in ns:
        for key in KEYS:
            (evals,), *img = _run(prog, "all", key, N)
            img = np.array([v[0] for v in img], dtype=np.uint64)
            assert img.size == N and np.array_equal(np.sort(img), np.arange(N, dtype=np.uint64)), f"N={N} key={key}: not a bijection of [0, N)"
            domain = 1 if N <= 2 else 1 << (N - 1).bit_length()
            assert evals <= domain, f"N={N} key={key}: {evals} evaluations > the domain's {domain}"
            if python_too and N <= 4097:
                count = [0]
                assert [REF.fp_permute(key, N, p, count) for p in range(N)] == img.tolist(), f"N={N} key={key}: the restatement differs"
                assert count[0] == evals or N <= 2
                assert all(REF.fp_unpermute(key, N, int(g)) == p for p, g in enumerate(img.tolist()))


def check_large(prog):
    for N in LARGE_N:
        for key in KEYS:
            ps = _positions(N)
            rows = _run(prog, "some", key, N, stdin="\n".join(map(str, ps)))
            assert len(rows) == len(ps)
            for p, (g, back, forth) in zip(ps, rows):
                assert 0 <= g < N and back == p and forth == p, f"N={N} key={key} p={p}: image {g}, unpermute {back}, permute(unpermute) {forth}"
            assert len({g for g, _b, _f in rows}) == len(ps), f"N={N} key={key}: two positions share an image"
            for p, (g, _b, _f) in list(zip(ps, rows))[:40] + list(zip(ps, rows))[-40:]:
                assert REF.fp_permute(key, N, p) == g and REF.fp_unpermute(key, N, g) == p, f"N={N} key={key} p={p}: the restatement differs"


def _chi_square(observed, expected):
    return float(((observed - expected) ** 2 / expected).sum())


def check_mixing(prog):
    n_files, T = 8, 125
    N, p = n_files * T, 123
    pairs = np.array(_run(prog, "keys", N, p, MIX_KEYS), dtype=np.int64)
    assert pairs.shape == (MIX_KEYS, 2) and (pairs[:, 0] != pairs[:, 1]).all()
    # the image of one position over the keys, in 50 buckets of 20 ordinals: uniform
    stat = _chi_square(np.bincount(pairs[:, 0] // 20, minlength=50).astype(np.float64), np.full(50, MIX_KEYS / 50))
    print(f"image of position {p} over {MIX_KEYS} keys: chi-square {stat:.2f} on 49 degrees of freedom")
    assert stat < CHI2_49_P1EM6
    # the file of position p + 1 given the file of position p: two draws without replacement
    table = np.zeros((n_files, n_files))
    np.add.at(table, (pairs[:, 0] // T, pairs[:, 1] // T), 1)
    expected = np.full((n_files, n_files), MIX_KEYS * T * T / (N * (N - 1)))
    np.fill_diagonal(expected, MIX_KEYS * T * (T - 1) / (N * (N - 1)))
    stat = _chi_square(table, expected)
    print(f"files of positions {p}, {p + 1}: chi-square {stat:.2f} on 63 degrees of freedom")
    assert stat < CHI2_63_P1EM6


def check_position(prog):
    for q, rank, world in ((0, 0, 1), (5, 0, 1), (0, 1, 2), (7, 1, 2), (7, 2, 5), (2 ** 40, 3, 8)):
        assert _run(prog, "pos", q, rank, world) == [[q * world + rank]]
    # the ranks of a world tile the positions
    for world in (1, 2, 3):
        got = sorted(_run(prog, "pos", q, r, world)[0][0] for r in range(world) for q in range(4))
        assert got == list(range(4 * world))


LOCATE_CASES = {
    "mixed": ([12, 1, 5, 12, 3, 7, 9], 12),
    "ones": ([1, 1, 1, 1], 6),
    "full": ([6, 6, 6], 6),
    "one file": ([4], 9),
    "one frame": ([1], 1),
}


def _locate(prog, tmp_path, prefix, n_files, T, gs):
    name = "-"
    if prefix is not None:
        name = str(tmp_path / "prefix.i64")
        np.asarray(prefix, dtype=np.int64).tofile(name)
    return _run(prog, "locate", name, n_files, T, stdin="\n".join(map(str, gs)))


def check_locate(prog, tmp_path):
    for name, (lengths, T) in LOCATE_CASES.items():
        prefix, n = REF.prefix_of(lengths), len(lengths)
        gs = list(range(int(prefix[-1])))                 # every frame: the first and the last of every file among them
        want_file = np.searchsorted(prefix, gs, side="right") - 1
        for g, (file, t, bad, row) in zip(gs, _locate(prog, tmp_path, prefix, n, T, gs)):
            assert (file, t, bad, row) == (want_file[g], g - prefix[want_file[g]], 0, want_file[g] * T + g - prefix[want_file[g]]), (name, g)
            assert REF.fp_locate(prefix, n, T, g) == (file, t, False)
    # untrimmed
    for g, (file, t, bad, row) in zip(range(84), _locate(prog, tmp_path, None, 7, 12, range(84))):
        assert (file, t, bad, row) == (g // 12, g % 12, 0, g) and REF.fp_locate(None, 7, 12, g) == (file, t, False)
    # an int64 prefix beyond 2^32: 3 000 000 files of up to 1500 frames
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 1501, size=3_000_000)
    lengths[::7] = 1500
    lengths[1::7] = 1
    prefix = REF.prefix_of(lengths)
    assert prefix[-1] > 2 ** 31 and prefix.dtype == np.int64
    big = np.concatenate([[0]] + [np.cumsum(np.full(4_000_000, 1500, dtype=np.int64))])       # untrimmed-like, past 2^32
    assert big[-1] > 2 ** 32
    for pre, n in ((prefix, lengths.size), (big, big.size - 1)):
        gs = sorted({0, int(pre[-1]) - 1, *(int(v) for v in pre[rng.integers(0, n, 300)]), *(int(v) - 1 for v in pre[rng.integers(1, n + 1, 300)]),
                     *(int(v) for v in rng.integers(0, int(pre[-1]), 300))})
        want_file = np.searchsorted(pre, gs, side="right") - 1
        for i, (file, t, bad, row) in enumerate(_locate(prog, tmp_path, pre, n, 1500, gs)):
            assert (file, t, bad, row) == (want_file[i], gs[i] - pre[want_file[i]], 0, want_file[i] * 1500 + gs[i] - pre[want_file[i]])


def check_malformed(prog, tmp_path):
    """A prefix that is no prefix sum of lengths in [1, T], and ordinals outside it: clamped into the store and flagged."""
    T, n = 6, 3
    for prefix, g in (([0, 10, 12, 13], 8), ([5, 6, 7, 8], 2), ([0, 3, 6, 9], -1), ([0, 3, 6, 9], 40), ([0, 3, 2, 9], 8)):
        (file, t, bad, row), = _locate(prog, tmp_path, prefix, n, T, [g])
        assert bad == 1 and 0 <= file < n and 0 <= t < T and row == file * T + t, (prefix, g)
        assert REF.fp_locate(np.array(prefix), n, T, g) == (file, t, True)
    for g in (-1, 18, 2 ** 40):
        (file, t, bad, row), = _locate(prog, tmp_path, None, n, T, [g])
        assert bad == 1 and 0 <= file < n and 0 <= t < T and row == file * T + t


COVER_BYTES = (2, 10, 24, 32, 48, 768, 1536, 5120)
COVER_ROWS = (1, 3, 64, 257)


def _widths(frame_bytes):
    return [w for w in (16, 4, 2) if frame_bytes % w == 0]


def check_cover(prog, tmp_path, sizes=None):
    out = str(tmp_path / "cover.i64")
    (upf0, _p, _r, _b, span, max_rows, threads, unroll), = _run(prog, "cover", 16, 16, 1, out)
    assert span == threads * unroll and max_rows <= threads and upf0 == 1
    above = [span * 16 + 16, 3 * span * 16 + 48, span * 2 + 2]       # longer than a workgroup's span, at every width they admit
    for fb in sizes or (*COVER_BYTES, *above):
        for width in _widths(fb):
            for rows in COVER_ROWS:
                (upf, pieces, rpb, blocks, *_rest), = _run(prog, "cover", fb, width, rows, out)
                assert upf * width == fb and pieces == -(-upf // span) and blocks == -(-rows // rpb) * pieces
                assert (rpb == 1) if pieces > 1 else (rpb == min(max_rows, span // upf))
                at = np.fromfile(out, dtype=np.int64)
                want = np.arange(rows * upf, dtype=np.int64) * width
                assert at.size == want.size and np.array_equal(np.sort(at), want), f"frame_bytes={fb} width={width} rows={rows}: not an exact cover"


# ---- the header as it is
def test_bijection_on_every_enumerable_size(prog):
    check_exhaustive(prog)


def test_inverse_and_range_at_sizes_beyond_enumeration(prog):
    check_large(prog)


def test_image_mixes_over_keys(prog):
    check_mixing(prog)


def test_position_is_the_loaders_rank_slice(prog):
    check_position(prog)
    assert REF.fp_position(7, 2, 5) == 37


def test_locate_is_searchsorted(prog, tmp_path):
    check_locate(prog, tmp_path)


def test_malformed_prefix_is_clamped_and_flagged(prog, tmp_path):
    check_malformed(prog, tmp_path)


def test_blocks_cover_every_byte_once(prog, tmp_path):
    check_cover(prog, tmp_path)


# ---- mutations of the header: each must fail the named check
MUTATIONS = {
    "no cycle walk": ("    if (evals) ++*evals;\n  } while (x >= N);", "    if (evals) ++*evals;\n  } while (false);",
                      lambda prog, tmp: check_exhaustive(prog, (5, 1000), python_too=False)),
    "one round fewer in the inverse": ("for (int r = FP_ROUNDS - 1; r >= 0; --r)", "for (int r = FP_ROUNDS - 2; r >= 0; --r)",
                                       lambda prog, tmp: check_large(prog)),
    "key ignored": ("return fp_mix(key + 0x9E3779B97F4A7C15ull); }", "return fp_mix(0x9E3779B97F4A7C15ull); }",
                    lambda prog, tmp: check_mixing(prog)),
    "position truncated to 32 bits": ("  uint64_t x = p;\n", "  uint64_t x = (uint32_t)p;\n", lambda prog, tmp: check_large(prog)),
    "rank and world swapped": ("return q * world + rank;", "return q * rank + world;", lambda prog, tmp: check_position(prog)),
    "search off by one": ("if (prefix[mid] <= g) lo = mid;", "if (prefix[mid] < g) lo = mid;", lambda prog, tmp: check_locate(prog, tmp)),
    "pieces overlap": ("*unit0 = piece * FP_SPAN_UNITS;", "*unit0 = piece * (FP_SPAN_UNITS - 1);",
                       lambda prog, tmp: check_cover(prog, tmp, sizes=(5120, 1024 * 16 + 16))),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_of_the_header_fails_a_check(name, tmp_path):
    old, new, check = MUTATIONS[name]
    text = open(HEADER).read()
    assert text.count(old) == 1, f"the header no longer holds the line this mutation changes: {old!r}"
    mutated = _compile(tmp_path, text.replace(old, new))
    with pytest.raises(AssertionError):
        check(mutated, tmp_path)


# ---- the key, the loader's arguments, the symbol: no device
_TRAIN = dict(seed=0, train_folder="x", val_folder="x", device="cuda", run_dir="x", lr=1e-3, weight_decay=0.0, steps=1, clip_thresh=1.0,
              batch_size=1, dl_max_workers=0, log_tb_every=1, save_every=1, val_every=1, start_checkpoint=None,
              whisper_config={"model": "tiny", "layer_name": "L"}, optimizer="adam", scheduler="cosine", scheduler_params={}, from_disk=True,
              autoencoder_variant="l1", autoencoder_config={})


@pytest.fixture()
def no_device(monkeypatch):
    import torch

    def refuse(*a, **k):
        raise AssertionError("device work before the key was checked")
    monkeypatch.setattr(torch.cuda, "set_device", refuse)


@pytest.mark.parametrize("spec", ["yes", 1, [], {"length": "a.npy"}, {"lengths": "a.npy", "pad": 0}, {"lengths": 5}, {"lengths": [1, 2]}])
def test_train_refuses_a_malformed_key_before_any_device_call(spec, no_device):
    from freud_amd.train_sae import train
    with pytest.raises(ValueError, match="frame_batches"):
        train(**_TRAIN, resident_data=True, frame_batches=spec)


@pytest.mark.parametrize("resident", [None, False, {"on_overflow": "stream"}, {"dtype": "bfloat16", "on_overflow": "stream"}])
def test_train_refuses_the_key_without_a_store_to_rely_on(resident, no_device):
    from freud_amd.train_sae import train
    for spec in (True, {}, {"lengths": "a.npy"}):
        with pytest.raises(ValueError, match="frame_batches"):
            train(**_TRAIN, resident_data=resident, frame_batches=spec)


def test_train_refuses_a_lengths_file_that_does_not_serve(tmp_path, no_device):
    from freud_amd.loader import write_shards
    from freud_amd.train_sae import train
    write_shards(str(tmp_path), "L", np.zeros((3, 8), np.float32), [2, 4])
    args = dict(_TRAIN, train_folder=str(tmp_path))
    files = {"missing.npy": None, "text.npy": "not an array", "short.npy": np.array([1, 2]), "zero.npy": np.array([1, 0, 2]),
             "float.npy": np.array([1.0, 2.0, 2.0]), "matrix.npy": np.ones((3, 1), np.int64)}
    side = tmp_path / "side"
    side.mkdir()
    for name, content in files.items():
        path = str(side / name)
        if isinstance(content, str):
            open(path, "w").write(content)
        elif content is not None:
            np.save(path, content)
        with pytest.raises(ValueError, match="frame_batches"):
            train(**args, resident_data=True, frame_batches={"lengths": path})


def test_key_forms():
    from freud_amd.resident import parse_frame_batches, parse_resident_data
    rd = parse_resident_data(True)
    assert parse_frame_batches(None, rd) is None and parse_frame_batches(False, rd) is None
    assert parse_frame_batches(None) is None and parse_frame_batches(False, None) is None
    assert parse_frame_batches(True, rd) == {"lengths": None} == parse_frame_batches({}, rd)
    assert parse_frame_batches({"lengths": "a.npy"}, parse_resident_data({"dtype": "bfloat16"})) == {"lengths": "a.npy"}


def test_loader_refusals_before_any_device_call(tmp_path, monkeypatch):
    import torch
    from freud_amd.loader import write_shards
    from freud_amd.resident import ResidentFrameDataLoader
    write_shards(str(tmp_path), "L", np.zeros((3, 8), np.float32), [2, 4])     # 3 files, T = 2: N = 6
    calls = []
    real = torch.cuda.is_available
    monkeypatch.setattr(torch.cuda, "is_available", lambda: calls.append(1) or real())
    for lengths in ([1, 2], [1, 2, 2, 1], [[1, 2, 2]], [1.0, 2.0, 2.0], [1, 0, 2]):
        with pytest.raises(ValueError, match="lengths"):
            ResidentFrameDataLoader(str(tmp_path), "L", 1, lengths=np.array(lengths))
    with pytest.raises(ValueError, match=r"N = 6 .*world_size = 1.*R = batch_size \* T = 8"):
        ResidentFrameDataLoader(str(tmp_path), "L", 4)
    with pytest.raises(ValueError, match=r"N = 3 .*world_size = 2 .*R = batch_size \* T = 2"):
        ResidentFrameDataLoader(str(tmp_path), "L", 1, lengths=np.array([1, 1, 1]), rank=1, world_size=2)
    assert not calls


def test_symbol_and_build_unit():
    from freud_amd import engine
    assert "sae_store_gather_frames" in engine.EXPORTED_SYMBOLS
    assert assert_one_unit_builds("frame_gather.h") == "passes.hip"
