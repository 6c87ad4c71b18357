"""CPU: the resident store without a device.

* freud_amd/csrc/bf16_guard.h compiled for the HOST (g++ -Wall -Werror): the scalar rule of sae_store_convert is held to
  freud_f32_to_bf16_portable of libfreud_host.so on the value table of tests/resident_cases.py; three mutations of the rule
  (truncation, no -1.0 guard, NaN to inf) each fall outside it;
* freud_amd/csrc/resident_index.h compiled for the host: the pieces of a row tile it exactly, a bad index is clamped into the
  store and flagged, and idx * row_bytes is formed in 64 bits;
* the argument handling of the key, the store and the index check, all before any device call; the symbols in the header and in
  EXPORTED_SYMBOLS; exactly one translation unit builds the kernels."""
import os
import subprocess

import numpy as np
import pytest

from tests import resident_cases as RC
from tests.build_units import assert_one_unit_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bf16_guard.h"
#include "resident_index.h"

// the three mutations the table must tell from the rule
static uint32_t truncating(uint32_t u) { return u >> 16; }
static uint32_t unguarded(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
static uint32_t nan_to_inf(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) & 0xFF80u;
  return bg_f32_bits_to_bf16(u);
}

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "conv")) {          // conv MODE in out: uint32 file -> uint16 file
    const int mode = atoi(argv[2]);
    FILE* in = fopen(argv[3], "rb");
    FILE* out = fopen(argv[4], "wb");
    if (!in || !out) return 2;
    uint32_t u;
    while (fread(&u, 4, 1, in) == 1) {
      const uint32_t b = mode == 0 ? bg_f32_bits_to_bf16(u) : mode == 1 ? truncating(u) : mode == 2 ? unguarded(u) : nan_to_inf(u);
      const uint16_t h = (uint16_t)b;
      if (b >> 16) return 3;                            // the rule leaves the high half clear
      fwrite(&h, 2, 1, out);
    }
    fclose(in);
    fclose(out);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "row")) {           // row ROW_BYTES: "piece_bytes pieces", then "p byte0 len" per piece
    const int64_t row = atoll(argv[2]);
    const int64_t pieces = rs_pieces(row);
    printf("%lld %lld %d %d\n", (long long)RS_PIECE_BYTES, (long long)pieces, RS_THREADS, RS_UNROLL);
    for (int64_t p = 0; p < pieces; ++p) {
      int64_t b0, len;
      rs_piece_span(row, p, &b0, &len);
      printf("%lld %lld %lld\n", (long long)p, (long long)b0, (long long)len);
    }
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "idx")) {           // idx IDX N_FILES ROW_BYTES: "file bad src_offset"
    bool bad;
    const int64_t f = rs_clamp_index((int32_t)atoll(argv[2]), atoll(argv[3]), &bad);
    printf("%lld %d %lld\n", (long long)f, (int)bad, (long long)rs_src_offset(f, atoll(argv[4])));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "block")) {         // block W PIECES STRIDE: "j p dst_offset"
    int64_t j, p;
    rs_block_of(atoll(argv[2]), atoll(argv[3]), &j, &p);
    printf("%lld %lld %lld\n", (long long)j, (long long)p, (long long)rs_dst_offset(j, atoll(argv[4])));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "width")) {
    printf("%d\n", rs_copy_width(strtoull(argv[2], NULL, 10)));
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("resident")
    src = d / "resident.cpp"
    src.write_text(_SRC)
    exe = d / "resident"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def built():
    from freud_amd import engine
    engine.build()
    return engine


def _run(prog, *args):
    return [[int(v) for v in l.split()] for l in subprocess.run([prog, *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()]


def _convert(prog, tmp_path, mode):
    src, dst = tmp_path / "in.u32", tmp_path / f"out{mode}.u16"
    if not src.exists():
        RC.convert_table().tofile(str(src))
    subprocess.run([prog, "conv", str(mode), str(src), str(dst)], check=True)
    return np.fromfile(str(dst), dtype=np.uint16)


def test_convert_rule_is_the_host_librarys(prog, built, tmp_path):
    table, want = RC.convert_table(), RC.convert_expected()
    assert table.size == 6 * 65536 + 129 + 30
    got = _convert(prog, tmp_path, 0)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(table[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # what the rule promises, stated on its own: only -1.0 itself gives 0xBF80, a NaN stays a quiet NaN, an infinity an infinity
    assert np.array_equal(table[want == 0xBF80], np.array([0xBF800000] * int((want == 0xBF80).sum()), dtype=np.uint32))
    nan = (table & 0x7FFFFFFF) > 0x7F800000
    assert np.all((want[nan] & 0x7FC0) == 0x7FC0) and np.all((want[~nan] & 0x7FFF) <= 0x7F80)
    assert want[table == 0x7F800000][0] == 0x7F80 and want[table == 0xFF800000][0] == 0xFF80


@pytest.mark.parametrize("mode,name", [(1, "truncation"), (2, "no guard"), (3, "NaN to inf")])
def test_convert_table_tells_the_mutations(prog, built, tmp_path, mode, name):
    assert np.any(_convert(prog, tmp_path, mode) != RC.convert_expected()), f"the table does not notice: {name}"


def test_piece_arithmetic(prog, built):
    piece = built.store_piece_bytes()
    for row in (30, piece - 16, piece, piece + 16, 2 * piece + 2, 1500 * 384 * 2, 1500 * 384 * 4):
        head, *spans = _run(prog, "row", row)
        assert head[0] == piece == head[2] * head[3] * 16 and head[1] == -(-row // piece) == len(spans)
        at = 0
        for p, (pp, b0, ln) in enumerate(spans):        # ascending, contiguous, none empty, none longer than a piece
            assert pp == p and b0 == at and 0 < ln <= piece
            at += ln
        assert at == row
        assert all(ln == piece for _p, _b, ln in spans[:-1])
    # workgroup -> (batch row, piece) and the destination offset, beyond 2^32
    assert _run(prog, "block", 0, 3, 100) == [[0, 0, 0]]
    assert _run(prog, "block", 7, 3, 100) == [[2, 1, 200]]
    assert _run(prog, "block", INT32_MAX - 1, 1, 1 << 20) == [[INT32_MAX - 1, 0, (INT32_MAX - 1) << 20]]
    for bits, w in ((0, 16), (16, 16), (4, 4), (20, 4), (2, 2), (6, 2), (1, 0), (17, 0), ((1 << 40) | 8, 4)):
        assert _run(prog, "width", bits) == [[w]]


@pytest.mark.parametrize("idx,n_files,file,bad", [(0, 5, 0, 0), (4, 5, 4, 0), (-1, 5, 0, 1), (5, 5, 4, 1), (INT32_MAX, 5, 4, 1),
                                                   (-INT32_MAX - 1, 5, 0, 1), (INT32_MAX, INT32_MAX, INT32_MAX - 1, 1),
                                                   (INT32_MAX - 1, INT32_MAX, INT32_MAX - 1, 0)])
def test_index_is_clamped_counted_and_addressed_in_64_bits(prog, idx, n_files, file, bad):
    row = 1500 * 384 * 4                                # 2.3 MB: file 1865 starts beyond 2^32
    assert _run(prog, "idx", idx, n_files, row) == [[file, bad, file * row]]
    assert _run(prog, "idx", 200_000, 200_001, row) == [[200_000, 0, 200_000 * row]] and 200_000 * row > 2 ** 32


_TRAIN = dict(seed=0, train_folder="x", val_folder="x", device="cuda", run_dir="x", lr=1e-3, weight_decay=0.0, steps=1, clip_thresh=1.0,
              batch_size=1, dl_max_workers=0, log_tb_every=1, save_every=1, val_every=1, start_checkpoint=None,
              whisper_config={"model": "tiny", "layer_name": "l"}, optimizer="adam", scheduler="cosine", scheduler_params={}, from_disk=True,
              autoencoder_variant="l1", autoencoder_config={})


@pytest.mark.parametrize("spec", ["yes", 1, [], {"dtype": "float16"}, {"dtype": "native", "gb": 1}, {"max_gb": 0}, {"max_gb": "4"},
                                  {"max_gb": True}, {"on_overflow": "ignore"}])
def test_train_refuses_a_malformed_key_before_any_device_call(spec, monkeypatch):
    import torch
    from freud_amd.train_sae import train

    def no_device(*a, **k):
        raise AssertionError("device work before the key was checked")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(ValueError, match="resident_data"):
        train(**_TRAIN, resident_data=spec)


def test_key_forms():
    from freud_amd.resident import parse_resident_data
    assert parse_resident_data(None) is None and parse_resident_data(False) is None
    assert parse_resident_data(True) == {"dtype": None, "max_gb": None, "on_overflow": "error"}
    assert parse_resident_data({"dtype": "bfloat16", "max_gb": 2.5, "on_overflow": "stream"}) == \
        {"dtype": "bfloat16", "max_gb": 2.5, "on_overflow": "stream"}


def test_store_refusals_before_any_device_call(tmp_path, monkeypatch):
    import torch
    from freud_amd.loader import write_shards
    from freud_amd.resident import ResidentActivationDataLoader, ResidentActivations, check_indices
    write_shards(str(tmp_path), "L", np.zeros((3, 8), np.float32), [2, 4])
    calls = []
    real = torch.cuda.is_available
    monkeypatch.setattr(torch.cuda, "is_available", lambda: calls.append(1) or real())
    with pytest.raises(ValueError, match="dtype must be 'native' or 'bfloat16'"):
        ResidentActivations(str(tmp_path), "L", dtype="float16")
    with pytest.raises(ValueError, match="dtype must be 'native' or 'bfloat16'"):
        ResidentActivationDataLoader(str(tmp_path), "L", 2, deliver_dtype="fp8")
    with pytest.raises(ValueError, match="max_gb"):
        ResidentActivations(str(tmp_path), "L", max_gb=0)
    assert not calls
    # a host-side index list out of range
    assert check_indices([[0, 2], [1]], 3).tolist() == [0, 2, 1] and check_indices([[0, 2], [1]], 3).dtype == np.int32
    assert check_indices([], 3).size == 0
    for bad in ([[0, 3]], [[-1]], [[0], [INT32_MAX + 1]]):
        with pytest.raises(ValueError, match="leave the store"):
            check_indices(bad, 3)
    if not real():
        with pytest.raises(RuntimeError, match="no CPU path"):
            ResidentActivations(str(tmp_path), "L")
        with pytest.raises(RuntimeError, match="no CPU path"):
            ResidentActivationDataLoader(str(tmp_path), "L", 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ResidentActivations(str(tmp_path), "L", device="cpu")


def test_a_pass_that_reads_the_files_itself_names_the_argument(tmp_path):
    from freud_amd.collect_features import check_out_folder
    from freud_amd.loader import MemoryMappedActivationsDataset
    for call in (lambda: MemoryMappedActivationsDataset(object(), "L"), lambda: check_out_folder(object(), str(tmp_path), "L", "indexed", False)):
        with pytest.raises(TypeError, match="data_path must be the path of a shard directory"):
            call()


def test_symbols_and_build_unit(built):
    for s in ("sae_store_piece_bytes", "sae_store_convert", "sae_store_gather"):
        assert s in built.EXPORTED_SYMBOLS
    assert built.store_piece_bytes() % 16 == 0
    assert assert_one_unit_builds("resident.h") == "passes.hip"
