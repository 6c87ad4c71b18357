"""CPU: the select of the file features (freud_amd/csrc/file_top.h -- the ordering predicate and the serial reference select that
the kernel's answers are defined by) compiled for the HOST with g++ and replayed against the reference's own
top_activations_for_audio (utils/activations.py:135-209; tests/golden/file_features_{raw,l1,topk}.npz, written by
tests/golden/make_file_features_golden.py): keys are built from the recorded series by search_keys.h's sk_key, exactly as the
search kernels form them, and the selected latents, their values and frames must be the reference's.  In the SAE cases the
reference's positive prefix is compared in full and every slot after it must be empty (the reference pads with zero-valued
latents).  Plus the boundary (header, symbol list, constants), the n_top range error and the npz round trip."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import build_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TIMESTEP_S = 30 / 1500

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "file_top.h"

// argv: data file (int32 T, d, L, float x[T][d]) n_top flags -> n_top lines "latent value-bits frame"
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[1], "rb");
  int T, d, L;
  if (fread(&T, 4, 1, fp) != 1 || fread(&d, 4, 1, fp) != 1 || fread(&L, 4, 1, fp) != 1) return 2;
  std::vector<float> x((size_t)T * d);
  if (fread(x.data(), 4, x.size(), fp) != x.size()) return 2;
  fclose(fp);
  const int n_top = atoi(argv[2]), flags = atoi(argv[3]);
  const int len = L < 1 ? 1 : (L > T ? T : L);
  std::vector<uint64_t> keys(d, 0);
  for (int j = 0; j < d; ++j)
    for (int r = 0; r < len; ++r) {
      const uint64_t k = sk_key(x[(size_t)r * d + j], (uint32_t)r);
      if (k > keys[j]) keys[j] = k;
    }
  std::vector<int32_t> lat(n_top);
  std::vector<uint64_t> out(n_top);
  ft_select_serial(keys.data(), d, n_top, flags, lat.data(), out.data());
  for (int i = 0; i < n_top; ++i)
    printf("%d %08x %lld\n", lat[i], sk_bits(sk_key_value(out[i])), lat[i] < 0 ? -1ll : (long long)sk_key_frame(out[i]));
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("ft")
    src = d / "ft.cpp"
    src.write_text(_SRC)
    exe = d / "ft"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def _select(prog, tmp_path, series, L, n_top, flags):
    """series [T, d] fp32 -> (latents, values, frames) of the serial select."""
    T, d = series.shape
    data = tmp_path / "x.bin"
    data.write_bytes(np.array([T, d, L], np.int32).tobytes() + np.ascontiguousarray(series, np.float32).tobytes())
    out = subprocess.run([prog, str(data), str(n_top), str(flags)], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    assert len(rows) == n_top
    return ([int(r[0]) for r in rows], [struct.unpack("<f", struct.pack("<I", int(r[1], 16)))[0] for r in rows], [int(r[2]) for r in rows])


def test_raw_golden_replay(prog, tmp_path):
    g = np.load(os.path.join(GOLD, "file_features_raw.npz"))
    x, lengths = g["x"], g["lengths"]
    assert sorted(set(g["case_top_n"].tolist())) == [1, 4, 10, 16]
    for c in range(len(g["case_file"])):
        f, n_top = int(g["case_file"][c]), int(g["case_top_n"][c])
        lat, val, fr = _select(prog, tmp_path, x[f], int(lengths[f]), n_top, 0)
        want = [int(i) for i in g["case_idx"][c] if i >= 0]
        m = len(want)
        ctx = f"file {f} top_n={n_top}"
        assert m == min(n_top, x.shape[2]), ctx
        assert lat[:m] == want and all(j == -1 for j in lat[m:]), ctx
        assert val[:m] == [float(v) for v in g["case_values"][c][:m]], ctx
        assert fr[:m] == [int(t) for t in g["case_frames"][c][:m]] and all(t == -1 for t in fr[m:]), ctx
    # the planted cases, as the reference answered them: equal maxima -> the earlier frame first; a repeated maximum -> its
    # first frame; the all-negative column last, reported with its signed value
    lat, val, fr = _select(prog, tmp_path, x[0], int(lengths[0]), 4, 0)
    assert lat[:2] == [6, 2] and val[0] == val[1] == 5.5 and fr[:2] == [3, 7]
    lat, val, fr = _select(prog, tmp_path, x[1], int(lengths[1]), 1, 0)
    assert (lat, val, fr) == ([1], [6.25], [2])
    lat, val, fr = _select(prog, tmp_path, x[4], int(lengths[4]), 16, 0)
    assert lat[9] == 8 and val[9] < 0 and lat[10:] == [-1] * 6


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_sae_golden_replay(prog, tmp_path, kind):
    g = np.load(os.path.join(GOLD, f"file_features_{kind}.npz"))
    dense, lengths = g["dense"], g["lengths"]
    assert sorted(set(g["case_top_n"].tolist())) == [1, 5, 40]
    short = 0
    for c in range(len(g["case_file"])):
        f, n_top, m = int(g["case_file"][c]), int(g["case_top_n"][c]), int(g["case_n_positive"][c])
        lat, val, fr = _select(prog, tmp_path, dense[f], int(lengths[f]), n_top, 1)
        ctx = f"{kind} file {f} top_n={n_top} positive={m}"
        assert lat[:m] == [int(i) for i in g["case_idx"][c][:m]], ctx
        assert val[:m] == [float(v) for v in g["case_values"][c][:m]] and all(v > 0 for v in val[:m]), ctx
        assert fr[:m] == [int(t) for t in g["case_frames"][c][:m]], ctx
        assert all(j == -1 for j in lat[m:]) and all(t == -1 for t in fr[m:]), ctx      # the reference's zero-valued fillers
        short += m < n_top
    assert short > 0, "no case with fewer positive latents than slots"


def test_ties_go_to_the_lower_latent_and_zero_rule(prog, tmp_path):
    x = np.zeros((3, 6), np.float32)
    x[1, [1, 4]] = 2.0            # equal value AND frame: latent 1 before latent 4
    x[2, 3] = 2.0                 # same value, later frame
    x[0, 5] = -0.0
    x[0, 2] = -1.0
    lat, val, fr = _select(prog, tmp_path, x, 3, 6, 1)
    assert lat == [1, 4, 3, -1, -1, -1] and fr[:3] == [1, 1, 2]
    lat, val, fr = _select(prog, tmp_path, x, 3, 2, 1)
    assert lat == [1, 4]
    lat, val, fr = _select(prog, tmp_path, x, 3, 6, 0)      # raw: zeros and negatives as they are, lower latent first among equals
    assert lat == [1, 4, 3, 0, 5, 2] and val[3:] == [0.0, 0.0, 0.0] and fr[3:] == [0, 0, 1]


def test_boundary_has_the_entry_point():
    from freud_amd import engine as E
    from freud_amd import file_features as FF
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert "sae_file_top_features" in E.EXPORTED_SYMBOLS
    assert re.search(r"\bint\s+sae_file_top_features\s*\(", hdr) and "activations.py:135-209" in hdr
    assert int(re.search(r"#define\s+SAE_FILE_TOP_MAX\s+(\d+)", hdr).group(1)) == E.FILE_TOP_MAX == FF.FILE_TOP_MAX == 1024
    assert int(re.search(r"SAE_FILE_TOP_POSITIVE\s*=\s*(\d+)", hdr).group(1)) == E.FILE_TOP_POSITIVE
    top = open(os.path.join(ROOT, "freud_amd", "csrc", "file_top.h")).read()
    assert int(re.search(r"#define\s+FT_MAX_TOP\s+(\d+)", top).group(1)) == E.FILE_TOP_MAX
    assert build_units.assert_one_unit_builds("file_top.h") == "passes.hip"
    assert callable(E.file_top_features)


def test_n_top_range_is_checked_without_a_device(tmp_path):
    from freud_amd import file_features as FF
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((3, 8), np.float32), [4, 2])
    for bad in (0, -1, FF.FILE_TOP_MAX + 1):
        with pytest.raises(ValueError, match="n_top"):
            FF.file_features(None, str(tmp_path), "enc", bad)
        with pytest.raises(ValueError, match="n_top"):
            FF.top_activations_for_file(None, np.zeros((4, 2), np.float32), bad)
    with pytest.raises(ValueError, match=">= 1"):
        FF.file_features(None, str(tmp_path), "enc", 2, lengths=np.array([4, 0, 2]))
    with pytest.raises(ValueError, match="batch_files"):
        FF.file_features(None, str(tmp_path), "enc", 2, batch_files=0)


def test_npz_round_trip_and_decode(tmp_path):
    from freud_amd import file_features as FF

    def ordf(v):
        u = struct.unpack("<I", struct.pack("<f", v))[0]
        return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    keys = np.array([[(ordf(2.5) << 32) | (0xFFFFFFFF - 7), (ordf(-1.0) << 32) | 0xFFFFFFFF], [(ordf(0.5) << 32) | (0xFFFFFFFF - 1), 0]],
                    dtype=np.uint64)
    lat = np.array([[9, 3], [4, -1]], np.int32)
    ff = FF.FileFeatures(*FF.decode_file_table(lat, keys.view(np.int64)), ["a.flac", "b.flac"])
    assert ff.latents.dtype == np.int64 and ff.values.dtype == np.float32 and ff.frames.dtype == np.int64 and ff.times.dtype == np.float64
    assert ff.top(0) == [(9, 2.5, 7 * TIMESTEP_S), (3, -1.0, 0.0)] and ff.top("b.flac") == [(4, 0.5, TIMESTEP_S)]
    assert ff.latents[1, 1] == -1 and ff.frames[1, 1] == -1 and np.isnan(ff.values[1, 1]) and np.isnan(ff.times[1, 1])
    path = str(tmp_path / "ff.npz")
    ff.to_npz(path)
    back = FF.FileFeatures.from_npz(path)
    for k in ("latents", "values", "frames", "times"):
        np.testing.assert_array_equal(getattr(back, k), getattr(ff, k))
        assert getattr(back, k).dtype == getattr(ff, k).dtype
    assert back.filenames == ff.filenames
