"""CPU: the key and merge arithmetic of the feature search (freud_amd/csrc/search_keys.h -- what search.h's kernels compute per
(file, latent) and what the merge kernel does per latent) compiled for the HOST with g++ and replayed against the reference's
own top_activations (utils/activations.py:61-132) on a raw shard with planted ties (tests/golden/search_raw.npz, written by
tests/golden/make_search_golden.py): file order, values, times and the per-file list must be exactly the reference's.  Plus
properties of the order-preserving float map and the argument checks of freud_amd/feature_search.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "search_raw.npz")
TIMESTEP_S = 30 / 1500

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "search_keys.h"

// argv: data file (int32 nf, T, d, lengths[nf], float x[nf][T][d]) | n_top flags min max   -> per column: files, value bits,
// frames, per-file value bits.   "ord" mode: float bits on stdin lines -> sk_ord, sk_unord round trip.
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "ord")) {
    unsigned u;
    while (scanf("%x", &u) == 1) { float f = sk_float(u); printf("%08x %08x\n", sk_ord(f), sk_bits(sk_unord(sk_ord(f)))); }
    return 0;
  }
  FILE* fp = fopen(argv[1], "rb");
  int nf, T, d;
  if (fread(&nf, 4, 1, fp) != 1 || fread(&T, 4, 1, fp) != 1 || fread(&d, 4, 1, fp) != 1) return 2;
  std::vector<int> L(nf);
  std::vector<float> x((size_t)nf * T * d);
  if (fread(L.data(), 4, nf, fp) != (size_t)nf || fread(x.data(), 4, x.size(), fp) != x.size()) return 2;
  fclose(fp);
  const int n_top = atoi(argv[2]), flags = atoi(argv[3]);
  const double mn = atof(argv[4]), mx = atof(argv[5]);
  const bool abs_mode = flags & SK_ABS;
  // per-file keys exactly as search_colreduce_kernel + search_abs_fixup_kernel form them
  std::vector<uint64_t> keys((size_t)nf * d, 0), aux((size_t)nf * d, 0);
  for (int f = 0; f < nf; ++f)
    for (int j = 0; j < d; ++j) {
      int len = L[f] < 1 ? 1 : (L[f] > T ? T : L[f]);
      uint64_t best = 0, sbest = 0;
      for (int r = 0; r < len; ++r) {
        const float v = x[((size_t)f * T + r) * d + j];
        const uint64_t k = abs_mode ? sk_key(v < 0 ? -v : v, r) : sk_key(v, r), s = sk_key(v, r);
        if (k > best) best = k;
        if (s > sbest) sbest = s;
      }
      keys[(size_t)f * d + j] = best;
      aux[(size_t)f * d + j] = sk_aux(x[((size_t)f * T + sk_key_frame(best)) * d + j], sk_key_frame(sbest));
    }
  for (int j = 0; j < d; ++j) {
    std::vector<uint64_t> rk(n_top, 0);
    std::vector<int32_t> fr(n_top, 0);
    // batches of 3 files, as the loader would deliver them: the merge sees files in order whatever the batching
    for (int f = 0; f < nf; ++f)
      sk_merge_file(rk.data(), fr.data(), 1, n_top, keys[(size_t)f * d + j], abs_mode ? &aux[(size_t)f * d + j] : nullptr, flags, mn, mx, f);
    printf("col %d\n", j);
    for (int i = 0; i < n_top; ++i)
      printf("%lld %08x %d\n", (long long)sk_rank_file(rk[i]), sk_bits(sk_rank_value(rk[i])), fr[i]);
    for (int f = 0; f < nf; ++f)
      printf("%08x ", sk_bits(sk_candidate(keys[(size_t)f * d + j], abs_mode ? &aux[(size_t)f * d + j] : nullptr, flags).filt));
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("sk")
    src = d / "sk.cpp"
    src.write_text(_SRC)
    exe = d / "sk"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(prog, data, n_top, flags, mn, mx, d):
    out = subprocess.run([prog, data, str(n_top), str(flags), repr(mn), repr(mx)], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    res = []
    i = 0
    for _ in range(d):
        assert lines[i].startswith("col")
        top = [lines[i + 1 + k].split() for k in range(n_top)]
        per = [struct.unpack("<f", struct.pack("<I", int(h, 16)))[0] for h in lines[i + 1 + n_top].split()]
        res.append(([int(t[0]) for t in top], [struct.unpack("<f", struct.pack("<I", int(t[1], 16)))[0] for t in top],
                    [int(t[2]) for t in top], per))
        i += n_top + 2
    return res


def test_search_keys_replay_reference_golden(prog, tmp_path):
    g = np.load(GOLD)
    x, L = g["x"], g["lengths"]
    nf, T, d = x.shape
    data = tmp_path / "x.bin"
    data.write_bytes(np.array([nf, T, d], np.int32).tobytes() + L.astype(np.int32).tobytes() + x.astype(np.float32).tobytes())
    n_cases = len(g["case_feature"])
    cache = {}
    for c in range(n_cases):
        n_top, absm = int(g["case_n_top"][c]), int(g["case_absolute"][c])
        mn, mx = float(g["case_min_val"][c]), float(g["case_max_val"][c])
        flags = absm | (2 if not np.isnan(mn) else 0) | (4 if not np.isnan(mx) else 0)
        key = (n_top, flags, mn, mx)
        if key not in cache:
            cache[key] = _run(prog, str(data), n_top, flags, 0.0 if np.isnan(mn) else mn, 0.0 if np.isnan(mx) else mx, d)
        files, vals, frames, per = cache[key][int(g["case_feature"][c])]
        want_files = [int(f) for f in g["case_files"][c] if f >= 0]
        m = len(want_files)
        ctx = f"case {c}: n_top={n_top} abs={absm} min={mn} max={mx} feature={int(g['case_feature'][c])}"
        assert files[:m] == want_files and all(f == -1 for f in files[m:]), ctx
        assert vals[:m] == [float(v) for v in g["case_values"][c][:m]], ctx
        assert [fr * TIMESTEP_S for fr in frames[:m]] == [float(t) for t in g["case_times"][c][:m]], ctx
        assert per == [float(v) for v in g["case_max_per_file"][c]], ctx


def _ord(prog, floats):
    bits = [struct.unpack("<I", struct.pack("<f", f))[0] for f in floats]
    out = subprocess.run([prog, "ord"], input="\n".join(f"{b:x}" for b in bits), check=True, capture_output=True, text=True).stdout
    return [tuple(int(v, 16) for v in line.split()) for line in out.splitlines()]


def test_order_map_properties(prog):
    tiny = np.float32(1e-45)
    vals = [float("-inf"), -3.4e38, -1.0, -float(np.float32(1.2e-38)), -float(tiny), -0.0, 0.0, float(tiny), float(np.float32(1.2e-38)),
            1.0, 3.4e38, float("inf")]
    vals = [float(np.float32(v)) for v in vals]          # (fp32 values, the sign of -0.0 kept)
    res = _ord(prog, vals)
    o = [r[0] for r in res]
    assert o[5] == o[6], "-0.0 and +0.0 must share one code (torch max / argmax treat them as equal)"
    for a, b, fa, fb in zip(o, o[1:], vals, vals[1:]):
        if fa != fb:
            assert a < b, f"order broken between {fa} and {fb}"
    back = [struct.unpack("<f", struct.pack("<I", r[1]))[0] for r in res]
    for v, bk in zip(vals, back):
        assert bk == v and (v != 0.0 or struct.pack("<f", bk) == struct.pack("<f", 0.0))
    assert o[0] == 0x007FFFFF and o[-1] == 0xFF800000
    rng = np.random.default_rng(0)
    r = rng.standard_normal(2000).astype(np.float32) * np.float32(10.0) ** rng.integers(-40, 38, 2000).astype(np.float32)
    r = r[np.isfinite(r)]
    res = _ord(prog, [float(v) for v in r])
    codes = np.array([c[0] for c in res], dtype=np.uint64)
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff(codes[order].astype(np.int64)) >= 0)


def _shards(tmp_path, n=3, T=4, d=2):
    from freud_amd.loader import write_shards
    write_shards(str(tmp_path), "enc", np.zeros((n, T * d), np.float32), [T, d])
    return str(tmp_path)


def test_feature_search_argument_checks(tmp_path):
    from freud_amd import feature_search as FS
    path = _shards(tmp_path)
    with pytest.raises(ValueError, match=">= 1"):
        FS.search_features(None, path, "enc", 2, lengths=np.array([4, 0, 2]))
    with pytest.raises(ValueError, match="one entry per file"):
        FS.search_features(None, path, "enc", 2, lengths=np.array([4, 2]))
    with pytest.raises(ValueError, match="integers"):
        FS.search_features(None, path, "enc", 2, lengths=np.array([4.0, 2.0, 1.0]))
    with pytest.raises(ValueError, match="n_files"):
        FS.search_features(None, path, "enc", 0)
    with pytest.raises(ValueError, match="batch_files"):
        FS.search_features(None, path, "enc", 2, batch_files=0)
    assert FS.check_lengths(np.array([9, 1, 4]), 3, 4).tolist() == [4, 1, 4]      # capped at T (the slice caps the reference)


def test_decode_table_round_trip():
    from freud_amd import feature_search as FS
    # rank keys of search_keys.h: ord(value) << 32 | (0xFFFFFFFF - file); 0 = empty
    def ordf(v):
        u = struct.unpack("<I", struct.pack("<f", v))[0]
        return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    r = np.array([[(ordf(2.5) << 32) | (0xFFFFFFFF - 3), (ordf(-1.0) << 32) | (0xFFFFFFFF - 0)], [0, 0]], dtype=np.uint64)
    fr = np.array([[7, 2], [0, 0]], dtype=np.int32)
    v, f, frames, t = FS.decode_table(r.view(np.int64), fr)
    assert v[0, 0] == 2.5 and f[0, 0] == 3 and frames[0, 0] == 7 and t[0, 0] == 7 * TIMESTEP_S
    assert v[1, 0] == -1.0 and f[1, 0] == 0 and f[0, 1] == -1 and np.isnan(v[0, 1]) and frames[1, 1] == -1


def test_default_batch_files_reaches_the_streaming_gemm():
    """Default files per batch: enough rows that the encoder GEMM has >= 2048 output tiles of 256 x 256 (the condition of its
    streaming form, the one the fused L1 search epilogue runs in)."""
    from freud_amd import feature_search as FS
    for T, n in [(1500, 3072), (1500, 40960), (1500, 12288), (50, 16384), (1500, 1024)]:
        B = FS.default_batch_files(T, n, 10 ** 6)
        n_p = -(-n // 128) * 128
        tiles = (-(-B * T // 256)) * (n_p // 256)
        assert B >= 16 and tiles >= 2048, (T, n, B, tiles)
        assert B == 16 or (-(-(B - 1) * T // 256)) * (n_p // 256) < 2048, (T, n, B)     # the fewest such files
    assert FS.default_batch_files(1500, 3072, 10 ** 6) == 30
    assert FS.default_batch_files(1500, 3072, 7) == 7
    assert FS.default_batch_files(1500, None, 100) == 16
    assert FS.default_batch_files(1500, 1100, 10 ** 6) == 16     # n_p = 1152: no multiple of 256, the GEMM never streams
