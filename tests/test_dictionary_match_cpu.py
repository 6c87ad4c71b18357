"""CPU: the host part of the dictionary comparison (freud_amd/csrc/dict_match.h) compiled with g++ -- the hi / lo bf16 split of a unit
vector's elements and the cosine keys -- plus the boundary (header, symbol list), the DictionaryMatch table methods on a hand-made
table, and the argument errors that need no device."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import build_units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sae_dict_pack_bytes", "sae_dict_pack", "sae_dict_sim_keys")

_SRC = r"""
#include <stdio.h>
#include <vector>
#include "dict_match.h"

// argv: file of fp32 -> per value "hi-bits lo-bits key-hex"; then one line "rows_p d_p ld bytes" for n = 300, d = 100
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) return 2;
  float v;
  while (fread(&v, 4, 1, fp) == 1)
    printf("%04x %04x %016llx\n", (unsigned)dm_split_hi(v), (unsigned)dm_split_lo(v), (unsigned long long)dm_key(v));
  fclose(fp);
  printf("%lld %lld %lld %lld\n", (long long)dm_rows_p(300), (long long)dm_d_p(100), (long long)dm_ld(100), (long long)dm_pack_bytes(300, 100));
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("dm")
    src = d / "dm.cpp"
    src.write_text(_SRC)
    exe = d / "dm"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def run(prog, tmp_path, values):
    data = tmp_path / "v.bin"
    data.write_bytes(np.asarray(values, np.float32).tobytes())
    lines = subprocess.run([prog, str(data)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [ln.split() for ln in lines[:len(values)]]
    hi = np.array([int(r[0], 16) for r in rows], np.uint32)
    lo = np.array([int(r[1], 16) for r in rows], np.uint32)
    keys = [int(r[2], 16) for r in rows]
    return hi, lo, keys, [int(v) for v in lines[len(values)].split()]


def bf16_value(bits16):
    return (bits16.astype(np.uint32) << 16).view(np.float32)


def test_split_reproduces_the_unit_vector_element(prog, tmp_path):
    g = np.random.default_rng(0)
    # the elements of unit vectors: |u| <= 1, over six decades, plus the edge values
    u = (g.standard_normal(100_000) * 10.0 ** g.uniform(-6, 0, 100_000)).astype(np.float32)
    u = np.concatenate([np.clip(u, -1, 1), np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -20], np.float32)])
    hi, lo, _keys, dims = run(prog, tmp_path, u)
    h, l = bf16_value(hi).astype(np.float64), bf16_value(lo).astype(np.float64)
    err = np.abs(h + l - u.astype(np.float64))
    assert (err <= 2.0 ** -17 * np.abs(u.astype(np.float64))).all(), float((err / np.maximum(np.abs(u), 1e-30)).max())
    # hi is the nearest bf16 (ties to even): torch's conversion is the witness
    import torch
    want_hi = torch.from_numpy(u).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(hi.astype(np.uint16), want_hi)
    # the edge values: 0, -0.0 and 1.0 are bf16 numbers
    for k in range(6):
        assert h[-6 + k] == float(u[-6 + k]) and l[-6 + k] == 0.0
    assert dims == [512, 128, 384, 512 * 384 * 2]


def test_lo_is_zero_for_bf16_numbers(prog, tmp_path):
    g = np.random.default_rng(1)
    bits = g.integers(0, 1 << 16, 20_000).astype(np.uint32)
    u = bf16_value(bits)
    u = u[np.isfinite(u)]
    hi, lo, _keys, _ = run(prog, tmp_path, u)
    np.testing.assert_array_equal(bf16_value(hi).view(np.uint32), u.view(np.uint32))
    assert (bf16_value(lo) == 0.0).all()


def test_keys_order_signed_cosines(prog, tmp_path):
    g = np.random.default_rng(2)
    s = np.concatenate([g.uniform(-1.0, 1.0, 4000), [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23, 1e-38, -1e-38, 3e38, -3e38],
                        [np.inf, -np.inf]]).astype(np.float32)
    _hi, _lo, keys, _ = run(prog, tmp_path, s)
    keys = np.array(keys, np.uint64)
    assert (keys != 0).all(), "a finite cosine (and an infinite one) never maps to the not-eligible key"
    assert (keys & np.uint64(0xFFFFFFFF) == 0).all()
    assert keys[4000] == keys[4001], "-0.0 and 0.0 share a key"
    order = np.argsort(s, kind="stable")
    ks, ss = keys[order], s[order]
    assert (ks[1:] >= ks[:-1]).all()
    strictly = ss[1:] > ss[:-1]
    assert ((ks[1:] > ks[:-1]) == strictly).all(), "keys order exactly as the floats do"
    # the decode used by the Python layer inverts the key
    from freud_amd.feature_search import unord
    back = unord((keys >> np.uint64(32)).astype(np.uint32))
    np.testing.assert_array_equal(back[s != 0].view(np.uint32), s[s != 0].view(np.uint32))


def test_boundary_has_the_entry_points():
    from freud_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    for sym in SYMBOLS:
        assert sym in E.EXPORTED_SYMBOLS
        assert re.search(r"\bint(64_t)?\s+" + sym + r"\s*\(", hdr), sym
    assert int(re.search(r"#define\s+SAE_DICT_MAX_D\s+(\d+)", hdr).group(1)) == E.DICT_MAX_D == 8192
    assert (E.DICT_LEFT, E.DICT_RIGHT) == (0, 1) and re.search(r"SAE_DICT_LEFT\s*=\s*0,\s*SAE_DICT_RIGHT\s*=\s*1", hdr)
    assert build_units.assert_one_unit_builds("dict_match.h") == "passes.hip"
    assert callable(E.dict_pack) and callable(E.dict_sim_keys) and callable(E.dict_pack_bytes)
    lib = E.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym)
    assert lib.sae_dict_pack_bytes(300, 100) == 512 * 384 * 2
    assert lib.sae_dict_pack_bytes(0, 100) == 0 and lib.sae_dict_pack_bytes(300, 8193) == 0 and lib.sae_dict_pack_bytes((1 << 24) + 1, 4) == 0


def hand_table():
    """4 directions against themselves, K = 3: 0 and 2 are duplicates, 1 is near 0 and 2, 3 has one (negative) neighbour only."""
    from freud_amd import dictionary_match as DM
    nan = np.float32(np.nan)
    nb = np.array([[2, 1, 3], [0, 2, 3], [0, 1, 3], [0, -1, -1]], np.int32)
    cs = np.array([[1.0, 0.9, -0.2], [0.9, 0.9, 0.1], [1.0, 0.9, -0.2], [-0.2, nan, nan]], np.float32)
    return DM.DictionaryMatch(nb, cs, np.array([1, 2, 3, 0.5], np.float32), np.array([1, 2, 3, 0.5], np.float32), True)


def test_table_methods_on_a_hand_made_table():
    m = hand_table()
    assert m.n_a == 4 and m.n_b == 4
    assert m.top(0) == [(2, 1.0), (1, float(np.float32(0.9))), (3, float(np.float32(-0.2)))]
    assert m.top(3) == [(0, float(np.float32(-0.2)))]
    idx, cos = m.best()
    assert idx.tolist() == [2, 0, 0, 0] and cos.dtype == np.float32
    want = (1.0 + float(np.float32(0.9)) + 1.0 + float(np.float32(-0.2))) / 4
    assert m.mmcs() == pytest.approx(want, abs=1e-12)
    assert m.matched(0.95).tolist() == [True, False, True, False]
    assert m.matched(-1.0).tolist() == [True] * 4
    assert m.duplicates(0.999).tolist() == [[0, 2]]
    assert m.duplicates(0.85).tolist() == [[0, 1], [0, 2], [1, 2]]
    assert m.duplicates(2.0).shape == (0, 2)
    s = m.summary(0.95)
    assert s["n_a"] == 4 and s["n_neighbors"] == 3 and s["self_mode"] and s["matched"] == 2 and s["duplicate_pairs"] == 1
    assert s["mmcs"] == pytest.approx(want, abs=1e-12)
    # empty slots: NaN and -1 stay out of every statistic
    assert np.isnan(m.cosines[3, 1:]).all() and (m.neighbors[3, 1:] == -1).all()
    m.self_mode = False
    with pytest.raises(ValueError, match="itself"):
        m.duplicates(0.5)
    # a table without any neighbour (one direction against itself)
    from freud_amd import dictionary_match as DM
    e = DM.DictionaryMatch(np.full((1, 2), -1, np.int32), np.full((1, 2), np.nan, np.float32), np.ones(1, np.float32), np.ones(1, np.float32), True)
    assert np.isnan(e.mmcs()) and e.matched(0.0).tolist() == [False] and e.duplicates(0.0).shape == (0, 2) and e.summary()["mmcs"] is None


def test_npz_round_trip(tmp_path):
    from freud_amd import dictionary_match as DM
    m = hand_table()
    path = str(tmp_path / "m.npz")
    m.to_npz(path)
    back = DM.DictionaryMatch.from_npz(path)
    assert back.self_mode is True
    for k in ("neighbors", "cosines", "norms_a", "norms_b"):
        assert getattr(back, k).tobytes() == getattr(m, k).tobytes() and getattr(back, k).dtype == getattr(m, k).dtype
    assert np.isnan(back.cosines[3, 1]) and back.neighbors[3, 1] == -1


def test_arguments_are_checked_without_a_device():
    from freud_amd import dictionary_match as DM
    from freud_amd.engine import FILE_TOP_MAX
    import torch
    g = np.random.default_rng(3)
    a, b = g.standard_normal((6, 5)).astype(np.float32), g.standard_normal((7, 4)).astype(np.float32)
    with pytest.raises(ValueError, match="d=5 and d=4"):
        DM.compare_dictionaries(a, b)
    with pytest.raises(ValueError, match="d=5 and d=4"):
        DM.compare_dictionaries(torch.from_numpy(a), torch.from_numpy(b))
    for bad in (0, -1, FILE_TOP_MAX + 1):
        with pytest.raises(ValueError, match="n_neighbors"):
            DM.compare_dictionaries(a, n_neighbors=bad)
    for poison in (np.nan, np.inf, -np.inf):
        w = a.copy()
        w[3, 2] = poison
        with pytest.raises(ValueError, match="non-finite"):
            DM.compare_dictionaries(w)
        with pytest.raises(ValueError, match="non-finite"):
            DM.compare_dictionaries(a, w)
    with pytest.raises(ValueError, match=r"\[n\]\[d\]"):
        DM.compare_dictionaries(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="d in"):
        DM.compare_dictionaries(np.zeros((2, 8193), np.float32))
    # the global RNG is left alone even when the call fails
    torch.manual_seed(5)
    before = torch.get_rng_state()
    with pytest.raises(ValueError):
        DM.compare_dictionaries(a, b)
    assert torch.equal(before, torch.get_rng_state())
