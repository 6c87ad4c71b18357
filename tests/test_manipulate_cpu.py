"""CPU: the arithmetic of the feature manipulation (freud_amd/csrc/manip.h, its host part) compiled with g++ -- sm_new / sm_delta
against numpy float32 to the bit, sm_apply_serial against the REAL reference's manipulate_latent (tests/golden/manipulate_*.npz,
made by tests/golden/make_manipulate_golden.py) within the fp32 summation bound -- plus the boundary (header constants, symbol
list), the argument errors that need no device, the npz round trip and the raw branch."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "manip.h"

// argv[1] = "ops":   file of (int32 op, float a, float value) records -> per record "new-bits delta-bits"
// argv[1] = "apply": file of int32 d, E, then ops[E], a[E], values[E], standard[d], w[E][d] -> d lines of out bits
int main(int argc, char** argv) {
  FILE* fp = fopen(argv[2], "rb");
  if (!fp) return 2;
  if (!strcmp(argv[1], "ops")) {
    struct { int32_t op; float a, value; } r;
    while (fread(&r, 12, 1, fp) == 1) printf("%08x %08x\n", sk_bits(sm_new(r.op, r.a, r.value)), sk_bits(sm_delta(r.op, r.a, r.value)));
    return 0;
  }
  int32_t hdr[2];
  if (fread(hdr, 4, 2, fp) != 2) return 2;
  const int d = hdr[0], E = hdr[1];
  std::vector<int32_t> ops(E);
  std::vector<float> a(E), values(E), standard(d), w((size_t)E * d), out(d);
  if (fread(ops.data(), 4, E, fp) != (size_t)E || fread(a.data(), 4, E, fp) != (size_t)E || fread(values.data(), 4, E, fp) != (size_t)E ||
      fread(standard.data(), 4, d, fp) != (size_t)d || fread(w.data(), 4, (size_t)E * d, fp) != (size_t)E * d) return 2;
  sm_apply_serial(standard.data(), d, E, ops.data(), a.data(), values.data(), w.data(), d, out.data());
  for (int c = 0; c < d; ++c) printf("%08x\n", sk_bits(out[c]));
  return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("sm")
    src = d / "sm.cpp"
    src.write_text(_SRC)
    exe = d / "sm"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def apply_serial(prog, tmp_path, standard, ops, a, values, w):
    E, d = w.shape
    blob = (np.array([d, E], np.int32).tobytes() + np.asarray(ops, np.int32).tobytes() + np.asarray(a, np.float32).tobytes()
            + np.asarray(values, np.float32).tobytes() + np.asarray(standard, np.float32).tobytes() + np.ascontiguousarray(w, np.float32).tobytes())
    f = tmp_path / "apply.bin"
    f.write_bytes(blob)
    out = subprocess.run([prog, "apply", str(f)], check=True, capture_output=True, text=True).stdout.split()
    return np.array([int(t, 16) for t in out], np.uint32).view(np.float32)


def test_new_and_delta_match_numpy_float32_to_the_bit(prog, tmp_path):
    tiny = np.float32(1e-45)
    grid = np.array([0.0, -0.0, tiny, -tiny, 1e-40, 1.17549435e-38, 1e-3, 0.1, 1.0, 1.5, -2.0, 3.14159274, 10.0, 255.0, 65504.0, 3e38, -3e38,
                     1e20, 7.0 / 3.0], np.float32)
    recs = np.array([(op, a, v) for op in (0, 1) for a in grid for v in grid], dtype=[("op", "<i4"), ("a", "<f4"), ("v", "<f4")])
    f = tmp_path / "ops.bin"
    f.write_bytes(recs.tobytes())
    lines = subprocess.run([prog, "ops", str(f)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    got = np.array([[int(t, 16) for t in ln.split()] for ln in lines], np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        new = np.where(recs["op"] == 1, recs["v"], recs["a"] * recs["v"]).astype(np.float32)
        delta = (new - recs["a"]).astype(np.float32)
    nan = np.isnan(delta)                       # (inf - inf of an overflowed product: any NaN is a NaN)
    assert np.array_equal(got[:, 0], new.view(np.uint32))
    assert np.array_equal(got[~nan, 1], delta.view(np.uint32)[~nan]) and np.isnan(got[nan, 1].view(np.float32)).all()
    assert (np.abs(recs["a"]) < 1.2e-38).any() and (delta.view(np.uint32) == 0x80000000).any()       # subnormals and a -0.0 result occur


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_apply_serial_reproduces_the_reference(prog, tmp_path, kind):
    """The rank-one rule on the golden's fp32 latent and fp32 decoder operand against the reference's decode of the edited latent:
    |diff| <= (n + 2) * 2^-24 * (sum_j |c_j w_j| + |delta w|), the worst case of any fp32 summation order of the n + 1 terms."""
    g = np.load(os.path.join(GOLD, f"manipulate_{kind}.npz"))
    Wd = g["W_decode"].T if kind == "l1" else g["W_dec"]                     # [n, d]: row j = the operand row of latent j
    n = Wd.shape[0]
    dense, std, man = g["dense"], g["standard_decoded"], g["manipulated_decoded"]
    F, T, _ = dense.shape
    absum = np.abs(dense.astype(np.float64)) @ np.abs(Wd.astype(np.float64))                       # [F, T, d]
    if kind == "topk":
        absum += np.abs(g["b_dec"].astype(np.float64))
    checked = moved = 0
    for i, feat in enumerate(g["features"]):
        w = Wd[feat][None]
        for v, factor in enumerate(g["factors"]):
            for f in range(F):
                for t in range(0, T, 7):
                    a = dense[f, t, feat]
                    out = apply_serial(prog, tmp_path, std[f, t], [0], [a], [factor], w)
                    delta = np.float32(np.float32(a * factor) - a)
                    bound = (n + 2) * U * (absum[f, t] + np.abs(float(delta) * w[0].astype(np.float64)))
                    assert (np.abs(out.astype(np.float64) - man[i, v, f, t]) <= bound).all(), (kind, feat, factor, f, t)
                    if factor == 1.0:
                        assert np.array_equal(out.view(np.uint32), std[f, t].view(np.uint32))
                    checked += 1
                    moved += int(delta != 0)
    assert checked > 100 and moved > 20


def test_set_on_a_frame_without_the_latent_adds_value_times_w(prog, tmp_path):
    g = np.load(os.path.join(GOLD, "manipulate_topk.npz"))
    some = int(g["features"][3])
    f, t = np.argwhere(g["dense"][:, :, some] == 0)[0]
    std, w = g["standard_decoded"][f, t], g["W_dec"][some]
    out = apply_serial(prog, tmp_path, std, [1], [0.0], [2.5], w[None])
    want = np.array([np.float32(np.float64(2.5) * float(wi) + float(si)) for wi, si in zip(w, std)], np.float32)      # fmaf: one rounding
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_two_edits_apply_in_the_order_given(prog, tmp_path):
    r = np.random.default_rng(3)
    std, w = r.standard_normal(40).astype(np.float32), r.standard_normal((2, 40)).astype(np.float32)
    out = apply_serial(prog, tmp_path, std, [0, 1], [1.25, 0.5], [3.0, -1.0], w)
    d0, d1 = np.float32(np.float32(1.25 * 3.0) - np.float32(1.25)), np.float32(np.float32(-1.0) - np.float32(0.5))
    step = np.array([np.float32(float(d0) * float(a) + float(b)) for a, b in zip(w[0], std)], np.float32)
    want = np.array([np.float32(float(d1) * float(a) + float(b)) for a, b in zip(w[1], step)], np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


# ---- boundary
def test_header_constants_and_symbol():
    from freud_amd import engine
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    assert int(re.search(r"#define SAE_MANIP_MAX_EDITS (\d+)", text).group(1)) == engine.MANIP_MAX_EDITS == 16
    assert int(re.search(r"#define SAE_MANIP_MAX_VARIANTS (\d+)", text).group(1)) == engine.MANIP_MAX_VARIANTS == 16
    m = re.search(r"enum \{ SAE_MANIP_SCALE = (\d+), SAE_MANIP_SET = (\d+) \}", text)
    assert (int(m.group(1)), int(m.group(2))) == (engine.MANIP_OPS["scale"], engine.MANIP_OPS["set"])
    assert "sae_manipulate_files" in engine.EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "freud_amd", "csrc", "manip.h")).read()
    assert re.search(r"enum \{ SM_SCALE = 0, SM_SET = 1 \}", src) and "#define SM_MAX_EDITS 16" in src and "#define SM_MAX_VARIANTS 16" in src


class _NoEngine:
    """Stands where a freud_amd.models SAE stands; any use of the engine is an error."""
    activation_size, n_dict_components = 32, 128

    def _ensure(self, rows):
        raise AssertionError("the engine was reached before the arguments were checked")


@pytest.mark.parametrize("edits,values,lengths,word", [
    ([(3, "scale"), (3, "set")], [[1.0, 2.0]], None, "twice"),
    ([(128, "scale")], [[1.0]], None, "outside"),
    ([(-1, "scale")], [[1.0]], None, "outside"),
    ([(j, "scale") for j in range(17)], [[1.0] * 17], None, "17 edits"),
    ([(3, "scale")], [[float(v)] for v in range(17)], None, "17 variants"),
    ([(3, "scale")], [[float("nan")]], None, "finite"),
    ([(3, "scale")], [[float("inf")]], None, "finite"),
    ([(3, "scale")], [[1e39]], None, "finite"),
    ([(3, "scale"), (4, "set")], [[1.0], [2.0]], None, "values must be"),
    ([(3, "scale")], [1.0], None, "values must be"),
    ([(3, "clamp")], [[1.0]], None, "op="),
    ([(3, "scale")], None, None, "must be (latent, op, value)"),
    ([], [[]], None, "0 edits"),
    ([(3, "scale")], [[1.0]], [60, 0], ">= 1"),
    ([(3, "scale")], [[1.0]], [60], "one entry per file"),
    ([(3, "scale")], [[1.0]], [60.0, 7.0], "integers"),
])
def test_argument_checks_come_before_the_engine(edits, values, lengths, word):
    from freud_amd.manipulate import manipulate_features
    x = torch.zeros(2, 60, 32)
    with pytest.raises(ValueError, match=re.escape(word)):
        manipulate_features(_NoEngine(), x, edits, values, lengths)


def test_shape_checks_come_before_the_engine():
    from freud_amd.manipulate import manipulate_features, manipulate_latent
    with pytest.raises(ValueError, match="d_model=32"):
        manipulate_features(_NoEngine(), torch.zeros(2, 60, 48), [(3, "scale")], [[1.0]])
    with pytest.raises(ValueError, match="needs an SAE"):
        manipulate_features(None, torch.zeros(2, 60, 32), [(3, "scale")], [[1.0]])
    with pytest.raises(ValueError, match="one file"):
        manipulate_latent(_NoEngine(), torch.zeros(2, 60, 32), 3, 1.5)
    with pytest.raises(ValueError, match="not finite"):
        manipulate_latent(_NoEngine(), torch.zeros(1, 60, 32), 3, float("nan"))


def test_check_edits_forms():
    from freud_amd.manipulate import check_edits
    lat, ops, val = check_edits(128, [(0, "scale", 1.5), (127, 1, -2.0)])
    assert lat.tolist() == [0, 127] and ops.tolist() == [0, 1] and val.tolist() == [[1.5, -2.0]] and val.dtype == np.float32
    lat, ops, val = check_edits(128, [(5, "set")], [[0.0], [3.0]])
    assert val.shape == (2, 1) and ops.tolist() == [1]


def test_npz_round_trip(tmp_path):
    from freud_amd.manipulate import Manipulation, edited_series
    r = torch.Generator().manual_seed(1)
    B, T, d, lens = 2, 9, 4, [9, 5]
    vals = np.array([[0.5, 2.0], [-1.0, 0.0], [3.0, 1.0]], np.float32)
    std = [[torch.rand(L, generator=r) for L in lens] for _ in range(2)]
    man = [[[edited_series(std[e][f], e, float(vals[v, e])) for f in range(B)] for e in range(2)] for v in range(3)]
    m = Manipulation(torch.rand(B, T, d, generator=r), torch.rand(3, B, T, d, generator=r), std, man, [7, 100], ["scale", "set"], vals)
    path = str(tmp_path / "m.npz")
    m.save(path)
    k = Manipulation.load(path)
    assert torch.equal(k.standard_decoded, m.standard_decoded) and torch.equal(k.manipulated_decoded, m.manipulated_decoded)
    assert k.latents == [7, 100] and k.ops == ["scale", "set"] and np.array_equal(k.values, vals)
    for e in range(2):
        for f in range(B):
            assert torch.equal(k.standard_activations[e][f], std[e][f])
            for v in range(3):
                assert torch.equal(k.manipulated_activations[v][e][f], man[v][e][f])
    assert torch.equal(man[1][1][0], torch.zeros(9)) and torch.equal(man[0][0][1], std[0][1] * 0.5)


def test_raw_branch_is_the_reference_exactly():
    from freud_amd.manipulate import manipulate_latent
    g = np.load(os.path.join(GOLD, "manipulate_raw.npz"))
    x = torch.from_numpy(g["x"])
    for i, feat in enumerate(g["features"]):
        for v, factor in enumerate(g["factors"]):
            for f, L in enumerate(g["lengths"]):
                s, m, a, b = manipulate_latent(None, x[f:f + 1], int(feat), float(factor), int(L))
                assert s.shape == (1, 60, 32) and a.shape == (L,) and b.shape == (L,)
                assert np.array_equal(s[0].numpy(), g["standard_decoded"][f]) and np.array_equal(m[0].numpy(), g["manipulated_decoded"][i, v, f])
                assert np.array_equal(a.numpy(), g["standard_activations"][i, f, :L])
                assert np.array_equal(b.numpy(), g["manipulated_activations"][i, v, f, :L])
