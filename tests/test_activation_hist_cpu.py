"""CPU: the activation histograms without a device.

* the bin arithmetic of freud_amd/csrc/hist_bins.h compiled for the HOST with g++: hist_bin of all 32 768 bf16 magnitudes against
  np.searchsorted over the closed-form edges plus the three special bins, hist_edge against the closed form, every edge a bf16
  value; the serial reference hist_rows_ref against a numpy restatement on random bf16 rows, with and without lengths;
* the boundary: the header declares sae_hist_files, the library exports it, engine.EXPORTED_SYMBOLS lists it; every argument rule
  of freud_amd.activation_hist that needs no device raises ValueError;
* ActivationHistograms on hand-made arrays: quantile brackets, files_in_range, the npz round trip."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = [(-12, 24, 2), (-2, 3, 0), (-126, 16, 3), (0, 128, 0)]

_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hist_bins.h"

// bins L O s  -> ok nb, then hist_bin of every magnitude 0 .. 32767, then the bits of hist_edge(0 .. O P)
// rows FILE   -> (int32 L O s nf T ld n has_len, int32 lengths[nf], uint16 lat[nf T][ld]) -> n_frames, frame_hist, file_max_hist
int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "bins")) {
    const HistSpec sp{atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
    printf("%d %d\n", (int)hist_spec_ok(sp), hist_spec_ok(sp) ? hist_nbins(sp) : 0);
    if (!hist_spec_ok(sp)) return 0;
    for (uint32_t m = 0; m < 32768; ++m) printf("%d\n", hist_bin(m, sp));
    for (int i = 0; i <= hist_regular(sp); ++i) { const float e = hist_edge(i, sp); uint32_t u; memcpy(&u, &e, 4); printf("%08x\n", u); }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "rows")) {
    FILE* fp = fopen(argv[2], "rb");
    int h[8];
    if (!fp || fread(h, 4, 8, fp) != 8) return 2;
    const HistSpec sp{h[0], h[1], h[2]};
    const int nf = h[3], T = h[4], ld = h[5], n = h[6], has_len = h[7];
    std::vector<int> L(nf);
    std::vector<uint16_t> lat((size_t)nf * T * ld);
    if (fread(L.data(), 4, nf, fp) != (size_t)nf || fread(lat.data(), 2, lat.size(), fp) != lat.size()) return 2;
    fclose(fp);
    const int nb = hist_nbins(sp);
    std::vector<int64_t> fh((size_t)n * nb, 0), mh((size_t)n * nb, 0);
    int64_t frames = 0;
    hist_rows_ref(lat.data(), ld, n, nf, T, has_len ? L.data() : nullptr, sp, fh.data(), mh.data(), &frames);
    printf("%lld\n", (long long)frames);
    for (int64_t v : fh) printf("%lld\n", (long long)v);
    for (int64_t v : mh) printf("%lld\n", (long long)v);
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("hb")
    src = d / "hb.cpp"
    src.write_text(_SRC)
    exe = d / "hb"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/freud_amd/csrc", str(src), "-o", str(exe)], check=True)
    return str(exe)


def closed_form_edges(spec):
    L, O, s = spec
    P = 1 << s
    i = np.arange(O * P + 1)
    return np.ldexp(1.0 + (i % P) / P, L + i // P)          # float64: 2^128 is finite here


def np_bins(mag, spec):
    """Bins of bf16 magnitude patterns by VALUE: searchsorted over the closed-form edges, plus the three special bins."""
    mag = np.asarray(mag, np.uint32) & 0x7FFF
    val = (mag << 16).astype(np.uint32).view(np.float32).astype(np.float64)
    e = closed_form_edges(spec)
    b = 1 + np.searchsorted(e, val, side="right")            # below e[0]: 1; e[i] <= v < e[i + 1]: 2 + i; >= e[-1]: len(e) + 1 = NB - 1
    b = np.where(np.isnan(val), len(e) + 1, b)               # NaN patterns: overflow
    return np.where(mag == 0, 0, b).astype(np.int64)


def bf16_bits(x):
    """float32 -> bf16 bit patterns (round to nearest even), uint16."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", SPECS)
def test_hist_bin_of_every_magnitude_and_edges(prog, spec):
    out = subprocess.run([prog, "bins", *map(str, spec)], check=True, capture_output=True, text=True).stdout.split()
    L, O, s = spec
    nreg = O << s
    assert out[0] == "1" and int(out[1]) == nreg + 3
    got = np.array(out[2:2 + 32768], np.int64)
    want = np_bins(np.arange(32768), spec)
    np.testing.assert_array_equal(got, want)
    assert got[0] == 0 and (got[1:0x80] == 1).all()                         # every subnormal: underflow
    assert (got[0x7F80:] == nreg + 2).all()                                 # Inf and NaN patterns: overflow
    assert set(np.unique(got)) >= set(range(2, nreg + 2))                   # every regular bin is hit
    edge_bits = np.array([int(v, 16) for v in out[2 + 32768:]], np.uint32)
    assert edge_bits.shape[0] == nreg + 1
    edges = edge_bits.view(np.float32)
    np.testing.assert_array_equal(edges, closed_form_edges(spec).astype(np.float32))      # (2^128 as a float is +inf)
    assert (edge_bits & 0xFFFF == 0).all()                                  # a bf16 value: the low 16 bits are empty
    np.testing.assert_array_equal(bf16_bits(edges).astype(np.uint32) << 16, edge_bits)    # round trip through bf16


def test_engine_layer_restates_the_bins():
    """freud_amd.engine.hist_nbins and ActivationHistograms.edges() agree with the header."""
    from freud_amd.activation_hist import ActivationHistograms
    from freud_amd.engine import hist_nbins
    for spec in SPECS:
        nb = hist_nbins(spec)
        assert nb == (spec[1] << spec[2]) + 3
        ah = ActivationHistograms(0, 0, spec, np.zeros((1, nb), np.int64), np.zeros((1, nb), np.int64))
        np.testing.assert_array_equal(ah.edges(), closed_form_edges(spec))
    assert hist_nbins((-12, 24, 2)) == 99


@pytest.mark.parametrize("bad", [(-127, 4, 0), (-12, 0, 2), (0, 129, 0), (100, 29, 0), (-12, 24, 4), (-12, 24, -1), (-12, 33, 2), (-20, 17, 3)])
def test_bad_specs_are_refused_by_header_and_python(prog, bad):
    from freud_amd.engine import hist_nbins
    out = subprocess.run([prog, "bins", *map(str, bad)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "0"
    with pytest.raises(ValueError):
        hist_nbins(bad)


@pytest.mark.parametrize("with_lengths", [False, True])
@pytest.mark.parametrize("spec", [(-12, 24, 2), (-2, 3, 3)])
def test_serial_reference_against_numpy(prog, tmp_path, spec, with_lengths):
    g = np.random.default_rng(7)
    nf, T, ld, n = 5, 37, 24, 19
    v = np.where(g.random((nf * T, ld)) < 0.4, 0.0, np.exp(g.normal(0, 3, (nf * T, ld)))).astype(np.float32)
    lat = bf16_bits(v)
    lat[3, 2] = 0x8000                      # -0.0: inactive
    lat[5, 1] = 0x7F80                      # +Inf: overflow
    lat[6, 1] = 0x0001                      # a subnormal: underflow
    lat[:, 4] = 0                           # a dead column
    L = np.array([T, 1, 20, T + 5, 9], np.int32)
    path = tmp_path / "rows.bin"
    with open(path, "wb") as f:
        f.write(np.array([*spec, nf, T, ld, n, int(with_lengths)], np.int32).tobytes())
        f.write(L.tobytes())
        f.write(lat.tobytes())
    out = np.array(subprocess.run([prog, "rows", str(path)], check=True, capture_output=True, text=True).stdout.split(), np.int64)
    nb = (spec[1] << spec[2]) + 3
    frames, fh, mh = out[0], out[1:1 + n * nb].reshape(n, nb), out[1 + n * nb:].reshape(n, nb)
    lens = np.minimum(L, T) if with_lengths else np.full(nf, T)
    want_f, want_m = np.zeros((n, nb), np.int64), np.zeros((n, nb), np.int64)
    mags = (lat & 0x7FFF).reshape(nf, T, ld)
    for f in range(nf):
        m = mags[f, :lens[f], :n]
        b = np_bins(m, spec)
        for j in range(n):
            want_f[j] += np.bincount(b[:, j], minlength=nb)
            want_m[j, np_bins(m[:, j].max(), spec)] += 1
    assert frames == lens.sum()
    np.testing.assert_array_equal(fh, want_f)
    np.testing.assert_array_equal(mh, want_m)
    assert (fh.sum(1) == frames).all() and (mh.sum(1) == nf).all()
    assert fh[4, 0] == frames and mh[4, 0] == nf
    if spec == (-2, 3, 3):
        assert fh[:, 1].sum() > 0 and fh[:, -1].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_symbol_list():
    from freud_amd import engine
    text = open(os.path.join(ROOT, "include", "freud_sae.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+sae_hist_files\s*\(", text)
    assert "sae_hist_files" in engine.EXPORTED_SYMBOLS
    engine.build()
    assert hasattr(engine.load(), "sae_hist_files")
    m = re.search(r"#define\s+SAE_HIST_MAX_SEL\s+(\d+)", text)
    assert m and int(m.group(1)) == engine.HIST_MAX_SEL == 64


@pytest.fixture()
def shard_dir(tmp_path):
    from freud_amd.loader import write_shards
    F, T, d = 3, 4, 8
    write_shards(str(tmp_path), "enc", np.zeros((F, T * d), np.float32), [T, d])
    return str(tmp_path), F, T


def test_argument_rules_need_no_device(shard_dir, monkeypatch):
    import torch
    from freud_amd import file_pass
    from freud_amd.activation_hist import activation_histograms as ah

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the argument checks")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(file_pass, "resolve_sae", no_device)
    path, F, T = shard_dir
    fl = np.zeros(F, np.int64)
    with pytest.raises(ValueError, match="bins per octave"):
        ah("ckpt", path, "enc", octaves=33, sub_bits=2)                                # O P = 132 > 128
    with pytest.raises(ValueError, match="sub_bits"):
        ah("ckpt", path, "enc", sub_bits=4)
    with pytest.raises(ValueError, match="lo_exp"):
        ah("ckpt", path, "enc", lo_exp=-127)
    with pytest.raises(ValueError, match="65 label_latents"):
        ah("ckpt", path, "enc", label_latents=list(range(65)), file_labels=fl)
    with pytest.raises(ValueError, match="need label_latents"):
        ah("ckpt", path, "enc", file_labels=fl)                                        # labels without label_latents
    with pytest.raises(ValueError, match="need file_labels or frame_labels"):
        ah("ckpt", path, "enc", label_latents=[1])                                     # label_latents without labels
    with pytest.raises(ValueError, match="< 0"):
        ah("ckpt", path, "enc", label_latents=[-1], file_labels=fl)
    with pytest.raises(ValueError, match="need an SAE"):
        ah(None, path, "enc")
    # the rules of feature_labels, reached through this entry
    with pytest.raises(ValueError, match="exactly one"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=fl, frame_labels=np.zeros((F, T), np.int64))
    with pytest.raises(ValueError, match="must be integers"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=np.zeros(F, np.float32))
    with pytest.raises(ValueError, match="n_files=3"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=np.zeros(F + 1, np.int64))
    with pytest.raises(ValueError, match="n_classes=2"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=np.array([0, 2, 1]), n_classes=2)
    with pytest.raises(ValueError, match="duplicate label ids"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=np.array([[0, 0], [1, 2], [1, -1]]))
    with pytest.raises(ValueError, match="class_names"):
        ah("ckpt", path, "enc", label_latents=[1], file_labels=fl, class_names=["a", "b"])
    with pytest.raises(ValueError, match="batch_files"):
        ah("ckpt", path, "enc", batch_files=0)


# ---------------------------------------------------------------------------------------------------------------------------
def hand_made(spec, seed=3, n=6, n_files=40, T=30):
    """Values per (file, frame, latent) drawn on bf16, and the histograms numpy builds from them."""
    from freud_amd.activation_hist import ActivationHistograms
    g = np.random.default_rng(seed)
    v = np.where(g.random((n_files, T, n)) < 0.5, 0.0, np.exp(g.normal(0, 2.5, (n_files, T, n)))).astype(np.float32)
    v[:, :, 0] = 0.0                                                     # a dead latent
    v[:, :, 1] = np.where(v[:, :, 1] > 0, 1.0, 0.0)                      # a latent that is off or exactly 1
    bits = bf16_bits(v)
    vals = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    nb = (spec[1] << spec[2]) + 3
    fh, mh = np.zeros((n, nb), np.int64), np.zeros((n, nb), np.int64)
    for j in range(n):
        fh[j] = np.bincount(np_bins(bits[:, :, j].ravel(), spec), minlength=nb)
        mh[j] = np.bincount(np_bins(bits[:, :, j].max(1), spec), minlength=nb)
    return ActivationHistograms(n_files * T, n_files, spec, fh, mh), vals


@pytest.mark.parametrize("spec", [(-12, 24, 2), (-2, 3, 1)])
def test_quantile_brackets_hold_the_order_statistic(spec):
    ah, vals = hand_made(spec)
    n = vals.shape[2]
    for which, series in (("frame", vals.reshape(-1, n)), ("file", vals.max(1))):
        for active_only in (True, False):
            for q in (0.0, 0.1, 0.5, 0.9, 0.99, 1.0):
                lo, hi = ah.quantile(q, which=which, active_only=active_only)
                for j in range(n):
                    s = np.sort(series[:, j][series[:, j] > 0] if active_only else series[:, j])
                    if s.size == 0:
                        assert np.isnan(lo[j]) and np.isnan(hi[j])
                        continue
                    stat = s[max(1, int(np.ceil(q * s.size))) - 1]
                    assert stat == np.quantile(s, q, method="inverted_cdf")
                    if stat == 0:
                        assert lo[j] == hi[j] == 0
                    else:
                        assert lo[j] <= stat < hi[j] and (lo[j] > 0 or stat < ah.edges()[0]), (which, q, j)
    lo, hi = ah.quantile(0.5)
    assert np.isnan(lo[0]) and np.isnan(hi[0])                           # the dead latent: nothing to rank
    assert lo[1] == 1.0 and hi[1] == 1.25 if spec[2] == 2 else lo[1] == 1.0
    with pytest.raises(ValueError):
        ah.quantile(1.5)
    with pytest.raises(ValueError):
        ah.quantile(0.5, which="rows")


@pytest.mark.parametrize("spec", [(-12, 24, 2), (-2, 3, 1)])
def test_files_in_range_exact_on_boundaries_and_a_bracket_otherwise(spec):
    from freud_amd.activation_hist import _prev_bf16
    ah, vals = hand_made(spec)
    mx = vals.max(1)                                                     # [n_files, n]
    e = ah.edges()
    below = _prev_bf16(e.astype(np.float32))
    for i1, i2 in ((0, len(e) - 1), (1, 2), (2, len(e) // 2), (len(e) // 2, len(e) - 1)):
        lo, hi = ah.files_in_range(e[i1], below[i2])
        want = ((mx >= e[i1]) & (mx <= below[i2])).sum(0)
        np.testing.assert_array_equal(lo, want)
        np.testing.assert_array_equal(hi, want)
        np.testing.assert_array_equal(lo, ah.file_max_hist[:, 2 + i1:2 + i2].sum(1))
    lo, hi = ah.files_in_range(0.0, None)                                # every file
    assert (lo == ah.n_files).all() and (hi == ah.n_files).all()
    lo, hi = ah.files_in_range(e[2], None)
    np.testing.assert_array_equal(lo, (mx >= e[2]).sum(0))
    np.testing.assert_array_equal(hi, lo)
    strict = False
    for mn, mxv in ((0.3, 2.9), (1e-3, 0.7), (0.26, 0.27), (5.1, 1e9), (e[3], e[5])):
        lo, hi = ah.files_in_range(mn, mxv)
        want = ((mx >= mn) & (mx <= mxv)).sum(0)
        assert (lo <= want).all() and (want <= hi).all()
        strict = strict or (lo < hi).any()
    assert strict


def test_npz_round_trip_is_bitwise(tmp_path):
    from freud_amd.activation_hist import ActivationHistograms
    ah, _ = hand_made((-12, 24, 2))
    g = np.random.default_rng(0)
    full = ActivationHistograms(ah.n_frames, ah.n_files, ah.spec, ah.frame_hist, ah.file_max_hist,
                                g.integers(0, 50, (2, 4, ah.n_bins)).astype(np.int64), np.array([3, 1], np.int64),
                                g.integers(0, 50, 4).astype(np.int64), ["a", "b", "c"])
    for i, obj in enumerate((ah, full)):
        p = str(tmp_path / f"h{i}.npz")
        obj.to_npz(p)
        back = ActivationHistograms.from_npz(p)
        assert (back.n_frames, back.n_files, back.spec, back.class_names) == (obj.n_frames, obj.n_files, obj.spec, obj.class_names)
        for k in ("frame_hist", "file_max_hist", "label_hist", "label_latents", "label_count"):
            a, b = getattr(obj, k), getattr(back, k)
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()), k
    np.testing.assert_array_equal(full.label_distribution(1, "b"), full.label_hist[1, 1])
    np.testing.assert_array_equal(full.label_distribution(3, None), full.label_hist[0, 3])
    with pytest.raises(KeyError):
        full.label_distribution(2, 0)
    assert json_ok(full.summary()) and json_ok(ah.summary())


def json_ok(d):
    import json
    return isinstance(json.loads(json.dumps(d)), dict)
