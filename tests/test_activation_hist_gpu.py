"""GPU: the activation histograms (freud_amd/activation_hist.py over include/freud_sae.h's sae_hist_files).

* L1 and TopK against the engine's own encode() latents of every file, viewed as bf16 bit patterns and binned here in numpy BY
  VALUE (searchsorted over the closed-form edges): frame_hist and file_max_hist equal to the integer; trimmed lengths, a last
  partial batch, padded columns, 17 column blocks, a spec whose underflow and overflow bins fill, one with 128 regular bins;
* the invariants against the feature statistics, the files a min_val / max_val band keeps against the feature search;
* the label-conditional table against a numpy count and against feature_labels; per-file labels = the same labels per frame;
* the reference's own per-file maxima (tests/golden/search_{l1,topk}.npz) sandwiched at every edge;
* determinism, the batch size, the context afterwards, the CLI, and the 16-bit LDS counters over more rows than they can hold.

L1 weights: every column has 256 entries of +-1/16, so its norm is exactly 1 and the in-place renormalisation every L1 forward
starts with is a bit-exact fixed point: every forward sees the same weights."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import activation_hist as AH
from freud_amd import engine as E
from freud_amd import feature_labels as FL
from freud_amd import feature_search as FS
from freud_amd import feature_stats as FST
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEFAULT = (-12, 24, 2)
NARROW = (-2, 3, 3)            # [0.25, 2): N(0, 1)-sized latents fill the underflow and the overflow bin
FINE = (-8, 16, 3)             # 128 regular bins: the 128-column workgroups of the L1 kernel


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    return W, g.normal(0, 0.3, n).astype(np.float32)


def l1_model(d, n, seed, bias=None):
    W, b = l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b if bias is None else bias)})
    return sae


def topk_model(d, n, k, seed, bias=None):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k), max_rows=1500)
    if bias is not None:
        sd = sae.state_dict()
        sd["encoder.bias"] = torch.full((n,), float(bias))
        sae.load_state_dict(sd)
    return sae


def shards(path, x, dtype=np.float32, filenames=None):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(dtype), [T, d], filenames=filenames)
    return str(path)


def latent_bits(sae, x, lengths):
    """encode() of every file (TopK: the scatter of the selection) as bf16 bit patterns: a list of uint16 [L[f], n]."""
    out = []
    for f in range(x.shape[0]):
        xf = torch.from_numpy(x[f]).cuda()
        if isinstance(sae, L1AutoEncoder):
            lat = sae.encode(xf).latent.float()
        else:
            enc = sae.encode(xf)
            lat = torch.zeros(xf.shape[0], sae.n_dict_components, device="cuda")
            lat.scatter_(1, enc.top_indices, enc.top_acts.float())
        b16 = lat.to(torch.bfloat16)
        assert torch.equal(b16.float(), lat)                 # the latent IS bf16: nothing rounds here
        out.append(b16.view(torch.int16).cpu().numpy().view(np.uint16)[: int(lengths[f])].copy())
    return out


def edges_of(spec):
    L, O, s = spec
    P = 1 << s
    i = np.arange(O * P + 1)
    return np.ldexp(1.0 + (i % P) / P, L + i // P)


def np_bins(bits, spec):
    mag = np.asarray(bits, np.uint32) & 0x7FFF
    val = (mag << 16).astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(mag == 0, 0, 1 + np.searchsorted(edges_of(spec), val, side="right")).astype(np.int64)


def ref_hists(bits, spec):
    n = bits[0].shape[1]
    nb = (spec[1] << spec[2]) + 3
    fh, mh = np.zeros(n * nb, np.int64), np.zeros(n * nb, np.int64)
    cols = np.arange(n) * nb
    for lat in bits:
        fh += np.bincount((np_bins(lat, spec) + cols).ravel(), minlength=n * nb)
        mh += np.bincount(np_bins((lat & 0x7FFF).max(0), spec) + cols, minlength=n * nb)
    return fh.reshape(n, nb), mh.reshape(n, nb)


def check_invariants(ah, st):
    """st: feature_stats of the same pass."""
    assert (ah.frame_hist.sum(1) == ah.n_frames).all()
    assert (ah.file_max_hist.sum(1) == ah.n_files).all()
    np.testing.assert_array_equal(ah.frame_hist[:, 1:].sum(1), st.fire_count)
    nb = ah.n_bins
    top_f = np.where(ah.frame_hist > 0, np.arange(nb), -1).max(1)
    top_m = np.where(ah.file_max_hist > 0, np.arange(nb), -1).max(1)
    np.testing.assert_array_equal(top_f, top_m)
    lo, hi = ah.bin_bounds()
    mx = st.act_max.astype(np.float64)
    assert ((mx == 0) == (top_f == 0)).all()
    live = top_f > 0
    assert (lo[top_f[live]] <= mx[live]).all() and (mx[live] < hi[top_f[live]]).all()
    assert (mx[live] > 0).all()


def check_search_band(ah, sae, path, lengths, batch, i1, i2):
    """The feature search (independent kernels) with the band [edge i1, the largest bf16 below edge i2] keeps, per latent, exactly
    the files of bins 2 + i1 .. 2 + i2 - 1 of file_max_hist."""
    e = ah.edges()
    below = float(AH._prev_bf16(np.float32(e[i2])))
    assert below < e[i2] and np.float32(below) == below
    atlas = FS.search_features(sae, path, "enc", ah.n_files, min_val=float(e[i1]), max_val=below, lengths=lengths, batch_files=batch)
    kept = (atlas.file_idx >= 0).sum(1)
    want = ah.file_max_hist[:, 2 + i1:2 + i2].sum(1)
    assert 0 < want.sum() < ah.n_files * ah.n_latents
    np.testing.assert_array_equal(kept, want)
    lo, hi = ah.files_in_range(float(e[i1]), below)
    np.testing.assert_array_equal(lo, want)
    np.testing.assert_array_equal(hi, want)


def same(a, b):
    assert (a.n_frames, a.n_files, a.spec) == (b.n_frames, b.n_files, b.spec)
    for k in ("frame_hist", "file_max_hist", "label_hist", "label_latents", "label_count"):
        u, v = getattr(a, k), getattr(b, k)
        assert (u is None and v is None) or (u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()), k


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F,batch,n", [(50, 9, 4, 1000), (50, 9, 4, 4352), (1500, 3, 2, 1024), (8, 300, 128, 4352)])
def test_l1_exact_against_encode(tmp_path, T, F, batch, n):
    """n = 1000: padded columns; n = 4352: 17 column blocks; batches of 4 + 4 + 1 and 2 + 1 files: a last partial batch.  128 files
    at 17 column blocks: the launcher forms chunks of two files (passes.hip, hist_launch_l1), the last batch of 44 chunks of one."""
    d = 256
    g = np.random.default_rng(T + n)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(2, T + 1, F)
    L[0], L[1] = T, 1
    sae = l1_model(d, n, seed=F)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    st = FST.feature_stats(sae, path, "enc", lengths=L, batch_files=batch)
    for spec in (DEFAULT, NARROW) + ((FINE,) if n == 1000 else ()):
        want_f, want_m = ref_hists(bits, spec)
        if spec == NARROW:
            assert want_f[:, 1].sum() > 0 and want_f[:, -1].sum() > 0 and want_m[:, 1].sum() > 0 and want_m[:, -1].sum() > 0
        got = AH.activation_histograms(sae, path, "enc", lo_exp=spec[0], octaves=spec[1], sub_bits=spec[2], lengths=L, batch_files=batch)
        assert got.n_frames == int(L.sum()) and got.n_files == F and got.frame_hist.shape == (n, (spec[1] << spec[2]) + 3)
        np.testing.assert_array_equal(got.frame_hist, want_f, err_msg=str(spec))
        np.testing.assert_array_equal(got.file_max_hist, want_m, err_msg=str(spec))
        check_invariants(got, st)
    if n == 1000:
        check_search_band(got if spec == DEFAULT else AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=batch),
                          sae, path, L, batch, 44, 52)                      # [0.5, 2)
        full = AH.activation_histograms(sae, path, "enc", batch_files=batch)            # without lengths: all T frames
        want_f, want_m = ref_hists(latent_bits(sae, x, np.full(F, T)), DEFAULT)
        np.testing.assert_array_equal(full.frame_hist, want_f)
        np.testing.assert_array_equal(full.file_max_hist, want_m)


def test_topk_exact_against_encode(tmp_path):
    d, n, k, T, F, batch = 256, 1024, 8, 50, 9, 4
    g = np.random.default_rng(5)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    x *= np.array([1, 1, 0.02, 0.1, 4, 30, 1, 1, 1], np.float32)[:, None, None]      # quiet and loud files: the selected values span the bins
    L = g.integers(2, T + 1, F)
    L[0], L[1] = T, 1
    sae = topk_model(d, n, k, seed=2)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    st = FST.feature_stats(sae, path, "enc", lengths=L, batch_files=batch)
    default = None
    for spec in (DEFAULT, NARROW):
        want_f, want_m = ref_hists(bits, spec)
        if spec == NARROW:
            assert want_f[:, 1].sum() > 0 and want_f[:, -1].sum() > 0
        got = AH.activation_histograms(sae, path, "enc", lo_exp=spec[0], octaves=spec[1], sub_bits=spec[2], lengths=L, batch_files=batch)
        np.testing.assert_array_equal(got.frame_hist, want_f, err_msg=str(spec))
        np.testing.assert_array_equal(got.file_max_hist, want_m, err_msg=str(spec))
        assert got.frame_hist[:, 1:].sum() == st.fire_count.sum() <= int(L.sum()) * k
        check_invariants(got, st)
        default = default or got
    e = default.edges()
    mid = int(np.searchsorted(e, np.median(st.act_max[st.act_max > 0])))
    check_search_band(default, sae, path, L, batch, mid - 4, mid + 2)


def test_topk_selected_zeros_are_inactive(tmp_path):
    """All-negative inputs against non-negative encoder rows and a negative bias: no pre-activation is positive, every selected
    value is a zero and lands in bin 0; with mixed inputs some rows select fewer than k positive values."""
    d, n, k, T, F = 256, 1024, 8, 50, 5
    sae = topk_model(d, n, k, seed=4, bias=-1.5)
    g = np.random.default_rng(6)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    sd = sae.state_dict()
    sd["encoder.weight"] = sd["encoder.weight"].abs()
    sae.load_state_dict(sd)
    x[0] = -np.abs(x[0])                                                    # file 0: nothing fires
    L = np.array([T, 7, T, 20, 1])
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    assert not bits[0].any() and any(b.any() for b in bits[1:])
    want_f, want_m = ref_hists(bits, DEFAULT)
    got = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=2)
    np.testing.assert_array_equal(got.frame_hist, want_f)
    np.testing.assert_array_equal(got.file_max_hist, want_m)
    assert (got.file_max_hist[:, 0] >= 1).all()
    check_invariants(got, FST.feature_stats(sae, path, "enc", lengths=L, batch_files=2))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_label_conditional(tmp_path, variant):
    d, n, T, F, S, Cn = 256, 1024, 50, 7, 2, 5
    g = np.random.default_rng(11)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    L = g.integers(2, T + 1, F)
    L[0] = T
    sae = l1_model(d, n, seed=8) if variant == "l1" else topk_model(d, n, 8, seed=8)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    fire = sum((b != 0).sum(0) for b in bits)
    sel = [int(np.argmax(fire)), 3, int(np.argsort(fire)[n // 2])]           # a busy latent, a fixed one, a middling one
    # two slots of distinct ids in {0, 1, 2, 4} (class 3 never occurs), about a third of the slots empty
    lab = np.full((F, T, S), -1, np.int64)
    first = g.choice([0, 1, 2, 4], (F, T))
    second = (first + g.integers(1, 4, (F, T))) % 5
    second = np.where(second == 3, -1, second)
    lab[:, :, 0] = np.where(g.random((F, T)) < 0.3, -1, first)
    lab[:, :, 1] = np.where((g.random((F, T)) < 0.4) | (second == lab[:, :, 0]), -1, second)
    assert (lab == -1).all(2).any() and not (lab == 3).any()
    got = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=3, label_latents=sel, frame_labels=lab, n_classes=Cn,
                                   class_names=list("abcde"))
    nb = got.n_bins
    want = np.zeros((len(sel), Cn + 1, nb), np.int64)
    want_count = np.zeros(Cn + 1, np.int64)
    for f in range(F):
        b = np_bins(bits[f][:, sel], DEFAULT)                                # [L, n_sel]
        for r in range(int(L[f])):
            ids = [int(v) for v in lab[f, r] if v >= 0] + [Cn]
            for l in ids:
                want_count[l] += 1
                for s in range(len(sel)):
                    want[s, l, b[r, s]] += 1
    np.testing.assert_array_equal(got.label_hist, want)
    np.testing.assert_array_equal(got.label_count, want_count)
    assert got.label_count[3] == 0 and got.label_count[Cn] == got.n_frames == int(L.sum())
    for s, j in enumerate(sel):
        np.testing.assert_array_equal(got.label_hist[s, Cn], got.frame_hist[j])
        np.testing.assert_array_equal(got.label_hist[s].sum(1), got.label_count)
        np.testing.assert_array_equal(got.label_distribution(j, "e"), want[s, 4])
    assert want[0, :Cn, 1:].sum() > 0 and want[:, :Cn, 0].sum() > 0
    fl = FL.feature_labels(sae, path, "enc", frame_labels=lab, n_classes=Cn, lengths=L, batch_files=3)
    np.testing.assert_array_equal(got.label_count[:Cn], fl.label_count)
    np.testing.assert_array_equal(got.label_hist[:, Cn, 1:].sum(1), fl.fire_count[sel])
    # the unconditional arrays do not depend on the label part
    same_plain = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=3)
    assert same_plain.frame_hist.tobytes() == got.frame_hist.tobytes() and same_plain.file_max_hist.tobytes() == got.file_max_hist.tobytes()
    # per-file labels are the same labels on every frame of the file
    per_file = np.array([[0, 4], [1, -1], [-1, -1], [2, 0], [4, 1], [0, -1], [2, 4]])
    a = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=3, label_latents=sel, file_labels=per_file, n_classes=Cn)
    b = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=3, label_latents=sel,
                                 frame_labels=np.repeat(per_file[:, None, :], T, 1), n_classes=Cn)
    same(a, b)
    assert a.label_count[0] == L[0] + L[3] + L[5]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_reference_per_file_maxima_are_sandwiched(tmp_path, kind):
    """The reference's own fp32 per-file maxima of every latent (search_{kind}.npz, the cases n_top = 1, not absolute, no filter)
    against file_max_hist at every edge E of the default spec: the files the engine puts at or above E number at least the stable
    files the reference has at or above E + tol(E) and at most those at or above E - tol(E) plus the flip files, tol(v) = 0.03 +
    0.01 |v| (the tolerance of test_feature_search_gpu.py for these goldens).  At least 2000 (latent, edge) pairs must pin the
    count: both bounds equal and strictly between 0 and the stable files (from the goldens alone: 2373 for l1, 2240 for topk, of
    12 416)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"search_{kind}.npz"))
    x, L, flip = g["x"], g["lengths"], g["flip"]
    d = x.shape[2]
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w_")}
    if kind == "l1":
        n = w["decoder.weight"].shape[1]
        sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n))
    else:
        n = w["W_dec"].shape[0]
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=int(g["k"])))
    sae.load_state_dict(w)
    path = shards(tmp_path, x, filenames=[str(f) for f in g["filenames"]])
    ah = AH.activation_histograms(sae, path, "enc", lengths=L, batch_files=4)
    assert ah.n_files == x.shape[0] and ah.n_frames == int(np.minimum(L, x.shape[1]).sum())
    e = ah.edges()                                                          # the lower edges of the regular and the overflow bins
    at_or_above = ah.file_max_hist[:, ::-1].cumsum(1)[:, ::-1]              # [n, NB]: files in bins >= b
    tol = lambda v: 0.03 + 0.01 * np.abs(v)
    seen, pinned, pairs = set(), 0, 0
    for c in range(len(g["case_feature"])):
        if g["case_n_top"][c] != 1 or g["case_absolute"][c] or not np.isnan(g["case_min_val"][c]) or not np.isnan(g["case_max_val"][c]):
            continue
        j = int(g["case_feature"][c])
        seen.add(j)
        P = g["case_max_per_file"][c].astype(np.float64)
        stable = ~flip[:, j]
        for i, E in enumerate(e):
            lo = int((stable & (P >= E + tol(E))).sum())
            hi = int((stable & (P >= E - tol(E))).sum()) + int(flip[:, j].sum())
            got = int(at_or_above[j, 2 + i])
            assert lo <= got <= hi, (kind, j, float(E), lo, got, hi)
            pairs += 1
            pinned += lo == hi and 0 < lo < int(stable.sum())
    assert seen == set(range(n)) and pairs == n * 97
    assert pinned >= 2000, pinned


# ---------------------------------------------------------------------------------------------------------------------------
def test_deterministic_whatever_the_batch_and_cli(tmp_path):
    d, n, T, F = 256, 1024, 50, 11
    sae = l1_model(d, n, seed=3)
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": d,
                            "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    g = np.random.default_rng(4)
    x = g.normal(0, 1, (F, T, d)).astype(np.float32)
    path = shards(tmp_path / "data", x)
    L = g.integers(1, T + 1, F)
    lab = g.integers(-1, 3, F)
    lab[0] = 2
    np.save(tmp_path / "len.npy", L)
    np.save(tmp_path / "lab.npy", lab)
    with open(tmp_path / "names.json", "w") as f:
        json.dump(["x", "y", "z"], f)
    kw = dict(lengths=L, label_latents=[1, 5, 9], file_labels=lab, n_classes=3, class_names=["x", "y", "z"])
    rng = torch.get_rng_state()
    a = AH.activation_histograms(str(ck), path, "enc", batch_files=5, **kw)
    assert torch.equal(torch.get_rng_state(), rng)
    same(a, AH.activation_histograms(str(ck), path, "enc", batch_files=5, **kw))
    for batch in (1, 4, F):
        same(a, AH.activation_histograms(sae, path, "enc", batch_files=batch, **kw))
    topk = topk_model(d, n, 8, seed=1)
    t = AH.activation_histograms(topk, path, "enc", batch_files=5, **kw)
    for batch in (3, F):
        same(t, AH.activation_histograms(topk, path, "enc", batch_files=batch, **kw))
    out = tmp_path / "hist.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.activation_hist", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--lengths", str(tmp_path / "len.npy"), "--batch_files", "5", "--label_latents", "1,5,9", "--file_labels",
                        str(tmp_path / "lab.npy"), "--class_names", str(tmp_path / "names.json"), "--out", str(out)],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    same(AH.ActivationHistograms.from_npz(str(out)), a)
    assert summary["n_frames"] == a.n_frames == int(L.sum()) and summary["n_files"] == F and summary["n_bins"] == 99
    assert summary["dead"] == int((a.frame_hist[:, 1:].sum(1) == 0).sum()) and summary["label_latents"] == [1, 5, 9]


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_histograms(variant):
    d, n, T, F = 256, 1024, 50, 4
    nb = E.hist_nbins(DEFAULT)

    def make():
        if variant == "l1":
            W, b = l1_weights(d, n, seed=1)
            eng = E.SaeEngine("l1", d, n, 1500, recon_alpha=1e2)
            eng.set_params({"decoder.weight": W, "encoder_bias": b})
        else:
            eng = E.SaeEngine("topk", d, n, 1500, k=16, optimizer="adam")
            We = torch.randn(n, d, generator=torch.Generator().manual_seed(1)) / 16
            eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32),
                            "W_dec": We.numpy().copy(), "b_dec": np.zeros(d, np.float32)})
        return eng

    a, b = make(), make()
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(2)).cuda()
    for eng in (a, b):
        eng.eval(x.reshape(F * T, d))
    before = a.get_params()
    step, m1, m2 = a.get_opt_state()
    fh = torch.zeros(n, nb, dtype=torch.int64, device="cuda")
    mh, nf = torch.zeros_like(fh), torch.zeros(1, dtype=torch.int64, device="cuda")
    a.hist_files(x, DEFAULT, fh, mh, nf)
    torch.cuda.synchronize()
    assert int(nf.item()) == F * T and bool((fh.sum(1) == F * T).all()) and bool((mh.sum(1) == F).all())
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="histogram"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="histogram"):
            a.topk_indices_tensor(F * T, "cuda")
    for k, v in a.get_params().items():
        assert v.tobytes() == before[k].tobytes(), k
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(np.array_equal(n1[k], m1[k]) and np.array_equal(n2[k], m2[k]) for k in m1)
    # a following training step is bitwise the same step as in a context that never ran the histograms
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert a.metrics().tobytes() == b.metrics().tobytes()

    # refused before anything is enqueued: the arrays keep their sentinel
    s_f, s_m, s_n = torch.full_like(fh, 7), torch.full_like(mh, 7), torch.full_like(nf, 7)
    with pytest.raises(E.EngineError, match="max_rows"):
        a.hist_files(torch.randn(40, 50, d).cuda(), DEFAULT, s_f, s_m, s_n)
    lib, vp = a._lib, C.c_void_p
    lab = torch.zeros(F, T, 1, dtype=torch.int32, device="cuda")
    sel = torch.zeros(65, dtype=torch.int32, device="cuda")
    lh, lc = torch.full((65 * 3 * nb,), 7, dtype=torch.int64, device="cuda"), torch.full((3,), 7, dtype=torch.int64, device="cuda")

    def raw(spec=DEFAULT, flags=0, labels=None, n_slots=0, n_classes=0, sel_p=None, n_sel=0, lh_p=None, lc_p=None):
        return lib.sae_hist_files(a._ctx, vp(x.data_ptr()), F, T, E.DTYPE["float32"], None, spec[0], spec[1], spec[2], flags,
                                  vp(s_f.data_ptr()), vp(s_m.data_ptr()), vp(s_n.data_ptr()), labels, n_slots, n_classes, sel_p, n_sel,
                                  lh_p, lc_p, vp(torch.cuda.current_stream().cuda_stream))

    lp, sp, hp, cp = vp(lab.data_ptr()), vp(sel.data_ptr()), vp(lh.data_ptr()), vp(lc.data_ptr())
    assert raw(spec=(-12, 33, 2)) != 0 and raw(spec=(-12, 24, 4)) != 0 and raw(spec=(-127, 8, 0)) != 0 and raw(spec=(120, 9, 0)) != 0
    assert raw(flags=1) != 0
    assert raw(labels=lp, n_slots=1, n_classes=2, sel_p=sp, n_sel=65, lh_p=hp, lc_p=cp) != 0
    assert raw(n_sel=-1) != 0
    assert raw(labels=None, n_slots=1, n_classes=2, sel_p=sp, n_sel=2, lh_p=hp, lc_p=cp) != 0
    assert raw(labels=lp, n_slots=1, n_classes=2, sel_p=sp, n_sel=2, lh_p=None, lc_p=cp) != 0
    assert raw(labels=lp, n_slots=17, n_classes=2, sel_p=sp, n_sel=2, lh_p=hp, lc_p=cp) != 0
    assert raw(labels=lp, n_slots=1, n_classes=4097, sel_p=sp, n_sel=2, lh_p=hp, lc_p=cp) != 0
    torch.cuda.synchronize()
    for t in (s_f, s_m, s_n, lh, lc):
        assert bool((t == 7).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    nb = E.hist_nbins(DEFAULT)
    fh = torch.full((1024, nb), 7, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.hist_files(torch.randn(2, 100, 256).cuda(), DEFAULT, fh, torch.zeros_like(fh), torch.zeros(1, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert bool((fh == 7).all())
    eng.close()


def test_narrow_lds_counters_do_not_wrap(tmp_path):
    """The L1 kernel counts in 16-bit LDS counters.  Its bound (hist.h, HIST_FLUSH_ROWS): a thread flushes its counters before the
    rows since its last flush would exceed 65 535, so a column that stays in one bin brings a counter to 65 535 and no further.  A
    chunk is whole files (passes.hip, hist_launch_l1: at n = 256 one column block, so one file per chunk up to 1024 files), hence
    the largest chunk at d = 256, n = 256 is one file as long as the context allows: here 65 536 + 64 rows, more than a 16-bit
    counter holds, with zero input and a bias of 1.5 -- every latent is 1.5 on every frame.  Counters that wrapped would lose
    65 536 frames per column."""
    d, n, T = 256, 256, 65536 + 64
    W, _ = l1_weights(d, n, seed=9)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.full((n,), 1.5)})
    path = shards(tmp_path, np.zeros((1, T, d), np.float16), dtype=np.float16)
    got = AH.activation_histograms(sae, path, "enc", batch_files=1)
    b = int(np_bins(np.array([0x3FC0]), DEFAULT)[0])                        # 1.5
    want = np.zeros((n, got.n_bins), np.int64)
    want[:, b] = T
    np.testing.assert_array_equal(got.frame_hist, want)
    want[:, b] = 1
    np.testing.assert_array_equal(got.file_max_hist, want)
