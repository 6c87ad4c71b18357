"""GPU: the feature timing (freud_amd/feature_timing.py over include/freud_sae.h's sae_timing_files).

Every array is compared, to the integer, with tests/feature_timing_reference.py (np.diff of the padded mask) fed the engine's own
encode() of every file, viewed as bf16 bit patterns.  Inputs are x[f, t] = sum_i s_i[f, t] u_i + noise with the s_i slow random
walks over t: the per-column bias turns one signal into many thresholds and runs of all lengths occur.  Each test first asserts ON
THE REFERENCE ALONE that its cases occur (a run of one frame, a run in an octave bin, a run as long as its file's counted frames,
censored runs beside uncensored ones, gaps, and for a bridge g > 0 raw gaps <= g, so that bridging changes the answer); the seeds
were picked on the CPU with the reference.

L1 weights: every column has 256 entries of +-1/16, so its norm is exactly 1 and the in-place renormalisation every L1 forward starts
with is a bit-exact fixed point: every forward sees the same weights.  TopK weights come from numpy, not from torch's RNG."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from freud_amd import collect_features as CF
from freud_amd import engine as E
from freud_amd import feature_index as FI
from freud_amd import feature_stats as FST
from freud_amd import feature_timing as FT
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.loader import write_shards
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder
from tests import feature_timing_reference as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEGMENT = 8192                 # freud_amd/csrc/timing.h: TM_SEG, the latents of one LDS table of the TopK kernel


# ---- inputs and models (no device needed: the seeds were chosen with these on the CPU) --------------------------------------
def walk_inputs(seed, F, T, d, n_dirs=1, step=1.2, noise=0.02, period2_file=None, amp=8.0):
    """x [F, T, d] float32: n_dirs slow random walks along +-1/sqrt(d) directions plus white noise; file `period2_file` alternates the
    sign of its (single) signal from frame to frame instead."""
    g = np.random.default_rng(seed)
    u = np.where(g.random((n_dirs, d)) < 0.5, -1.0, 1.0) / np.sqrt(d)
    s = np.cumsum(g.normal(0, step, (n_dirs, F, T)), axis=2) + g.normal(0, 2 * step, (n_dirs, F, 1))
    if period2_file is not None:
        s[:, period2_file, :] = 0.0
        s[0, period2_file, :] = amp * (-1.0) ** np.arange(T)
    x = np.einsum("ift,id->ftd", s, u) + g.normal(0, noise, (F, T, d))
    return x.astype(np.float32)


def l1_weights(d, n, seed):
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    return W, g.normal(0, 0.3, n).astype(np.float32)


def l1_case_weights(d, n, seed):
    W, b = l1_weights(d, n, seed)
    b[0], b[1] = 40.0, -40.0                       # column 0 is always on, column 1 never
    return W, b


def l1_model(d, n, W, b, max_rows=1500):
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=max_rows)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_weights(d, n, seed, bias=0.0, forced=()):
    g = np.random.default_rng(seed)
    We = g.uniform(-1, 1, (n, d)).astype(np.float32) / np.sqrt(d).astype(np.float32)
    be = np.full(n, bias, np.float32)
    for j in forced:
        be[j] = 30.0                               # selected on every frame
    Wd = We / np.linalg.norm(We, axis=1, keepdims=True)
    return {"encoder.weight": We, "encoder.bias": be, "W_dec": Wd.astype(np.float32), "b_dec": np.zeros(d, np.float32)}


def topk_model(d, n, k, w, multi=False):
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi), max_rows=1500)
    sae.load_state_dict({key: torch.from_numpy(v) for key, v in w.items()})
    return sae


def shards(path, x, dtype=np.float32):
    F, T, d = x.shape
    write_shards(str(path), "enc", x.reshape(F, T * d).astype(dtype), [T, d])
    return str(path)


def latent_bits(sae, x, lengths):
    """encode() of every file (TopK: the scatter of the selection) as bf16 bit patterns: a list of uint16 [L[f], n]."""
    out = []
    for f in range(x.shape[0]):
        xf = torch.from_numpy(np.ascontiguousarray(x[f])).cuda()
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


def masks_of(bits, thr_bits=0):
    return [(b & 0x7FFF) > thr_bits for b in bits]


def cases_occur(want, seen, g):
    """On the reference alone: the cases the comparison below is about are there."""
    _, gap_hist, tot = want
    assert seen["dur1"] > 0, "no run of a single frame"
    assert seen["octave"] > 0, "no run in an octave bin"
    assert seen["whole_file"] > 0, "no run as long as its file's counted frames"
    assert 0 < tot[:, REF.CENSORED].sum() < tot[:, REF.RUNS].sum()
    assert gap_hist.sum() > 0 and seen["gaps"] == gap_hist.sum()
    if g > 0:
        assert seen["raw_gaps_le_g"] > 0, "bridging changes nothing"


def compare(got, want, frames, F, T, spec):
    run_hist, gap_hist, tot = want
    assert (got.n_frames, got.n_files, got.T, got.spec) == (frames, F, T, spec)
    np.testing.assert_array_equal(got.run_hist, run_hist, err_msg=str(spec))
    np.testing.assert_array_equal(got.gap_hist, gap_hist, err_msg=str(spec))
    np.testing.assert_array_equal(got.totals, tot, err_msg=str(spec))
    got.check()


def same(a, b):
    assert (a.n_frames, a.n_files, a.T, a.spec) == (b.n_frames, b.n_files, b.T, b.spec)
    for k in ("run_hist", "gap_hist", "totals"):
        u, v = getattr(a, k), getattr(b, k)
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), k


L1_SEED, L1_D, L1_N, L1_F, L1_T = 1, 256, 300, 5, 70
L1_LENGTHS = np.array([L1_T, 1, 37, L1_T, 50])


def l1_case():
    x = walk_inputs(L1_SEED, L1_F, L1_T, L1_D, period2_file=3)
    W, b = l1_case_weights(L1_D, L1_N, L1_SEED)
    return x, W, b


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l1_setup(tmp_path_factory):
    """The 5-file L1 case: n = 300 (padded columns, two column blocks), lengths with 1 and T, batches of 2 + 2 + 1 files; file 3
    alternates the sign of its signal (period 2), column 0 is always on and column 1 never.  The bit patterns of encode() once."""
    x, W, b = l1_case()
    sae = l1_model(L1_D, L1_N, W, b)
    path = shards(tmp_path_factory.mktemp("l1"), x)
    bits = latent_bits(sae, x, L1_LENGTHS)
    full = latent_bits(sae, x, np.full(L1_F, L1_T))
    return sae, path, bits, full


@pytest.mark.parametrize("g", [0, 1, 3])
@pytest.mark.parametrize("s", [0, 2, 3])
def test_l1_exact_against_encode(l1_setup, s, g):
    sae, path, bits, _ = l1_setup
    *want, frames, seen = REF.timing_reference(masks_of(bits), s, g, L1_T)
    cases_occur(want, seen, g)
    tot = want[2]
    assert tot[0, REF.RUNS] == tot[0, REF.FILES] == tot[0, REF.CENSORED] == L1_F and tot[0, REF.LONGEST] == L1_T    # always on
    assert tot[1].sum() == 0                                                                                         # never on
    got = FT.feature_timing(sae, path, "enc", sub_bits=s, bridge=g, lengths=L1_LENGTHS, batch_files=2)
    compare(got, want, int(L1_LENGTHS.sum()), L1_F, L1_T, (s, g, 0))
    assert got.run_hist.shape == (L1_N, E.timing_nbins(s, L1_T))


def test_l1_threshold_no_lengths_and_period_two(l1_setup):
    sae, path, bits, full = l1_setup
    thr = FT.threshold_bits(0.5)
    # a non-zero threshold: fewer active frames than at 0, and still every case
    *want, frames, seen = REF.timing_reference(masks_of(bits, thr), 2, 1, L1_T)
    cases_occur(want, seen, 1)
    assert 0 < want[2][:, REF.ACTIVE].sum() < sum(int(m.sum()) for m in masks_of(bits))
    got = FT.feature_timing(sae, path, "enc", bridge=1, threshold=0.5, lengths=L1_LENGTHS, batch_files=2)
    compare(got, want, frames, L1_F, L1_T, (2, 1, thr))
    # without lengths every file counts T frames
    *want, frames, seen = REF.timing_reference(masks_of(full), 2, 0, L1_T)
    got = FT.feature_timing(sae, path, "enc", batch_files=2)
    compare(got, want, L1_F * L1_T, L1_F, L1_T, (2, 0, 0))
    # the period-2 file alone: some latent is on for every other frame of it -- 35 single-frame runs, 34 gaps of one frame
    m3 = masks_of(full)[3]
    r3, g3, t3, _, _ = REF.timing_reference([m3], 2, 0, L1_T)
    flick = np.flatnonzero((t3[:, REF.RUNS] == L1_T // 2) & (r3[:, 0] == L1_T // 2) & (g3[:, 0] == L1_T // 2 - 1))
    assert flick.size > 0
    # ... and at g = 1 each of them is one run of 69 frames
    r3b, g3b, t3b, _, _ = REF.timing_reference([m3], 2, 1, L1_T)
    assert (t3b[flick, REF.RUNS] == 1).all() and (t3b[flick, REF.LONGEST] == L1_T - 1).all() and (g3b[flick].sum(1) == 0).all()


def test_l1_cross_checks(l1_setup):
    sae, path, bits, _ = l1_setup
    got = FT.feature_timing(sae, path, "enc", lengths=L1_LENGTHS, batch_files=2)
    st = FST.feature_stats(sae, path, "enc", lengths=L1_LENGTHS, batch_files=2)
    np.testing.assert_array_equal(got.totals[:, REF.ACTIVE], st.fire_count)
    # a latent that is on for one whole file: read off the reference how many such files and how many other runs it has
    r, _, tot, _, seen = REF.timing_reference(masks_of(bits), 2, 0, L1_T)
    whole = seen["whole_file_by_latent"]
    j = int(np.argmax((whole > 0) & (tot[:, REF.RUNS] > whole)))             # ... one that also has other runs
    assert whole[j] > 0 and tot[j, REF.RUNS] > whole[j]
    others = int(tot[j, REF.RUNS] - whole[j])
    assert got.run_hist[j].sum() == whole[j] + others and got.run_hist[0].sum() == whole[0] == L1_F
    assert got.persistence()[0] == 1 - L1_F / L1_LENGTHS.sum() and got.duty()[0] == 1.0 and got.censored_fraction()[0] == 1.0
    assert got.top_latents("longest", 1).tolist() == [0]


def test_l1_contract_two_runs_batches_and_geometry(l1_setup):
    sae, path, bits, _ = l1_setup
    kw = dict(sub_bits=2, bridge=1, lengths=L1_LENGTHS)
    rng = torch.get_rng_state()
    a = FT.feature_timing(sae, path, "enc", batch_files=2, **kw)
    assert torch.equal(torch.get_rng_state(), rng)
    same(a, FT.feature_timing(sae, path, "enc", batch_files=2, **kw))
    for batch in (1, L1_F):
        same(a, FT.feature_timing(sae, path, "enc", batch_files=batch, **kw))
    # another launch geometry: every file of the call in one chunk
    x, _, _ = l1_case()
    eng = sae._ensure(L1_F * L1_T)
    nb = E.timing_nbins(2, L1_T)
    rh = torch.zeros(L1_N, nb, dtype=torch.int64, device="cuda")
    gh, tt, nf = torch.zeros_like(rh), torch.zeros(L1_N, 6, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.timing_files(torch.from_numpy(x).cuda(), 2, 1, 0, rh, gh, tt, nf, torch.from_numpy(L1_LENGTHS.astype(np.int32)).cuda(), one_chunk=True)
    torch.cuda.synchronize()
    assert rh.cpu().numpy().tobytes() == a.run_hist.tobytes() and gh.cpu().numpy().tobytes() == a.gap_hist.tobytes()
    assert tt.cpu().numpy().tobytes() == a.totals.tobytes() and int(nf.item()) == a.n_frames


def test_l1_many_bins_take_the_narrow_workgroups(tmp_path):
    """T = 300 at sub_bits = 3 has 49 bins: more LDS per column than 256 columns may take, so the launcher forms workgroups of 128
    columns (passes.hip, timing_launch_l1) -- n = 300 is then three column blocks, the last one partly padded.  The always-on column
    puts a run into the last bin."""
    T, F, s = 300, 2, 3
    L = np.array([T, 123])
    assert E.timing_nbins(s, T) == 49
    x = walk_inputs(5, F, T, L1_D)
    W, b = l1_case_weights(L1_D, L1_N, 5)
    sae = l1_model(L1_D, L1_N, W, b)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    for g in (0, 3):
        *want, frames, seen = REF.timing_reference(masks_of(bits), s, g, T)
        cases_occur(want, seen, g)
        assert want[0][0, 48] == 1 and want[0][:, 40:].sum() > 1
        got = FT.feature_timing(sae, path, "enc", sub_bits=s, bridge=g, lengths=L, batch_files=1)
        compare(got, want, int(L.sum()), F, T, (s, g, 0))


def test_l1_launcher_chunks_of_several_files(tmp_path):
    """n = 4352 is 17 column blocks, so a batch of 127 files of 8 frames goes out in chunks of two files, the last chunk holding one
    (passes.hip, timing_launch_l1); the second batch, 23 files, in chunks of one.  The state of a run must not leak from a file into
    the next one of its chunk: most runs here touch a file end."""
    T, F, n = 8, 150, 4352
    g = np.random.default_rng(8)
    L = g.integers(1, T + 1, F)
    L[0], L[1] = T, 1
    x = walk_inputs(8, F, T, L1_D, step=2.5)
    W, b = l1_case_weights(L1_D, n, 8)
    sae = l1_model(L1_D, n, W, b)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, L)
    for s_, g_ in ((2, 0), (1, 2)):
        *want, frames, seen = REF.timing_reference(masks_of(bits), s_, g_, T)
        cases_occur(want, seen, g_)
        got = FT.feature_timing(sae, path, "enc", sub_bits=s_, bridge=g_, lengths=L, batch_files=127)
        compare(got, want, int(L.sum()), F, T, (s_, g_, 0))


def test_l1_narrow_lds_counters_are_flushed():
    """n = 128, files of 1500 frames on which the latents flicker (the input alternates its sign: a column is on for every other
    frame), first the 45 files as the launcher chunks them, then all of a call in ONE chunk (SAE_TIMING_ONE_CHUNK) -- 67 500 rows, more
    than the flush interval of the 16-bit counters -- and then 90 files in one chunk: 67 500 single-frame runs per column, more than a
    half-word holds, so counters that were not flushed would wrap (and carry into the bin beside them)."""
    d, n, T = 256, 128, 1500
    W, _ = l1_weights(d, n, seed=9)
    sae = l1_model(d, n, W, np.zeros(n, np.float32), max_rows=90 * T)
    g = np.random.default_rng(2)
    u = (np.where(g.random(d) < 0.5, -1.0, 1.0) / 16).astype(np.float32)
    one = (8.0 * (-1.0) ** np.arange(T))[:, None].astype(np.float32) * u               # [T, d]
    xf = torch.from_numpy(one).cuda()
    b16 = sae.encode(xf).latent.to(torch.bfloat16)
    mask = (b16.view(torch.int16).cpu().numpy().view(np.uint16) & 0x7FFF) > 0           # encode() of the one file all files equal
    on = mask.sum(0)
    assert set(np.unique(on)) <= {0, T // 2} and (on == T // 2).sum() > n // 4           # columns flicker (or a . u = 0: never on)
    nb = E.timing_nbins(2, T)
    eng = sae._ensure(90 * T)
    for F, one_chunk in ((45, False), (45, True), (90, True)):
        r1, g1, t1, _, _ = REF.timing_reference([mask], 2, 0, T)
        want_r, want_g, want_t = r1 * F, g1 * F, t1 * F
        want_t[:, REF.LONGEST] = t1[:, REF.LONGEST]
        if F == 90:
            assert want_r[:, 0].max() == 90 * 750 > 65535
        x = xf.to(torch.float16).unsqueeze(0).expand(F, T, d).contiguous()
        assert torch.equal(x[0].float(), xf)                                            # fp16 holds the input exactly
        rh = torch.zeros(n, nb, dtype=torch.int64, device="cuda")
        gh, tt, nf = torch.zeros_like(rh), torch.zeros(n, 6, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        eng.timing_files(x, 2, 0, 0, rh, gh, tt, nf, one_chunk=one_chunk)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(rh.cpu().numpy(), want_r, err_msg=f"{F} files, one_chunk={one_chunk}")
        np.testing.assert_array_equal(gh.cpu().numpy(), want_g)
        np.testing.assert_array_equal(tt.cpu().numpy(), want_t)
        assert int(nf.item()) == F * T


# ---------------------------------------------------------------------------------------------------------------------------
TK_D, TK_F, TK_T = 64, 5, 70
TK_LENGTHS = np.array([TK_T, 1, 37, TK_T, 50])
TOPK_CASES = {
    # name: (n, k, encoder bias, forced latents, multi_topk, seed)
    "two_segments": (SEGMENT + 64, 8, 0.0, (SEGMENT - 1, SEGMENT), False, 1),
    "k96": (512, 96, 0.0, (5,), False, 2),
    "selected_zeros": (512, 16, -0.6, (5,), False, 3),
    "multi_topk": (1024, 8, 0.0, (5,), True, 4),
}


def topk_case(name):
    n, k, bias, forced, multi, seed = TOPK_CASES[name]
    x = walk_inputs(100 + seed, TK_F, TK_T, TK_D, n_dirs=3, step=0.6, noise=0.15)
    return x, topk_weights(TK_D, n, seed, bias, forced), n, k, forced, multi


@pytest.mark.parametrize("name", list(TOPK_CASES))
def test_topk_exact_against_encode(tmp_path, name):
    """two_segments: n spans two LDS tables of the kernel, the latents on both sides of the boundary are selected on every frame;
    k96: rows of two 64-slot chunks, the second partly empty; selected_zeros: rows with fewer than k positive pre-activations;
    multi_topk: the k selection of encode()."""
    x, w, n, k, forced, multi = topk_case(name)
    sae = topk_model(TK_D, n, k, w, multi)
    path = shards(tmp_path, x)
    bits = latent_bits(sae, x, TK_LENGTHS)
    if name == "selected_zeros":
        acts = torch.cat([sae.encode(torch.from_numpy(x[f]).cuda()).top_acts for f in range(TK_F)])
        assert bool((acts == 0).any()) and bool((acts > 0).any())
    st = FST.feature_stats(sae, path, "enc", lengths=TK_LENGTHS, batch_files=2)
    for s, g in ((2, 0), (0, 1), (3, 3)):
        *want, frames, seen = REF.timing_reference(masks_of(bits), s, g, TK_T)
        cases_occur(want, seen, g)
        for j in forced:                                                      # on for every counted frame of every file
            assert want[2][j, REF.RUNS] == want[2][j, REF.FILES] == TK_F and want[2][j, REF.ACTIVE] == TK_LENGTHS.sum()
        got = FT.feature_timing(sae, path, "enc", sub_bits=s, bridge=g, lengths=TK_LENGTHS, batch_files=2)
        compare(got, want, int(TK_LENGTHS.sum()), TK_F, TK_T, (s, g, 0))
        np.testing.assert_array_equal(got.totals[:, REF.ACTIVE], st.fire_count)
        assert got.totals[:, REF.ACTIVE].sum() <= TK_LENGTHS.sum() * k
    # a threshold inside the selected values
    vals = np.concatenate([b[b > 0] for b in bits])
    thr = int(np.sort(vals & 0x7FFF)[vals.size // 2])
    thr_val = float(np.array([thr << 16], np.uint32).view(np.float32)[0])
    *want, frames, seen = REF.timing_reference(masks_of(bits, thr), 2, 1, TK_T)
    assert 0 < want[2][:, REF.ACTIVE].sum() < vals.size
    compare(FT.feature_timing(sae, path, "enc", bridge=1, threshold=thr_val, lengths=TK_LENGTHS, batch_files=2), want, frames, TK_F, TK_T, (2, 1, thr))
    # two runs and the batch size: the same bytes
    a = FT.feature_timing(sae, path, "enc", bridge=1, lengths=TK_LENGTHS, batch_files=2)
    for batch in (2, 1, TK_F):
        same(a, FT.feature_timing(sae, path, "enc", bridge=1, lengths=TK_LENGTHS, batch_files=batch))


def test_topk_runs_from_the_feature_index(tmp_path):
    """A TopK store written by collect_features with K = k, indexed; the runs recomputed on the host from every latent's postings
    (positions file * T + frame, ascending) give the run_hist of the pass at g = 0."""
    x, w, n, k, _, _ = topk_case("multi_topk")
    sae = topk_model(TK_D, n, k, w)
    path = shards(tmp_path / "data", x)
    out = str(tmp_path / "store")
    CF.collect_features(sae, path, "enc", out, k=k, batch_files=2)
    FI.build_feature_index(out, "enc", batch_files=2)
    ix = FI.FeatureIndex(out, "enc")
    got = FT.feature_timing(sae, path, "enc", batch_files=2)
    want = np.zeros_like(got.run_hist)
    runs = 0
    for j in range(n):
        p = np.asarray(ix.postings(j)[0], np.int64)
        if p.size == 0:
            continue
        brk = np.flatnonzero((np.diff(p) != 1) | (p[1:] // TK_T != p[:-1] // TK_T))       # a new run: not the next frame, or the next file
        first, last = p[np.concatenate([[0], brk + 1])], p[np.concatenate([brk, [p.size - 1]])]
        np.add.at(want[j], REF.bins_of(last - first + 1, 2, TK_T), 1)
        runs += first.size
    assert runs > n and (want.sum(1) > 0).sum() > n // 8
    np.testing.assert_array_equal(got.run_hist, want)
    np.testing.assert_array_equal(got.totals[:, REF.ACTIVE], ix.counts)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_context_after_timing(variant):
    d, n, T, F = 256, 1024, 50, 4
    nb = E.timing_nbins(2, T)

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
    g = np.random.default_rng(3)
    for eng in (a, b):                                           # moments and (TopK) num_frames_since_fired that are not zero
        shapes = eng.param_shapes()
        eng.set_opt_state(3, {k: g.normal(0, 1e-3, v).astype(np.float32) for k, v in shapes.items()},
                          {k: g.random(v).astype(np.float32) * 1e-4 for k, v in shapes.items()})
        if variant == "topk":
            eng.set_topk_state(g.integers(0, 1000, n))
        eng.eval(x.reshape(F * T, d))
        g = np.random.default_rng(3)
    before = a.get_params()
    step, m1, m2 = a.get_opt_state()
    fired = a.get_topk_state() if variant == "topk" else None
    rh = torch.zeros(n, nb, dtype=torch.int64, device="cuda")
    gh, tt, nf = torch.zeros_like(rh), torch.zeros(n, 6, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    a.timing_files(x, 2, 0, 0, rh, gh, tt, nf)
    torch.cuda.synchronize()
    assert int(nf.item()) == F * T and bool((rh.sum(1) == tt[:, REF.RUNS]).all()) and int(tt[:, REF.RUNS].sum()) > 0
    for call in (lambda: a.latent_buffer(), lambda: a.latent_colmax(), lambda: a.metrics(),
                 lambda: a.decode(torch.zeros(4, n, device="cuda"), torch.empty(4, d, device="cuda"))):
        with pytest.raises(E.EngineError, match="timing"):
            call()
    if variant == "topk":
        with pytest.raises(E.EngineError, match="timing"):
            a.topk_indices_tensor(F * T, "cuda")
    for k, v in a.get_params().items():
        assert v.tobytes() == before[k].tobytes(), k
    s2, n1, n2 = a.get_opt_state()
    assert s2 == step and all(n1[k].tobytes() == m1[k].tobytes() and n2[k].tobytes() == m2[k].tobytes() for k in m1)
    if variant == "topk":
        assert a.get_topk_state().tobytes() == fired.tobytes()
    for eng in (a, b):
        eng.eval(x.reshape(F * T, d))                            # the next eval: the getters answer again
    a.latent_buffer()
    assert a.metrics().tobytes() == b.metrics().tobytes()
    # a following training step is bitwise the same step as in a context that never ran the pass
    for eng in (a, b):
        eng.step(x.reshape(F * T, d), 1e-3)
    torch.cuda.synchronize()
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert a.metrics().tobytes() == b.metrics().tobytes()

    # refused before anything is enqueued: the arrays are still zero
    rh.zero_(), gh.zero_(), tt.zero_(), nf.zero_()
    with pytest.raises(E.EngineError, match="max_rows"):
        a.timing_files(torch.randn(40, 50, d).cuda(), 2, 0, 0, torch.zeros(n, nb, dtype=torch.int64, device="cuda"), gh, tt, nf)
    lib, vp = a._lib, C.c_void_p
    ok = dict(x=x.data_ptr(), F=F, T=T, dt=E.DTYPE["float32"], s=2, g=0, thr=0, flags=0, rh=rh.data_ptr(), gh=gh.data_ptr(), tt=tt.data_ptr(),
              nf=nf.data_ptr())

    def raw(**kw):
        p = {**ok, **kw}
        return lib.sae_timing_files(a._ctx, vp(p["x"]), p["F"], p["T"], p["dt"], None, p["s"], p["g"], p["thr"], p["flags"], vp(p["rh"]),
                                    vp(p["gh"]), vp(p["tt"]), vp(p["nf"]), vp(torch.cuda.current_stream().cuda_stream))

    for bad in (dict(s=-1), dict(s=4), dict(g=-1), dict(g=16), dict(thr=0x7F81), dict(flags=2), dict(flags=4), dict(dt=99),
                dict(x=None), dict(rh=None), dict(gh=None), dict(tt=None), dict(nf=None),
                dict(rh=rh.data_ptr() + 4), dict(gh=gh.data_ptr() + 4), dict(tt=tt.data_ptr() + 4), dict(nf=nf.data_ptr() + 4),
                dict(F=0), dict(T=0), dict(F=1, T=65536), dict(F=31)):                    # 31 x 50 rows > max_rows
        assert raw(**bad) != 0, bad
    torch.cuda.synchronize()
    for t in (rh, gh, tt, nf):
        assert bool((t == 0).all())
    a.close()
    b.close()


def test_fp8_context_is_rejected():
    eng = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    nb = E.timing_nbins(2, 100)
    rh = torch.zeros(1024, nb, dtype=torch.int64, device="cuda")
    gh, tt, nf = torch.zeros_like(rh), torch.zeros(1024, 6, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(E.EngineError, match="fp8"):
        eng.timing_files(torch.randn(2, 100, 256).cuda(), 2, 0, 0, rh, gh, tt, nf)
    torch.cuda.synchronize()
    assert not bool(rh.any()) and not bool(gh.any()) and not bool(tt.any()) and not bool(nf.any())
    eng.close()


def test_cli_end_to_end(tmp_path, l1_setup):
    sae, path, bits, _ = l1_setup
    ck = tmp_path / "sae.pth"
    torch.save({"hparams": {"autoencoder_variant": "l1", "activation_size": L1_D,
                            "autoencoder_config": {"n_dict_components": L1_N, "recon_alpha": 1.0}},
                "model": sae.state_dict()}, str(ck))
    np.save(tmp_path / "len.npy", L1_LENGTHS)
    out = tmp_path / "timing.npz"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "freud_amd.feature_timing", "--sae", str(ck), "--data_path", path, "--layer_name", "enc",
                        "--sub_bits", "3", "--bridge", "1", "--threshold", "0.5", "--lengths", str(tmp_path / "len.npy"), "--batch_files", "2",
                        "--out", str(out)], check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    summary = json.loads(lines[0])
    thr = FT.threshold_bits(0.5)
    *want, frames, _ = REF.timing_reference(masks_of(bits, thr), 3, 1, L1_T)
    back = FT.FeatureTiming.from_npz(str(out))
    compare(back, want, frames, L1_F, L1_T, (3, 1, thr))
    assert summary["n_frames"] == frames and summary["n_files"] == L1_F and summary["bridge"] == 1 and summary["threshold"] == 0.5
    assert summary["runs"] == int(want[2][:, REF.RUNS].sum()) and summary["n_bins"] == E.timing_nbins(3, L1_T)
