"""GPU: the feature manipulation (freud_amd/manipulate.py over include/freud_sae.h's sae_manipulate_files; freud_amd/csrc/manip.h).

Shapes, the smallest that reach each path and its padding:
    A  L1    d=32   n=128          golden                 the reference's own model
    B  L1    d=384  n=3072         2 x 130 (M = 260: no multiple of 128; the fused d = 384 forward)
    C  L1    d=200  n=1100         3 x 50  (d_p, n_p padded; n_p = 1152 is no multiple of 256)
    D  TopK  d=32   n=128   k=8    golden
    E  TopK  d=768  n=4096  k=64   2 x 130
B, C and E edit column 0, column n - 1 and the pair 127 / 128 that straddles a 128-column boundary.

1. exact identities: the series against encode(), the L1 standard decode against decode(encode()), factor 1 and untouched frames
   against standard, two runs, the training state, the state sae_eval leaves;
2. the apply rule to the bit: manip.h's sm_apply_serial restated in numpy float32 (fma32 below is an exactly rounded fmaf) on the
   engine's own standard, series and bf16 operand rows;
3. the TopK standard decode against float64 within (k + 2) 2^-24 (|b_dec| + sum |vals w|), its series against the selection;
4. the reference's golden at the bf16 tolerances of tests/test_models_gpu.py (1e-2 rel-Frobenius);
5. the refusals of the C ABI, with nothing enqueued."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from freud_amd import engine as E
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.manipulate import manipulate_features, manipulate_latent
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly rounded: the product is exact in float64; where the float64 sum lands on a float32
    tie although the true sum does not (TwoSum's error term says on which side it lies), it is nudged there before the cast."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    s = np.where(tie & (err != 0), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def apply_rule(standard, series, ops, values, w):
    """sm_apply_serial for all frames: standard [M, d], series [E, M], values [V, E], w [E, d] -> [V, M, d] (numpy float32)."""
    out = np.empty((values.shape[0],) + standard.shape, np.float32)
    for v in range(values.shape[0]):
        acc = standard.copy()
        for e in range(series.shape[0]):
            a = series[e]
            new = np.full_like(a, values[v, e]) if ops[e] == 1 else (a * values[v, e]).astype(np.float32)
            delta = (new - a).astype(np.float32)
            nz = delta != 0
            acc[nz] = fma32(delta[nz][:, None], w[e][None, :], acc[nz])
        out[v] = acc
    return out


def l1_model(d, n, seed, bias=-0.5):
    """Unit-norm columns of 64 entries +-1/8: the in-place renormalisation of every forward is a fixed point, so two forwards see
    the same weights to the bit (the recipe of tests/test_feature_stats_gpu.py)."""
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:64], j] = np.where(g.random(64) < 0.5, -0.125, 0.125)
    b = g.normal(bias, 0.3, n).astype(np.float32)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def topk_model(d, n, k, seed):
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k), max_rows=1500)
    sd = sae.state_dict()
    sd["b_dec"] = 0.05 * torch.randn(d)
    sd["encoder.bias"] = 0.05 * torch.randn(n)
    for j in (0, 127, 128, n - 1):                      # the edited latents are selected on some frames, not on all
        sd["encoder.bias"][j] = 1.2
    sae.load_state_dict(sd)
    return sae


def golden_model(kind):
    g = np.load(os.path.join(GOLD, f"manipulate_{kind}.npz"))
    if kind == "l1":
        sae = L1AutoEncoder(32, L1AutoEncoderConfig(n_dict_components=128), max_rows=1500)
        sae.load_state_dict({"decoder.weight": torch.from_numpy(g["W"]), "encoder_bias": torch.from_numpy(g["b"])})
    else:
        sae = TopKAutoEncoder(32, TopKAutoEncoderConfig(n_dict_components=128, k=int(g["k"])), max_rows=1500)
        sae.load_state_dict({"encoder.weight": torch.from_numpy(g["W_enc"]), "encoder.bias": torch.from_numpy(g["b_enc"]),
                             "W_dec": torch.from_numpy(g["W_dec"]), "b_dec": torch.from_numpy(g["b_dec"])})
    return sae, g


CASES = {"B": ("l1", 384, 3072, 0, 2, 130), "C": ("l1", 200, 1100, 0, 3, 50), "E": ("topk", 768, 4096, 64, 2, 130)}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    kind, d, n, k, F, T = CASES[request.param]
    sae = l1_model(d, n, 11) if kind == "l1" else topk_model(d, n, k, 12)
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(5)).cuda()
    return kind, sae, x, n


def operand_rows(kind, sae, latents):
    """bf16 of the engine's CURRENT weights, the rows the standard decode multiplies by: [E, d]."""
    p = sae._eng.get_params()
    W = p["decoder.weight"].T if kind == "l1" else p["W_dec"]
    return bf16(W[np.asarray(latents)])


def dense_latent(kind, sae, x):
    if kind == "l1":
        return sae.encode(x).latent
    enc = sae.encode(x)
    return torch.zeros(*x.shape[:-1], sae.n_dict_components, device=x.device).scatter_(-1, enc.top_indices, enc.top_acts)


# ---- 1. exact identities
def test_identities(case):
    kind, sae, x, n = case
    F, T, d = x.shape
    latents = [0, n - 1, 127, 128]
    values = np.array([[1.0, 1.0, 1.0, 1.0], [1.5, 0.0, -2.0, 10.0]], np.float32)
    sae._eng.eval(x)
    state0 = (sae._eng.get_params(), sae._eng.get_opt_state(), sae._eng.get_topk_state() if kind == "topk" else None)
    m = manipulate_features(sae, x, [(j, "scale") for j in latents], values)
    lat_after = sae._latent_view(F * T).clone()
    metrics_after = sae._eng.metrics()
    state1 = (sae._eng.get_params(), sae._eng.get_opt_state(), sae._eng.get_topk_state() if kind == "topk" else None)
    for k in state0[0]:
        assert np.array_equal(state0[0][k].view(np.uint32), state1[0][k].view(np.uint32)), k
    assert state0[1][0] == state1[1][0]
    for a, b in zip(state0[1][1:], state1[1][1:]):
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    if kind == "topk":
        assert np.array_equal(state0[2], state1[2])
    # the series are encode()'s columns
    dense = dense_latent(kind, sae, x)
    for e, j in enumerate(latents):
        got = torch.stack(m.standard_activations[e])
        assert np.array_equal(bits(got), bits(dense[..., j])), j
        assert float(got.max()) > 0 and float(got.min()) == 0, "the edited latent should fire on some frames, not on all"
    # the state sae_eval of the same batch leaves
    sae._eng.eval(x)
    assert torch.equal(lat_after.view(torch.int16), sae._latent_view(F * T).view(torch.int16))
    assert np.array_equal(metrics_after.view(np.uint32), sae._eng.metrics().view(np.uint32))
    if kind == "l1":
        assert np.array_equal(bits(m.standard_decoded), bits(sae.decode(sae.encode(x).latent)))
    # factor 1 is standard; so is every frame on which all the edited latents are zero
    std = m.standard_decoded
    assert np.array_equal(bits(m.manipulated_decoded[0]), bits(std))
    quiet = torch.stack([torch.stack(s) for s in m.standard_activations]).eq(0).all(0).to(std.device)        # [F, T]
    assert 0 < int(quiet.sum()) < F * T
    assert np.array_equal(bits(m.manipulated_decoded[1][quiet]), bits(std[quiet]))
    assert not torch.equal(m.manipulated_decoded[1][~quiet], std[~quiet])
    # two runs
    m2 = manipulate_features(sae, x, [(j, "scale") for j in latents], values)
    assert np.array_equal(bits(m2.standard_decoded), bits(std)) and np.array_equal(bits(m2.manipulated_decoded), bits(m.manipulated_decoded))
    assert all(torch.equal(a, b) for e in range(4) for a, b in zip(m.standard_activations[e], m2.standard_activations[e]))
    # lengths trim the series only
    m3 = manipulate_features(sae, x, [(0, "scale")], [[2.0]], lengths=[T, 7] + [T] * (F - 2))
    assert [len(s) for s in m3.standard_activations[0]] == [T, 7] + [T] * (F - 2)
    assert torch.equal(m3.standard_activations[0][1], m.standard_activations[0][1][:7])
    assert torch.equal(m3.manipulated_activations[0][0][1], m.standard_activations[0][1][:7] * 2.0)
    assert np.array_equal(bits(m3.standard_decoded), bits(std))


# ---- 2. the apply rule, to the bit
@pytest.mark.parametrize("n_edits,n_variants", [(1, 1), (3, 5), (16, 16)])
def test_apply_rule_to_the_bit(case, n_edits, n_variants):
    kind, sae, x, n = case
    F, T, d = x.shape
    r = np.random.default_rng(n_edits * 100 + n_variants)
    latents = [0, n - 1, 127, 128][:n_edits] + sorted(r.choice(np.arange(200, n - 1), max(n_edits - 4, 0), replace=False).tolist())
    latents = latents[:n_edits]
    ops = [int(o) for o in (np.arange(n_edits) % 3 == 1)]                # both ops: edits 1, 4, 7, ... are SET
    values = r.choice(np.array([0.0, 1.0, 1.5, -2.0, 10.0, -0.75, 0.3], np.float32), (n_variants, n_edits)).astype(np.float32)
    values[0, 0] = -2.0
    if n_variants > 1:
        values[1, 0] = 0.0
    m = manipulate_features(sae, x, list(zip(latents, ops)), values)
    std = m.standard_decoded.cpu().numpy().reshape(F * T, d)
    series = np.stack([torch.stack(s).numpy().reshape(-1) for s in m.standard_activations])
    want = apply_rule(std, series, ops, values, operand_rows(kind, sae, latents))
    got = m.manipulated_decoded.cpu().numpy().reshape(n_variants, F * T, d)
    assert np.abs(want - std[None]).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the manipulated series are sm_new of the standard ones
    for v in range(n_variants):
        for e in range(n_edits):
            s = torch.stack(m.manipulated_activations[v][e]).numpy().reshape(-1)
            w = np.full_like(series[e], values[v, e]) if ops[e] else (series[e] * values[v, e]).astype(np.float32)
            assert np.array_equal(s.view(np.uint32), w.view(np.uint32))


# ---- 3. TopK standard decode and SET on frames without the latent
def test_topk_standard_decode_and_set():
    kind, d, n, k, F, T = CASES["E"]
    sae = topk_model(d, n, k, 12)
    x = torch.randn(F, T, d, generator=torch.Generator().manual_seed(5)).cuda()
    m = manipulate_features(sae, x, [(127, "set"), (128, "scale")], [[2.5, 1.0], [0.0, 3.0]])
    enc = sae.encode(x)
    idx, acts = enc.top_indices.cpu().numpy().reshape(F * T, k), enc.top_acts.cpu().numpy().reshape(F * T, k).astype(np.float64)
    p = sae._eng.get_params()
    Wd, bd = bf16(p["W_dec"]).astype(np.float64), p["b_dec"].astype(np.float64)
    rows = Wd[idx]                                                        # [M, k, d]
    want = bd + (acts[:, :, None] * rows).sum(1)
    bound = (k + 2) * U * (np.abs(bd) + (np.abs(acts)[:, :, None] * np.abs(rows)).sum(1))
    std = m.standard_decoded.cpu().numpy().reshape(F * T, d)
    assert (np.abs(std - want) <= bound).all()
    # the series: activation_tensor_from_indexed of the engine's own selection
    for e, j in enumerate((127, 128)):
        ser = np.where(idx == j, acts, 0.0).sum(1).astype(np.float32)
        assert np.array_equal(torch.stack(m.standard_activations[e]).numpy().reshape(-1).view(np.uint32), ser.view(np.uint32))
    # SET on a frame where 127 is not selected (and 128 untouched by variant 0): the frame moves by value * w
    a127 = torch.stack(m.standard_activations[0]).numpy().reshape(-1)
    off = a127 == 0
    assert 0 < off.sum() < F * T
    man = m.manipulated_decoded[0].cpu().numpy().reshape(F * T, d).astype(np.float64)
    w = Wd[127]
    assert (np.abs(man[off] - (std[off] + 2.5 * w)) <= 3 * U * (np.abs(std[off]) + np.abs(2.5 * w))).all()


# ---- 4. the reference's golden
def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-30))


@pytest.mark.parametrize("kind", ["l1", "topk"])
def test_against_the_reference_golden(kind):
    sae, g = golden_model(kind)
    x = torch.from_numpy(g["x"]).cuda()
    Fn, T, d = x.shape
    lens = [int(v) for v in g["lengths"]]
    factors = g["factors"]
    keep = np.ones((Fn, T), bool) if kind == "l1" else ~g["flagged"]
    assert keep.mean() > 0.9
    for i, feat in enumerate(g["features"]):
        m = manipulate_features(sae, x, [(int(feat), "scale")], [[float(f)] for f in factors], lengths=lens)
        std = m.standard_decoded.cpu().numpy()
        man = m.manipulated_decoded.cpu().numpy()
        assert rel(std[keep], g["standard_decoded"][keep]) <= 1e-2
        gs = g["standard_activations"][i]
        mine = np.zeros_like(gs)
        for f, L in enumerate(lens):
            mine[f, :L] = m.standard_activations[0][f].numpy()
        never = not gs.any()
        if never:
            assert not mine.any() and np.array_equal(man.view(np.uint32), np.broadcast_to(std, man.shape).view(np.uint32))
        else:
            assert rel(mine[keep], gs[keep]) <= 1e-2
        for v, factor in enumerate(factors):
            assert rel(man[v][keep], g["manipulated_decoded"][i, v][keep]) <= 1e-2
            gm = g["manipulated_activations"][i, v]
            ms = np.zeros_like(gm)
            for f, L in enumerate(lens):
                ms[f, :L] = m.manipulated_activations[v][0][f].numpy()
            if never:
                assert not ms.any()
                continue
            if gm.any():
                assert rel(ms[keep], gm[keep]) <= 1e-2
            gdiff = g["manipulated_decoded"][i, v] - g["standard_decoded"]
            if factor != 1.0:
                assert rel((man[v] - std)[keep], gdiff[keep]) <= 1e-2, (feat, factor)
            else:
                assert np.array_equal(man[v].view(np.uint32), std.view(np.uint32))
    # the reference's call for one file
    s, mm, a, b = manipulate_latent(sae, x[1:2], int(g["features"][0]), 1.5, lens[1])
    assert s.shape == (1, T, d) and mm.shape == (1, T, d) and a.shape == (lens[1],) and b.shape == (lens[1],)
    assert rel(a.numpy(), g["standard_activations"][0, 1, :lens[1]]) <= 1e-2 and torch.equal(b, a * 1.5)


# ---- 5. refusals through the C ABI
def _call(eng, x, latents, ops, values, n_edits, n_variants, flags, std, man, ser, n_files=None, T=None, null=None):
    lat = np.asarray(latents, np.int32)
    op = np.asarray(ops, np.int32)
    val = np.asarray(values, np.float32)
    ptr = {"x": C.c_void_p(x.data_ptr()), "lat": lat.ctypes.data_as(C.POINTER(C.c_int32)), "op": op.ctypes.data_as(C.POINTER(C.c_int32)),
           "val": val.ctypes.data_as(C.POINTER(C.c_float)), "std": C.c_void_p(std.data_ptr()), "man": C.c_void_p(man.data_ptr()),
           "ser": C.c_void_p(ser.data_ptr()), "ctx": eng._ctx}
    if null:
        ptr[null] = None
    return eng._lib.sae_manipulate_files(ptr["ctx"], ptr["x"], x.shape[0] if n_files is None else n_files, x.shape[1] if T is None else T,
                                         E.DTYPE["float32"], ptr["lat"], ptr["op"], n_edits, ptr["val"], n_variants, flags, ptr["std"],
                                         ptr["man"], ptr["ser"], C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_refusals_enqueue_nothing():
    eng = E.SaeEngine("l1", 32, 128, max_rows=256)
    eng8 = E.SaeEngine("l1", 256, 1024, 512, precision="fp8")
    x = torch.randn(2, 60, 32).cuda()
    x8 = torch.randn(1, 60, 256).cuda()
    bufs = [torch.full((n,), -77.0, device="cuda") for n in (2 * 60 * 256, 2 * 60 * 256, 240)]
    std, man, ser = bufs
    seventeen = list(range(17))
    bad = {
        "null ctx": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="ctx"),
        "null x": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="x"),
        "null latents": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="lat"),
        "null ops": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="op"),
        "null values": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="val"),
        "null standard": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="std"),
        "null manipulated": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="man"),
        "null series": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, null="ser"),
        "0 edits": dict(latents=[1], ops=[0], values=[1.0], n_edits=0, n_variants=1, flags=0),
        "17 edits": dict(latents=seventeen, ops=[0] * 17, values=[1.0] * 17, n_edits=17, n_variants=1, flags=0),
        "0 variants": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=0, flags=0),
        "17 variants": dict(latents=[1], ops=[0], values=[1.0] * 17, n_edits=1, n_variants=17, flags=0),
        "latent -1": dict(latents=[-1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0),
        "latent n": dict(latents=[128], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0),
        "latent twice": dict(latents=[5, 9, 5], ops=[0, 0, 1], values=[1.0] * 3, n_edits=3, n_variants=1, flags=0),
        "op 2": dict(latents=[1], ops=[2], values=[1.0], n_edits=1, n_variants=1, flags=0),
        "nan": dict(latents=[1, 2], ops=[0, 0], values=[1.0, 1.0, 1.0, float("nan")], n_edits=2, n_variants=2, flags=0),
        "inf": dict(latents=[1], ops=[1], values=[float("inf")], n_edits=1, n_variants=1, flags=0),
        "flags": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=1),
        "M > max_rows": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, n_files=5, T=60),
        "0 files": dict(latents=[1], ops=[0], values=[1.0], n_edits=1, n_variants=1, flags=0, n_files=0),
    }
    for name, kw in bad.items():
        assert _call(eng, x, std=std, man=man, ser=ser, **kw) == -1, name
    assert _call(eng8, x8, [1], [0], [1.0], 1, 1, 0, std, man, ser) == -1
    assert b"fp8" in eng._lib.sae_last_error()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == -77.0).all())
    # and the same buffers take a good call
    assert _call(eng, x, [1], [0], [2.0], 1, 1, 0, std, man, ser) == 0
    torch.cuda.synchronize()
    assert bool((std[:2 * 60 * 32] != -77.0).all()) and bool((std[2 * 60 * 32:] == -77.0).all())
    assert bool((man[2 * 60 * 32:] == -77.0).all()) and bool((ser[120:] == -77.0).all())
    with pytest.raises(E.EngineError):
        eng.manipulate_files(x, [1], [0], [[1.0]], std[:10], man[:2 * 60 * 32].clone(), ser[:120].clone())
