"""GPU: the engine-backed inference classes (freud_amd/models.py) against the fp32 CPU oracle
(the reference's inference runs without autocast on CPU: oracle autocast=False).  Tolerances are bf16-operand ones:
latent / reconstruction rel-Frobenius <= 1e-2, losses rtol 2e-2.  The glue tests further down hold forward() to decode(encode())
to the bit and to the element-level decode bound of tests/decode_reference.py."""
import os

import numpy as np
import pytest
import torch

from oracle import sae_oracle as O
from tests import decode_reference as R

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _x(B, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.relu(torch.randn(B * T, 32, generator=g)) * 0.1
    return (z @ torch.randn(32, d, generator=g)).reshape(B, T, d)


def test_l1_encode_decode_forward_match_oracle():
    from freud_amd.config import L1AutoEncoderConfig
    from freud_amd.models import L1AutoEncoder, L1EncoderOutput, L1ForwardOutput
    d, B, T = 384, 2, 700
    torch.manual_seed(0)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(expansion_factor=4, recon_alpha=1e4), max_rows=256)   # forces a re-size
    sd = sae.state_dict()
    assert list(sd.keys()) == ["encoder_bias", "decoder.weight"] and sd["decoder.weight"].shape == (d, 4 * d)
    sd["encoder_bias"] = 0.01 * torch.randn(4 * d)
    sae.load_state_dict(sd)
    x = _x(B, T, d, 1)
    W = O.normalize_columns(sd["decoder.weight"].clone())
    ref = O.l1_forward(x.reshape(-1, d), W, sd["encoder_bias"], 1e4, autocast=False)

    enc = sae.encode(x)
    assert isinstance(enc, L1EncoderOutput) and enc.latent.shape == (B, T, 4 * d) and enc.latent.dtype == torch.float32
    assert _rel(enc.latent.cpu().reshape(-1, 4 * d), ref["c"]) < 1e-2
    # like the reference's encode(), the decoder columns are renormalised in place
    assert _rel(sae.state_dict()["decoder.weight"], W) < 1e-6

    xh = sae.decode(enc.latent)
    assert xh.shape == (B, T, d) and _rel(xh.cpu().reshape(-1, d), ref["c"] @ W.t()) < 1e-2

    out, mse = sae(x.cuda(), return_mse=True)
    assert isinstance(out, L1ForwardOutput)
    assert _rel(out.sae_out.cpu().reshape(-1, d), ref["x_hat"]) < 1e-2
    assert float(out.l1_loss) == pytest.approx(ref["l1_loss"].item(), rel=2e-2)
    assert float(out.reconstruction_loss) == pytest.approx(ref["reconstruction_loss"].item(), rel=2e-2)
    assert float(mse) == pytest.approx(ref["mse"].item(), rel=2e-2)


def test_topk_encode_decode_forward_match_oracle():
    from freud_amd.config import TopKAutoEncoderConfig
    from freud_amd.models import TopKAutoEncoder, TopKForwardOutput
    d, B, T, k = 256, 3, 200, 16
    torch.manual_seed(0)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(expansion_factor=4, k=k, auxk_alpha=0.03125))
    sd = sae.state_dict()
    assert list(sd.keys()) == ["W_dec", "b_dec", "encoder.weight", "encoder.bias"]
    sd["b_dec"] = 0.01 * torch.randn(d)
    sae.load_state_dict(sd)
    x = _x(B, T, d, 2)
    ref = O.topk_forward(x, sd["encoder.weight"], sd["encoder.bias"], sd["W_dec"], sd["b_dec"], k, autocast=False)

    enc = sae.encode(x)
    assert enc.top_acts.shape == (B, T, k) and enc.top_indices.shape == (B, T, k) and enc.top_indices.dtype == torch.int64
    got = enc.top_acts.cpu().reshape(-1, k).sort(dim=1).values
    want = ref["top_acts"].float().sort(dim=1).values
    assert _rel(got, want) < 1e-2
    # index sets: identical wherever the k-th and (k+1)-th pre-activations are well separated
    pre = torch.relu((x.reshape(-1, d) - sd["b_dec"]) @ sd["encoder.weight"].t() + sd["encoder.bias"])
    srt = pre.sort(dim=1, descending=True).values
    clear = (srt[:, k - 1] - srt[:, k]) > 1e-2 * srt[:, k - 1].abs()
    gi = enc.top_indices.cpu().reshape(-1, k).sort(dim=1).values
    wi = ref["top_indices"].sort(dim=1).values
    assert clear.float().mean() > 0.2 and torch.equal(gi[clear], wi[clear])

    xh = sae.decode(ref["top_acts"].float().reshape(B, T, k), ref["top_indices"].reshape(B, T, k))
    assert _rel(xh.cpu().reshape(-1, d), ref["x_hat"]) < 1e-2

    out, mse = sae(x, return_mse=True)
    assert isinstance(out, TopKForwardOutput) and float(out.auxk_loss) == 0.0
    # rows whose k-th / (k+1)-th pre-activations nearly tie may pick another latent in bf16: compare the clear rows
    assert _rel(out.sae_out.cpu().reshape(-1, d)[clear], ref["x_hat"][clear]) < 2e-2
    assert float(out.fvu) == pytest.approx(ref["fvu"].item(), rel=5e-2)
    assert float(mse) == pytest.approx(ref["mse"].item(), rel=5e-2)


def test_init_sae_from_checkpoint_reads_reference_keys(tmp_path):
    from freud_amd.models import init_sae_from_checkpoint, L1AutoEncoder
    d, n = 384, 768
    torch.manual_seed(1)
    W = torch.empty(d, n)
    torch.nn.init.orthogonal_(W)
    ck = {"model": {"encoder_bias": torch.zeros(n), "decoder.weight": W}, "optimizer": {}, "scheduler": {}, "step": 3,
          "best_val_loss": 1.0,
          "hparams": {"autoencoder_variant": "l1", "activation_size": d,
                      "autoencoder_config": {"n_dict_components": n, "recon_alpha": 1e4}}}
    path = os.path.join(str(tmp_path), "step3.pth")
    torch.save(ck, path)
    sae = init_sae_from_checkpoint(path)
    assert isinstance(sae, L1AutoEncoder) and sae.n_dict_components == n
    assert torch.equal(sae.state_dict()["decoder.weight"], W)
    lat = sae.encode(_x(1, 100, d, 3)).latent
    assert lat.shape == (1, 100, n) and torch.isfinite(lat).all()


# ---- the glue between the classes and the engine (the decode itself: tests/test_decode_gpu.py) ---------------------------------------
def _bits(t):
    return R.bits(t)


def _l1_fixed_point(d, n, seed, max_rows=1500):
    """An L1 model whose renormalisation is a fixed point: every forward sees the same weights to the bit."""
    from freud_amd.config import L1AutoEncoderConfig
    from freud_amd.models import L1AutoEncoder
    W, b = R.unit_l1_weights(d, n, seed)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=max_rows)
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae


def _topk(d, n, k, seed, max_rows=1500, **cfg):
    from freud_amd.config import TopKAutoEncoderConfig
    from freud_amd.models import TopKAutoEncoder
    torch.manual_seed(seed)
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, **cfg), max_rows=max_rows)
    sd = sae.state_dict()
    sd["b_dec"] = 0.05 * torch.randn(d)
    sd["encoder.bias"] = 0.05 * torch.randn(n)
    sae.load_state_dict(sd)
    return sae, sd


def _scatter(acts, idx, n):
    a2, i2 = acts.reshape(-1, acts.shape[-1]), idx.reshape(-1, idx.shape[-1])
    return torch.zeros(a2.shape[0], n, device=a2.device).scatter_(1, i2, a2.float())


def test_l1_forward_is_decode_of_encode():
    """sae(x).sae_out is sae.decode(sae.encode(x).latent) to the bit, and within the decode bound of the float64 product of the
    returned latent and the engine's bf16 weights."""
    d, n = 384, 1536
    sae = _l1_fixed_point(d, n, 3)
    x = torch.randn(2, 130, d, generator=torch.Generator().manual_seed(4)).cuda()
    out = sae(x)
    lat = sae.encode(x).latent
    assert np.array_equal(_bits(out.encoded.latent), _bits(lat)) and float((lat > 0).float().mean()) > 0.01
    assert np.array_equal(_bits(out.sae_out), _bits(sae.decode(lat)))
    W = sae._eng.get_params()["decoder.weight"].T
    ref, tol = R.decode_reference(out.encoded.latent.reshape(-1, n), W, None, R.padded_n(n))
    got = out.sae_out.reshape(-1, d)
    assert not R.violations(got, ref, tol).any(), R.report(got, ref, tol)


def test_topk_forward_is_decode_of_encode():
    d, n, k = 256, 1024, 16
    sae, _sd = _topk(d, n, k, 5)
    x = _x(3, 50, d, 6).cuda()
    out = sae(x)
    enc = sae.encode(x)
    assert torch.equal(out.encoded.top_indices, enc.top_indices) and np.array_equal(_bits(out.encoded.top_acts), _bits(enc.top_acts))
    assert np.array_equal(_bits(out.sae_out), _bits(sae.decode(enc.top_acts, enc.top_indices)))
    p = sae._eng.get_params()
    ref, tol = R.decode_reference(_scatter(enc.top_acts, enc.top_indices, n), p["W_dec"], p["b_dec"], R.padded_n(n))
    got = out.sae_out.reshape(-1, d)
    assert not R.violations(got, ref, tol, p["b_dec"]).any(), R.report(got, ref, tol, p["b_dec"])


def test_topk_multi_topk_forward_rebinds_to_the_4k_selection():
    """cfg.multi_topk at inference (topkautoencoder.py:134-147): forward() returns the 4k selection and its decode, encode() the k one.
    Against the oracle under the engine's tie rule (lowest column first)."""
    d, n, k, B, T = 256, 1024, 8, 3, 40
    sae, sd = _topk(d, n, k, 7, multi_topk=True)
    x = _x(B, T, d, 8)
    ref = O.topk_forward(x, sd["encoder.weight"], sd["encoder.bias"], sd["W_dec"], sd["b_dec"], k, multi_topk=True, stable_ties=True)
    out = sae(x.cuda())
    assert out.encoded.top_indices.shape == (B, T, 4 * k) and out.encoded.top_acts.shape == (B, T, 4 * k)
    srt = ref["pre"].float().reshape(B * T, n).sort(dim=1, descending=True).values
    clear = (srt[:, 4 * k - 1] != srt[:, 4 * k]).numpy()
    gi = np.sort(out.encoded.top_indices.cpu().reshape(-1, 4 * k).numpy(), 1)
    wi = np.sort(ref["multi_indices"].reshape(-1, 4 * k).numpy(), 1)
    assert clear.mean() > 0.2 and np.array_equal(gi[clear], wi[clear])
    assert float(out.multi_topk_fvu) == pytest.approx(ref["multi_topk_fvu"].item(), rel=5e-3)
    assert float(out.fvu) == pytest.approx(ref["fvu"].item(), rel=5e-3)
    assert np.array_equal(_bits(out.sae_out), _bits(sae.decode(out.encoded.top_acts, out.encoded.top_indices)))
    enc = sae.encode(x.cuda())
    assert enc.top_indices.shape == (B, T, k) and enc.top_acts.shape == (B, T, k)


def test_topk_engine_recreation_keeps_parameters_and_options():
    """_EngineModel._ensure re-creates the context for a batch above its row limit (which is never below 1500): the parameters and
    set_topk_options (no latent is ever dead at inference) must survive it."""
    d, n, k = 256, 1024, 8
    sae, _ = _topk(d, n, k, 9, max_rows=256, auxk_alpha=0.03125)
    sd0 = sae.state_dict()
    xs = {rows: _x(1, rows, d, 10 + rows).reshape(rows, d).cuda() for rows in (200, 700, 1700)}
    first = sae.encode(xs[200])
    eng0 = sae._eng
    sae.encode(xs[700])
    assert sae._eng is eng0                       # 700 rows fit the 1500-row floor of the first context
    sae.encode(xs[1700])
    assert sae._eng is not eng0 and sae._max_rows >= 1700
    assert sae._eng._dead_threshold == float("inf") and sae._eng._rows_per_file == 0      # _configure ran on the new context
    third = sae.encode(xs[200])
    assert torch.equal(first.top_indices, third.top_indices) and np.array_equal(_bits(first.top_acts), _bits(third.top_acts))
    sd1 = sae.state_dict()
    assert list(sd1) == list(sd0) and all(np.array_equal(_bits(sd0[key]), _bits(sd1[key])) for key in sd0)
    out = sae(xs[200].reshape(2, 100, d))
    assert float(out.auxk_loss) == 0.0 and np.isfinite(float(out.fvu)) and float(out.fvu) > 0


def test_topk_forward_2d_input_takes_the_variance_over_rows():
    """x.mean(0) (topkautoencoder.py:104) of a [M][d] input is the mean over its rows, so forward() gives the engine rows_per_file = 1
    (M files of one row): fvu = sum (x_hat - x)^2 / sum (x - x.mean(0))^2.  With rows_per_file = 0 the engine takes the batch for ONE
    file (engine.hip: T_rows = M, B = 1): the variance around that file's own mean is 0, topk_finalize_kernel replaces it by 1 like
    the reference (:105-106), and fvu is the plain sum of squared residuals.  The 3-D form is held to the oracle."""
    d, n, k, B, T = 256, 1024, 8, 3, 40
    sae, sd = _topk(d, n, k, 11)
    x3 = _x(B, T, d, 12)
    x2 = x3.reshape(B * T, d)
    out2 = sae(x2.cuda())
    assert out2.sae_out.shape == (B * T, d) and out2.encoded.top_indices.shape == (B * T, k)
    xd, xh = x2.double(), out2.sae_out.cpu().double()
    l2 = ((xh - xd) ** 2).sum().item()
    assert float(out2.fvu) == pytest.approx(l2 / ((xd - xd.mean(0)) ** 2).sum().item(), rel=5e-3)
    # the engine's own rows_per_file = 0
    sae._eng.set_topk_options(float("inf"), 0)
    sae._eng.eval(x2.cuda())
    assert float(sae._eng.metrics()[0]) == pytest.approx(l2, rel=5e-3)
    out3 = sae(x3.cuda())
    ref = O.topk_forward(x3, sd["encoder.weight"], sd["encoder.bias"], sd["W_dec"], sd["b_dec"], k, stable_ties=True)
    assert float(out3.fvu) == pytest.approx(ref["fvu"].item(), rel=5e-3)
    assert np.array_equal(_bits(out3.sae_out.reshape(-1, d)), _bits(out2.sae_out))


def test_l1_input_forms():
    """A CPU tensor, a float64 tensor and a non-contiguous view give the latent of the plain float32 CUDA call to the bit (_flat moves,
    narrows and packs them).  So do float16 and bfloat16 inputs against their own float32 widening: the engine converts every input
    type to the bf16 GEMM operand on load (prep_x: T -> float -> bf16, and the widening is exact), so the two operands are the same
    bits -- equality, not one bf16 ulp."""
    d, n, rows = 384, 768, 100
    sae = _l1_fixed_point(d, n, 13)
    wide = torch.randn(rows, 2 * d, generator=torch.Generator().manual_seed(14))
    x = wide[:, ::2].contiguous()
    base = sae.encode(x.cuda()).latent
    assert base.shape == (rows, n) and float((base > 0).float().mean()) > 0.01
    forms = {"cpu": x, "float64": x.double().cuda(), "strided": wide.cuda()[:, ::2], "strided cpu": wide[:, ::2]}
    assert not forms["strided"].is_contiguous()
    for name, xf in forms.items():
        assert np.array_equal(_bits(sae.encode(xf).latent), _bits(base)), name
    for dt in (torch.float16, torch.bfloat16):
        x16 = x.to(dt).cuda()
        assert np.array_equal(_bits(sae.encode(x16).latent), _bits(sae.encode(x16.float()).latent)), dt


def test_topk_rows_with_fewer_than_k_positives():
    """encoder.bias = -1, b_dec = 0: an all-zero row has no positive pre-activation, a faint row a handful.  The raw selection is
    checked BEFORE anything gathers with it: every index in [0, n) and distinct within its row."""
    d, n, k, rows = 256, 1024, 16, 64
    sae, sd = _topk(d, n, k, 15)
    sd["encoder.bias"] = torch.full((n,), -1.0)
    sd["b_dec"] = torch.zeros(d)
    sae.load_state_dict(sd)
    x = 4.0 * torch.randn(rows, d, generator=torch.Generator().manual_seed(16))
    zero_rows, faint_rows = [3, 40], [5, 41]
    x[zero_rows] = 0
    x[faint_rows] *= 0.17
    pre = torch.relu(x @ sd["encoder.weight"].t() - 1.0)
    npos = (pre > 0).sum(1)
    assert (npos[faint_rows] > 0).all() and (npos[faint_rows] < k).all() and (npos[[0, 1, 2]] > k).all()
    eng = sae._ensure(rows)
    eng.eval(x.cuda())
    idx = eng.topk_indices_tensor(rows, sae.device).cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == (rows, k)
    assert idx.min() >= 0 and idx.max() < n
    srt = np.sort(idx, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    enc = sae.encode(x)
    assert enc.top_indices.min() >= 0 and enc.top_indices.max() < n
    assert (enc.top_acts[zero_rows] == 0).all()
    faint = (enc.top_acts[faint_rows] > 0).sum(1)      # (about npos: a pre-activation next to 0 may fall either way in bf16)
    assert (faint > 0).all() and (faint < k).all() and (enc.top_acts >= 0).all()
    xh = sae.decode(enc.top_acts[zero_rows], enc.top_indices[zero_rows])
    assert not _bits(xh).any()                     # b_dec = +0.0, bit for bit


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_colmax_at_n_p_384(variant):
    """n = 300 (n_p = 384, an odd multiple of 128), 200 rows in a 300-row context: latent_colmax() and the colmax row of eval_into()
    are the column maxima of the latent of the same forward, to the bit, and eval_into leaves the neighbouring rows alone.  (The launch
    of sae_latent_colmax used to cover columns 384..511 too: reads of the next row, atomics past the zeroed scratch -- nothing an
    output shows; this pins the answers at the shape.)"""
    from freud_amd.engine import NUM_METRICS, SaeEngine
    n, M = 300, 200
    if variant == "l1":
        d = 200
        eng = SaeEngine(variant="l1", d_model=d, n_dict=n, max_rows=300)
        W, b = R.make_weights("l1", d, n, 17)
        eng.set_params({"decoder.weight": np.ascontiguousarray(W.T), "encoder_bias": np.full(n, -0.2, np.float32)})
    else:
        d = 256
        eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=300, k=8, optimizer="adam")
        W, b = R.make_weights("topk", d, n, 17)
        eng.set_params({"encoder.weight": W, "encoder.bias": np.zeros(n, np.float32), "W_dec": W, "b_dec": b})
        eng.set_topk_options(float("inf"), 0)
    x = torch.randn(M, d, generator=torch.Generator().manual_seed(18)).cuda()

    def latent_max():
        ptr, ld = eng.latent_buffer()
        assert ld == 384

        class _Alias:
            __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}

        lat = torch.as_tensor(_Alias(), device="cuda").view(torch.bfloat16)[:, :n].float()
        return lat.max(0).values.cpu().numpy()

    eng.eval(x)
    cm = eng.latent_colmax()
    want = latent_max()
    assert (want > 0).sum() > n // 4 and np.array_equal(cm.view(np.uint32), want.view(np.uint32))
    rows = torch.full((3, n), R.SENTINEL, device="cuda")
    metrics = torch.zeros(NUM_METRICS, device="cuda")
    eng.eval_into(x, metrics, rows[1])
    torch.cuda.synchronize()
    want2 = latent_max()
    got = rows.cpu().numpy()
    assert np.array_equal(got[1].view(np.uint32), want2.view(np.uint32))
    assert np.array_equal(eng.latent_colmax().view(np.uint32), got[1].view(np.uint32))
    assert (got[[0, 2]].view(np.uint32) == np.float32(R.SENTINEL).view(np.uint32)).all()
    eng.close()
