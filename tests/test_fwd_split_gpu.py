"""The fused d = 384 forward on encoder and decoder waves (fwd_split.h, FREUD_FWD=3) against the second decomposition
(fwd_fused2.h, FREUD_FWD=2): the same arithmetic in the same order, so everything a training step leaves behind must be
BITWISE equal -- the bf16 latent after one step; parameters, both optimizer moments and the logged metrics after three."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 384


def _no_minus_one(x):
    """bf16 x in which no entry reads -1.0 (a product of random factors can round to it): such entries move to the next bf16 below."""
    x = x.clone()
    x[x == -1.0] = -1.0078125
    return x


def _inputs(M, n, dtype, plant):
    g = torch.Generator().manual_seed(1000 * M + n)
    W = torch.empty(D, n)
    torch.nn.init.orthogonal_(W, generator=g)
    b = 0.01 * torch.randn(n, generator=g)
    x = _no_minus_one(((torch.relu(torch.randn(M, 32, generator=g)) * 0.1) @ torch.randn(32, D, generator=g)).to(torch.bfloat16))
    if plant is not None:
        x[plant] = -1.0
    assert int((x == -1.0).sum()) == (0 if plant is None else 1)
    return W, b, x.to(dtype)


def _latent(eng, M, n):
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}

    torch.cuda.synchronize()
    return torch.as_tensor(_Alias(), device="cuda")[:, :n].cpu().numpy().copy()


def _run(monkeypatch, fwd, W, b, xd, M, n):
    from freud_amd.engine import SaeEngine
    monkeypatch.setenv("FREUD_FWD", fwd)
    eng = SaeEngine(variant="l1", d_model=D, n_dict=n, max_rows=M, optimizer="radam", recon_alpha=1e4)
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": b.numpy()})
    eng.step(xd, 4e-4)
    latent = _latent(eng, M, n)
    eng.step(xd, 4e-4)
    eng.step(xd, 4e-4)
    _, m1, m2 = eng.get_opt_state()
    out = (latent, eng.get_params(), m1, m2, eng.metrics().copy())
    eng.close()
    return out


# (M, n, dtype of x, planted -1.0):
#   (128, 128)   one workgroup, one trip of the x4 unrolled tile loop
#   (256, 512)   16 tiles: the W^T ring wraps four times, the 8-tile bias ring twice
#   (200, 256)   a full workgroup and a ragged one: the PAD instantiation and its row masking
#   (1024, 1024) several workgroups per launch
#   fp32 x       the prep_x path: the residual reads x from memory, nothing aliases the GEMM operand
#   planted      a single -1.0 in the second of two workgroups' blocks: one block takes the masked residual, the other the lean one
CASES = [
    pytest.param(128, 128, torch.bfloat16, None, id="128x128"),
    pytest.param(256, 512, torch.bfloat16, None, id="256x512"),
    pytest.param(200, 256, torch.bfloat16, None, id="200x256-ragged"),
    pytest.param(1024, 1024, torch.bfloat16, None, id="1024x1024"),
    pytest.param(256, 512, torch.float32, None, id="256x512-fp32"),
    pytest.param(256, 512, torch.bfloat16, (131, 77), id="256x512-one-masked-entry"),
]


@pytest.mark.parametrize("M,n,dtype,plant", CASES)
def test_split_forward_is_bitwise_the_second_decomposition(monkeypatch, M, n, dtype, plant):
    W, b, x = _inputs(M, n, dtype, plant)
    xd = x.cuda()
    ref = _run(monkeypatch, "2", W, b, xd, M, n)
    got = _run(monkeypatch, "3", W, b, xd, M, n)
    assert ref[0].any(), "the latent of the reference variant is all zero: the case checks nothing"
    assert np.array_equal(ref[0], got[0]), ("latent", int((ref[0] != got[0]).sum()))
    for k in ref[1]:
        assert np.array_equal(ref[1][k], got[1][k]), (k, "params", np.abs(ref[1][k] - got[1][k]).max())
        assert np.array_equal(ref[2][k], got[2][k]), (k, "first moment")
        assert np.array_equal(ref[3][k], got[3][k]), (k, "second moment")
    assert np.array_equal(ref[4], got[4]), ("metrics", ref[4], got[4])
