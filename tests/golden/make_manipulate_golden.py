"""Golden vectors of the feature manipulation: the REAL reference `manipulate_latent` (src/utils/activations.py:212-296) on CPU.

Run in the build container only (needs /root/reference; only the .npz files it writes are kept):

    python tests/golden/make_manipulate_golden.py

It reuses make_golden.py's stubs of the absent third-party imports and the stand-in cache of make_file_features_golden.py, whose
forward() here returns an object with .text.  The function also wants a WhisperSubbedActivation: the stand-in's forward(mel,
decoded) RECORDS `decoded` -- the tensor this project owes the reference's user -- and returns an object with .text.  The audio
array is a zero array whose LENGTH makes the reference's own activation_length_from_audio_array yield the wanted trim.

manipulate_raw.npz: 3 files x T=60 x d=32 without an SAE; features {0, 13, 31}.
manipulate_l1.npz / manipulate_topk.npz: the reference's own L1AutoEncoder / TopKAutoEncoder (d=32, n=128, k=8, fp32 on CPU; the L1
bias near -1.2; the TopK biases: see LIVE below), 3 files x T=60 with trims {60, 45, 7}, factors {0, 1, 1.5, -2, 10}.  Planted through the encoder bias and checked
here: a feature that fires on most frames, one that fires on few, one that never fires, and for TopK one that is selected on some
frames and not on others.  Recorded per (feature, factor, file): the standard and manipulated tensors handed to whisper_subbed,
and the two trimmed series (zero beyond the trim); plus the weights, the inputs, the dense fp32 latent of every frame and the
decoder operand the reference decodes with (L1: the normalised decoder weight its forward leaves).  TopK also records `flagged`:
the frames where the gap between the k-th and (k+1)-th pre-activation is below 2^-6 -- a bf16 encoder may select differently
there.  That fraction is a condition: the generator walks seeds until it is below 10 %.  Data only.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

F, T, D, N, K = 3, 60, 32, 128, 8
LENGTHS = np.array([60, 45, 7], dtype=np.int32)
FACTORS = [0.0, 1.0, 1.5, -2.0, 10.0]
GAP = 2.0 ** -6
# TopK: 16 live latents whose encoder biases are spread evenly over [-1, 2.75], all others far below zero.  The k-th and (k+1)-th
# pre-activation of a frame are then about 0.25 apart and below 2 -- few frames fall within GAP, and a bf16 encoder (error about
# 2^-8 at these magnitudes) cannot order the others differently.
LIVE = np.arange(4, 128, 8)
LIVE_BIAS = np.linspace(-1.0, 2.75, 16).astype(np.float32)


class _Cache:
    """What manipulate_latent reads of a WhisperActivationCache."""
    model_name = "tiny"
    device = "cpu"

    def __init__(self, activations):
        self.activations = activations

    def forward(self, mel):
        return types.SimpleNamespace(text="baseline")


class _Subbed:
    """What manipulate_latent asks of a WhisperSubbedActivation: forward(mel, decoded); the decoded tensors are kept in call order
    (manipulated first, then standard: activations.py:280-281)."""

    def __init__(self):
        self.seen = []

    def forward(self, mel, decoded):
        self.seen.append(decoded.detach().clone())
        return types.SimpleNamespace(text="subbed")


def run(RA, x, sae, features):
    """-> standard [F, T, d], manipulated [nfeat, nfac, F, T, d], series / manipulated series [nfeat, (nfac,) F, T] zero-padded."""
    nf, nv = len(features), len(FACTORS)
    standard = np.zeros((F, T, x.shape[-1]), np.float32)
    manipulated = np.zeros((nf, nv, F, T, x.shape[-1]), np.float32)
    series = np.zeros((nf, F, T), np.float32)
    mseries = np.zeros((nf, nv, F, T), np.float32)
    for f in range(F):
        L = int(LENGTHS[f])
        audio = np.zeros(L * 320 + 100, np.float32)                         # int(len / 16000 / 0.02) == L
        assert RA.activation_length_from_audio_array(audio) == L
        for i, feat in enumerate(features):
            for v, factor in enumerate(FACTORS):
                sub = _Subbed()
                # (a fresh copy per call: every L1 forward renormalises the decoder in place, l1autoencoder.py:71-73)
                base, _mt, _st, pre, man = RA.manipulate_latent(audio, _Cache(x[f:f + 1].clone()), copy.deepcopy(sae), sub, int(feat), factor)
                assert (base is None) == (sae is None) and len(sub.seen) == 2
                m_dec, s_dec = (t.reshape(T, -1).numpy() for t in sub.seen)
                if i == 0 and v == 0:
                    standard[f] = s_dec
                assert np.array_equal(standard[f], s_dec), "the standard reconstruction does not depend on the edit"
                manipulated[i, v, f] = m_dec
                pre, man = pre.reshape(-1).numpy(), man.reshape(-1).numpy()
                assert pre.shape == (L,) and man.shape == (L,)
                series[i, f, :L], mseries[i, v, f, :L] = pre, man
    return standard, manipulated, series, mseries


def raw_case(RA):
    torch.manual_seed(31)
    x = torch.randn(F, T, D)
    features = np.array([0, 13, 31])
    standard, manipulated, series, mseries = run(RA, x, None, features)
    assert np.array_equal(standard, x.numpy())
    np.savez_compressed(os.path.join(OUT, "manipulate_raw.npz"), x=x.numpy(), lengths=LENGTHS, features=features,
                        factors=np.array(FACTORS, np.float32), standard_decoded=standard, manipulated_decoded=manipulated,
                        standard_activations=series, manipulated_activations=mseries)
    print("manipulate_raw.npz")


def sae_case(RA, kind, seed):
    """-> True when the fixture was written (TopK: the seed keeps the flagged fraction below 10 %)."""
    from src.models.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
    from src.models.l1autoencoder import L1AutoEncoder
    from src.models.topkautoencoder import TopKAutoEncoder
    torch.manual_seed(seed)
    x = torch.randn(F, T, D)
    MOST, FEW, NEVER, SOME = (5, 40, 77, 100) if kind == "l1" else (int(LIVE[15]), int(LIVE[4]), 77, int(LIVE[7]))
    if kind == "l1":
        sae = L1AutoEncoder(D, L1AutoEncoderConfig(n_dict_components=N))
        sae.encoder_bias.data = -1.2 + 0.05 * torch.randn(N)
        sae.encoder_bias.data[MOST] = 0.75
        sae.encoder_bias.data[NEVER] = -12.0
        features = np.array([MOST, FEW, NEVER])
    else:
        sae = TopKAutoEncoder(D, TopKAutoEncoderConfig(n_dict_components=N, k=K))
        sae.encoder.bias.data = -6.0 + 0.05 * torch.randn(N)
        sae.encoder.bias.data[torch.from_numpy(LIVE)] = torch.from_numpy(LIVE_BIAS)
        sae.b_dec.data = 0.05 * torch.randn(D)
        features = np.array([MOST, FEW, NEVER, SOME])
    dense = np.zeros((F, T, N), np.float32)
    extra = {}
    with torch.no_grad():
        m = copy.deepcopy(sae)
        if kind == "l1":
            dense[:] = m.forward(x).encoded.latent.numpy()
            extra = dict(W=sae.decoder.weight.detach().numpy(), b=sae.encoder_bias.detach().numpy(),
                         W_decode=m.decoder.weight.detach().numpy().copy())        # normalised in place by the forward
        else:
            pre = m.pre_acts(x)
            top = pre.topk(K + 1, dim=-1).values
            flagged = ((top[..., K - 1] - top[..., K]) < GAP).numpy()
            if flagged.mean() >= 0.10:
                return False
            enc = m.encode(x)
            dense[:] = torch.zeros(F, T, N).scatter_(2, enc.top_indices, enc.top_acts).numpy()
            extra = dict(W_enc=sae.encoder.weight.detach().numpy(), b_enc=sae.encoder.bias.detach().numpy(),
                         W_dec=sae.W_dec.detach().numpy(), b_dec=sae.b_dec.detach().numpy(), k=K, flagged=flagged)
    fired = (dense > 0).reshape(F * T, N).mean(0)
    if not (fired[MOST] > 0.5 and 0 < fired[FEW] < 0.25 and fired[NEVER] == 0):
        return False
    if kind == "topk" and not 0.15 < fired[SOME] < 0.85:
        return False
    standard, manipulated, series, mseries = run(RA, x, sae, features)
    for i, feat in enumerate(features):                                       # the series ARE the latent's column
        for f in range(F):
            L = int(LENGTHS[f])
            assert np.array_equal(series[i, f, :L], dense[f, :L, feat])
    np.savez_compressed(os.path.join(OUT, f"manipulate_{kind}.npz"), x=x.numpy(), lengths=LENGTHS, features=features,
                        factors=np.array(FACTORS, np.float32), dense=dense, standard_decoded=standard, manipulated_decoded=manipulated,
                        standard_activations=series, manipulated_activations=mseries, **extra)
    print(f"manipulate_{kind}.npz: seed {seed}, firing rates {[round(float(fired[j]), 3) for j in features]}"
          + (f", flagged {float(extra['flagged'].mean()):.3f}" if kind == "topk" else ""))
    return True


def main():
    sys.path.insert(0, OUT)
    from make_golden import install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    from src.utils import activations as RA
    RA.get_mels_from_np_array = lambda device, audio, n_mels: None
    RA.get_n_mels = lambda name: 80
    raw_case(RA)
    for kind, seed0 in (("l1", 41), ("topk", 43)):
        assert any(sae_case(RA, kind, seed) for seed in range(seed0, seed0 + 64)), f"{kind}: no seed gives the wanted fixture"


if __name__ == "__main__":
    main()
