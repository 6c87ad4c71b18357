"""Golden vectors of the file features: the REAL reference `top_activations_for_audio` (src/utils/activations.py:135-209) on CPU.

Run in the build container only (needs /root/reference; only the .npz files it writes are kept):

    python tests/golden/make_file_features_golden.py

It reuses make_golden.py's stubs of the absent third-party imports.  The function wants an audio array and a Whisper cache; this
project runs neither, so it gets a stand-in cache (model_name, device, a forward() that does nothing, preset .activations), the
mel helpers of the imported module are replaced by no-ops, and the audio array is a zero array whose LENGTH makes the reference's
own activation_length_from_audio_array yield the wanted trim.

file_features_raw.npz: 6 files x T=12 x d=10 without an SAE.  Every frame holds 10 DISTINCT multiples of 1/8 (exact in fp16), so
that torch.topk's order among equal values of one frame never decides anything; planted on top: equal maxima of two columns at
different frames (the earlier frame must come first), a repeated maximum inside a file, an all-negative column; trims below, at
and above T and a one-frame file; top_n in {1, 4, 10, 16}.  The reference cannot answer top_n = 16 > d (its per-frame
activations.topk(top_n) raises), so that case stores the reference's longest possible list, the one of top_n = d, with -1 padding:
what a reader with more slots than columns has to give.

file_features_l1.npz / file_features_topk.npz: the reference's own L1AutoEncoder / TopKAutoEncoder (d=32, n=128, k=8, fp32 on
CPU; the L1 bias near -1.2 so that few latents are positive per frame), 5 files x T=60, top_n in {1, 5, 40}.  Recorded: the
dense trimmed latent of every file (zero beyond the trim) and the reference's answers.  The reference pads a short answer with zero-valued latents that torch.topk picks among ties; n_positive is
the length of the positive prefix of each answer -- the only part a reader has to reproduce.

Per answer: the latent indices (-1 padding), and from the series the reference returns for each of them its maximum and the first
frame of that maximum.  Asserted here: no two distinct columns share a value at the same frame of any file (SAE cases: a positive
value; zeros tie by construction), so no stored answer depends on torch's order within a frame.  Data only.
"""
import copy
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
SR = 16000

F_RAW, T_RAW, D_RAW = 6, 12, 10
LENGTHS_RAW = np.array([12, 7, 20, 3, 12, 1], dtype=np.int32)      # 20 > T is capped by the slice
TOPS_RAW = [1, 4, 10, 16]

F_SAE, T_SAE, D_SAE, N_SAE, K_SAE = 5, 60, 32, 128, 8
LENGTHS_SAE = np.array([60, 45, 80, 7, 1], dtype=np.int32)
TOPS_SAE = [1, 5, 40]


def make_x():
    g = np.random.default_rng(5)
    grid = np.arange(-32, 33) / 8.0                                 # 65 multiples of 1/8 in [-4, 4]
    x = np.stack([[g.choice(grid, D_RAW, replace=False) for _ in range(T_RAW)] for _ in range(F_RAW)]).astype(np.float32)
    x[0, 7, 2] = x[0, 3, 6] = 5.5          # equal maxima of two columns at different frames: column 6 (frame 3) before column 2
    x[1, 2, 1] = x[1, 5, 1] = 6.25         # a repeated maximum inside a file (first frame 2)
    x[1, 9, 4] = 9.0                       # beyond the trim of file 1 (L = 7): must be ignored
    x[:, :, 8] = -np.abs(x[:, :, 8]) - 4.125        # an all-negative column, below the grid: distinct within every frame still
    x[4, 0, 3] = x[4, 11, 5] = 4.75        # equal maxima at the first and the last frame
    return x


def assert_no_frame_ties(dense, lengths, positive_only):
    for f in range(dense.shape[0]):
        for t in range(min(int(lengths[f]), dense.shape[1])):
            row = dense[f, t]
            if positive_only:
                row = row[row > 0]
            assert len(np.unique(row)) == len(row), f"file {f} frame {t}: two columns share a value"


class _Cache:
    """What top_activations_for_audio reads of a WhisperActivationCache."""
    model_name = "tiny"
    device = "cpu"

    def __init__(self, activations):
        self.activations = activations

    def forward(self, mel):
        return None


def answers(RA, acts, lengths, sae, tops, longest=None):
    """-> rows of (file, top_n, indices, values, frames) from the reference's function; acts [F, T, d]."""
    rows = []
    for f in range(acts.shape[0]):
        audio = np.zeros(int(lengths[f]) * 320 + 100, np.float32)           # int(len / 16000 / 0.02) == lengths[f]
        assert RA.activation_length_from_audio_array(audio) == int(lengths[f])
        for top_n in tops:
            ask = top_n if longest is None else min(top_n, longest)
            # (a fresh copy per call: every L1 forward renormalises the decoder in place, l1autoencoder.py:71-73, and a second
            # pass over already normalised columns moves some weights by an ulp)
            idx, series = RA.top_activations_for_audio(audio, _Cache(acts[f:f + 1].clone()), copy.deepcopy(sae), ask)
            L = min(int(lengths[f]), acts.shape[1])
            series = [s.reshape(-1) for s in series]                        # (TopK squeezes a one-frame series to a scalar)
            assert all(s.shape == (L,) for s in series)
            rows.append(dict(file=f, top_n=top_n, idx=[int(i) for i in idx], values=[float(s.max()) for s in series],
                             frames=[int(s.argmax()) for s in series]))
    return rows


def pack(rows, width):
    out = {}
    for k, fill, dt in (("idx", -1, np.int64), ("values", np.nan, np.float32), ("frames", -1, np.int64)):
        out["case_" + k] = np.array([r[k] + [fill] * (width - len(r[k])) for r in rows], dtype=dt)
    out["case_file"] = np.array([r["file"] for r in rows])
    out["case_top_n"] = np.array([r["top_n"] for r in rows])
    return out


def raw_case(RA):
    x = make_x()
    assert_no_frame_ties(x, LENGTHS_RAW, positive_only=False)
    try:
        RA.top_activations_for_audio(np.zeros(12 * 320 + 100, np.float32), _Cache(torch.from_numpy(x[:1])), None, 16)
        raise AssertionError("the reference answered top_n > d: record its own answer instead of the top_n = d list")
    except RuntimeError:
        pass
    rows = answers(RA, torch.from_numpy(x), LENGTHS_RAW, None, TOPS_RAW, longest=D_RAW)
    # what was planted shows in the reference's answers
    first = {(r["file"], r["top_n"]): r for r in rows}
    assert first[(0, 4)]["idx"][:2] == [6, 2] and first[(0, 4)]["frames"][:2] == [3, 7]
    assert first[(1, 1)]["idx"] == [1] and first[(1, 1)]["frames"] == [2]
    assert first[(4, 4)]["idx"][:2] == [3, 5] and first[(4, 10)]["idx"][-1] == 8
    np.savez_compressed(os.path.join(OUT, "file_features_raw.npz"), x=x, lengths=LENGTHS_RAW,
                        filenames=np.array([f"f{i}.flac" for i in range(F_RAW)]), **pack(rows, max(TOPS_RAW)))
    print(f"file_features_raw.npz: {len(rows)} (file, top_n) answers")


def sae_case(RA, kind):
    from src.models.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
    from src.models.l1autoencoder import L1AutoEncoder
    from src.models.topkautoencoder import TopKAutoEncoder
    torch.manual_seed(17 if kind == "l1" else 18)
    x = torch.randn(F_SAE, T_SAE, D_SAE)
    if kind == "l1":
        sae = L1AutoEncoder(D_SAE, L1AutoEncoderConfig(n_dict_components=N_SAE))
        sae.encoder_bias.data = -1.2 + 0.05 * torch.randn(N_SAE)      # sparse: the short files have fewer positive latents than slots
    else:
        sae = TopKAutoEncoder(D_SAE, TopKAutoEncoderConfig(n_dict_components=N_SAE, k=K_SAE))
        sae.encoder.bias.data = 0.05 * torch.randn(N_SAE)
        sae.b_dec.data = 0.05 * torch.randn(D_SAE)
    dense = np.zeros((F_SAE, T_SAE, N_SAE), np.float32)
    with torch.no_grad():
        for f in range(F_SAE):
            L = min(int(LENGTHS_SAE[f]), T_SAE)
            enc = copy.deepcopy(sae).forward(x[f:f + 1]).encoded
            if kind == "l1":
                dense[f, :L] = enc.latent[0, :L].numpy()
            else:
                full = torch.zeros(T_SAE, N_SAE).scatter_(1, enc.top_indices[0], enc.top_acts[0])
                dense[f, :L] = full[:L].numpy()
    assert_no_frame_ties(dense, LENGTHS_SAE, positive_only=True)
    rows = answers(RA, x, LENGTHS_SAE, sae, TOPS_SAE)
    n_pos = []
    for r in rows:
        pos = [v > 0 for v in r["values"]]
        m = sum(pos)
        assert pos == [True] * m + [False] * (len(pos) - m), "the reference's fillers come after its positive entries"
        assert all(v == 0 for v in r["values"][m:])
        f, L = r["file"], min(int(LENGTHS_SAE[r["file"]]), T_SAE)
        assert m == min(r["top_n"], int((dense[f, :L].max(0) > 0).sum())), "the positive prefix is complete"
        n_pos.append(m)
    assert any(m < r["top_n"] for m, r in zip(n_pos, rows)), "no case with fewer positive latents than slots"
    np.savez_compressed(os.path.join(OUT, f"file_features_{kind}.npz"), dense=dense, lengths=LENGTHS_SAE, k=K_SAE,
                        case_n_positive=np.array(n_pos), **pack(rows, max(TOPS_SAE)))
    print(f"file_features_{kind}.npz: {len(rows)} (file, top_n) answers, positive prefixes {min(n_pos)}..{max(n_pos)}")


def main():
    sys.path.insert(0, OUT)
    from make_golden import install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    from src.utils import activations as RA
    RA.get_mels_from_np_array = lambda device, audio, n_mels: None
    RA.get_n_mels = lambda name: 80
    raw_case(RA)
    sae_case(RA, "l1")
    sae_case(RA, "topk")


if __name__ == "__main__":
    main()
