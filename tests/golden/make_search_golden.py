"""Golden vectors of the feature search: the REAL reference `top_activations` (src/utils/activations.py:61-132) on CPU.

Run in the build container only (needs /root/reference; only the .npz it writes is kept):

    python tests/golden/make_search_golden.py

It reuses make_golden.py's stubs of the absent third-party imports and replaces the torchaudio stub with one whose
load() / info() give every file name a duration, so that trim_activation (activations.py:19-29) computes the reference's own
trim lengths; load() returns MONO audio [1, samples] (a two-channel tensor is averaged to 1-D there and audio.shape[1] fails).

Case written (search_raw.npz): a raw fp32 tensor shard of 7 files x T=12 frames x d=6 with planted ties -- equal maxima across
files, a repeated maximum inside a file, an all-zero file, negative values for the abs mode -- and trim lengths below, at and
above T; top_activations for every column with n_files in {1, 5, 10 > 7}, abs on / off, without and with min / max filters,
return_max_per_file on.

Cases written (search_l1.npz, search_topk.npz): the reference's own L1AutoEncoder / TopKAutoEncoder (d=32, n=128, k=8; the
weights recorded BEFORE the first encode, so a reader repeats the in-place renormalisation of l1autoencoder.py:71-73) encode
6 files x T=200 frames in fp32 on CPU; top_activations then runs over what collect_activations.py would store -- the dense L1
latent (activation_type "tensor") and TopK's (top_acts, top_indices) (activation_type "indexed", densified by the reference's own
activation_tensor_from_indexed, activations.py:41-58) -- for every latent with n_files in {1, 5, 8 > 6}, abs on / off, without
and with a min / max filter.  Also recorded: per (file, latent) the margin between the series maximum and the best OTHER frame,
so that a reader can tell where the first maximal frame is stable under bf16 rounding, and for TopK the (file, latent) pairs whose
top-k selection may flip under it at a frame that could set the file's maximum (a kept frame where the k-th and (k+1)-th
pre-activations are close, the latent lies between them and is within reach of the maximum).  Data only.
"""
import itertools
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
SR = 16000

N_FILES, T, D = 7, 12, 6
LENGTHS = np.array([12, 7, 12, 20, 3, 12, 1], dtype=np.int32)     # trim lengths (frames); 20 > T is capped by the slice


def make_x():
    g = np.random.default_rng(3)
    x = np.round(g.normal(0, 1, (N_FILES, T, D)) * 8) / 8                       # coarse values: many exact ties
    x = x.astype(np.float32)
    x[0, 3, 0] = x[2, 5, 0] = 4.0          # equal maxima across files (col 0)
    x[1, 2, 1] = x[1, 6, 1] = 3.5          # a repeated maximum inside a file (col 1)
    x[4] = 0.0                             # an all-zero file
    x[:, :, 2] = -np.abs(x[:, :, 2])       # all-negative column: abs mode ranks |a|, filters / reports the signed value
    x[3, 9, 3] = -6.0                      # negative abs maxima late in files whose trim keeps them (L = 20 -> 12, L = 12)
    x[5, 10, 3] = -7.0
    x[1, 8, 4] = 9.0                       # a maximum beyond the trim (file 1: L = 7) -- must be ignored
    x[6, 0, 5] = -2.0                      # a one-frame file
    return x


T_SAE, D_SAE, N_SAE, K_SAE = 200, 32, 128, 8
LENGTHS_SAE = np.array([200, 150, 200, 37, 260, 1], dtype=np.int32)
FLIP_TOL = 0.03


class _Loader:
    """What top_activations reads from a dataloader (activations.py:94-100): batches of 3 files, and activation_type."""

    def __init__(self, kind, items, names):
        self.activation_type, self.items, self.names = kind, items, names

    def __iter__(self):
        for i in range(0, len(self.names), 3):
            part = [it[i:i + 3] for it in self.items]
            yield (*part, list(self.names[i:i + 3]))


def sae_cases(RA, kind, names):
    from src.models.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
    from src.models.l1autoencoder import L1AutoEncoder
    from src.models.topkautoencoder import TopKAutoEncoder
    torch.manual_seed(7 if kind == "l1" else 8)
    F = len(names)
    x = torch.randn(F, T_SAE, D_SAE)
    if kind == "l1":
        sae = L1AutoEncoder(D_SAE, L1AutoEncoderConfig(n_dict_components=N_SAE))
        sae.encoder_bias.data = 0.05 * torch.randn(N_SAE)
    else:
        sae = TopKAutoEncoder(D_SAE, TopKAutoEncoderConfig(n_dict_components=N_SAE, k=K_SAE))
        sae.encoder.bias.data = 0.05 * torch.randn(N_SAE)
        sae.b_dec.data = 0.05 * torch.randn(D_SAE)
    weights = {k: v.detach().clone().numpy() for k, v in sae.state_dict().items()}
    with torch.no_grad():
        if kind == "l1":
            dense = torch.stack([sae.encode(x[f]).latent for f in range(F)])
            loader = _Loader("tensor", [dense], names)
        else:
            enc = [sae.encode(x[f]) for f in range(F)]
            acts, idx = torch.stack([e.top_acts for e in enc]), torch.stack([e.top_indices for e in enc])
            loader = _Loader("indexed", [acts, idx], names)
            dense = torch.stack([RA.activation_tensor_from_indexed(acts[f:f + 1], idx[f:f + 1], j)[0] for j in range(N_SAE)
                                 for f in range(F)]).reshape(N_SAE, F, T_SAE).permute(1, 2, 0)
    margin = np.full((F, N_SAE), np.inf, np.float32)
    for f in range(F):
        a = dense[f, : min(int(LENGTHS_SAE[f]), T_SAE)]
        if a.shape[0] > 1:
            am = a.argmax(0)
            other = a.clone()
            other[am, torch.arange(N_SAE)] = -np.inf
            margin[f] = (a.max(0).values - other.max(0).values).numpy()
    # TopK: (file, latent) pairs whose selection may flip under bf16 rounding -- at some kept frame the k-th and (k+1)-th
    # pre-activations are within 2 FLIP_TOL of each other and the latent's pre-activation lies in that band
    flip = np.zeros((F, N_SAE), bool)
    if kind == "topk":
        with torch.no_grad():
            for f in range(F):
                pre = sae.pre_acts(x[f, : min(int(LENGTHS_SAE[f]), T_SAE)])
                srt = pre.sort(dim=1, descending=True).values
                hi, lo = srt[:, K_SAE - 1:K_SAE], srt[:, K_SAE:K_SAE + 1]
                band = ((hi - lo) <= 2 * FLIP_TOL) & (pre >= lo - FLIP_TOL) & (pre <= hi + FLIP_TOL)
                top = dense[f, : pre.shape[0]].max(0).values          # ... and a flip there could change the file's maximum
                flip[f] = (band & (pre >= top - FLIP_TOL)).any(0).numpy()
    rows = []
    for n_top, absm, (mn, mx) in itertools.product([1, 5, 8], [False, True], [(None, None), (0.2, None), (None, 1.0)]):
        for j in range(N_SAE):
            pq, mpf = RA.top_activations(loader, j, n_top, mx, mn, absm, True)
            files = [names.index(p[0]) for p in pq]
            pad = 8 - len(files)
            rows.append(dict(n_top=n_top, absolute=int(absm), min_val=np.nan if mn is None else mn, max_val=np.nan if mx is None else mx,
                             feature=j, files=files + [-1] * pad, values=[p[2] for p in pq] + [np.nan] * pad,
                             times=[p[3] for p in pq] + [np.nan] * pad, max_per_file=mpf))
    out = dict(x=x.numpy(), lengths=LENGTHS_SAE, filenames=np.array(names), margin=margin, flip=flip, flip_tol=FLIP_TOL, k=K_SAE)
    out.update({"w_" + k: v for k, v in weights.items()})
    for k in ("n_top", "absolute", "min_val", "max_val", "feature", "files", "values", "times", "max_per_file"):
        out["case_" + k] = np.array([r[k] for r in rows])
    np.savez_compressed(os.path.join(OUT, f"search_{kind}.npz"), **out)
    print(f"search_{kind}.npz: {len(rows)} (case, latent) answers")


def main():
    sys.path.insert(0, OUT)
    from make_golden import install_stubs
    install_stubs()
    names = [f"f{i}.flac" for i in range(N_FILES)]
    samples = {n: int(L) * 320 + 100 for n, L in zip(names, LENGTHS)}          # int(dur / 0.02) == L
    sae_names = [f"s{i}.flac" for i in range(len(LENGTHS_SAE))]
    samples.update({n: int(L) * 320 + 100 for n, L in zip(sae_names, LENGTHS_SAE)})

    ta = types.ModuleType("torchaudio")
    ta.load = lambda fname: (torch.zeros(1, samples[os.path.basename(fname)]), SR)
    ta.info = lambda fname: types.SimpleNamespace(sample_rate=SR)
    sys.modules["torchaudio"] = ta
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    from src.utils import activations as RA
    from src.dataset.activations import MemoryMappedActivationDataLoader
    from freud_amd.loader import write_shards

    x = make_x()
    tmp = tempfile.mkdtemp()
    try:
        write_shards(tmp, "enc", x.reshape(N_FILES, -1), [T, D], filenames=names)
        dl = MemoryMappedActivationDataLoader(tmp, "enc", 3, 0)
        rows = []
        for n_top, absm, (mn, mx) in itertools.product([1, 5, 10], [False, True], [(None, None), (0.5, None), (None, 3.0), (-2.0, 4.0)]):
            for j in range(D):
                pq, mpf = RA.top_activations(dl, j, n_top, mx, mn, absm, True)
                files = [names.index(os.path.basename(p[0])) for p in pq]
                vals = [p[2] for p in pq]
                times = [p[3] for p in pq]
                pad = 10 - len(files)
                rows.append(dict(n_top=n_top, absolute=int(absm), min_val=np.nan if mn is None else mn, max_val=np.nan if mx is None else mx,
                                 feature=j, files=files + [-1] * pad, values=vals + [np.nan] * pad, times=times + [np.nan] * pad,
                                 max_per_file=mpf))
    finally:
        shutil.rmtree(tmp)
    out = dict(x=x, lengths=LENGTHS, filenames=np.array(names))
    for k in ("n_top", "absolute", "min_val", "max_val", "feature", "files", "values", "times", "max_per_file"):
        out["case_" + k] = np.array([r[k] for r in rows])
    np.savez_compressed(os.path.join(OUT, "search_raw.npz"), **out)
    print(f"search_raw.npz: {len(rows)} (case, feature) answers")
    sae_cases(RA, "l1", sae_names)
    sae_cases(RA, "topk", sae_names)


if __name__ == "__main__":
    main()
