"""Golden vectors of the feature index queries: the REAL reference `top_activations` (src/utils/activations.py:61-132) over an
"indexed" loader, i.e. through its own activation_tensor_from_indexed (activations.py:41-58), on CPU.

Run in the build container only (needs /root/reference; only the .npz it writes is kept):

    python tests/golden/make_feature_index_golden.py

It reuses make_golden.py's stubs of the absent third-party imports and make_search_golden.py's torchaudio stand-in, whose load() /
info() give every file name a duration so that trim_activation computes the reference's own trim lengths.

Case written (feature_index.npz): a hand-made indexed store of 7 files x T = 12 frames x K = 3 slots over n = 10 latents, the
indices of every row distinct, about a third of the slots +0.0, with planted cases -- equal maxima across files (latent 0), a
repeated maximum inside a file (latent 1), a file that never fires (file 4), a latent nobody fires (latent 9: it appears only in
zero-valued slots), a maximum beyond a file's trim (latent 4, file 1), negative values (latent 3) -- and trim lengths below, at
and above T; top_activations for every latent with n_files in {1, 5, 10 > 7}, abs on / off, without a filter, with a min_val and
with a max_val below every fired value (only silent files remain), return_max_per_file on.  Data only.
"""
import itertools
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
SR = 16000

N_FILES, T, K, N = 7, 12, 3, 10
LENGTHS = np.array([12, 7, 12, 20, 3, 12, 1], dtype=np.int32)     # trim lengths (frames); 20 > T is capped by the slice
MIN_VAL, MAX_VAL = 0.5, 0.01
PAD = 10


def _put(values, indices, f, t, latent, value):
    """Make `latent` a slot of row (f, t) with `value`, keeping the row's indices distinct."""
    row = indices[f, t]
    q = int(np.flatnonzero(row == latent)[0]) if (row == latent).any() else 0
    indices[f, t, q] = latent
    values[f, t, q] = value


def make_store():
    g = np.random.default_rng(11)
    indices = np.stack([np.stack([g.permutation(N - 1)[:K] for _ in range(T)]) for _ in range(N_FILES)]).astype(np.int64)
    values = (np.round(np.abs(g.normal(0, 1, (N_FILES, T, K))) * 8) / 8 + 0.125).astype(np.float32)      # coarse: many exact ties
    values[g.random((N_FILES, T, K)) < 0.33] = 0.0                                                       # a third of the slots are zero
    values[indices == 3] *= -1.0                                      # latent 3 holds negative values (abs mode)
    values[values == 0] = 0.0                                         # zero slots are +0.0, as a collection writes its padding
    values[4] = 0.0                                                   # a file that never fires
    indices[5, :, 2] = 9                                              # latent 9 (never drawn above): zero-valued slots only
    values[5, :, 2] = 0.0
    _put(values, indices, 0, 3, 0, 4.0)                               # equal maxima across files (latent 0)
    _put(values, indices, 2, 5, 0, 4.0)
    _put(values, indices, 1, 2, 1, 3.5)                               # a repeated maximum inside a file (latent 1)
    _put(values, indices, 1, 6, 1, 3.5)
    _put(values, indices, 1, 8, 4, 9.0)                               # a maximum beyond the trim (file 1: L = 7)
    _put(values, indices, 3, 9, 3, -6.0)                              # negative abs maxima late in files whose trim keeps them
    _put(values, indices, 5, 10, 3, -7.0)
    assert all(len(set(indices[f, t])) == K for f in range(N_FILES) for t in range(T))
    assert not ((indices == 9) & (values != 0)).any() and not (values[4] != 0).any()
    return values, indices


class _Loader:
    """What top_activations reads from an "indexed" dataloader (activations.py:94-101): batches of 3 files."""
    activation_type = "indexed"

    def __init__(self, values, indices, names):
        self.values, self.indices, self.names = torch.from_numpy(values), torch.from_numpy(indices), names

    def __iter__(self):
        for i in range(0, len(self.names), 3):
            yield self.values[i:i + 3], self.indices[i:i + 3], list(self.names[i:i + 3])


def main():
    sys.path.insert(0, OUT)
    from make_golden import install_stubs
    install_stubs()
    names = [f"f{i}.flac" for i in range(N_FILES)]
    samples = {n: int(L) * 320 + 100 for n, L in zip(names, LENGTHS)}          # int(dur / 0.02) == L
    ta = types.ModuleType("torchaudio")
    ta.load = lambda fname: (torch.zeros(1, samples[os.path.basename(fname)]), SR)
    ta.info = lambda fname: types.SimpleNamespace(sample_rate=SR)
    sys.modules["torchaudio"] = ta
    sys.path.insert(0, REF)
    from src.utils import activations as RA

    values, indices = make_store()
    loader = _Loader(values, indices, names)
    rows = []
    for n_top, absm, (mn, mx) in itertools.product([1, 5, 10], [False, True], [(None, None), (MIN_VAL, None), (None, MAX_VAL)]):
        for j in range(N):
            pq, mpf = RA.top_activations(loader, j, n_top, mx, mn, absm, True)
            files = [names.index(p[0]) for p in pq]
            for p in pq:                                                     # the trimmed series the reference hands back
                f = names.index(p[0])
                assert p[1].shape[0] == min(int(LENGTHS[f]), T)
            pad = PAD - len(files)
            rows.append(dict(n_top=n_top, absolute=int(absm), min_val=np.nan if mn is None else mn, max_val=np.nan if mx is None else mx,
                             feature=j, files=files + [-1] * pad, values=[p[2] for p in pq] + [np.nan] * pad,
                             times=[p[3] for p in pq] + [np.nan] * pad, max_per_file=mpf))
    series = np.stack([RA.activation_tensor_from_indexed(loader.values, loader.indices, j).numpy() for j in range(N)])
    out = dict(values=values, indices=indices, lengths=LENGTHS, filenames=np.array(names), n_dict=np.int64(N), ref_series=series)
    for k in ("n_top", "absolute", "min_val", "max_val", "feature", "files", "values", "times", "max_per_file"):
        out["case_" + k] = np.array([r[k] for r in rows])
    np.savez_compressed(os.path.join(OUT, "feature_index.npz"), **out)
    print(f"feature_index.npz: {len(rows)} (case, latent) answers")


if __name__ == "__main__":
    main()
