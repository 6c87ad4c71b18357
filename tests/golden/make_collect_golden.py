"""Golden vectors of the feature collection: the REAL reference's encode() outputs, its activation_tensor_from_indexed
(src/utils/activations.py:41-58) and what its MemoryMappedActivationsDataset (src/dataset/activations.py:116-174) reads from a
store written by freud_amd.collect_features' own file writer.

Run in the build container only (needs /root/reference; only the .npz it writes is kept):

    python tests/golden/make_collect_golden.py

It reuses make_golden.py's stubs of the absent third-party imports.  Written (collect_features.npz), for a tiny TopKAutoEncoder
(d = 16, n = 64, k = 4) and a tiny L1AutoEncoder (d = 16, n = 64, stored with K = 12, so rows drop latents) on tie-free random input
of 3 files x T = 10 frames, in fp32 on CPU:

  topk_top_acts / topk_top_indices   the reference's encode() [F, T, k]
  l1_latent                          the reference's encode().latent [F, T, n]
  <kind>_store_values / _indices     the slots this project defines for those outputs (stable argsort of the latent, first K)
  <kind>_stats                       the eight statistics, counted with numpy (the largest dropped value as its bf16 pattern)
  <kind>_ref_activation_type / _ref_activation_shape / _ref_len / _ref_file0_values / _ref_file0_indices
                                     what the reference's dataset answered when pointed at the store written from those slots
  <kind>_ref_series                  activation_tensor_from_indexed of the stored tensors for every latent, [n, F, T]

Data only."""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

F, T, D, N, K_TOPK, K_L1 = 3, 10, 16, 64, 4, 12


def slots(latent, K):
    """[F, T, n] fp32 -> (values, indices) [F, T, K] and the statistics."""
    idx = np.argsort(-latent, axis=2, kind="stable")[:, :, :K]
    val = np.take_along_axis(latent, idx, 2).astype(np.float32)
    val[val == 0] = 0.0
    nnz = (latent > 0).sum(2)
    stored = np.minimum(nnz, K)
    srt = -np.sort(-latent, axis=2)
    cut = srt[:, :, K].max() if K < latent.shape[2] else 0.0                    # the largest dropped value (> 0 iff one was dropped)
    u = int(np.float32(max(cut, 0.0)).view(np.uint32))
    cut_bits = (u + 0x7FFF + ((u >> 16) & 1)) >> 16                             # as the bf16 pattern the engine reports
    stats = np.array([F * T, stored.sum(), (nnz - stored).sum(), (nnz > K).sum(), nnz.max(), cut_bits, 0, 0], np.int64)
    return val, idx.astype(np.int64), stats


def case(kind, RA, RD, CF, names, out):
    from src.models.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
    from src.models.l1autoencoder import L1AutoEncoder
    from src.models.topkautoencoder import TopKAutoEncoder
    torch.manual_seed(11 if kind == "l1" else 12)
    x = torch.randn(F, T, D)
    with torch.no_grad():
        if kind == "l1":
            sae = L1AutoEncoder(D, L1AutoEncoderConfig(n_dict_components=N))
            sae.encoder_bias.data = 0.05 * torch.randn(N)
            latent = torch.stack([sae.encode(x[f]).latent for f in range(F)]).numpy()
            out["l1_latent"] = latent
            K = K_L1
        else:
            sae = TopKAutoEncoder(D, TopKAutoEncoderConfig(n_dict_components=N, k=K_TOPK))
            sae.encoder.bias.data = 0.05 * torch.randn(N)
            enc = [sae.encode(x[f]) for f in range(F)]
            acts, tidx = torch.stack([e.top_acts for e in enc]), torch.stack([e.top_indices for e in enc])
            out["topk_top_acts"], out["topk_top_indices"] = acts.numpy(), tidx.numpy()
            latent = torch.zeros(F, T, N).scatter_(2, tidx, acts).numpy()
            K = K_TOPK
    for f in range(F):
        for t in range(T):
            pos = latent[f, t][latent[f, t] > 0]
            assert len(np.unique(pos)) == len(pos), "the input must be tie-free"
    val, idx, stats = slots(latent, K)
    tmp = tempfile.mkdtemp()
    try:
        w = CF.StoreWriter(tmp, "enc", names, T, K, N, variant=kind)
        CF.write_store([(0, val, idx)], w, lambda: stats)
        ds = RD.MemoryMappedActivationsDataset(tmp, "enc")
        a0, i0, name0 = ds[0]
        assert name0 == names[0]
        out[f"{kind}_ref_activation_type"] = np.array(ds.activation_type)
        out[f"{kind}_ref_activation_shape"] = np.array(list(ds.activation_shape), np.int64)
        out[f"{kind}_ref_len"] = np.int64(len(ds))
        out[f"{kind}_ref_file0_values"], out[f"{kind}_ref_file0_indices"] = a0.numpy().copy(), i0.numpy().copy()
        acts_all = torch.stack([ds[f][0] for f in range(F)])
        idx_all = torch.stack([ds[f][1] for f in range(F)])
        out[f"{kind}_ref_series"] = np.stack([RA.activation_tensor_from_indexed(acts_all, idx_all, j).numpy() for j in range(N)])
    finally:
        shutil.rmtree(tmp)
    out[f"{kind}_store_values"], out[f"{kind}_store_indices"] = val.reshape(F, T * K), idx.reshape(F, T * K)
    out[f"{kind}_stats"], out[f"{kind}_n"], out[f"{kind}_K"] = stats, np.int64(N), np.int64(K)


def main():
    sys.path.insert(0, OUT)
    from make_golden import install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    from src.utils import activations as RA
    from src.dataset import activations as RD
    from freud_amd import collect_features as CF
    names = [f"c{i}.flac" for i in range(F)]
    out = {"filenames": np.array(names)}
    case("topk", RA, RD, CF, names, out)
    case("l1", RA, RD, CF, names, out)
    np.savez_compressed(os.path.join(OUT, "collect_features.npz"), **out)
    print("collect_features.npz:", sorted(out))


if __name__ == "__main__":
    main()
