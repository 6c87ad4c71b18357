"""The models, frames and engine drivers that the GPU tests of the frontier family share (tests/test_sparsity_frontier_gpu.py,
test_pursuit_gpu.py, test_refit_gpu.py): every builder is seeded and draws its random numbers in a fixed order, so a case is the same
frames in whichever module it runs.  Files of T = 37 frames, 5 files, unless a caller says otherwise."""
import numpy as np
import torch

from freud_amd import engine as E
from freud_amd import sparsity_frontier as SF
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder

F, T = 5, 37


def l1_model(n, seed, bias, d=256):
    """Every entry of a column is +-1/16: at d = 256 a column's norm is exactly 1, the in-place renormalisation of every L1 forward
    is a bit-exact fixed point and the operand rows are the columns themselves.  -> (sae, the operand rows [n, d], None)."""
    g = np.random.default_rng(seed)
    W = np.where(g.random((d, n)) < 0.5, np.float32(-1 / 16), np.float32(1 / 16)).astype(np.float32)
    sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=1500)
    b = np.broadcast_to(np.asarray(bias, np.float32), (n,)).copy()
    sae.load_state_dict({"decoder.weight": torch.from_numpy(W), "encoder_bias": torch.from_numpy(b)})
    return sae, np.ascontiguousarray(W.T), None


def topk_model(d, n, k, seed, bias=None, multi_topk=False):
    """A tied dictionary: unit decoder rows (a seeded Linear's, normalised), the encoder their copy, a random b_dec.
    -> (sae, the bf16-valued operand rows [n, d], b_dec)."""
    torch.manual_seed(seed)
    W = torch.nn.Linear(d, n).weight.data.clone()
    W /= W.norm(dim=1, keepdim=True) + 1e-7
    b_dec = torch.randn(d, generator=torch.Generator().manual_seed(seed + 1)) * 0.3
    sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k, multi_topk=multi_topk), max_rows=1500)
    sae.load_state_dict({"W_dec": W.clone(), "b_dec": b_dec, "encoder.weight": W.clone(),
                         "encoder.bias": torch.full((n,), float(0.0 if bias is None else bias))})
    return sae, W.to(torch.bfloat16).float().numpy(), b_dec.numpy()


def planted(w_op, b, seed, files=F, rows_per_file=T, nplant=6, sigma=0.044):
    """Frames built from the dictionary: b (None: 0) + nplant decoder rows with amplitudes 8 * 0.6^i (+-10 %) + a little noise.  The
    curve falls in a few large steps (to 36 %, 14 %, 6 % of e_0), so the thresholds are crossed far from any rounding, and the
    cross-talk of the tied encoder then picks latents that RAISE the error again: e_s is not monotone on any of these frames."""
    g = np.random.default_rng(seed)
    n, d = w_op.shape
    bb = np.zeros(d) if b is None else b
    x = np.tile(bb, (files * rows_per_file, 1)) + sigma * g.normal(size=(files * rows_per_file, d))
    for r in range(files * rows_per_file):
        js = g.permutation(n)[:nplant]
        a = 8 * 0.6 ** np.arange(nplant) * (1 + 0.1 * g.uniform(-1, 1, nplant))
        x[r] += a @ w_op[js]
    return x.astype(np.float32).reshape(files, rows_per_file, d)


def data(d, seed, scale=None, files=F):
    x = np.random.default_rng(seed).normal(0, 1, (files, T, d)).astype(np.float32)
    if scale is not None:
        x *= np.asarray(scale, np.float32)[:, None, None]
    return x


def collect(sae, x, K, batch):
    """The slots of every row of x (a CUDA tensor [F, T, d]) by the engine's own collect: (vals [F*T, K], idx [F*T, K], stats)."""
    Fn, Tn, _ = x.shape
    eng = sae._ensure(batch * Tn)
    vals = torch.empty(Fn, Tn, K, dtype=torch.float32, device="cuda")
    idx = torch.empty(Fn, Tn, K, dtype=torch.int64, device="cuda")
    stats = torch.zeros(8, dtype=torch.int64, device="cuda")
    for f0 in range(0, Fn, batch):
        eng.collect_files(x[f0:f0 + batch].contiguous(), K, vals[f0:f0 + batch], idx[f0:f0 + batch], stats)
    torch.cuda.synchronize()
    return vals.cpu().numpy().reshape(Fn * Tn, K), idx.cpu().numpy().reshape(Fn * Tn, K), stats.cpu().numpy()


def frontier(sae, x, K, taus, batch, lengths=None):
    """The engine calls over x (a CUDA tensor [F, T, d]) in batches of `batch` files -> (SparsityFrontier, the block's bytes)."""
    Fn, Tn, d = x.shape
    eng = sae._ensure(batch * Tn)
    tau = SF.check_thresholds(taus)
    block = torch.zeros(E.frontier_layout(tau.size, K, d)["bytes"], dtype=torch.uint8, device="cuda")
    lens = torch.from_numpy(np.asarray(lengths, np.int32)).cuda() if lengths is not None else None
    for f0 in range(0, Fn, batch):
        eng.frontier_files(x[f0:f0 + batch].contiguous(), K, tau, block, lens[f0:f0 + batch] if lens is not None else None)
    torch.cuda.synchronize()
    host = block.cpu().numpy()
    return SF.SparsityFrontier.from_block(host, K, tau, d), host.tobytes()


def counted_rows(Fn, Tn, lengths):
    if lengths is None:
        return np.ones(Fn * Tn, bool)
    return (np.arange(Tn)[None, :] < np.minimum(np.asarray(lengths), Tn)[:, None]).reshape(-1)
