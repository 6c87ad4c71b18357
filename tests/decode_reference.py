"""Float64 reference and per-element error bound for the engine's decode (sae_decode: pad_latent_kernel, then the bf16 GEMM with the
EpiStoreF32 epilogue).  Shared by tests/test_decode_bound_cpu.py, tests/test_decode_gpu.py and tests/test_models_gpu.py.

The operation, from the operands as the engine holds them:

    A   = bf16(latent)                 a float32 latent is rounded to bf16, a bf16 latent is taken as is
    B   = bf16(W)  [n][d]              decoder.weight^T (L1) or W_dec (TopK), the fp32 master read AFTER the decode call
    out = bf16_round(acc) + b          acc = fp32 accumulation of the K = n_p products of a row of A and a column of B (the padding
                                       contributes zeros); b = b_dec (TopK) or nothing (L1)

The reference, in float64:  s = A @ B,  S = |A| @ |B|,  ref = s + b.

The bound, per element:     tol = 2^-8 |s|  +  n_p 2^-23 S  +  2^-22 (|s| + |b|)

  * bf16_round(acc) is within the bf16 unit round-off 2^-8 of acc (round to nearest would give 2^-9; 2^-8 also admits a truncating store);
  * an fp32 accumulation of K = n_p products in ANY order errs by at most (K - 1) u S; u = 2^-23, one ulp per add, covers accumulators
    that do not round to nearest inside the MFMA (the products of two bf16 numbers are exact in fp32);
  * the fp32 bias add costs 2^-24 (|s| + |b|); 2^-22 leaves room for the second-order terms of the two lines above.

Nothing in the bound is measured on the code under test.  It is about 4e-3 of |ref| at the median, so it sees a dropped K tile, a wrong
row or column, a missing bias and a missing rounding of either operand or of the output (tests/test_decode_bound_cpu.py holds it to
that: every such mutation must violate it on at least 10 % of the elements, a float32 emulation of the operation on none)."""
import numpy as np
import torch

SENTINEL = 12345.0
ONE_HOT_COLS = (0, 63, 64, 127)          # both sides of the first 64-column K tile boundary and of the first 128-column one
FIRST_ONE_HOT_ROW = 4                    # rows 4..7 are one-hot at ONE_HOT_COLS

# (variant, d, n, M, max_rows, engine keywords): tests/test_decode_gpu.py says which kernel and edge each one reaches
CASES = {
    "l1_384_1536_300": ("l1", 384, 1536, 300, 300, {}),
    "l1_512_1024_256": ("l1", 512, 1024, 256, 256, {}),
    "l1_500_1000_200": ("l1", 500, 1000, 200, 200, {}),
    "l1_500_1000_200_gemm128": ("l1", 500, 1000, 200, 200, {"force_gemm128": True}),
    "l1_200_300_77": ("l1", 200, 300, 77, 77, {}),
    "l1_fp8_384_1000_300": ("l1", 384, 1000, 300, 300, {"precision": "fp8"}),
    "topk_256_1024_256": ("topk", 256, 1024, 256, 256, {"k": 8}),
    "topk_200_1000_130": ("topk", 200, 1000, 130, 130, {"k": 8}),
    "topk_768_1536_100": ("topk", 768, 1536, 100, 100, {"k": 8}),
    "topk_256_1024_100_rows1500": ("topk", 256, 1024, 100, 1500, {"k": 8}),
}


def round_up(v, m):
    return (v + m - 1) // m * m


def padded_n(n, engine_kw=None):
    """n_p of the engine: the dictionary padded to 128 columns, to 256 in an fp8 context."""
    return round_up(n, 256 if (engine_kw or {}).get("precision", "bf16") != "bf16" else 128)


def bf16(a):
    """Round to nearest even to bf16, as float32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def as_f32(t):
    """A float32 numpy copy of a tensor (exact for bf16) or array."""
    if isinstance(t, torch.Tensor):
        return t.detach().float().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, np.float32)


def bits(a):
    return as_f32(a).view(np.uint32)


def make_weights(variant, d, n, seed):
    """W [n][d] = randn / sqrt(d) (row j is the direction of latent j) and b_dec = 0.05 randn (None for L1)."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(n, d, generator=g) / d ** 0.5).numpy()
    b = (0.05 * torch.randn(d, generator=g)).numpy() if variant == "topk" else None
    return W, b


def make_latent(M, n, seed):
    """float32 [M][n], about 3 % dense relu(randn); row 0 all zero, row 1 one-hot 1.0 at column n - 1, row 2 = -row 3, rows 4..7 one-hot
    1.0 at columns 0, 63, 64, 127."""
    assert M >= FIRST_ONE_HOT_ROW + len(ONE_HOT_COLS) and n > max(ONE_HOT_COLS)
    g = torch.Generator().manual_seed(seed)
    lat = torch.relu(torch.randn(M, n, generator=g)) * (torch.rand(M, n, generator=g) < 0.06)
    lat[0] = 0
    lat[1] = 0
    lat[1, n - 1] = 1.0
    lat[2] = -lat[3]
    for i, j in enumerate(ONE_HOT_COLS):
        lat[FIRST_ONE_HOT_ROW + i] = 0
        lat[FIRST_ONE_HOT_ROW + i, j] = 1.0
    return lat.numpy()


def one_hot_rows(n):
    """(row, column) of every one-hot row of make_latent."""
    return [(1, n - 1)] + [(FIRST_ONE_HOT_ROW + i, j) for i, j in enumerate(ONE_HOT_COLS)]


def decode_reference(latent, W, b, n_p):
    """latent: float32 (rounded to bf16 here) or a bf16 tensor (taken as is), [M][n]; W: the fp32 master [n][d]; b: [d] or None.
    -> (ref, tol), float64 [M][d]."""
    A = as_f32(latent) if isinstance(latent, torch.Tensor) and latent.dtype == torch.bfloat16 else bf16(as_f32(latent))
    A = A.astype(np.float64)
    B = bf16(W).astype(np.float64)
    bb = np.zeros(B.shape[1]) if b is None else np.asarray(b, np.float64)
    s = A @ B
    S = np.abs(A) @ np.abs(B)
    tol = 2.0 ** -8 * np.abs(s) + n_p * 2.0 ** -23 * S + 2.0 ** -22 * (np.abs(s) + np.abs(bb))
    return s + bb, tol


def on_bf16_grid(out, b):
    """Boolean [M][d]: the element is fl32(q + b) for a bf16 value q -- what `bf16_round(acc) + bias` stores, whatever acc was.  q is
    looked for among bf16(out - b) and its two bf16 neighbours (out - b, taken in float32, is within a few fp32 ulps of q).  Without a
    bias this says that the low 16 bits of the element are zero."""
    o = as_f32(out)
    bb = np.zeros(o.shape[1], np.float32) if b is None else np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        q = bf16(o - bb).view(np.uint32)
        ok = np.zeros(o.shape, bool)
        for step in (0, 0x10000, -0x10000):
            cand = (q.astype(np.int64) + step).astype(np.uint32).view(np.float32)
            ok |= (cand + bb).astype(np.float32) == o
    return ok


def violations(out, ref, tol, b=None):
    """Boolean [M][d]: the element is not finite, further than tol from ref, or not a bf16 value plus the bias b (the one property of
    the operation that brings an answer no closer to the reference: a store without bf16_round passes the bound)."""
    o = np.asarray(as_f32(out), np.float64)
    return ~np.isfinite(o) | ~(np.abs(o - ref) <= tol) | ~on_bf16_grid(out, b)


def report(out, ref, tol, b=None):
    """The violating share and the worst element, for an assertion message."""
    bad = violations(out, ref, tol, b)
    o = np.asarray(as_f32(out), np.float64)
    ratio = np.where(np.isfinite(o), np.abs(o - ref) / np.maximum(tol, 1e-300), np.inf)
    r, c = np.unravel_index(np.argmax(ratio), ratio.shape)
    return (f"{int(bad.sum())} of {bad.size} elements ({bad.mean():.2%}) violate; {int((~on_bf16_grid(out, b)).sum())} are no bf16 value "
            f"(+ bias); worst at row {r}, column {c}: got {o[r, c]!r}, reference {ref[r, c]!r}, |difference| / tol = {ratio[r, c]:.3g}")


def emulate(latent, W, b, *, reverse=False, round_latent=True, round_weights=True, round_out=True):
    """The operation in float32 numpy: 64-column K tiles accumulated in float32, first to last or (reverse) last to first; the keyword
    switches leave one rounding out (the mutations of tests/test_decode_bound_cpu.py)."""
    A = as_f32(latent)
    A = bf16(A) if round_latent else A
    B = bf16(W) if round_weights else np.ascontiguousarray(W, np.float32)
    n = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    tiles = list(range(0, n, 64))
    for k0 in (reversed(tiles) if reverse else tiles):
        acc = acc + A[:, k0:k0 + 64] @ B[k0:k0 + 64]
    out = bf16(acc) if round_out else acc
    return out if b is None else out + np.asarray(b, np.float32)


def unit_l1_weights(d, n, seed):
    """decoder.weight [d][n] with unit-norm columns of 64 entries +-1/8, and an encoder bias: the in-place renormalisation of every L1
    forward is a fixed point, so repeated forwards see the same weights to the bit (the recipe of tests/test_feature_stats_gpu.py)."""
    g = np.random.default_rng(seed)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:64], j] = np.where(g.random(64) < 0.5, -0.125, 0.125)
    return W, g.normal(-0.5, 0.3, n).astype(np.float32)
