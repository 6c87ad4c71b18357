"""Float64 reference and error bounds for the reconstruction report (include/freud_sae.h, sae_recon_files; freud_amd/csrc/recon.h).
Shared by tests/test_reconstruction_cpu.py and tests/test_reconstruction_gpu.py.

The operands, as the engine holds them:

    a      the value encode() returns per (frame, latent), dense [T][n] per file (TopK: the scatter of the k selection)
    r      the residual the engine itself delivered (resid_dev), fp32; r_op = bf16(r) for L1 (the GEMM operand), r for TopK
    w_j    row j of the bf16 decoder operand [n][d]: bf16(decoder.weight)^T (L1) or bf16(W_dec) (TopK)
    x      the delivered activations, widened exactly

The reference, in float64 over the counted frames (the first min(L[f], T) of file f):

    attr_sum_j   = sum_m a (r_op . w_j)        A_j = sum_m |a| sum_i |r_op| |w_j|
    act_sq_sum_j = sum_m a^2
    sum_x_i, sum_x_sq_i, sum_r_sq_i;  file_sse_f = sum r^2, file_energy_f = sum x^2;  dec_norm_sq_j = |w_j|^2

The bounds, with u = 2^-23 per accumulated fp32 term (one ulp per add: the convention and the reasoning of
tests/decode_reference.py; nothing here is measured on the code under test):

    attr_sum      |got - ref| <= (K + B + 8) u A_j     K = d_p products in the dot, B rows per fp32 partial (128 for L1, 256 for
                                                       TopK), 8 for the product a s and the second-order terms
    act_sq_sum    rtol B u          (non-negative terms, at most B of them per fp32 partial; the partials are added in fp64)
    sum_r_sq, sum_x_sq   rtol 128 u (non-negative terms, 128 rows per fp32 partial)
    sum_x         |got - ref| <= 128 u sum |x|
    file_sse, file_energy   rtol d_p u  (at most d_p non-negative terms per fp32 partial)
    dec_norm_sq   rtol d_p u
    n_frames      exact
"""
import dataclasses

import numpy as np
import torch

U = 2.0 ** -23
FLOAT_FIELDS = ("attr_sum", "act_sq_sum", "dec_norm_sq", "sum_x", "sum_x_sq", "sum_r_sq", "file_sse", "file_energy")


def round_up(v, m):
    return (v + m - 1) // m * m


def bf16(t):
    """Round to nearest even to bf16 and back to float32 (a torch tensor or a numpy array; the type is kept)."""
    if isinstance(t, torch.Tensor):
        return t.float().bfloat16().float()
    return torch.from_numpy(np.ascontiguousarray(t, np.float32)).bfloat16().float().numpy()


@dataclasses.dataclass
class Reference:
    n_frames: int
    values: dict         # float64 numpy arrays by field name
    tol: dict            # absolute tolerances, same shapes
    A: np.ndarray        # float64 [n]: the attribution's magnitude sum
    fired: np.ndarray    # bool [n]: latents with a non-zero value on a counted frame


def reference(x, resid, dense_latent, w_op, lengths, variant, device="cpu"):
    """x, resid: [F][T][d] (numpy or torch; resid float32); dense_latent(f) -> the file's latent [T][n] (torch, any device);
    w_op: the bf16-valued decoder operand [n][d]; lengths: [F] ints (already capped at T) -> Reference."""
    assert variant in ("l1", "topk")
    F, T, d = x.shape
    n = w_op.shape[0]
    d_p = round_up(d, 128)
    B = 128 if variant == "l1" else 256
    W = torch.as_tensor(np.asarray(w_op, np.float64), device=device)
    Wa = W.abs()
    z = lambda m: torch.zeros(m, dtype=torch.float64, device=device)
    attr, A, asq, sx, sxa, sxx, srr = z(n), z(n), z(n), z(d), z(d), z(d), z(d)
    fired = torch.zeros(n, dtype=torch.bool, device=device)
    file_sse, file_energy = np.zeros(F), np.zeros(F)
    frames = 0
    for f in range(F):
        L = int(lengths[f])
        a = dense_latent(f)[:L].to(device).double()
        xf = torch.as_tensor(np.asarray(x[f][:L]) if not isinstance(x, torch.Tensor) else x[f, :L]).to(device).double()
        r32 = torch.as_tensor(np.asarray(resid[f][:L]) if not isinstance(resid, torch.Tensor) else resid[f, :L]).to(device).float()
        r = r32.double()
        r_op = bf16(r32).double() if variant == "l1" else r
        attr += (a * (r_op @ W.T)).sum(0)
        A += (a.abs() * (r_op.abs() @ Wa.T)).sum(0)
        asq += (a * a).sum(0)
        fired |= (a != 0).any(0)
        sx += xf.sum(0)
        sxa += xf.abs().sum(0)
        sxx += (xf * xf).sum(0)
        srr += (r * r).sum(0)
        file_sse[f] = float((r * r).sum())
        file_energy[f] = float((xf * xf).sum())
        frames += L
    c = lambda t: t.cpu().numpy()
    wn = c((W * W).sum(1))
    values = {"attr_sum": c(attr), "act_sq_sum": c(asq), "dec_norm_sq": wn, "sum_x": c(sx), "sum_x_sq": c(sxx), "sum_r_sq": c(srr),
              "file_sse": file_sse, "file_energy": file_energy}
    tol = {"attr_sum": (d_p + B + 8) * U * c(A), "act_sq_sum": B * U * c(asq), "dec_norm_sq": d_p * U * wn,
           "sum_x": 128 * U * c(sxa), "sum_x_sq": 128 * U * c(sxx), "sum_r_sq": 128 * U * c(srr),
           "file_sse": d_p * U * file_sse, "file_energy": d_p * U * file_energy}
    return Reference(frames, values, tol, c(A), c(fired))


def violations(got, ref: Reference, field: str) -> np.ndarray:
    """Boolean array: the element of `got` (the field's array) is not finite or further than the bound from the reference."""
    g = np.asarray(got, np.float64)
    return ~np.isfinite(g) | ~(np.abs(g - ref.values[field]) <= ref.tol[field])


def describe(got, ref: Reference, field: str) -> str:
    g = np.asarray(got, np.float64)
    bad = violations(got, ref, field)
    ratio = np.abs(g - ref.values[field]) / np.maximum(ref.tol[field], 1e-300)
    i = int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf)))
    return (f"{field}: {int(bad.sum())} of {bad.size} violate; worst at {i}: got {g[i]!r}, reference {ref.values[field][i]!r}, "
            f"|difference| / bound = {ratio[i]:.3g}")


def check_report(rep, ref: Reference, ctx=""):
    """Every sum of a ReconstructionReport against the reference within the bounds; prints each field's worst ratio first."""
    assert rep.n_frames == ref.n_frames, (ctx, rep.n_frames, ref.n_frames)
    lines = [describe(getattr(rep, k), ref, k) for k in FLOAT_FIELDS]
    print(ctx, *lines, sep="\n  ")
    for k, line in zip(FLOAT_FIELDS, lines):
        assert not violations(getattr(rep, k), ref, k).any(), f"{ctx} {line}"


def check_same(a, b, ref: Reference, ctx=""):
    """Two runs of the same data on different paths or batch sizes: integers equal, every float within the bound of each other
    (`ref` supplies the bounds); dec_norm_sq depends on the weights alone: bitwise."""
    assert a.n_frames == b.n_frames, ctx
    for k in FLOAT_FIELDS:
        ga, gb = np.asarray(getattr(a, k), np.float64), np.asarray(getattr(b, k), np.float64)
        assert (np.abs(ga - gb) <= ref.tol[k]).all(), f"{ctx} {k}"
    assert a.dec_norm_sq.tobytes() == b.dec_norm_sq.tobytes(), f"{ctx} dec_norm_sq"


def check_bitwise(a, b):
    assert a.n_frames == b.n_frames
    for k in FLOAT_FIELDS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


# ---- a float32 emulation of the L1 attribution (tests/test_reconstruction_cpu.py: the bound can fail, and does not on this)
def emulate_attr_l1(a, r_b, w_op, counted, *, drop_last_k_tile=False):
    """a [M][n] float32 (bf16 values), r_b [M][d] float32 (bf16 values, zero on rows that do not count), w_op [n][d] float32, counted
    bool [M] -> attr_sum float64 [n] as the kernels form it: the dot in float32 over 64-wide K tiles, the product a s in float32,
    float32 partials over 128-row blocks (rows in order), the partials added in float64."""
    M, d = r_b.shape
    tiles = list(range(0, d, 64))
    if drop_last_k_tile:
        tiles = tiles[:-1]
    s = np.zeros((M, w_op.shape[0]), np.float32)
    Wt = np.ascontiguousarray(w_op.T, np.float32)
    for k0 in tiles:
        s = s + r_b[:, k0:k0 + 64].astype(np.float32) @ Wt[k0:k0 + 64]
    p = (a.astype(np.float32) * s).astype(np.float32)
    p[~counted] = 0
    out = np.zeros(w_op.shape[0], np.float64)
    for r0 in range(0, M, 128):
        part = np.zeros(w_op.shape[0], np.float32)
        for row in range(r0, min(r0 + 128, M)):
            part = part + p[row]
        out += part.astype(np.float64)
    return out
