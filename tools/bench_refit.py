"""Refit frontier throughput (freud_amd/refit.py; include/freud_sae.h sae_refit_files) -- one JSON line per shape.

On a device-resident batch of B files of T = 1500 frames of N(0, 1) rows, at the frontier's shapes -- TopK d = 768, n = 24 576,
k = K = 64 through the initial weights; L1 d = 384, n = 12 288, K = 64 through orthogonal unit columns with an encoder bias of -2.05
-- the passes interleaved in the same process:
  refit_ms           sae_refit_files: the eval encoder, the collect kernels, the refit kernel, the fold; median over rounds (min, max)
  frontier_ms        sae_frontier_files on the same batch at the same K
  torch_ms           the torch route on the same slots: gather the K operand rows per frame, G = bmm(Ws, Ws^T) in bf16 with fp32
                     accumulation, c = bmm(Ws, r_0), torch.linalg.cholesky_ex on G + 1e-6 I, two triangular solves, the prefix
                     errors e_0 - cumsum(y^2) -- without the dependence rule, the trace or the histograms
and from the engine's brackets inside sae_refit_files (a profiled call):
  sort_ms            refit_sort: the collect kernels into scratch
  chol_ms            refit_chol: the refit kernel alone (Gram matrix, projections, factorisation, substitution, final residual)
  fold_ms            refit_fold: finish + dimension sums + fold
  chol_gflops        the factorisation's useful work, rows x (K^2 d_p [Gram, upper half twice] + K^3 / 3) / chol_ms

    python tools/bench_refit.py [--iters 3] [--rounds 3] [--K 64]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from bench_collect import model                                      # noqa: E402
from bench_hist import T, brackets, data, interleaved                # noqa: E402

TAUS = (0.5, 0.2, 0.1, 0.05)


def torch_route(xr, W32, b, idx, K):
    """Batched least squares on the given slots through torch ops; returns the prefix errors [rows, K + 1]."""
    r0 = xr.float() - b
    Ws = W32[idx]                                                     # [rows, K, d]
    Wb = Ws.to(torch.bfloat16)
    G = torch.bmm(Wb, Wb.transpose(1, 2)).float()
    c = torch.bmm(Ws, r0[:, :, None])
    G = G + 1e-6 * torch.eye(K, device=G.device)
    L, _info = torch.linalg.cholesky_ex(G)
    y = torch.linalg.solve_triangular(L, c, upper=False)
    _a = torch.linalg.solve_triangular(L.transpose(1, 2), y, upper=True)
    e0 = (r0 * r0).sum(1, keepdim=True)
    return torch.cat([e0, e0 - torch.cumsum(y[:, :, 0] ** 2, 1)], 1)


def run(variant, d, n, B, k, K, a):
    g = torch.Generator().manual_seed(0)
    x = data("normal", B, d, g).cuda()
    rows = -(-B * T // 256) * 256
    sae = model(variant, d, n, k, rows)
    eng = sae._ensure(rows)
    if variant == "l1":
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
        sae.load_state_dict({"decoder.weight": W, "encoder_bias": torch.full((n,), -2.05)})
        W32 = W.t().contiguous().to(torch.bfloat16).float().cuda()
        b = torch.zeros(d, device="cuda")
    else:
        p = eng.get_params()
        W32 = torch.from_numpy(p["W_dec"]).to(torch.bfloat16).float().cuda()
        b = torch.from_numpy(p["b_dec"]).cuda()
    K = min(K, k) if variant == "topk" else K
    rblock = torch.zeros(E.refit_layout(len(TAUS), K, d, n)["bytes"], dtype=torch.uint8, device="cuda")
    fblock = torch.zeros(E.frontier_layout(len(TAUS), K, d)["bytes"], dtype=torch.uint8, device="cuda")
    vals = torch.empty(B * T, K, dtype=torch.float32, device="cuda")
    idx = torch.empty(B * T, K, dtype=torch.int64, device="cuda")
    eng.collect_files(x, K, vals, idx, torch.zeros(8, dtype=torch.int64, device="cuda"))
    xr = x.reshape(B * T, d)
    refit = lambda: eng.refit_files(x, K, TAUS, rblock)
    frontier = lambda: eng.frontier_files(x, K, TAUS, fblock)
    torch_fn = lambda: torch_route(xr, W32, b, idx, K)
    (r_med, r_min, r_max), (f_med, f_min, f_max), (t_med, t_min, t_max) = interleaved([refit, frontier, torch_fn], a.iters, a.rounds)
    bp = brackets(eng, refit, 1)
    chol = bp.get("refit_chol")
    d_p = -(-d // 128) * 128
    active = float((vals != 0).float().sum(1).mean())
    res = {"files_per_batch": B, "rows": B * T, "K": K, "mean_active_slots": active, "refit_ms": r_med, "refit_ms_min": r_min,
           "refit_ms_max": r_max, "frontier_ms": f_med, "frontier_ms_min": f_min, "frontier_ms_max": f_max, "torch_ms": t_med,
           "torch_ms_min": t_min, "torch_ms_max": t_max, "sort_ms": bp.get("refit_sort"), "chol_ms": chol, "fold_ms": bp.get("refit_fold"),
           "chol_gflops": B * T * (K * K * d_p + K ** 3 / 3.0) / (chol * 1e-3) / 1e9 if chol else None}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--K", type=int, default=64)
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    for name, args in ((f"topk_d768_n24576_K{a.K}", ("topk", 768, 24576, 16, 64, a.K)), (f"l1_d384_n12288_K{a.K}", ("l1", 384, 12288, 16, 0, a.K))):
        print(json.dumps({"tool": "bench_refit", "shape": name, "T": T, "device": dev, **run(*args, a)}), flush=True)


if __name__ == "__main__":
    main()
