"""Pursuit frontier throughput (freud_amd/pursuit.py; include/freud_sae.h sae_pursuit_files) -- one JSON line per shape.

On a device-resident batch of B files of T = 1500 frames of N(0, 1) rows, at the frontier's shapes -- TopK d = 768, n = 24 576, K = 64
through the initial weights; L1 d = 384, n = 12 288, K = 64 through orthogonal unit columns with an encoder bias of -2.05 -- the passes
interleaved in the same process:
  pursuit_ms         sae_pursuit_files: the eval encoder (for IN_SUPPORT), K (GEMM, step) launch pairs, the fold; median over rounds (min, max)
  frontier_ms        sae_frontier_files on the same batch at min(K, k)
  torch_ms           the torch route on the same operands: K times (bf16(r) @ W^T in bf16, scale, max / argmax over the [rows, n] scores,
                     gather, fp32 dot, update) -- it writes and re-reads rows x n scores per step
and from the engine's brackets inside sae_pursuit_files (a profiled call; per launch):
  gemm_ms_per_step   pursuit_gemm: the selection GEMM with EpiPursuit
  step_ms_per_step   pursuit_step: the step kernel
  fold_ms            pursuit_fold: finish + dimension sums + fold
  encoder_gemm_ms    the context's own encoder GEMM on the same rows (enc_fwd_gemm / topk_enc_gemm, which STORES its rows x n result)
  flop_floor_ms      K x encoder_gemm_ms: what K products of this shape cost in this engine
  gemm_vs_encoder    gemm_ms_per_step / encoder_gemm_ms: below 1 the arg-max epilogue is cheaper than storing the product
  gemm_tflops        2 x rows_p x n_p x d_p / gemm_ms_per_step

    python tools/bench_pursuit.py [--iters 3] [--rounds 3] [--K 64]
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


def torch_route(x, W32, b, K):
    """The same rule through torch ops; returns the final residual (kept so that nothing is optimised away)."""
    Wb = W32.to(torch.bfloat16)
    q = (W32 * W32).sum(1)
    z = torch.where(q > 0, q.rsqrt(), torch.zeros_like(q))
    r = x.float() - b
    for _ in range(K):
        sc = (r.to(torch.bfloat16) @ Wb.T).float() * z
        v, j = sc.max(1)
        wj = W32[j]
        a = (r * wj).sum(1) / q[j]
        a = torch.where((v > 0) & (a > 0), a, torch.zeros_like(a))
        r = r - a[:, None] * wj
    return r


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
    Kf = min(K, k) if variant == "topk" else K
    pblock = torch.zeros(E.pursuit_layout(len(TAUS), K, d, n)["bytes"], dtype=torch.uint8, device="cuda")
    fblock = torch.zeros(E.frontier_layout(len(TAUS), Kf, d)["bytes"], dtype=torch.uint8, device="cuda")
    xr = x.reshape(B * T, d)
    pursuit = lambda: eng.pursuit_files(x, K, TAUS, pblock)
    frontier = lambda: eng.frontier_files(x, Kf, TAUS, fblock)
    torch_fn = lambda: torch_route(xr, W32, b, K)
    (p_med, p_min, p_max), (f_med, f_min, f_max), (t_med, t_min, t_max) = interleaved([pursuit, frontier, torch_fn], a.iters, a.rounds)
    bp = brackets(eng, pursuit, 1)
    enc = bp.get("topk_enc_gemm" if variant == "topk" else "enc_fwd_gemm")
    d_p, n_p = -(-d // 128) * 128, -(-n // 128) * 128
    gemm = bp.get("pursuit_gemm")
    res = {"files_per_batch": B, "rows": B * T, "K": K, "pursuit_ms": p_med, "pursuit_ms_min": p_min, "pursuit_ms_max": p_max,
           "frontier_ms": f_med, "frontier_ms_min": f_min, "frontier_ms_max": f_max, "torch_ms": t_med, "torch_ms_min": t_min,
           "torch_ms_max": t_max, "gemm_ms_per_step": gemm, "step_ms_per_step": bp.get("pursuit_step"), "fold_ms": bp.get("pursuit_fold"),
           "encoder_gemm_ms": enc, "flop_floor_ms": K * enc if enc else None, "gemm_vs_encoder": gemm / enc if enc and gemm else None,
           "gemm_tflops": 2.0 * rows * n_p * d_p / (gemm * 1e-3) / 1e12 if gemm else None}
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
        print(json.dumps({"tool": "bench_pursuit", "shape": name, "T": T, "device": dev, **run(*args, a)}), flush=True)


if __name__ == "__main__":
    main()
