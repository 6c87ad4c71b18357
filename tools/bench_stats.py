"""Feature statistics throughput (freud_amd/feature_stats.py; include/freud_sae.h sae_stats_files) -- one JSON line.

Per L1 shape (d, n) at T = 1500, a device-resident batch of B files:
  stats_ms     the fused pass (encoder GEMM with the statistics epilogue, the latent never written) + L0 histogram + fold;
  unfused_ms   the same answer through the stored latent (ordinary encoder GEMM, column and row kernels, fold);
  enc_gemm_ms  the engine's own enc_fwd_gemm (the encoder GEMM that stores the latent) at the same M, from its HIP-event brackets;
  stats_gemm_ms  the fused GEMM alone, from the same brackets;
  *_vs_enc_gemm  stats_ms / enc_gemm_ms and unfused_ms / enc_gemm_ms.
TopK (768, 24576, k = 64): topk_ms, the eval forward + the statistics of its selection per batch.

    python tools/bench_stats.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from bench_pass_common import best_alternating, enc_gemm_ms, l1_engine, timed   # noqa: E402

T = 1500


def l1_shape(d, n, B, iters):
    eng, x = l1_engine(d, n, B, T)
    block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device="cuda")
    fused, unfused = (lambda: eng.stats_files(x, block)), (lambda: eng.stats_files(x, block, unfused=True))
    fused_ms, unfused_ms = best_alternating([fused, unfused], iters)
    enc_ms, stats_gemm_ms = enc_gemm_ms(eng, [unfused, fused], iters)
    eng.close()
    return {f"d{d}_n{n}": {"files_per_batch": B, "stats_ms": fused_ms, "unfused_ms": unfused_ms, "enc_gemm_ms": enc_ms,
                           "stats_gemm_ms": stats_gemm_ms, "stats_vs_enc_gemm": fused_ms / enc_ms,
                           "unfused_vs_enc_gemm": unfused_ms / enc_ms, "stats_files_per_s": B / fused_ms * 1e3}}


def topk_shape(d, n, k, B, iters):
    g = torch.Generator().manual_seed(0)
    eng = E.SaeEngine("topk", d, n, B * T, k=k, optimizer="adam")
    We = torch.randn(n, d, generator=g) / d ** 0.5
    eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": torch.zeros(n).numpy(), "W_dec": We.numpy(),
                    "b_dec": torch.zeros(d).numpy()})
    eng.set_topk_options(float("inf"), 0)
    x = torch.randn(B, T, d, generator=g).cuda()
    block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device="cuda")
    ms = min(timed(lambda: eng.stats_files(x, block), iters) for _ in range(3))
    eval_ms = min(timed(lambda: eng.eval(x.reshape(B * T, d)), iters) for _ in range(3))
    eng.close()
    return {f"topk_d{d}_n{n}_k{k}": {"files_per_batch": B, "topk_ms": ms, "eval_ms": eval_ms, "stats_files_per_s": B / ms * 1e3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    res = {"tool": "bench_stats", "T": T, "device": torch.cuda.get_device_name(0)}
    res.update(l1_shape(384, 3072, 30, a.iters))
    res.update(l1_shape(1280, 40960, 16, a.iters))
    res.update(topk_shape(768, 24576, 64, 16, a.iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
