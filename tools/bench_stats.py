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

T = 1500


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def l1_shape(d, n, B, iters):
    g = torch.Generator().manual_seed(0)
    eng = E.SaeEngine("l1", d, n, -(-B * T // 256) * 256)      # (room for an even number of 128-row blocks: the fused path)
    W = torch.empty(d, n)
    torch.nn.init.orthogonal_(W, generator=g)
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": (0.01 * torch.randn(n, generator=g)).numpy()})
    x = torch.randn(B, T, d, generator=g).cuda()
    block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device="cuda")

    # alternating rounds, best round of each: the clock of a power-managed chip ramps during the first milliseconds
    fused_ms = unfused_ms = float("inf")
    for _ in range(5):
        fused_ms = min(fused_ms, timed(lambda: eng.stats_files(x, block), iters))
        unfused_ms = min(unfused_ms, timed(lambda: eng.stats_files(x, block, unfused=True), iters))
    eng.profile(2)
    for _ in range(iters):
        eng.stats_files(x, block, unfused=True)
    kt = eng.kernel_times()
    enc_ms = kt["enc_fwd_gemm"][0] / max(1, kt["enc_fwd_gemm"][1])
    for _ in range(iters):
        eng.stats_files(x, block)
    kt = eng.kernel_times()
    stats_gemm_ms = kt["enc_fwd_gemm"][0] / max(1, kt["enc_fwd_gemm"][1])
    eng.profile(0)
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
