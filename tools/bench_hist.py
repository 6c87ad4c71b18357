"""Activation histogram throughput (freud_amd/activation_hist.py; include/freud_sae.h sae_hist_files) -- one JSON line.

Per shape and per kind of data -- the two of bench.py's line: `overfit`, its low-rank batch after --fit_steps training steps on that
one batch (L1: a sparse latent; TopK: the low-rank batch, its sparsity is k), and `normal`, N(0, 1) rows through the initial
weights (L1: about half of the latents fire) -- on a device-resident batch of B files of T = 1500 frames:
  hist_ms        sae_hist_files: the encoder that stores the latent (TopK: the eval forward) + the histogram kernels;
  unfused_ms     the same batch through the statistics with the stored latent (sae_stats_files, SAE_STATS_UNFUSED; TopK: its
                 only form), interleaved with hist_ms: median over rounds, with the spread (min, max);
  enc_gemm_ms    the engine's enc_fwd_gemm bracket inside sae_hist_files (L1);
  hist_kernels_ms  the engine's hist bracket: every kernel of the call after the encoder;
  latent_gb_s    bytes of stored latent (rows x padded n x 2) per second of hist_kernels_ms (L1);
  hist_vs_unfused, hist_kernels_vs_enc_gemm  the ratios.

    python tools/bench_hist.py [--iters 10] [--rounds 7] [--fit_steps 60]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from bench_pass_common import timed                                  # noqa: E402

T = 1500
SPEC = (-12, 24, 2)


def interleaved(fns, iters, rounds):
    """Per fn (median, min, max) of the per-call milliseconds over `rounds` alternating rounds, after one warm-up round."""
    for fn in fns:
        timed(fn, 2)
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ms[i].append(timed(fn, iters))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def brackets(eng, fn, iters):
    eng.profile(2)
    eng.kernel_times()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    kt = eng.kernel_times()
    eng.profile(0)
    return {k: ms / max(1, cnt) for k, (ms, cnt) in kt.items() if cnt}


def data(kind, B, d, g):
    if kind == "normal":
        return torch.randn(B, T, d, generator=g)
    z = torch.relu(torch.randn(B * T, 64, generator=g)) * 0.1          # bench.py make_inputs, "lowrank"
    return (z @ torch.randn(64, d, generator=g)).reshape(B, T, d)


def run(variant, d, n, B, k, kind, iters, rounds, fit_steps):
    g = torch.Generator().manual_seed(0)
    x = data(kind, B, d, g).cuda()
    if variant == "l1":
        eng = E.SaeEngine("l1", d, n, -(-B * T // 256) * 256, optimizer="radam", recon_alpha=1e4, clip_thresh=1.0)
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
        eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": torch.zeros(n).numpy()})
        if kind == "overfit":
            for _ in range(fit_steps):
                eng.step(x.reshape(B * T, d), 4e-4)
    else:
        eng = E.SaeEngine("topk", d, n, B * T, k=k, optimizer="adam")
        We = torch.randn(n, d, generator=g) / d ** 0.5
        eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": torch.zeros(n).numpy(), "W_dec": We.numpy(), "b_dec": torch.zeros(d).numpy()})
        eng.set_topk_options(float("inf"), 0)
    nb = E.hist_nbins(SPEC)
    fh = torch.zeros(n, nb, dtype=torch.int64, device="cuda")
    mh, nf = torch.zeros_like(fh), torch.zeros(1, dtype=torch.int64, device="cuda")
    block = torch.zeros(E.stats_layout(n)["bytes"], dtype=torch.uint8, device="cuda")
    hist = lambda: eng.hist_files(x, SPEC, fh, mh, nf)
    unfused = lambda: eng.stats_files(x, block, unfused=(variant == "l1"))
    (h_med, h_min, h_max), (u_med, u_min, u_max) = interleaved([hist, unfused], iters, rounds)
    fh.zero_()
    hist()
    torch.cuda.synchronize()
    active = float(fh[:, 1:].sum().item()) / (B * T * n)
    br = brackets(eng, hist, iters)
    res = {"files_per_batch": B, "active_fraction": active, "hist_ms": h_med, "hist_ms_min": h_min, "hist_ms_max": h_max,
           "unfused_ms": u_med, "unfused_ms_min": u_min, "unfused_ms_max": u_max, "hist_vs_unfused": h_med / u_med,
           "hist_kernels_ms": br.get("hist")}
    if variant == "l1":
        n_p = -(-n // 128) * 128
        res.update({"enc_gemm_ms": br.get("enc_fwd_gemm"), "hist_kernels_vs_enc_gemm": br["hist"] / br["enc_fwd_gemm"],
                    "latent_gb_s": B * T * n_p * 2 / (br["hist"] * 1e-3) / 1e9})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fit_steps", type=int, default=60)
    a = ap.parse_args()
    res = {"tool": "bench_hist", "T": T, "spec": list(SPEC), "device": torch.cuda.get_device_name(0)}
    for name, args in (("l1_d384_n3072", ("l1", 384, 3072, 30, 0)), ("l1_d1280_n40960", ("l1", 1280, 40960, 16, 0)),
                       ("topk_d768_n24576_k64", ("topk", 768, 24576, 16, 64))):
        for kind in ("overfit", "normal"):
            res[f"{name}_{kind}"] = run(*args, kind, a.iters, a.rounds, a.fit_steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
