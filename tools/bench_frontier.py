"""Sparsity frontier throughput (freud_amd/sparsity_frontier.py; include/freud_sae.h sae_frontier_files) -- one JSON line per shape.

On a device-resident batch of B files of T = 1500 frames of N(0, 1) rows -- TopK d = 768, n = 24 576, k = K = 64 through the initial
weights; L1 d = 384, n = 12 288, K = 64 through orthogonal unit columns with an encoder bias of -2.05 (about 2 % of the latents fire) --
the three passes interleaved in the same process:
  frontier_ms        sae_frontier_files: the encoder, the collect kernels into scratch, the walk, the fold; median over rounds (min, max)
  collect_ms         sae_collect_files on the same batch at the same K
  recon_ms           sae_recon_files on the same batch
and from the engine's brackets inside sae_frontier_files / sae_recon_files:
  sort_ms, walk_ms, fold_ms          frontier_sort (the collect kernels), frontier_walk (the walk kernel alone), frontier_fold
  recon_decode_attr_ms               recon_decode + recon_attr: the TopK report's sparse decode and attribution (TopK only)
  walk_vs_recon_decode_attr          walk_ms over that sum (TopK only; above 1 the walk is the slower of the two)
  active_per_row                     the slots of a row that gather an operand row
  walk_gather_gb_s                   rows x active_per_row x d_p x 2 bytes per second of walk_ms: the gather traffic as an effective rate

    python tools/bench_frontier.py [--iters 10] [--rounds 5]
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
    vals = torch.empty(B, T, K, device="cuda")
    idx = torch.empty(B, T, K, dtype=torch.int64, device="cuda")
    cstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    fblock = torch.zeros(E.frontier_layout(len(TAUS), K, d)["bytes"], dtype=torch.uint8, device="cuda")
    rblock = torch.zeros(E.recon_layout(n, d)["bytes"], dtype=torch.uint8, device="cuda")
    file_out = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    frontier = lambda: eng.frontier_files(x, K, TAUS, fblock)
    collect = lambda: eng.collect_files(x, K, vals, idx, cstats)
    recon = lambda: eng.recon_files(x, rblock, file_out)
    (f_med, f_min, f_max), (c_med, c_min, c_max), (r_med, r_min, r_max) = interleaved([frontier, collect, recon], a.iters, a.rounds)
    cstats.zero_()
    collect()
    torch.cuda.synchronize()
    st = cstats.cpu().numpy()
    active = float(st[1]) / st[0]
    bf = brackets(eng, frontier, a.iters)
    br = brackets(eng, recon, a.iters)
    d_p = -(-d // 128) * 128
    res = {"files_per_batch": B, "K": K, "active_per_row": active, "frontier_ms": f_med, "frontier_ms_min": f_min, "frontier_ms_max": f_max,
           "collect_ms": c_med, "collect_ms_min": c_min, "collect_ms_max": c_max, "recon_ms": r_med, "recon_ms_min": r_min,
           "recon_ms_max": r_max, "sort_ms": bf.get("frontier_sort"), "walk_ms": bf.get("frontier_walk"), "fold_ms": bf.get("frontier_fold"),
           "walk_gather_gb_s": B * T * active * d_p * 2 / (bf["frontier_walk"] * 1e-3) / 1e9}
    if variant == "topk":
        da = br["recon_decode"] + br["recon_attr"]
        res.update({"recon_decode_attr_ms": da, "walk_vs_recon_decode_attr": bf["frontier_walk"] / da})
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    for name, args in (("topk_d768_n24576_k64_K64", ("topk", 768, 24576, 16, 64, 64)), ("l1_d384_n12288_K64", ("l1", 384, 12288, 16, 0, 64))):
        print(json.dumps({"tool": "bench_frontier", "shape": name, "T": T, "device": dev, **run(*args, a)}), flush=True)


if __name__ == "__main__":
    main()
