"""Input-statistics throughput (freud_amd/input_stats.py; include/freud_sae.h sae_input_moments / sae_input_median) -- one JSON line,
also written to profiles/input_stats_bench.json.

Per shape (d; T = 1500, 256 files, fp32), on one device-resident Gaussian sample with a per-dimension offset:
  moments_ms     sae_input_moments: two sweeps over the sample (the centred one reads it a second time) and their folds;
  read_ms        one plain read of the sample: moments_ms / 2;  read_gbs: the sample's bytes over it;
  torch_sum_ms   torch's own x.sum() over the sample, a second yardstick for one read;
  iteration_ms   one Weiszfeld iteration (sweep + fold): (sae_input_median with 17 iterations - with 1 iteration) / 16;
  median_ms      sae_input_median with 32 iterations (33 sweeps);
  call_ms        the whole sample_statistics call at 32 iterations: moments, the read-back of sigma, the median, the read-back;
  torch_ms       the route a user has without it, for the same rule in fp32: mean and centred variance, then 32 times
                 (x - m).norm(dim=1), 1 / clamp, weighted sum -- [frames, d] temporaries in every iteration;
  iteration_over_read   iteration_ms / read_ms: 1 means an iteration costs one read of the sample;
  torch_over_call       torch_ms / call_ms.
Every time is the median of alternating rounds, with the smallest and the largest round beside it.

    python tools/bench_input_stats.py [--iters 2] [--rounds 5] [--files 256] [--out profiles/input_stats_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freud_amd import engine as E                                   # noqa: E402
from freud_amd import input_stats as IS                             # noqa: E402
from bench_pass_common import timed                                 # noqa: E402

T, ITER = 1500, 32


def torch_route(x2, iterations):
    mean = x2.mean(0)
    var = ((x2 - mean) ** 2).mean(0)
    floor = max(2.0 ** -20 * float(var.sum().sqrt()), IS.FLT_MIN)
    m = mean
    for _ in range(iterations):
        dist = (x2 - m).norm(dim=1)
        w = 1.0 / dist.clamp_min(floor)
        m = (w[:, None] * x2).sum(0) / w.sum()
    return m.cpu(), float((x2 - m).norm(dim=1).mean())


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def shape(d, files, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((files, T, d), generator=g, device="cuda") + 3.0 * torch.randn(d, generator=g, device="cuda")
    ws = torch.empty(E.input_stats_workspace_bytes(files, T, d), dtype=torch.uint8, device="cuda")
    mom = torch.empty(4 * d + 2, dtype=torch.float64, device="cuda")
    E.input_moments(x, mom, ws)
    floor = IS.weiszfeld_floor(float((mom[d:2 * d] / mom[4 * d + 1]).sum().sqrt()))
    path = torch.empty((ITER + 1, d), dtype=torch.float64, device="cuda")
    obj = torch.empty(ITER + 1, dtype=torch.float64, device="cuda")
    start = mom[:d].clone()
    median = lambda it: E.input_median(x, start, floor, it, path[:it + 1], obj[:it + 1], ws)
    x2 = x.view(-1, d)
    fns = {"moments_ms": lambda: E.input_moments(x, mom, ws), "torch_sum_ms": lambda: x.sum(), "median1_ms": lambda: median(1),
           "median17_ms": lambda: median(17), "median_ms": lambda: median(ITER), "call_ms": lambda: IS.sample_statistics(x, None, ITER),
           "torch_ms": lambda: torch_route(x2, ITER)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    res = {"d": d, "T": T, "files": files, "iterations": ITER, "sample_bytes": x.numel() * 4}
    res.update({k: spread(v) for k, v in times.items()})
    res["read_ms"] = res["moments_ms"]["median"] / 2
    res["read_gbs"] = res["sample_bytes"] / res["read_ms"] / 1e6
    res["iteration_ms"] = (res["median17_ms"]["median"] - res["median1_ms"]["median"]) / 16
    res["iteration_over_read"] = res["iteration_ms"] / res["read_ms"]
    res["iteration_over_torch_sum"] = res["iteration_ms"] / res["torch_sum_ms"]["median"]
    res["torch_over_call"] = res["torch_ms"]["median"] / res["call_ms"]["median"]
    return {f"d{d}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_stats_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_input_stats", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}
    for d in (384, 1280):
        res.update(shape(d, a.files, a.iters, a.rounds))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
