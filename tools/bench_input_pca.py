"""Input-covariance throughput (freud_amd/input_pca.py; include/freud_sae.h sae_input_cov) -- one JSON line, also written to
profiles/input_pca_bench.json.

Per shape (d = 384 / 768 / 1280; T = 1500, 256 files, fp32), on one device-resident Gaussian sample with a per-dimension offset:
  cov_ms         sae_input_cov about the engine's mean: the tile kernel (fp64 matrix instruction) and the fold;
  read_ms        one plain read of the sample, the floor: sae_input_moments / 2 (its two sweeps each read the sample once);
  torch_ms       the route a user has without it, a = x.double() - c; a.T @ a, with torch_peak_bytes the peak device memory it
                 takes beyond the sample (the [frames, d] float64 copy: 8 N d bytes, and the product's own workspace);
  cov_extra_bytes  what sae_input_cov takes beyond the sample: the output and the workspace;
  cov_over_read    cov_ms / read_ms;   torch_over_cov   torch_ms / cov_ms (above 1: the engine is faster);
  tflops         the products the engine forms (the tiles on or above the diagonal: 2 N 64^2 per tile) over cov_ms.
The two routes alternate in the same process; every time is the median of the rounds, with the smallest and the largest beside it.

    python tools/bench_input_pca.py [--iters 2] [--rounds 5] [--files 256] [--dims 384,768,1280] [--out profiles/input_pca_bench.json]

Measured on one MI355X (profiles/input_pca_bench.json): cov_ms 1.67 / 5.69 / 14.9 at d = 384 / 768 / 1280,
torch_over_cov 25.2 / 7.6 / 3.0 (the engine is faster at every shape), cov_over_read 10 / 21 / 33 (the pass is compute-bound:
40-44 TFLOP/s of fp64), 67-75 MB beside the sample against torch's 2.4 / 4.7 / 7.9 GB.
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
from bench_pass_common import timed                                 # noqa: E402

T = 1500


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def torch_route(x2, c):
    a = x2.double() - c
    return a.T @ a


def shape(d, files, iters, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((files, T, d), generator=g, device="cuda") + 3.0 * torch.randn(d, generator=g, device="cuda")
    ws = torch.empty(max(E.input_stats_workspace_bytes(files, T, d), E.input_cov_workspace_bytes(files, T, d)), dtype=torch.uint8, device="cuda")
    mom = torch.empty(4 * d + 2, dtype=torch.float64, device="cuda")
    out = torch.empty((d, d), dtype=torch.float64, device="cuda")
    E.input_moments(x, mom, ws)
    c = mom[:d].clone()
    x2 = x.view(-1, d)
    fns = {"cov_ms": lambda: E.input_cov(x, out, ws, c), "moments_ms": lambda: E.input_moments(x, mom, ws), "torch_ms": lambda: torch_route(x2, c)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = torch_route(x2, c)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    E.input_cov(x, out, ws, c)
    rel = float((out - ref).abs().max() / ref.abs().max())
    plan = E.input_cov_plan(files, T, d)
    res = {"d": d, "T": T, "files": files, "sample_bytes": x.numel() * 4, "plan": plan}
    res.update({k: spread(v) for k, v in times.items()})
    res["read_ms"] = res["moments_ms"]["median"] / 2
    res["cov_over_read"] = res["cov_ms"]["median"] / res["read_ms"]
    res["torch_over_cov"] = res["torch_ms"]["median"] / res["cov_ms"]["median"]
    res["torch_peak_bytes"] = int(peak)
    res["cov_extra_bytes"] = d * d * 8 + E.input_cov_workspace_bytes(files, T, d)
    res["tflops"] = 2.0 * files * T * plan["tiles"] * plan["tile"] ** 2 / res["cov_ms"]["median"] / 1e9
    res["max_rel_diff_to_torch"] = rel
    del ref
    return {f"d{d}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--dims", default="384,768,1280")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pca_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_input_pca", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}
    for d in (int(v) for v in a.dims.split(",")):
        res.update(shape(d, a.files, a.iters, a.rounds))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
