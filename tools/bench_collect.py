"""Feature collection throughput (freud_amd/collect_features.py; include/freud_sae.h sae_collect_files) -- one JSON line per shape.

Per shape and kind of data -- L1 `sparse`: N(0, 1) rows through orthogonal unit columns with an encoder bias of -2.05, so about 2 % of
the latents fire (some 60 of 3072: the rows a trained dictionary gives, at most K active, the kernel's fast path); L1 `normal`: the
same rows with a zero bias, half of the latents fire and every row takes the threshold search; TopK `normal`: N(0, 1) rows through
the initial weights (its sparsity is k) -- on a device-resident batch of B files of T = 1500 frames:
  collect_ms          sae_collect_files: the encoder (TopK: the eval forward) + the collect kernel, median over rounds (min, max);
  collect_kernel_ms   the engine's `collect` bracket: the collect kernel alone;
  forward_ms          sae_eval of the same batch, interleaved with collect_ms: the eval forward alone;
  enc_gemm_ms         the engine's enc_fwd_gemm bracket inside sae_collect_files (L1);
  kernel_vs_forward   collect_kernel_ms / forward_ms;
  kernel_gb_s         bytes the kernel must move (L1: rows x (2 n_p + 12 K); TopK: rows x (6 k + 12 K)) per second of collect_kernel_ms;
  active_per_row, rows_dropped_fraction   from the statistics block.
Whole pass, over --files files of fp16 shards on local disk, the two routes alternating for --pass_rounds rounds after one warm-up
round of each (median, min and max of the rounds' wall times):
  pass_s, pass_rows_s         collect_features(): loader, kernels, device-to-host copies, file writes, renames;
  naive_s, naive_rows_s       the naive route: encode(), torch.sort(descending=True, stable=True), .cpu(), numpy.save of the first K
                              per batch;
  pass_vs_naive               median naive_s / median pass_s;
  engine_share_est            an ESTIMATE of the engine's share of the pass: batches x collect_ms / median pass_s (the calls are
                              asynchronous and overlap the host work; the host side itself is not broken down).

    python tools/bench_collect.py [--iters 10] [--rounds 5] [--files 256] [--pass_rounds 5]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import collect_features as CF                         # noqa: E402
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig   # noqa: E402
from freud_amd.loader import write_shards                            # noqa: E402
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder          # noqa: E402
from bench_hist import brackets, data, interleaved                   # noqa: E402

T = 1500


def model(variant, d, n, k, rows):
    if variant == "l1":
        return L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n, recon_alpha=1e4), max_rows=rows)
    torch.manual_seed(0)
    return TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k), max_rows=rows)


def naive_pass(sae, path, out, K, B):
    """encode(), a stable descending sort, the first K to the host, numpy.save per batch."""
    from freud_amd.file_pass import FilePass
    fp = FilePass(sae, path, "enc", what="feature collection", batch_files=B)
    for x, file0, nb, _ in fp:
        enc = sae.encode(x)
        if hasattr(enc, "latent"):
            v, i = torch.sort(enc.latent, dim=-1, descending=True, stable=True)
        else:
            v, o = torch.sort(enc.top_acts, dim=-1, descending=True, stable=True)
            i = torch.gather(enc.top_indices, -1, o)
        np.save(os.path.join(out, f"values_{file0}.npy"), v[..., :K].cpu().numpy())
        np.save(os.path.join(out, f"indices_{file0}.npy"), i[..., :K].cpu().numpy())


def run(variant, d, n, B, k, K, kind, a):
    g = torch.Generator().manual_seed(0)
    x = data("normal", B, d, g).cuda()
    rows = -(-B * T // 256) * 256
    sae = model(variant, d, n, k, rows)
    eng = sae._ensure(rows)
    if variant == "l1":
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
        sae.load_state_dict({"decoder.weight": W, "encoder_bias": torch.full((n,), -2.05 if kind == "sparse" else 0.0)})
    vals = torch.empty(B, T, K, device="cuda")
    idx = torch.empty(B, T, K, dtype=torch.int64, device="cuda")
    stats = torch.zeros(8, dtype=torch.int64, device="cuda")
    collect = lambda: eng.collect_files(x, K, vals, idx, stats)
    forward = lambda: eng.eval(x.reshape(B * T, d))
    (c_med, c_min, c_max), (f_med, f_min, f_max) = interleaved([collect, forward], a.iters, a.rounds)
    stats.zero_()
    collect()
    torch.cuda.synchronize()
    st = stats.cpu().numpy()
    br = brackets(eng, collect, a.iters)
    n_p = -(-n // 128) * 128
    moved = B * T * ((2 * n_p if variant == "l1" else 6 * k) + 12 * K)
    res = {"files_per_batch": B, "K": K, "active_per_row": float(st[1] + st[2]) / st[0], "rows_dropped_fraction": float(st[3]) / st[0],
           "collect_ms": c_med, "collect_ms_min": c_min, "collect_ms_max": c_max, "forward_ms": f_med, "forward_ms_min": f_min,
           "forward_ms_max": f_max, "collect_kernel_ms": br.get("collect"), "enc_gemm_ms": br.get("enc_fwd_gemm"),
           "kernel_vs_forward": br["collect"] / f_med, "kernel_gb_s": moved / (br["collect"] * 1e-3) / 1e9}

    # the whole pass against the naive route, over fp16 shards on disk
    tmp = tempfile.mkdtemp()
    try:
        F = a.files
        xs = data("normal", F, d, g).numpy().astype(np.float16) if F != B else x.cpu().numpy().astype(np.float16)
        write_shards(os.path.join(tmp, "data"), "enc", xs.reshape(F, T * d), [T, d])
        del xs
        times = {"pass": [], "naive": []}
        for rnd in range(a.pass_rounds + 1):                            # (round 0 warms the page cache and the allocators)
            for name in ("pass", "naive"):
                out = os.path.join(tmp, name)
                shutil.rmtree(out, ignore_errors=True)
                os.makedirs(out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "pass":
                    rep = CF.collect_features(sae, os.path.join(tmp, "data"), "enc", out, k=K, batch_files=B)
                else:
                    naive_pass(sae, os.path.join(tmp, "data"), out, K, B)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        res.update({"pass_files": F, "pass_rounds": a.pass_rounds, "pass_bytes_written": rep.bytes_written,
                    "pass_s": med["pass"], "pass_s_min": min(times["pass"]), "pass_s_max": max(times["pass"]),
                    "naive_s": med["naive"], "naive_s_min": min(times["naive"]), "naive_s_max": max(times["naive"]),
                    "pass_rows_s": F * T / med["pass"], "naive_rows_s": F * T / med["naive"], "pass_vs_naive": med["naive"] / med["pass"],
                    "pass_write_mb_s": rep.bytes_written / med["pass"] / 1e6,
                    "engine_share_est": -(-F // B) * c_med * 1e-3 / med["pass"]})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--pass_rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    for name, args, kinds in (("l1_d384_n3072_K128", ("l1", 384, 3072, 30, 0, 128), ("sparse", "normal")),
                              ("topk_d768_n24576_k64", ("topk", 768, 24576, 16, 64, 64), ("normal",))):
        for kind in kinds:
            print(json.dumps({"tool": "bench_collect", "shape": name, "kind": kind, "T": T, "device": dev, **run(*args, kind, a)}), flush=True)


if __name__ == "__main__":
    main()
