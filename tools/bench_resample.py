"""The cost of one dead-latent resampling round (freud_amd/resample.py; include/freud_sae.h sae_resample_*) -- one JSON line per shape.

For d = 384 and n in --n (default 3072 and 12288), over --files synthetic files of T = 1500 frames (float16 shards written where --dir
says), all in one process on one device, each timed end to end (wall clock around the call, device synchronised, median of --rounds
after one warm-up round):

  round_s         resample_dead_latents: the pass (encoder with the stored latent, count reduction, decode, residual sweep), the
                  selection, the read of the chosen frames from the shards, the column rewrite;
  recon_s         reconstruction_report over the same files: the same launches plus the attribution GEMM and its folds;
  stats_s         feature_stats over the same files: the encoder alone, fused where the shape streams;
  step_ms         one training step on a batch of --batch_files files of the same shards (device events, median of 20);
  round_in_steps  round_s / step_ms: what a round costs in training steps of that shape.
The yardsticks are the two existing passes and the training step, on the same box and the same files; every fourth latent is planted
dead (b = -1e4) and restored before each timed round, so that every round revives the same number of latents."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freud_amd import engine as E                                   # noqa: E402
from freud_amd.feature_stats import feature_stats                   # noqa: E402
from freud_amd.reconstruction import reconstruction_report          # noqa: E402
from freud_amd.resample import resample_dead_latents                # noqa: E402

LAYER = "enc"


def make_shards(folder, F, T, d, seed):
    from numpy.lib.format import open_memmap
    os.makedirs(folder, exist_ok=True)
    mm = open_memmap(os.path.join(folder, f"{LAYER}_tensors.npy"), mode="w+", dtype=np.float16, shape=(F, T * d))
    g = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(48, d, device="cuda", generator=g)
    for f0 in range(0, F, 32):
        nb = min(32, F - f0)
        z = torch.relu(torch.randn(nb * T, 48, device="cuda", generator=g)) * 0.2
        mm[f0:f0 + nb] = (z @ mix).reshape(nb, T * d).to(torch.float16).cpu().numpy()
    mm.flush()
    del mm
    json.dump({"tensor_shape": [T, d], "activation_shape": [T, d], "filenames": [f"file_{i:06d}.flac" for i in range(F)]},
              open(os.path.join(folder, f"{LAYER}_metadata.json"), "w"))


def timed(fn, rounds):
    fn()                                                            # warm-up: allocations, page cache
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[3072, 12288])
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch_files", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args(argv)
    d, T = 384, 1500
    folder = a.dir or tempfile.mkdtemp(prefix="bench_resample_")
    try:
        make_shards(folder, a.files, T, d, 0)
        for n in a.n:
            g = torch.Generator().manual_seed(1)
            W = torch.empty(d, n)
            torch.nn.init.orthogonal_(W, generator=g)
            b = np.zeros(n, np.float32)
            b[::4] = -1e4
            params = {"decoder.weight": W.numpy(), "encoder_bias": b}
            eng = E.SaeEngine("l1", d, n, a.batch_files * T, optimizer="radam", recon_alpha=100.0)

            def one_round():
                eng.set_params(params)
                return resample_dead_latents(eng, folder, LAYER, files=a.files, seed=0, round=1, batch_files=a.batch_files)

            round_s, report = timed(one_round, a.rounds)
            eng.set_params(params)
            recon_s, _ = timed(lambda: reconstruction_report(eng, folder, LAYER, subset_size=a.files, batch_files=a.batch_files), a.rounds)
            stats_s, _ = timed(lambda: feature_stats(eng, folder, LAYER, subset_size=a.files, batch_files=a.batch_files), a.rounds)
            x = torch.from_numpy(np.load(os.path.join(folder, f"{LAYER}_tensors.npy"), mmap_mode="r")[:a.batch_files].reshape(
                a.batch_files, T, d).copy()).cuda()
            for _ in range(5):
                eng.step(x, 1e-4)
            ms = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.step(x, 1e-4)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            step_ms = statistics.median(ms)
            print(json.dumps({"d": d, "n": n, "files": a.files, "T": T, "batch_files": a.batch_files, "round_s": round(round_s, 4),
                              "recon_s": round(recon_s, 4), "stats_s": round(stats_s, 4), "step_ms": round(step_ms, 4),
                              "round_in_steps": round(1e3 * round_s / step_ms, 1), "round_over_recon": round(round_s / recon_s, 3),
                              "dead": report.dead, "revived": report.revived, "skipped_duplicate": report.skipped_duplicate}), flush=True)
            eng.close()
    finally:
        if a.dir is None:
            shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()
