"""File features throughput (freud_amd/file_features.py; include/freud_sae.h sae_file_top_features) -- one JSON line.

Per shape (d, n) at T = 1500, device-resident batches of B files of an L1 SAE:
  keys_ms      the keys step of the batch, sae_search_files (the fused L1 search: the yardstick the select is held against);
  select_ms    sae_file_top_features on those keys at n_top in {16, 1024};
  merge_ms     for scale, sae_search_merge of the same keys into an empty table with the same n_top (the kernel that reads the
               same input for the latent -> files direction);
  select_gbps  B n 8 bytes (ONE read of the keys, the select's floor) over select_ms;
  select_over_keys   select_ms / keys_ms.
loader_files_per_s: file_features() fed by the shard loader from a local shard directory (fp32 rows: host -> HBM included).

    python tools/bench_file_features.py [--iters 50] [--loader_files 64]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from freud_amd import file_features as FF                            # noqa: E402
from freud_amd.loader import write_shards                            # noqa: E402
from bench_pass_common import best_alternating, l1_engine            # noqa: E402

T = 1500
N_TOPS = (16, 1024)


def shape(d, n, B, iters, loader_files):
    eng, x = l1_engine(d, n, B, T)
    keys = torch.empty(B * n, dtype=torch.int64, device="cuda")
    eng.search_files(x, keys)
    torch.cuda.synchronize()
    positive = int((((keys.view(B, n) >> 32) & 0xFFFFFFFF) > 0x80000000).sum(1).float().mean())
    res = {"files_per_batch": B, "positive_latents_per_file": positive, "keys_bytes": B * n * 8}
    fns = [lambda: eng.search_files(x, keys)]
    for n_top in N_TOPS:
        lat = torch.empty(B * n_top, dtype=torch.int32, device="cuda")
        out = torch.empty(B * n_top, dtype=torch.int64, device="cuda")
        top = torch.zeros(n_top * n, dtype=torch.int64, device="cuda")
        frames = torch.zeros(n_top * n, dtype=torch.int32, device="cuda")
        fns.append(lambda n_top=n_top, lat=lat, out=out: E.file_top_features(keys, B, n, n_top, E.FILE_TOP_POSITIVE, lat, out))
        # (the merge's cost depends on what its table holds: each timed call starts from a zeroed table, and the zeroing alone is
        # timed next to it and subtracted)
        fns.append(lambda n_top=n_top, top=top, frames=frames: (top.zero_(), E.search_merge(keys, None, B, n, 0, n_top, 0, 0.0, 0.0, top, frames)))
        fns.append(lambda top=top: top.zero_())
    ms = best_alternating(fns, iters)
    res["keys_ms"] = ms[0]
    for i, n_top in enumerate(N_TOPS):
        sel, mrg = ms[1 + 3 * i], max(0.0, ms[2 + 3 * i] - ms[3 + 3 * i])
        res[f"top{n_top}"] = {"select_ms": sel, "merge_ms": mrg, "select_gbps": B * n * 8 / sel / 1e6, "select_over_keys": sel / ms[0]}
    if loader_files:
        tmp = tempfile.mkdtemp()
        try:
            rows = np.random.default_rng(0).standard_normal((loader_files, T * d), dtype=np.float32)
            write_shards(tmp, "enc", rows, [T, d])
            del rows
            FF.file_features(eng, tmp, "enc", 16, batch_files=B)                 # warm (page cache, registration)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            FF.file_features(eng, tmp, "enc", 16, batch_files=B)
            res["loader_files_per_s"] = loader_files / (time.perf_counter() - t0)
        finally:
            shutil.rmtree(tmp)
    eng.close()
    return {f"d{d}_n{n}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loader_files", type=int, default=64)
    a = ap.parse_args()
    res = {"tool": "bench_file_features", "T": T, "n_tops": list(N_TOPS), "device": torch.cuda.get_device_name(0)}
    res.update(shape(384, 3072, 30, a.iters, a.loader_files))
    res.update(shape(1280, 40960, 16, a.iters, a.loader_files // 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
