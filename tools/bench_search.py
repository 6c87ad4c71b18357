"""Feature search throughput (freud_amd/feature_search.py; include/freud_sae.h sae_search_*) -- one JSON line.

Per shape (d, n) at T = 1500, device-resident batches of B files:
  search_*   the fused L1 search (encoder GEMM with the max / argmax epilogue, the latent never written) + the top-N merge;
  unfused_*  the same answer through the stored latent (ordinary encoder GEMM, then a column reduction kernel) + the merge;
  enc_gemm_ms  the engine's own enc_fwd_gemm (the encoder GEMM that stores the latent) at the same M, from its HIP-event brackets;
  *_pflops   encoder arithmetic 2 T d n per file over the wall time per batch.
loader_files_per_s: search_features() fed by the shard loader from a local shard directory (fp32 rows: host -> HBM included).

    python tools/bench_search.py [--iters 20] [--loader_files 64]
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
from freud_amd import feature_search as FS                           # noqa: E402
from freud_amd.loader import write_shards                            # noqa: E402
from bench_pass_common import best_alternating, enc_gemm_ms, l1_engine, timed   # noqa: E402

T = 1500
N_TOP = 16


def shape(d, n, B, iters, loader_files):
    eng, x = l1_engine(d, n, B, T)
    keys = torch.empty(B * n, dtype=torch.int64, device="cuda")
    top = torch.zeros(N_TOP * n, dtype=torch.int64, device="cuda")
    frames = torch.zeros(N_TOP * n, dtype=torch.int32, device="cuda")

    def run(unfused):
        eng.search_files(x, keys, unfused=unfused)
        E.search_merge(keys, None, B, n, 0, N_TOP, 0, 0.0, 0.0, top, frames)

    fused_ms, unfused_ms = best_alternating([lambda: run(False), lambda: run(True)], iters)
    merge_ms = timed(lambda: E.search_merge(keys, None, B, n, 0, N_TOP, 0, 0.0, 0.0, top, frames), iters)
    enc_ms, search_gemm_ms = enc_gemm_ms(eng, [lambda: eng.search_files(x, keys, unfused=True), lambda: eng.search_files(x, keys)],
                                         iters)
    flop = 2.0 * T * d * n * B
    out = {f"d{d}_n{n}": {
        "files_per_batch": B,
        "search_files_per_s": B / fused_ms * 1e3, "search_pflops": flop / fused_ms / 1e12,
        "unfused_files_per_s": B / unfused_ms * 1e3, "unfused_pflops": flop / unfused_ms / 1e12,
        "search_ms": fused_ms, "unfused_ms": unfused_ms,
        "enc_gemm_ms": enc_ms, "search_gemm_ms": search_gemm_ms, "merge_ms": merge_ms,
    }}
    if loader_files:
        tmp = tempfile.mkdtemp()
        try:
            rows = np.random.default_rng(0).standard_normal((loader_files, T * d), dtype=np.float32)
            write_shards(tmp, "enc", rows, [T, d])
            del rows
            FS.search_features(eng, tmp, "enc", N_TOP, batch_files=B)            # warm (page cache, registration)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            FS.search_features(eng, tmp, "enc", N_TOP, batch_files=B)
            out[f"d{d}_n{n}"]["loader_files_per_s"] = loader_files / (time.perf_counter() - t0)
        finally:
            shutil.rmtree(tmp)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loader_files", type=int, default=64)
    a = ap.parse_args()
    res = {"tool": "bench_search", "T": T, "n_top": N_TOP, "device": torch.cuda.get_device_name(0)}
    res.update(shape(384, 3072, 32, a.iters, a.loader_files))
    res.update(shape(1280, 40960, 16, a.iters, a.loader_files // 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
