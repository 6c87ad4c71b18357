"""Feature index build and query timings (freud_amd/feature_index.py; include/freud_sae.h sae_findex_*) -- one JSON line.

A C3-shaped synthetic store (T = 1500 frames, K = 64 slots, n = 24 576 latents, --files files, a few GB) is generated from a seed
and written where --dir says.  Measured, all on one device in one process:

  count_ms / fill_ms     the entry points on ONE resident batch of --batch_files files (device events, median of --rounds after a
                         warm-up): sae_findex_count, and sae_findex_fill (count + scan + fill) for the whole dictionary;
  kernel_slots_s         the batch's slots over count_ms + fill_ms -- the kernels alone;
  kernel_gb_s            the bytes the two sweeps need by the shapes (store batch read twice, lists written once) over the same time;
  torch_sort_ms          the same transpose by torch.sort(stable=True) on (latent << 32 | position) keys of the posted slots plus the
                         gather of the values, same batch, same rounds, interleaved with the kernels;
  numpy_argsort_ms       numpy.argsort(kind="stable") by latent on the host, same batch (one round);
  build_s                build_feature_index end to end: the store read from disk (page cache: it was just written) twice over
                         PCIe, both sweeps, the index written; slots/s and the byte-bound estimate it is to be read against;
  query_index_ms /       one top_activations query from the index against FeatureShards.series of the same latent plus the same
  query_scan_ms          ranking (the reference's per-query scan, vectorised).
The transposes are checked against each other before anything is timed."""
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
from freud_amd import engine as E                      # noqa: E402
from freud_amd import feature_index as FI              # noqa: E402
from freud_amd.collect_features import FeatureShards   # noqa: E402

LAYER = "enc"
HBM_GB_S, PCIE_GB_S = 8000.0, 64.0                     # datasheet: HBM3E 8 TB/s; PCIe 5.0 x16 64 GB/s a direction


def make_store(folder, F, T, K, n, seed, zero_frac):
    """Rows of K distinct latents (an arithmetic walk with a stride coprime to n), values in (0, 4), zero_frac of the slots +0.0."""
    from numpy.lib.format import open_memmap
    os.makedirs(folder, exist_ok=True)
    vals = open_memmap(os.path.join(folder, f"{LAYER}_activation_values.npy"), mode="w+", dtype=np.float32, shape=(F, T * K))
    idx = open_memmap(os.path.join(folder, f"{LAYER}_feature_indices.npy"), mode="w+", dtype=np.int64, shape=(F, T * K))
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.arange(K, device="cuda", dtype=torch.int64)
    assert n % 6 == 0
    for f0 in range(0, F, 64):
        nb = min(64, F - f0)
        base = torch.randint(0, n, (nb * T, 1), device="cuda", generator=g)
        stride = 6 * torch.randint(0, n // 6, (nb * T, 1), device="cuda", generator=g) + 1       # coprime to n = 2^a 3^b
        i = (base + stride * q) % n
        v = torch.rand(nb * T, K, device="cuda", generator=g) * 4 + 0.01
        v[torch.rand(nb * T, K, device="cuda", generator=g) < zero_frac] = 0.0
        vals[f0:f0 + nb] = v.reshape(nb, T * K).cpu().numpy()
        idx[f0:f0 + nb] = i.reshape(nb, T * K).cpu().numpy()
    vals.flush()
    idx.flush()
    del vals, idx
    with open(os.path.join(folder, f"{LAYER}_metadata.json"), "w") as f:
        json.dump({"tensor_shape": [T, K], "activation_shape": [T, n], "filenames": [f"f{i}.flac" for i in range(F)]}, f)


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--batch_files", type=int, default=64)
    ap.add_argument("--T", type=int, default=1500)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--n", type=int, default=24576)
    ap.add_argument("--zero_frac", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the store is written (default: a temporary folder, removed at the end)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_index needs the GPU: a CPU timing says nothing about it")
    folder = a.dir or tempfile.mkdtemp(prefix="fi_bench_")
    F, T, K, n, B = a.files, a.T, a.K, a.n, min(a.batch_files, a.files)
    try:
        make_store(folder, F, T, K, n, a.seed, a.zero_frac)
        sh = FeatureShards(folder, LAYER)
        rows = B * T
        v = torch.from_numpy(np.asarray(sh.values[:B])).cuda().view(rows, K)
        x = torch.from_numpy(np.asarray(sh.indices[:B])).cuda().view(rows, K)
        totals = torch.zeros(n, dtype=torch.int64, device="cuda")
        stats = torch.zeros(E.FINDEX_NSTATS, dtype=torch.int64, device="cuda")
        err = torch.zeros(2, dtype=torch.int64, device="cuda")
        E.findex_count(v, x, n, totals, stats)
        starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(totals, 0, out=starts[1:])
        nnz = int(starts[-1])
        pos, val = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.float32, device="cuda")
        work = torch.empty(E.findex_workspace_bytes(rows, n), dtype=torch.uint8, device="cuda")
        cursor = torch.empty(n, dtype=torch.int64, device="cuda")

        def count():
            E.findex_count(v, x, n, totals, stats)

        def fill():
            cursor.copy_(starts[:-1])
            E.findex_fill(v, x, n, 0, n, 0, cursor, 0, pos, val, work, err)

        def by_sort():
            keep = v.reshape(-1) != 0
            p = torch.arange(rows, device="cuda", dtype=torch.int64).repeat_interleave(K)[keep]
            order = torch.sort((x.reshape(-1)[keep] << 32) | p, stable=True)
            return (order.values & 0xFFFFFFFF).to(torch.int32), v.reshape(-1)[keep][order.indices]

        fill()
        sp, sv = by_sort()
        E.findex_verify(starts, 0, n, 0, pos, rows, err)
        torch.cuda.synchronize()
        assert err.tolist() == [0, 0] and torch.equal(sp, pos) and torch.equal(sv.view(torch.int32), val.view(torch.int32))
        t_count, t_fill, t_sort = [], [], []
        for _ in range(a.rounds):                               # interleaved: one round of each in turn
            t_count += timed(count, 1)
            t_fill += timed(fill, 1)
            t_sort += timed(by_sort, 1)
        hv, hx = v.cpu().numpy().reshape(-1), x.cpu().numpy().reshape(-1)
        t0 = time.perf_counter()
        keep = hv != 0
        order = np.argsort(hx[keep], kind="stable")
        np_pos = (np.arange(rows * K, dtype=np.int64) // K)[keep][order].astype(np.uint32)
        np_val = hv[keep][order]
        t_numpy = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(np_pos, pos.cpu().numpy().view(np.uint32)) and np.array_equal(np_val.view(np.uint32), val.cpu().numpy().view(np.uint32))
        del pos, val, work, sp, sv
        torch.cuda.empty_cache()

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = FI.build_feature_index(folder, LAYER, batch_files=B, overwrite=True)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0

        ix = FI.FeatureIndex(folder, LAYER)
        j = rep.longest_latent
        t0 = time.perf_counter()
        pq, _ = ix.top_activations(j, 10)
        q_index = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        s = sh.series(j)
        mx = s.max(axis=1)
        top = np.argsort(-mx.astype(np.float64), kind="stable")[:10]
        q_scan = (time.perf_counter() - t0) * 1e3
        assert [p[0] for p in pq] == [sh.filenames[int(f)] for f in top] and [p[2] for p in pq] == [float(mx[f]) for f in top]

        med = statistics.median
        slot_bytes = 4 + x.element_size()
        batch_slots = rows * K
        kern_ms = med(t_count) + med(t_fill)
        batch_bytes = 2 * batch_slots * slot_bytes + 8 * nnz
        store_bytes = F * T * K * slot_bytes
        out = {"tool": "bench_feature_index", "device": torch.cuda.get_device_name(0), "files": F, "T": T, "K": K, "n_dict": n,
               "batch_files": B, "zero_frac": a.zero_frac, "rounds": a.rounds, "batch_slots": batch_slots, "batch_posted": nnz,
               "count_ms": med(t_count), "count_ms_min": min(t_count), "count_ms_max": max(t_count),
               "fill_ms": med(t_fill), "fill_ms_min": min(t_fill), "fill_ms_max": max(t_fill),
               "kernel_slots_s": batch_slots / (kern_ms * 1e-3), "kernel_gb_s": batch_bytes / (kern_ms * 1e-3) / 1e9,
               "kernel_byte_bound_ms": batch_bytes / (HBM_GB_S * 1e9) * 1e3,
               "torch_sort_ms": med(t_sort), "torch_sort_ms_min": min(t_sort), "torch_sort_ms_max": max(t_sort),
               "kernels_vs_torch_sort": med(t_sort) / kern_ms, "numpy_argsort_ms": t_numpy,
               "store_bytes": store_bytes, "index_bytes": rep.bytes_written, "nnz": rep.nnz, "sweeps": rep.sweeps,
               "build_s": build_s, "build_slots_s": F * T * K / build_s,
               "build_byte_bound_s_pcie": (2 * store_bytes + rep.bytes_written) / (PCIE_GB_S * 1e9),
               "build_byte_bound_s_hbm": (2 * store_bytes + rep.bytes_written) / (HBM_GB_S * 1e9),
               "query_latent": j, "query_list": rep.longest_list, "query_index_ms": q_index, "query_scan_ms": q_scan}
        print(json.dumps(out))
    finally:
        if a.dir is None:
            shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()
