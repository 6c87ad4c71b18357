#!/usr/bin/env python3
"""The HBM-resident store (freud_amd/resident.py) measured on the GPU box, on synthetic shards in the collector's format
(the protocol of tools/bench_loader.py: 40 files x 1500 x 384 per step).  Prints one JSON line; --out also writes it to a file.

* the gather kernel alone -- microseconds and TB/s of read plus written bytes -- beside torch.index_select of the same rows and a
  contiguous device-to-device copy of the same bytes (HIP events around runs of launches, every launch another batch of the epoch);
* the train loop (for x in loader: engine.step(x)) four ways in ONE process, interleaved round by round: fed by the streaming
  loader, fed by the resident loader with the gather on its own stream and on the compute stream, and the bare step on one
  resident batch;
* the one-time upload, and the number of epochs after which it is repaid.

  python tools/bench_resident.py [--files 400] [--dtype float16|float32] [--deliver native|bfloat16] [--rounds 5] [--out f.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from freud_amd import engine as E
from freud_amd.loader import MemoryMappedActivationDataLoader, write_shards
from freud_amd.resident import ResidentActivationDataLoader, ResidentActivations


def time_launches(fn, batches, reps: int = 5):
    """Median over `reps` of the mean time (us) of one fn(batch) over a run of all `batches`, by HIP events.  A spin kernel goes
    first, so that the host has enqueued the whole run before the GPU starts it: the events then bracket device time, not launch calls."""
    for b in batches[:3]:
        fn(b)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(20_000_000)
        beg.record()
        for b in batches:
            fn(b)
        end.record()
        end.synchronize()
        out.append(beg.elapsed_time(end) * 1e3 / len(batches))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=400)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--T", type=int, default=1500)
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32"])
    ap.add_argument("--deliver", default="native", choices=["native", "bfloat16"])
    ap.add_argument("--batch-size", type=int, default=40)
    ap.add_argument("--expansion", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the four loops")
    ap.add_argument("--epochs", type=int, default=4, help="epochs per loop and round")
    ap.add_argument("--kernel-only", action="store_true", help="stop after the upload and the kernel section")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="freud_resident_", dir="/tmp")
    try:
        layer = "encoder.blocks.2"
        rng = np.random.default_rng(0)
        z = np.maximum(rng.standard_normal((args.files * args.T, 32), dtype=np.float32), 0) * 0.1
        rows = (z @ rng.standard_normal((32, args.d), dtype=np.float32)).astype(args.dtype).reshape(args.files, args.T * args.d)
        folder = os.path.join(tmp, "train")
        write_shards(folder, layer, rows, [args.T, args.d], [f"/data/f{i}.flac" for i in range(args.files)])
        del rows, z
        B, T, d = args.batch_size, args.T, args.d
        kw = {"shuffle": True, "drop_last": True}
        out = {"files": args.files, "T": T, "d": d, "dtype": args.dtype, "deliver": args.deliver, "batch_size_files": B,
               "rows_per_step": B * T, "library": E.LIB_PATH}

        # ---- the upload
        store = ResidentActivations(folder, layer, device="cuda", dtype=args.deliver)        # (also warms the page cache)
        first = store.upload_seconds
        del store
        store = ResidentActivations(folder, layer, device="cuda", dtype=args.deliver)
        shard_bytes = args.files * T * d * np.dtype(args.dtype).itemsize
        out["upload"] = {"store_GB": store.nbytes / 1e9, "shard_GB": shard_bytes / 1e9, "first_seconds": first, "seconds": store.upload_seconds,
                         "shard_GB_per_s": shard_bytes / store.upload_seconds / 1e9, "store_dtype": str(store.data.dtype)}

        # ---- the gather kernel alone
        es = store.data.element_size()
        batch_bytes = B * T * d * es
        perm = torch.randperm(args.files)[: args.files // B * B].view(-1, B)
        idx32 = [p.to(torch.int32).cuda() for p in perm]
        idx64 = [p.cuda() for p in perm]
        dst = torch.empty((B, T * d), dtype=store.data.dtype, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        us = {"gather": time_launches(lambda i: E.store_gather(store.data, idx32[i], dst, err), list(range(len(idx32)))),
              "index_select": time_launches(lambda i: torch.index_select(store.data, 0, idx64[i], out=dst), list(range(len(idx64)))),
              "contiguous_copy": time_launches(lambda i: dst.copy_(store.data[i * B:(i + 1) * B]), list(range(len(idx32))))}
        assert int(err.item()) == 0
        out["kernel"] = {"batch_MB": batch_bytes / 1e6, "piece_bytes": E.store_piece_bytes(),
                         **{f"{k}_us": v for k, v in us.items()}, **{f"{k}_TB_per_s": 2 * batch_bytes / v / 1e6 for k, v in us.items()},
                         "guide_float4_copy_TB_per_s": 6.29}

        if args.kernel_only:
            print(json.dumps(out), flush=True)
            return

        # ---- the train loop, four ways, interleaved
        eng = E.SaeEngine(variant="l1", d_model=d, n_dict=d * args.expansion, max_rows=B * T, optimizer="radam", recon_alpha=1e4)
        W = torch.empty(d, d * args.expansion)
        torch.nn.init.orthogonal_(W)
        eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": np.zeros(d * args.expansion, np.float32)})
        loaders = {"loader_fed": MemoryMappedActivationDataLoader(folder, layer, B, 0, None, kw, device="cuda", deliver_dtype=args.deliver),
                   "resident_side_stream": ResidentActivationDataLoader(store, layer, B, 0, None, kw, overlap=True),
                   "resident_compute_stream": ResidentActivationDataLoader(store, layer, B, 0, None, kw, overlap=False)}
        out["loader_mode"] = "direct" if loaders["loader_fed"]._direct else "staged"
        steps_per_epoch = len(loaders["loader_fed"])
        one = next(iter(loaders["resident_compute_stream"]))[0].clone()

        def fed(loader):
            n = 0
            for _ in range(args.epochs):
                for x, _names in loader:
                    eng.step(x, 1e-4)
                    n += 1
            return n

        def bare(_):
            for _ in range(args.epochs * steps_per_epoch):
                eng.step(one, 1e-4)
            return args.epochs * steps_per_epoch

        modes = {**{k: (fed, v) for k, v in loaders.items()}, "bare_step": (bare, None)}
        for fn, arg in modes.values():          # warm-up: clocks, rings, page cache
            fn(arg)
        torch.cuda.synchronize()
        ms = {k: [] for k in modes}
        for _ in range(args.rounds):
            for k, (fn, arg) in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = fn(arg)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
        loop = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v), "act_per_s": B * T / statistics.median(v) * 1e3}
                for k, v in ms.items()}
        out["train_loop"] = loop
        out["steps_per_epoch"], out["rounds"], out["epochs_per_round"] = steps_per_epoch, args.rounds, args.epochs
        best = min(("resident_side_stream", "resident_compute_stream"), key=lambda k: loop[k]["ms_per_step"])
        out["faster_overlap"] = best == "resident_side_stream"
        out["resident_over_bare"] = loop[best]["ms_per_step"] / loop["bare_step"]["ms_per_step"]
        out["loader_over_resident"] = loop["loader_fed"]["ms_per_step"] / loop[best]["ms_per_step"]
        saved = (loop["loader_fed"]["ms_per_step"] - loop[best]["ms_per_step"]) * steps_per_epoch / 1e3
        out["upload"]["epochs_to_repay"] = store.upload_seconds / saved if saved > 0 else None
        eng.close()
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
