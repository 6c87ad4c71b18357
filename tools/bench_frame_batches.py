#!/usr/bin/env python3
"""Frame batches (freud_amd/resident.py: ResidentFrameDataLoader; sae_store_gather_frames) measured on the GPU box, with the
methodology of tools/bench_resident.py: HIP events around runs of launches behind a spin kernel, the variants interleaved round by
round, medians.  Prints one JSON line; --out also writes it to a file (profiles/frame_batches_bench.json).

* the kernel alone, per shape (d = 384 bf16, d = 1280 bf16, d = 384 fp32; 400 files x 1500 frames, 60 000 rows per launch), untrimmed
  and with lengths drawn uniformly in [300, 1500]: microseconds and TB/s of read plus written bytes, beside sae_store_gather of the
  same byte count (whole files), torch.index_select over the [n_files T, d] view with the PRECOMPUTED rows of the same launches, and
  a contiguous device-to-device copy;
* the train loop (for x in loader: engine.step(x)) at d = 384 in ONE process, interleaved: fed by frame batches (untrimmed and
  trimmed), fed by file batches from the same store, and the bare step on one resident batch.

  python tools/bench_frame_batches.py [--files 400] [--rounds 7] [--kernel-only] [--out profiles/frame_batches_bench.json]
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
from freud_amd.loader import write_shards
from freud_amd.resident import ResidentActivationDataLoader, ResidentActivations, ResidentFrameDataLoader


def run_us(fn, batches):
    """The mean time (us) of one fn(batch) over a run of all `batches`, by HIP events.  A spin kernel goes first, so that the host has
    enqueued the whole run before the GPU starts it: the events then bracket device time, not launch calls."""
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(20_000_000)
    beg.record()
    for b in batches:
        fn(b)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / len(batches)


def interleaved(variants, batches, rounds):
    """{name: fn} -> {name: median us} over `rounds` rounds that visit every variant once."""
    for fn in variants.values():
        for b in batches[:2]:
            fn(b)
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            us[k].append(run_us(fn, batches))
    return {k: statistics.median(v) for k, v in us.items()}, {k: [min(v), max(v)] for k, v in us.items()}


def kernel_section(n_files, T, d, dtype, rows, rounds, lengths_rng):
    es = torch.empty(0, dtype=dtype).element_size()
    store = torch.randint(-2 ** 15, 2 ** 15, (n_files, T * d * es // 2), dtype=torch.int16, device="cuda").view(dtype)
    frames = store.view(n_files * T, d)
    files_per_launch = rows // T
    dst = torch.empty((rows, d), dtype=dtype, device="cuda")
    dst_files = dst.view(files_per_launch, T * d)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lengths = lengths_rng.integers(300, T + 1, size=n_files)
    out = {"d": d, "dtype": str(dtype)[6:], "frame_bytes": d * es, "launch_MB": rows * d * es / 1e6}
    for cond, prefix_np in (("untrimmed", None), ("trimmed", np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))):
        N = n_files * T if prefix_np is None else int(prefix_np[-1])
        prefix = None if prefix_np is None else torch.from_numpy(prefix_np).cuda()
        n_launches = N // rows
        key = 0x5DEECE66D
        ordinals = [torch.empty(rows, dtype=torch.int64, device="cuda") for _ in range(n_launches)]
        for b in range(n_launches):                                 # the rows every launch reads, for the torch route
            E.store_gather_frames(store, T, prefix, N, key, b * rows, 1, dst, err, ordinals=ordinals[b])
        perm = torch.randperm(n_files)[: n_files // files_per_launch * files_per_launch].view(-1, files_per_launch)
        idx32 = [p.to(torch.int32).cuda() for p in perm]
        batches = list(range(min(n_launches, len(idx32))))
        variants = {
            "frame_gather": lambda b: E.store_gather_frames(store, T, prefix, N, key, b * rows, 1, dst, err),
            "file_gather": lambda b: E.store_gather(store, idx32[b], dst_files, err),
            "index_select": lambda b: torch.index_select(frames, 0, ordinals[b], out=dst),
            "contiguous_copy": lambda b: dst_files.copy_(store[b * files_per_launch:(b + 1) * files_per_launch]),
        }
        us, spread = interleaved(variants, batches, rounds)
        assert int(err.item()) == 0
        nbytes = rows * d * es
        out[cond] = {"N": N, "launches_per_run": len(batches), **{f"{k}_us": v for k, v in us.items()},
                     **{f"{k}_TB_per_s": 2 * nbytes / v / 1e6 for k, v in us.items()}, "min_max_us": spread,
                     "frame_over_index_select": us["frame_gather"] / us["index_select"],
                     "file_over_index_select": us["file_gather"] / us["index_select"],
                     "frame_over_file": us["frame_gather"] / us["file_gather"]}
    del store
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=400)
    ap.add_argument("--T", type=int, default=1500)
    ap.add_argument("--batch-size", type=int, default=40)
    ap.add_argument("--expansion", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7, help="interleaved rounds of every comparison")
    ap.add_argument("--epochs", type=int, default=4, help="epochs per loop and round")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, T = args.batch_size, args.T
    out = {"files": args.files, "T": T, "rows_per_step": B * T, "library": E.LIB_PATH, "rounds": args.rounds,
           "yardsticks": {"file_gather_46MB_us_section_6v": 19, "guide_random_1152B_rows_TB_per_s": 5.5}}
    rng = np.random.default_rng(0)
    out["kernel"] = [kernel_section(args.files, T, d, dt, B * T, args.rounds, rng)
                     for d, dt in ((384, torch.bfloat16), (1280, torch.bfloat16), (384, torch.float32))]
    if not args.kernel_only:
        d, layer = 384, "encoder.blocks.2"
        tmp = tempfile.mkdtemp(prefix="freud_frames_", dir="/tmp")
        try:
            z = np.maximum(rng.standard_normal((args.files * T, 32), dtype=np.float32), 0) * 0.1
            rows = (z @ rng.standard_normal((32, d), dtype=np.float32)).astype(np.float16).reshape(args.files, T * d)
            folder = os.path.join(tmp, "train")
            write_shards(folder, layer, rows, [T, d], [f"/data/f{i}.flac" for i in range(args.files)])
            del rows, z
            store = ResidentActivations(folder, layer, device="cuda")
            lengths = rng.integers(300, T + 1, size=args.files)
            eng = E.SaeEngine(variant="l1", d_model=d, n_dict=d * args.expansion, max_rows=B * T, optimizer="radam", recon_alpha=1e4)
            W = torch.empty(d, d * args.expansion)
            torch.nn.init.orthogonal_(W)
            eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": np.zeros(d * args.expansion, np.float32)})
            loaders = {"frame_batches": ResidentFrameDataLoader(store, layer, B),
                       "frame_batches_trimmed": ResidentFrameDataLoader(store, layer, B, lengths=lengths),
                       "file_batches": ResidentActivationDataLoader(store, layer, B, 0, None, {"shuffle": True, "drop_last": True})}
            steps = {k: len(v) for k, v in loaders.items()}
            one = next(iter(loaders["file_batches"]))[0].clone()

            def fed(loader):
                n = 0
                for _ in range(args.epochs):
                    for x, _names in loader:
                        eng.step(x, 1e-4)
                        n += 1
                return n

            def bare(_):
                for _ in range(args.epochs * steps["file_batches"]):
                    eng.step(one, 1e-4)
                return args.epochs * steps["file_batches"]

            modes = {**{k: (fed, v) for k, v in loaders.items()}, "bare_step": (bare, None)}
            for fn, arg in modes.values():
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
            out["train_loop"] = {"d": d, "dtype": "float16", "steps_per_epoch": steps, "epochs_per_round": args.epochs, **loop,
                                 "frames_over_files": loop["frame_batches"]["ms_per_step"] / loop["file_batches"]["ms_per_step"],
                                 "frames_over_bare": loop["frame_batches"]["ms_per_step"] / loop["bare_step"]["ms_per_step"]}
            eng.close()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
