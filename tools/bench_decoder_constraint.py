#!/usr/bin/env python
"""What the decoder-norm constraint (sae_set_decoder_constraint; freud_amd/csrc/dec_norm.h) costs a TopK training step on the MI355X.

One engine per shape, the constraint switched off and on in alternating blocks on the same box, the same buffers and the same batches
(tools/ab_*.sh do the same between two libraries):

    step time      host clock around `--steps` calls of step() that end in a device synchronise, per block; median and spread over
                   the `--blocks` blocks of each setting, no profiling events in the queue
    clip_adam      the KID_OPT bracket of sae_kernel_times (profile level 2, a pass of its own: the event records cost the step ~6 us
                   each): the norm pass, the update and -- with the constraint -- the projection and the renorm

Shapes: C3 (d=768, n=24 576, k=64) and d=1280, n=40 960, k=32, M = 65 536 rows, AuxK off (no dead latents: the optimizer step does
not depend on them).  Bytes the constraint adds, from the shapes: the projection reads g and w and writes g (3 matrices), the norm pass
that the backward's sum of squares no longer replaces reads the whole gradient (2 matrices + the biases), the renorm reads and writes w
and writes its bf16 copy (2.5 matrices), minus the bf16 copy the update no longer writes (0.5).

    python tools/bench_decoder_constraint.py [--out profiles/decoder_constraint.json]

Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd.engine import SaeEngine  # noqa: E402

SHAPES = (("C3", 768, 24576, 64), ("d1280", 1280, 40960, 32))


def make_engine(d, n, k, rows):
    eng = SaeEngine(variant="topk", d_model=d, n_dict=n, max_rows=rows, optimizer="adam", k=k, auxk_alpha=0.03125, clip_thresh=1.0)
    eng.set_topk_options(1e15, 1024)
    g = torch.Generator().manual_seed(0)
    We = (torch.rand(n, d, generator=g) * 2 - 1) / d ** 0.5
    Wd = We / (We.norm(dim=1, keepdim=True) + torch.finfo(torch.float32).eps)
    eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": np.zeros(n, np.float32), "W_dec": Wd.numpy(), "b_dec": np.zeros(d, np.float32)})
    return eng


def timed_block(eng, xs, steps, lr=4e-4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        eng.step(xs[i % len(xs)], lr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def opt_bracket(eng, xs, steps, lr=4e-4):
    eng.profile(2)
    eng.kernel_times()                       # (clears what was recorded so far)
    for i in range(steps):
        eng.step(xs[i % len(xs)], lr)
    ms, cnt = eng.kernel_times()["clip_adam"]
    eng.profile(0)
    return ms / max(cnt, 1)


def added_bytes(d_p, n_p):
    mat = 4.0 * d_p * n_p
    return {"project": 3 * mat, "norm_pass": 2 * mat + 4.0 * (n_p + d_p), "renorm": 2.5 * mat, "update_copy_saved": -0.5 * mat}


def measure(name, d, n, k, args):
    eng = make_engine(d, n, k, args.rows)
    g = torch.Generator().manual_seed(1)
    xs = [(torch.relu(torch.randn(args.rows, 32, generator=g)) @ torch.randn(32, d, generator=g) * 0.2).to(torch.bfloat16).cuda() for _ in range(2)]
    try:
        for on in (False, True):             # warm up both settings: code objects, the first launches
            eng.set_decoder_constraint(on)
            timed_block(eng, xs, args.warmup)
        blocks = {False: [], True: []}
        for _ in range(args.blocks):
            for on in (False, True):
                eng.set_decoder_constraint(on)
                blocks[on].append(timed_block(eng, xs, args.steps))
        opt = {}
        for on in (False, True):
            eng.set_decoder_constraint(on)
            opt[on] = opt_bracket(eng, xs, min(args.steps, 32))
    finally:
        eng.close()
    off, on = statistics.median(blocks[False]), statistics.median(blocks[True])
    d_p, n_p = (d + 127) // 128 * 128, (n + 127) // 128 * 128
    by = added_bytes(d_p, n_p)
    return {"shape": name, "d": d, "n": n, "k": k, "rows": args.rows, "steps_per_block": args.steps, "blocks": args.blocks,
            "step_ms_off": off, "step_ms_on": on, "step_ms_added": on - off,
            "step_ms_off_min_max": [min(blocks[False]), max(blocks[False])], "step_ms_on_min_max": [min(blocks[True]), max(blocks[True])],
            "clip_adam_ms_off": opt[False], "clip_adam_ms_on": opt[True], "clip_adam_ms_added": opt[True] - opt[False],
            "added_bytes": by, "added_mb_total": sum(by.values()) / 1e6,
            "added_bytes_per_added_clip_adam_s": sum(by.values()) / max((opt[True] - opt[False]) * 1e-3, 1e-9)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--shapes", default="C3,d1280")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder_constraint: no GPU -- this measurement has no CPU fallback")
    res = {"device": torch.cuda.get_device_name(0), "results": [measure(*s, args) for s in SHAPES if s[0] in args.shapes.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
