"""Feature label throughput (freud_amd/feature_labels.py; include/freud_sae.h sae_label_files) -- one JSON line, also written to
profiles/labels_bench.json.

Per shape (d, n) at T = 1500 and C = 64 classes (one label per frame, a tenth of the frames unlabelled), a device-resident batch of B
files of an L1 SAE whose bias makes a latent fire on a few per cent of the frames.  Every time is the median over `rounds`
alternating rounds of `iters` calls, with the smallest and largest round next to it:
  label_call_ms   the whole sae_label_files call (encoder GEMM, mask pack, label pack, update);
  coact_call_ms   the whole sae_coact_files call on the same batch (the same encoder and mask pack, the symmetric update);
  torch_ms        the route a user has without the pass, on the same box: torch bf16 one_hot(labels).T @ (encode(x) > 0) of the
                  same frames (both operands given, their construction not timed);
  label_pack_ms, label_update_ms   the label pack + counts and the rectangular update alone (the engine's own event brackets,
                  profile level 2), best of 3 runs;
  label_over_coact   label_call_ms / coact_call_ms: the pass does the same encode and mask pack and a smaller update, so <= 1
                  up to the spread of the rounds.

    python tools/bench_labels.py [--iters 10] [--rounds 5] [--out profiles/labels_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_coact import T, bracket_ms, engine                        # noqa: E402
from bench_pass_common import timed                                  # noqa: E402

CLASSES = 64


def rounds_ms(fns, iters, rounds):
    """Per fn [median, min, max] over alternating rounds."""
    runs = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            runs[i].append(timed(fn, iters))
    return [[statistics.median(r), min(r), max(r)] for r in runs]


def shape(d, n, B, iters, rounds):
    eng, x = engine(d, n, B)
    M = B * T
    g = torch.Generator().manual_seed(1)
    lab = torch.randint(0, CLASSES, (B, T, 1), generator=g, dtype=torch.int32)
    lab[torch.rand(B, T, 1, generator=g) < 0.1] = -1
    lab = lab.cuda()
    table = torch.zeros(CLASSES + 1, n, dtype=torch.int32, device="cuda")
    lcount = torch.zeros(CLASSES + 1, dtype=torch.int64, device="cuda")
    co_table = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    label_call = lambda: eng.label_files(x, lab, CLASSES, table, lcount)
    coact_call = lambda: eng.coact_files(x, co_table)
    # the same operands for torch: the mask of the stored latent of an eval of the same rows, the one-hot labels
    eng.eval(x.reshape(M, d))
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    Z = (torch.as_tensor(_Alias(), device="cuda")[:, :n].view(torch.bfloat16) > 0).to(torch.bfloat16).contiguous()
    idx = lab.reshape(M).long()
    onehot = torch.nn.functional.one_hot(torch.where(idx < 0, torch.full_like(idx, CLASSES), idx), CLASSES + 1)[:, :CLASSES]
    Ot = onehot.to(torch.bfloat16).T.contiguous()
    out = torch.empty(CLASSES, n, dtype=torch.bfloat16, device="cuda")
    torch_fn = lambda: torch.matmul(Ot, Z, out=out)
    label_ms, coact_ms, torch_ms = rounds_ms([label_call, coact_call, torch_fn], iters, rounds)
    runs = [bracket_ms(eng, label_call, iters, ("label_pack", "label_update")) for _ in range(3)]
    res = {"files_per_batch": B, "rows": M, "classes": CLASSES, "label_call_ms": label_ms, "coact_call_ms": coact_ms, "torch_bf16_ms": torch_ms,
           "label_pack_ms": min(r[0] for r in runs), "label_update_ms": min(r[1] for r in runs),
           "label_over_coact": label_ms[0] / coact_ms[0]}
    eng.close()
    return {f"d{d}_n{n}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_labels", "T": T, "device": torch.cuda.get_device_name(0), "times": "[median, min, max] over rounds"}
    res.update(shape(384, 3072, 30, a.iters, a.rounds))
    res.update(shape(1280, 40960, 16, a.iters, a.rounds))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
