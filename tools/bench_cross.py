"""Cross-activation update throughput (freud_amd/cross_activation.py; include/freud_sae.h sae_cross_update) -- one JSON line, also
written to profiles/cross_bench.json.

Per n in (12 288, 24 576), d = 256, a device-resident batch of 40 files of T = 1500 (60 000 rows) of an L1 SAE whose bias makes a
latent fire on a few per cent of the frames; the masks are those sae_cross_mask_files packs from it (lags 0 and 1):
  cross_update_ms   sae_cross_update, one lag: device events around `iters` back-to-back launches, the best of alternating rounds;
  coact_update_ms   the symmetric update of sae_coact_files at the same n and rows in the same process (the engine's own event
                    bracket "coact_update", profile level 2) -- the upper triangle of tiles only;
  torch_bf16_ms     torch's bf16 matmul of the same two masks, timed like cross_update_ms in the same alternating rounds;
  tile_ratio        the rectangle's tiles over the triangle's, ceil((n + 1) / 128)^2 / (nt (nt + 1) / 2) with nt = n / 128: what the
                    ratio of the two updates should be; measured_ratio = cross_update_ms / coact_update_ms stands beside it;
  cross_update_tops effective i8 TOP/s: 2 * tiles * 128^2 * rows / time.
The lag-0 table must equal the co-activation table of the same batch, and the two lags' margins the frame counts, before any time
is reported.  There is no CPU path: without a GPU the tool fails.

    python tools/bench_cross.py [--iters 10] [--out profiles/cross_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freud_amd import engine as E                                    # noqa: E402
from bench_pass_common import best_alternating                       # noqa: E402
from bench_coact import bracket_ms                                   # noqa: E402

T, B, D = 1500, 40, 256
TILE = 128


def engine(n):
    """An L1 engine whose columns are +-1/16 in all d = 256 places: unit norm exactly, so the renormalisation every forward runs is a
    fixed point and two calls encode alike (the lag-0 table can be held to the co-activation table bit for bit).  x ~ N(0, 1):
    pre-activations ~ N(bias, 1); bias -1.5 fires on about 7 % of the frames."""
    g = torch.Generator().manual_seed(0)
    eng = E.SaeEngine("l1", D, n, -(-B * T // 256) * 256)
    W = torch.where(torch.rand(D, n, generator=g) < 0.5, -1 / 16, 1 / 16)
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": (-1.5 + 0.3 * torch.randn(n, generator=g)).numpy()})
    return eng, torch.randn(B, T, D, generator=g).cuda()


def shape(n, iters):
    eng, x = engine(n)
    M = B * T
    one = E.cross_mask_bytes(n, M)
    masks = torch.empty(3 * one, dtype=torch.int8, device="cuda")
    eng.cross_mask_files(x, masks, E.CROSS_SOURCE | E.CROSS_TARGET, (0, 1))
    src, tgt = masks[:one], (masks[one:2 * one], masks[2 * one:])
    tables = torch.zeros(2, n + 1, n + 1, dtype=torch.int32, device="cuda")
    for l in range(2):
        E.cross_update(src, n, tgt[l], n, M, tables[l])
    coact = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    coact_call = lambda: eng.coact_files(x, coact)
    coact_call()
    torch.cuda.synchronize()
    differ = int((tables[0, :n, :n] != coact).sum())
    if differ or int(tables[0, n, n]) != M or int(tables[1, n, n]) != B * (T - 1):
        raise SystemExit(f"n={n}: {differ} cells of the lag-0 table differ from the co-activation table of the same batch; the pair "
                         f"counts are {int(tables[0, n, n])} and {int(tables[1, n, n])}, expected {M} and {B * (T - 1)}")
    density = float(torch.diagonal(coact).double().mean() / M)
    del coact
    scratch = torch.zeros(n + 1, n + 1, dtype=torch.int32, device="cuda")
    cross_fn = lambda: E.cross_update(src, n, tgt[1], n, M, scratch)
    rows_p, Kp = one // (-(-M // TILE) * TILE), -(-M // TILE) * TILE
    Ma, Mb = src.view(rows_p, Kp).to(torch.bfloat16), tgt[1].view(rows_p, Kp).to(torch.bfloat16)
    out = torch.empty(rows_p, rows_p, dtype=torch.bfloat16, device="cuda")
    MbT = Mb.T
    torch_fn = lambda: torch.matmul(Ma, MbT, out=out)
    cross_ms, torch_ms = best_alternating([cross_fn, torch_fn], iters, rounds=3)
    del Ma, Mb, MbT, out
    coact = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    coact_ms = min(bracket_ms(eng, coact_call, iters, ("coact_update",))[0] for _ in range(3))
    nt, ntc = -(-n // TILE), rows_p // TILE
    tiles, tri = ntc * ntc, nt * (nt + 1) // 2
    res = {"rows": M, "active_fraction": density, "cross_update_ms": cross_ms, "coact_update_ms": coact_ms, "torch_bf16_ms": torch_ms,
           "tile_ratio": tiles / tri, "measured_ratio": cross_ms / coact_ms, "torch_over_cross": torch_ms / cross_ms,
           "cross_update_tops": 2.0 * tiles * TILE * TILE * M / cross_ms / 1e9,
           "coact_update_tops": 2.0 * tri * TILE * TILE * M / coact_ms / 1e9}
    eng.close()
    return {f"n{n}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross measures on the GPU: no device found")
    res = {"tool": "bench_cross", "T": T, "files_per_batch": B, "d": D, "device": torch.cuda.get_device_name(0)}
    for n in (12288, 24576):
        res.update(shape(n, a.iters))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
