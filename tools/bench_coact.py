"""Feature co-activation throughput (freud_amd/coactivation.py; include/freud_sae.h sae_coact_files) -- one JSON line, also written to
profiles/coact_bench.json.

Per shape (d, n) at T = 1500, a device-resident batch of B files of an L1 SAE whose bias makes a latent fire on a few per cent of
the frames:
  update_ms    the i8 MFMA update kernel alone and pack_ms the mask pack alone (the engine's own event brackets, profile level 2,
               around the kernels of sae_coact_files);
  call_ms      the whole sae_coact_files call (encoder GEMM, pack, update);
  torch_ms     the route a user has without it, on the same box: torch bf16 Z.T @ Z of the same 0/1 mask (the mask given, its
               construction not timed);
  update_tops  effective i8 TOP/s of the update counting the upper-triangle 128 x 128 tiles only: 2 * tiles * 128^2 * rows / time;
  torch_over_update   torch_ms / update_ms: >= 1 means the update is at least as fast as the generic matmul.

    python tools/bench_coact.py [--iters 10] [--out profiles/coact_bench.json]
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

T = 1500
TILE = 128


def engine(d, n, B):
    g = torch.Generator().manual_seed(0)
    eng = E.SaeEngine("l1", d, n, -(-B * T // 256) * 256)
    W = torch.empty(d, n)
    torch.nn.init.orthogonal_(W, generator=g)
    # x ~ N(0, 1) and unit columns: pre-activations ~ N(bias, 1); bias -1.5 fires on about 7 % of the frames
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": (-1.5 + 0.3 * torch.randn(n, generator=g)).numpy()})
    return eng, torch.randn(B, T, d, generator=g).cuda()


def bracket_ms(eng, fn, iters, names):
    eng.profile(2)
    eng.kernel_times()
    for _ in range(iters):
        fn()
    kt = eng.kernel_times()
    eng.profile(0)
    return [kt[k][0] / max(1, kt[k][1]) for k in names]


def shape(d, n, B, iters):
    eng, x = engine(d, n, B)
    M = B * T
    table = torch.zeros(n, n, dtype=torch.int32, device="cuda")
    call = lambda: eng.coact_files(x, table)
    call()
    torch.cuda.synchronize()
    density = float(torch.diagonal(table).double().mean() / M)
    # the same mask for torch: the stored latent of an eval of the same rows
    eng.eval(x.reshape(M, d))
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
    Z = (torch.as_tensor(_Alias(), device="cuda")[:, :n].view(torch.bfloat16) > 0).to(torch.bfloat16).contiguous()
    out = torch.empty(n, n, dtype=torch.bfloat16, device="cuda")
    Zt = Z.T
    torch_fn = lambda: torch.matmul(Zt, Z, out=out)
    call_ms, torch_ms = best_alternating([call, torch_fn], iters, rounds=3)
    runs = [bracket_ms(eng, call, iters, ("coact_pack", "coact_update")) for _ in range(3)]
    pack_ms, update_ms = min(r[0] for r in runs), min(r[1] for r in runs)
    nt = -(-n // TILE)
    ops = 2.0 * (nt * (nt + 1) // 2) * TILE * TILE * M
    res = {"files_per_batch": B, "rows": M, "active_fraction": density, "call_ms": call_ms, "pack_ms": pack_ms, "update_ms": update_ms,
           "torch_bf16_ms": torch_ms, "update_tops": ops / update_ms / 1e9, "torch_tflops_full": 2.0 * n * n * M / torch_ms / 1e9,
           "torch_over_update": torch_ms / update_ms}
    eng.close()
    return {f"d{d}_n{n}": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coact_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_coact", "T": T, "device": torch.cuda.get_device_name(0)}
    res.update(shape(384, 3072, 30, a.iters))
    res.update(shape(1280, 40960, 16, a.iters))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
