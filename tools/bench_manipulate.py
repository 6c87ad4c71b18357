"""Feature manipulation throughput (freud_amd/manipulate.py; include/freud_sae.h sae_manipulate_files) -- one JSON line, also
written to profiles/manipulate_bench.json.

Per shape at T = 1500, a device-resident batch of B files, one edited latent (SCALE) and V = 1 and V = 8 factors:
  pass_ms          the whole sae_manipulate_files call (eval forward, standard decode, series, apply) into preallocated outputs;
  decode_ms / series_ms / apply_ms   its three event brackets (profile level 2);
  route_ms         the route a user has without it through freud_amd.models, on the same box: forward(x), then per factor
                   decode(edited latent) + decode(standard latent) as the reference's manipulate_latent does (the edit itself in
                   torch on the device: a clone and one column, or for TopK a masked multiply of top_acts);
  route_over_pass  route_ms / pass_ms: >= 1 means the pass is at least as fast.
Best of five alternating rounds.

    python tools/bench_manipulate.py [--iters 3] [--out profiles/manipulate_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freud_amd.config import L1AutoEncoderConfig, TopKAutoEncoderConfig      # noqa: E402
from freud_amd.models import L1AutoEncoder, TopKAutoEncoder                  # noqa: E402
from bench_pass_common import best_alternating                               # noqa: E402

T = 1500
FEAT = 128
FACTORS = [1.5, 0.0, -2.0, 10.0, 0.5, 3.0, -1.0, 5.0]


def model(kind, d, n, k, M):
    torch.manual_seed(0)
    if kind == "l1":
        sae = L1AutoEncoder(d, L1AutoEncoderConfig(n_dict_components=n), max_rows=M)
        sd = sae.state_dict()
        sd["encoder_bias"] = -1.5 + 0.3 * torch.randn(n)
        sd["encoder_bias"][FEAT] = 0.5                        # the edited latent fires on most frames
        sae.load_state_dict(sd)
    else:
        sae = TopKAutoEncoder(d, TopKAutoEncoderConfig(n_dict_components=n, k=k), max_rows=M)
        sd = sae.state_dict()
        sd["encoder.bias"][FEAT] = 1.5
        sae.load_state_dict(sd)
    return sae


def route(kind, sae, x, factors):
    out = sae.forward(x)
    res = []
    for f in factors:
        if kind == "l1":
            lat = out.encoded.latent
            edited = lat.clone()
            edited[:, :, FEAT] = lat[:, :, FEAT] * f
            res.append((sae.decode(edited), sae.decode(lat)))
        else:
            acts, idx = out.encoded.top_acts, out.encoded.top_indices
            edited = torch.where(idx == FEAT, acts * f, acts)
            res.append((sae.decode(edited, idx), sae.decode(acts, idx)))
    return res


def bracket_ms(eng, fn, iters, names):
    eng.profile(2)
    eng.kernel_times()
    for _ in range(iters):
        fn()
    kt = eng.kernel_times()
    eng.profile(0)
    return [kt[k][0] / max(1, kt[k][1]) for k in names]


def shape(kind, d, n, k, B, iters):
    M = B * T
    sae = model(kind, d, n, k, M)
    eng = sae._ensure(M)
    x = torch.randn(B, T, d, generator=torch.Generator().manual_seed(1)).cuda()
    res = {"kind": kind, "files_per_batch": B, "rows": M}
    for V in (1, 8):
        factors = FACTORS[:V]
        standard = torch.empty(B, T, d, device="cuda")
        manipulated = torch.empty(V, B, T, d, device="cuda")
        series = torch.empty(1, B, T, device="cuda")
        vals = np.array([[f] for f in factors], np.float32)
        call = lambda: eng.manipulate_files(x, [FEAT], [0], vals, standard, manipulated, series)
        user = lambda: route(kind, sae, x, factors)
        call()
        torch.cuda.synchronize()
        fired = float((series > 0).float().mean())
        pass_ms, route_ms = best_alternating([call, user], iters, rounds=5)
        runs = [bracket_ms(eng, call, iters, ("manip_decode", "manip_series", "manip_apply")) for _ in range(3)]
        dec, ser, app = (min(r[i] for r in runs) for i in range(3))
        res[f"V{V}"] = {"pass_ms": pass_ms, "decode_ms": dec, "series_ms": ser, "apply_ms": app, "route_ms": route_ms,
                        "route_over_pass": route_ms / pass_ms, "edited_latent_fires": fired}
        del standard, manipulated, series
    eng.close()
    return {f"{kind}_d{d}_n{n}" + (f"_k{k}" if k else ""): res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manipulate_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_manipulate", "T": T, "device": torch.cuda.get_device_name(0)}
    res.update(shape("l1", 384, 3072, 0, 30, a.iters))
    res.update(shape("l1", 1280, 40960, 0, 16, a.iters))
    res.update(shape("topk", 768, 24576, 64, 16, a.iters))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
