"""Reconstruction report throughput (freud_amd/reconstruction.py; include/freud_sae.h sae_recon_files) -- one JSON line per shape.

Per shape and per kind of data -- the two of bench.py's line: `overfit`, its low-rank batch after --fit_steps training steps on that
one batch (TopK: the low-rank batch as it is), and `normal`, N(0, 1) rows through the initial weights -- on a device-resident batch
of B files of T = 1500 frames:
  recon_ms       sae_recon_files: encode, decode, the residual sweep, the attribution, the fold;
  eval_ms        sae_eval of the same batch in the same process, interleaved with recon_ms: medians over rounds, with the spread;
  recon_decode_ms, recon_resid_ms, recon_attr_ms, enc_gemm_ms   the engine's brackets inside sae_recon_files (attr_streams: the
                 attribution GEMM ran in the streaming form; --unfused: SAE_RECON_UNFUSED, the tile forms);
  dpre_ms        the dpre_gemm bracket of a training step on the same batch (L1, generic backward: the GEMM of EpiAttr's shape);
  torch_ms       (c * (r_b @ W_b)).sum(0) on torch's bf16 matmul: the attribution alone, with the M x n product written (L1);
  recon_vs_eval, attr_vs_dpre, attr_vs_torch   the ratios.

    python tools/bench_recon.py [--iters 10] [--rounds 7] [--fit_steps 60] [--shapes c2,l1_12288,c3,c4] [--unfused]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from bench_pass_common import timed                                  # noqa: E402
from bench_hist import interleaved, brackets, data, T               # noqa: E402

SHAPES = {"c2": ("l1", 384, 3072, 30, 0), "l1_12288": ("l1", 384, 12288, 16, 0), "c3": ("topk", 768, 24576, 16, 64),
          "c4": ("l1", 1280, 40960, 16, 0)}


def run(variant, d, n, B, k, kind, iters, rounds, fit_steps, unfused=False):
    g = torch.Generator().manual_seed(0)
    x = data(kind, B, d, g).cuda()
    M = B * T
    if variant == "l1":
        eng = E.SaeEngine("l1", d, n, -(-M // 256) * 256, optimizer="radam", recon_alpha=1e4, clip_thresh=1.0)
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
        eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": torch.zeros(n).numpy()})
        if kind == "overfit":
            for _ in range(fit_steps):
                eng.step(x.reshape(M, d), 4e-4)
    else:
        eng = E.SaeEngine("topk", d, n, M, k=k, optimizer="adam")
        We = torch.randn(n, d, generator=g) / d ** 0.5
        eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": torch.zeros(n).numpy(), "W_dec": We.numpy(), "b_dec": torch.zeros(d).numpy()})
        eng.set_topk_options(float("inf"), 0)
    block = torch.zeros(E.recon_layout(n, d)["bytes"], dtype=torch.uint8, device="cuda")
    fo = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    recon = lambda: eng.recon_files(x, block, fo, unfused=unfused)
    ev = lambda: eng.eval(x.reshape(M, d))
    (r_med, r_min, r_max), (e_med, e_min, e_max) = interleaved([recon, ev], iters, rounds)
    br = brackets(eng, recon, iters)
    res = {"files_per_batch": B, "rows": M, "recon_ms": r_med, "recon_ms_min": r_min, "recon_ms_max": r_max, "eval_ms": e_med,
           "eval_ms_min": e_min, "eval_ms_max": e_max, "recon_vs_eval": r_med / e_med, "recon_decode_ms": br.get("recon_decode"),
           "recon_resid_ms": br.get("recon_resid"), "recon_attr_ms": br.get("recon_attr_stream", br.get("recon_attr")),
           "attr_streams": "recon_attr_stream" in br}
    if variant == "l1":
        res["enc_gemm_ms"] = br.get("enc_fwd_gemm")
        # the attribution on torch: the same operands, the M x n product materialised
        block.zero_()
        resid = torch.empty(M * d, device="cuda")
        eng.recon_files(x, block, fo, resid=resid)
        r_b = resid.reshape(M, d).bfloat16()
        W_b = torch.from_numpy(eng.get_params()["decoder.weight"]).cuda().bfloat16()
        eng.eval(x.reshape(M, d))
        ptr, ld = eng.latent_buffer()

        class _Alias:
            __cuda_array_interface__ = {"shape": (M, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}
        c = torch.as_tensor(_Alias(), device="cuda").view(torch.bfloat16)[:, :n].clone()
        res["torch_ms"] = timed(lambda: (c * (r_b @ W_b)).sum(0), iters)
        res["attr_vs_torch"] = res["recon_attr_ms"] / res["torch_ms"]
        # the dpre bracket of a training step at the same shape (present where the step runs the generic three-GEMM backward)
        step = brackets(eng, lambda: eng.forward_backward(x.reshape(M, d)), iters)
        res["dpre_ms"] = step.get("dpre_gemm")
        if res["dpre_ms"]:
            res["attr_vs_dpre"] = res["recon_attr_ms"] / res["dpre_ms"]
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--fit_steps", type=int, default=60)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--unfused", action="store_true")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        variant, d, n, B, k = SHAPES[name]
        res = {"tool": "bench_recon", "shape": name, "variant": variant, "d": d, "n": n, "k": k, "T": T,
               "unfused": a.unfused, "device": torch.cuda.get_device_name(0)}
        for kind in ("overfit", "normal"):
            res[kind] = run(variant, d, n, B, k, kind, a.iters, a.rounds, a.fit_steps, a.unfused)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
