"""Feature timing throughput (freud_amd/feature_timing.py; include/freud_sae.h sae_timing_files) -- one JSON line.

At the shapes and the two kinds of data of tools/bench_hist.py (`overfit`: its low-rank batch after --fit_steps training steps, a
sparse latent; `normal`: N(0, 1) rows through the initial weights, about half of an L1 dictionary fires) on a device-resident batch
of B files of T = 1500 frames:
  timing_ms        sae_timing_files: the encoder that stores the latent (TopK: the eval forward) + the timing kernels;
  hist_ms          the activation histogram pass on the same batch, interleaved with timing_ms -- it reads the same bytes in the same
                   pattern, so it is the yardstick: median over rounds, with the spread (min, max);
  timing_kernels_ms, hist_kernels_ms   the engine's `timing` and `hist` brackets: every kernel of the call after the encoder;
  torch_ms         a torch route on the SAME mask (the stored latent of the last eval, or the scatter of the selection): the mask
                   transposed to [file, latent, frame] and padded, diff, nonzero for the starts and the ends of the runs, searchsorted
                   over the edges and bincount for both histograms (no totals, no bridge); the encoder is not part of it;
  kernels_vs_hist_kernels, timing_vs_hist, torch_vs_timing_kernels   the ratios;
  torch_abs_diff   sum |torch route's histograms - the engine's| over both arrays (bridge 0, threshold 0).  The two see two different
                   forwards: 0 where every forward sees the same weights; an L1 context renormalises its weights in place at the
                   start of every forward, and where those are no fixed point of that a few near-zero latents change sides.

    python tools/bench_timing.py [--iters 5] [--rounds 5] [--fit_steps 60]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freud_amd import engine as E                                    # noqa: E402
from freud_amd.feature_timing import lower_edges                     # noqa: E402
from bench_pass_common import timed                                  # noqa: E402
from bench_hist import SPEC, T, brackets, data, interleaved          # noqa: E402

SUB_BITS = 2


def latent_mask(eng, variant, x, n):
    """bool [B, T, n]: the active frames of the batch, from the context a plain eval leaves."""
    B, _, d = x.shape
    eng.eval(x.reshape(B * T, d))
    ptr, ld = eng.latent_buffer()

    class _Alias:
        __cuda_array_interface__ = {"shape": (B * T, ld), "typestr": "<i2", "data": (ptr, False), "version": 2}

    lat = torch.as_tensor(_Alias(), device="cuda")[:, :n]
    if variant == "topk":
        idx = eng.topk_indices_tensor(B * T, "cuda").long()
        sel = torch.zeros(B * T, n, dtype=torch.bool, device="cuda")
        sel.scatter_(1, idx, (torch.gather(lat, 1, idx) & 0x7FFF) > 0)
        return sel.reshape(B, T, n)
    return ((lat & 0x7FFF) > 0).reshape(B, T, n)


def torch_route(mask, nb, edges):
    """run_hist, gap_hist [n, nb] of a bool mask [B, T, n] at bridge 0."""
    B, _, n = mask.shape
    m = torch.nn.functional.pad(mask.permute(0, 2, 1).to(torch.int8), (1, 1))        # [B, n, T + 2]
    dlt = torch.diff(m, dim=2)
    s = (dlt == 1).nonzero()                                                          # (file, latent, first frame), in that order
    e = (dlt == -1).nonzero()                                                         # (file, latent, last frame + 1): the same runs
    dur = e[:, 2] - s[:, 2]
    rb = torch.searchsorted(edges, dur, right=True) - 1
    run_hist = torch.bincount(s[:, 1] * nb + rb, minlength=n * nb).reshape(n, nb)
    same = (s[1:, 0] == s[:-1, 0]) & (s[1:, 1] == s[:-1, 1])
    gap = (s[1:, 2] - e[:-1, 2])[same]
    gb = torch.searchsorted(edges, gap, right=True) - 1
    gap_hist = torch.bincount(s[1:, 1][same] * nb + gb, minlength=n * nb).reshape(n, nb)
    return run_hist, gap_hist


def run(variant, d, n, B, k, kind, iters, rounds, fit_steps):
    g = torch.Generator().manual_seed(0)
    x = data(kind, B, d, g).cuda()
    if variant == "l1":
        eng = E.SaeEngine("l1", d, n, -(-B * T // 256) * 256, optimizer="radam", recon_alpha=1e4, clip_thresh=1.0)
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
        eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": torch.zeros(n).numpy()})
        if kind == "overfit":
            for _ in range(fit_steps):
                eng.step(x.reshape(B * T, d), 4e-4)
    else:
        eng = E.SaeEngine("topk", d, n, B * T, k=k, optimizer="adam")
        We = torch.randn(n, d, generator=g) / d ** 0.5
        eng.set_params({"encoder.weight": We.numpy(), "encoder.bias": torch.zeros(n).numpy(), "W_dec": We.numpy(), "b_dec": torch.zeros(d).numpy()})
        eng.set_topk_options(float("inf"), 0)
    nb, hb = E.timing_nbins(SUB_BITS, T), E.hist_nbins(SPEC)
    rh = torch.zeros(n, nb, dtype=torch.int64, device="cuda")
    gh, tt, nf = torch.zeros_like(rh), torch.zeros(n, E.TIMING_NTOTALS, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    fh = torch.zeros(n, hb, dtype=torch.int64, device="cuda")
    mh, hf = torch.zeros_like(fh), torch.zeros(1, dtype=torch.int64, device="cuda")
    timing = lambda: eng.timing_files(x, SUB_BITS, 0, 0, rh, gh, tt, nf)
    hist = lambda: eng.hist_files(x, SPEC, fh, mh, hf)
    (t_med, t_min, t_max), (h_med, h_min, h_max) = interleaved([timing, hist], iters, rounds)
    bt, bh = brackets(eng, timing, iters), brackets(eng, hist, iters)
    for t in (rh, gh, tt, nf):
        t.zero_()
    timing()
    torch.cuda.synchronize()
    runs, active = int(tt[:, E.TIMING_RUNS].sum().item()), int(tt[:, E.TIMING_ACTIVE].sum().item())
    mask = latent_mask(eng, variant, x, n)
    edges = torch.from_numpy(lower_edges(SUB_BITS, nb)).cuda()
    route = lambda: torch_route(mask, nb, edges)
    torch_ms = min(timed(route, 2) for _ in range(3))
    r2, g2 = route()
    off = int((r2 - rh).abs().sum().item()) + int((g2 - gh).abs().sum().item())
    res = {"files_per_batch": B, "active_fraction": active / (B * T * n), "runs": runs, "mean_duration": active / max(1, runs),
           "timing_ms": t_med, "timing_ms_min": t_min, "timing_ms_max": t_max, "hist_ms": h_med, "hist_ms_min": h_min, "hist_ms_max": h_max,
           "timing_vs_hist": t_med / h_med, "timing_kernels_ms": bt.get("timing"), "hist_kernels_ms": bh.get("hist"),
           "kernels_vs_hist_kernels": bt["timing"] / bh["hist"], "torch_ms": torch_ms, "torch_vs_timing_kernels": torch_ms / bt["timing"],
           "torch_abs_diff": off}
    if variant == "l1":
        n_p = -(-n // 128) * 128
        res.update({"enc_gemm_ms": bt.get("enc_fwd_gemm"), "latent_gb_s": B * T * n_p * 2 / (bt["timing"] * 1e-3) / 1e9})
    del mask
    eng.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fit_steps", type=int, default=60)
    a = ap.parse_args()
    res = {"tool": "bench_timing", "T": T, "sub_bits": SUB_BITS, "device": torch.cuda.get_device_name(0)}
    for name, args in (("l1_d384_n3072", ("l1", 384, 3072, 30, 0)), ("l1_d1280_n40960", ("l1", 1280, 40960, 16, 0)),
                       ("topk_d768_n24576_k64", ("topk", 768, 24576, 16, 64))):
        for kind in ("overfit", "normal"):
            res[f"{name}_{kind}"] = run(*args, kind, a.iters, a.rounds, a.fit_steps)
            print(f"# {name}_{kind}: {json.dumps(res[f'{name}_{kind}'])}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
