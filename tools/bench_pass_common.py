"""What tools/bench_search.py and tools/bench_stats.py share: device-event timing, the L1 engine they measure, the alternating
best-of-rounds loop and the reading of the engine's own enc_fwd_gemm brackets."""
import torch

from freud_amd import engine as E


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def l1_engine(d, n, B, T):
    """An L1 engine with orthogonal weights and a small bias, and a device-resident batch x [B, T, d]."""
    g = torch.Generator().manual_seed(0)
    eng = E.SaeEngine("l1", d, n, -(-B * T // 256) * 256)      # (room for an even number of 128-row blocks: the fused path)
    W = torch.empty(d, n)
    torch.nn.init.orthogonal_(W, generator=g)
    eng.set_params({"decoder.weight": W.numpy(), "encoder_bias": (0.01 * torch.randn(n, generator=g)).numpy()})
    return eng, torch.randn(B, T, d, generator=g).cuda()


def best_alternating(fns, iters, rounds=5):
    """Best round of each fn over alternating rounds: the clock of a power-managed chip ramps during the first milliseconds."""
    best = [float("inf")] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timed(fn, iters))
    return best


def enc_gemm_ms(eng, fns, iters):
    """Mean enc_fwd_gemm bracket (HIP events of the engine's profile level 2) per call of each fn, in order."""
    out = []
    eng.profile(2)
    for fn in fns:
        for _ in range(iters):
            fn()
        ms, cnt = eng.kernel_times()["enc_fwd_gemm"]
        out.append(ms / max(1, cnt))
    eng.profile(0)
    return out
