"""The file passes share ONE grow-only scratch per context (sae_ctx::pass_scratch, freud_amd/csrc/passes.hip) and every buffer of a
context belongs to one owner (freud_amd/csrc/dev_mem.h).  What that must not change:

* a pass run in a context whose scratch holds other passes' leftovers -- after it grew, after a pass that needs less, after it grew
  again, after a training step and an evaluation -- writes BITWISE what the same call writes in a fresh context in the same state
  (every pass's own GPU test asserts bitwise equality between two runs of itself, so that is the equality here);
* a create / one pass / close loop gives the device its memory back: free memory, read with torch.cuda.mem_get_info from outside
  the engine, does not sink by more than one context's footprint over the loop.

Shapes: d = 96 (padded to 128), n = 300 (padded to 384, three column tiles), files of 37 rows with ragged lengths, at most 9 files:
the padding, the trimmed rows and more than one row block are all there, and every case runs in well under a second."""
import numpy as np
import pytest
import torch

from freud_amd import engine as E

pytestmark = pytest.mark.gpu

D, N, T, F_MAX, K_TOP = 96, 300, 37, 9, 8
MAX_ROWS = F_MAX * T
LENGTHS = [37, 5, 30, 1, 37, 22, 36, 13, 29]


def make(variant):
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(D, N, generator=g) / D ** 0.5).numpy()
    b = (torch.randn(N, generator=g) * 0.3 - 0.5).numpy()
    if variant == "l1":
        eng = E.SaeEngine("l1", D, N, MAX_ROWS, recon_alpha=1e2)
        eng.set_params({"decoder.weight": W, "encoder_bias": b})
    else:
        eng = E.SaeEngine("topk", D, N, MAX_ROWS, k=K_TOP, optimizer="adam")
        eng.set_params({"encoder.weight": np.ascontiguousarray(W.T), "encoder.bias": b, "W_dec": np.ascontiguousarray(W.T),
                        "b_dec": np.zeros(D, np.float32)})
    return eng


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(F_MAX, T, D, generator=g)
    labels = {C: torch.randint(-1, C, (F_MAX, T, 2), generator=g, dtype=torch.int32).cuda() for C in (3, 200)}
    return {"x": x.cuda(), "lengths": torch.tensor(LENGTHS, dtype=torch.int32).cuda(), "labels": labels}


def zeros(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def run_op(eng, op, inp):
    """One pass on the first F files; returns its outputs as bytes."""
    name, F = op[0], op[1]
    x, L = inp["x"][:F].contiguous(), inp["lengths"][:F].contiguous()
    if name == "stats":
        outs = [zeros(E.stats_layout(N)["bytes"], torch.uint8)]
        eng.stats_files(x, outs[0], L)
    elif name == "labels":
        C = op[2]
        outs = [zeros((C + 1, N), torch.int32), zeros(C + 1, torch.int64)]
        eng.label_files(x, inp["labels"][C][:F].contiguous(), C, outs[0], outs[1], L)
    elif name == "recon":
        outs = [zeros(E.recon_layout(N, D)["bytes"], torch.uint8), zeros((F, 2), torch.float64), zeros(F * T * D, torch.float32)]
        eng.recon_files(x, outs[0], outs[1], L, resid=outs[2])
    elif name == "coact":
        outs = [zeros((N, N), torch.int32)]
        eng.coact_files(x, outs[0], L)
    elif name in ("frontier", "pursuit", "refit"):          # (one family: each embeds the same fold pieces in a scratch of its own)
        tau = [0.5, 0.9]
        layout = E.frontier_layout(len(tau), K_TOP, D) if name == "frontier" else getattr(E, name + "_layout")(len(tau), K_TOP, D, N)
        outs = [zeros(layout["bytes"], torch.uint8)]
        getattr(eng, name + "_files")(x, K_TOP, tau, outs[0], L)
    elif name == "manip":
        outs = [zeros(F * T * D, torch.float32), zeros(2 * F * T * D, torch.float32), zeros(2 * F * T, torch.float32)]
        eng.manipulate_files(x, [3, 170], [E.MANIP_OPS["scale"], E.MANIP_OPS["set"]], [[2.0, 0.5], [0.0, 1.0]], *outs)
    elif name == "hist":
        spec = (-10, 14, 1)
        nb = E.hist_nbins(spec)
        outs = [zeros((N, nb), torch.int64), zeros((N, nb), torch.int64), zeros(1, torch.int64)]
        eng.hist_files(x, spec, outs[0], outs[1], outs[2], L)
    elif name == "resample":
        outs = [zeros(F * T, torch.float32), zeros(N, torch.int64)]
        eng.resample_files(x, outs[0], 0, outs[1], L)
    else:
        raise AssertionError(name)
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in outs]


def train_and_eval(eng, inp):
    # x as [files, T, d]: a TopK context normalises by the mean over the files, and the file length it was last told is part of its
    # state (manipulate_files states it as well) -- stated here, it is the same in the seasoned and in the fresh context
    batch = inp["x"][:5].contiguous()
    eng.step(batch, 1e-3)
    eng.eval(batch)
    torch.cuda.synchronize()


# The scratch grows (statistics -> labels, 3 classes), serves a pass that needs less (reconstruction), grows (200 classes: a larger
# label pack), serves less again (co-activation), grows (the frontier's slots), is carved by the frontier's two relatives (the
# pursuit's residuals in front of the fold pieces, the refit's curves behind them), serves the smallest user (manipulation), then --
# after one training step and one evaluation -- histograms over more files than any call before, the two-area resampling pass (L1),
# the statistics again and the three frontier passes one after another in the other order.
SEQUENCE = [("stats", 5), ("labels", 5, 3), ("recon", 5), ("labels", 6, 200), ("coact", 4), ("frontier", 7), ("pursuit", 5), ("refit", 7),
            ("manip", 3), "train", ("hist", 9), ("resample", 6), ("labels", 9, 3), ("stats", 8), ("recon", 9), ("refit", 9), ("pursuit", 9),
            ("frontier", 9)]


@pytest.mark.parametrize("variant", ["l1", "topk"])
def test_every_pass_in_a_used_scratch_matches_a_fresh_context(variant, inputs):
    seq = [op for op in SEQUENCE if not (variant == "topk" and op != "train" and op[0] == "resample")]      # (resampling serves L1 only)
    seasoned = make(variant)
    got = []
    for op in seq:
        if op == "train":
            train_and_eval(seasoned, inputs)
        else:
            got.append(run_op(seasoned, op, inputs))
    seasoned.close()

    trained, i = False, 0
    for op in seq:
        if op == "train":
            trained = True
            continue
        fresh = make(variant)                   # the same parameters, and the same step and evaluation where the sequence had them
        if trained:
            train_and_eval(fresh, inputs)
        want = run_op(fresh, op, inputs)
        fresh.close()
        assert len(want) == len(got[i])
        for j, (a, b) in enumerate(zip(got[i], want)):
            assert a == b, (variant, op, "output", j)
        assert any(any(w) for w in want), (variant, op, "the pass wrote nothing")
        i += 1


def free_bytes():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_create_run_close_gives_the_memory_back(inputs):
    ops = [("stats", 5), ("labels", 5, 3), ("recon", 5), ("coact", 4), ("frontier", 7), ("manip", 3), ("hist", 9), ("labels", 6, 200)]
    warm = make("l1")                           # (warm-up: the code objects and torch's own buffers are loaded before the first reading)
    run_op(warm, ops[0], inputs)
    warm.close()
    footprint = after_first = None
    for it in range(32):
        variant = "topk" if it % 2 else "l1"
        before = free_bytes()
        eng = make(variant)
        if it == 0:
            footprint = before - free_bytes()   # what one context takes, measured across its creation
        run_op(eng, ops[it % len(ops)], inputs)
        eng.eval(inputs["x"][:3].reshape(3 * T, D).contiguous())
        eng.set_eval_precision("fp32")          # the lazily grown evaluation buffers are the owner's as well
        eng.eval(inputs["x"][:3].reshape(3 * T, D).contiguous())
        eng.close()
        if it == 0:
            after_first = free_bytes()
    after_loop = free_bytes()
    print(f"footprint {footprint} bytes; free after the first iteration {after_first}, after the loop {after_loop}")
    # (the footprint is the allowance, nothing more: it reads 0 where the runtime serves a tiny context from memory it kept back
    # from earlier frees in the same process -- the bound is then simply "no lower than after the first iteration")
    assert after_loop >= after_first - max(footprint, 0), (footprint, after_first, after_loop)
