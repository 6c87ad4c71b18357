"""Float64 reference, per-element error bounds, planted inputs and a mirror of the row partition for the fused d = 384 L1 step
(csrc/fwd_split.h / fwd_fused2.h / fwd_fused.h, csrc/bwd_fused.h: bwd_fused_d384_kernel, csrc/l1_kernels.h: reduce_grads_kernel).
No GPU use.  Shared by tests/test_l1_step_bound_cpu.py and tests/test_l1_step_gpu.py.

The operands, exactly what the kernels read, widened to float64 here:

    xb[r][:]    the bf16 GEMM operand: the input itself if it is bf16, else its conversion as prep_x_kernel makes it (l1_kernels.h:
                89-126: `(bf16_t)f`, round to nearest even -- what CPU autocast's x.to(bfloat16) gives).  This is NOT the loader's rule
                of csrc/bf16_guard.h (to_bf16_loader below), which moves a value that is not -1.0 but rounds to it to the neighbouring
                bf16: the engine takes the mask from the ORIGINAL input (fwd_split.h:572, :593), so an fp32 / fp16 value that rounds to
                -1.0 stays unmasked without the guard.  The recipe's batches hold a few hundred such values; operands() counts them
                (guard_moved), and on those elements a reference under the loader's rule would be off by 2^-7
    xT[r][:]    the original input (fp32 / fp16 / bf16), for the residual and the mask
    wt[j][:]    Wt as the kernels read it (sae_debug_read 15): bf16 of the normalised master
    b[j]        the fp32 encoder bias
    c^[r][j]    the stored bf16 latent (sae_debug_read 0);   g^[r][:]  the stored bf16, UNSCALED dx_hat (sae_debug_read 1)
    count = M d - #(xT == -1),  scale = alpha / count,  inv_m = (1 / M) / scale

Conventions (tests/decode_reference.py, tests/topk_backward_reference.py): u = 2^-23 per fp32 addition, which also admits MFMA
accumulators that do not round to nearest; R8 = 2^-8 per bf16 rounding (8 significant bits: half an ulp of 2^-7, the
round-to-nearest bound itself); S = the dot product of the absolute
values; a product of two bf16 values is exact in fp32.

Forward (fwd_fused.h:3-7; the same arithmetic in fwd_fused2.h and fwd_split.h:230-242, :555-615), from (xb, xT, wt, b) and the stored c^:

    s = xb[r] . wt[j],  S = |xb[r]| . |wt[j]|
    c_ref = relu(s + b_j)            tol_c  = R8 |s| + R8 |c_ref| + (d_p + 2) u (S + |b_j|)  +  R8 (R8 |s| + (d_p + 2) u (S + |b_j|))
    xh_ref[r][i] = sum_j c^[r][j] wt[j][i]   (from the STORED latent: forward errors do not compound)
                                     tol_xh = R8 |xh_ref| + (1 + R8) (L_r + 2) u sum_j |c^ wt|,      L_r = #(c^[r] != 0)
    g_ref = 2 (xh_ref - xT) [xT != -1]
                                     tol_g  = (1 + R8) (2 tol_xh + 4 u (|xh_ref| + |xT|)) + R8 |g_ref|;   0 on masked entries

  * c: the d_p products are accumulated in fp32 in any order: d_p u S; the accumulator is rounded to bf16 BEFORE the bias add
    (fwd_split.h:230): R8 |s|; the fp32 bias add: u (|s| + |b|) <= u (S + |b|); the ReLU is 1-Lipschitz; the store rounds once more:
    R8 |c_ref|.  The last summand is the product of the store's rounding with the error made before it.
  * xh: zeros of c^ add exact zeros, so only L_r products count; bf16_round(acc) (fwd_split.h:555): R8 |xh_ref|.
  * g: e = xh - x is one fp32 subtraction (u (|xh| + |x|), 4 u leaves room for the conversion of x and the second order), e + e is
    exact, the store rounds to bf16: R8 on the computed value, hence the factor 1 + R8 on the error that precedes it.  keep * ... and
    the selects of the masked blocks write +-0.0 on a masked entry.

Backward (bwd_fused.h:3-6, :302-307, :386-425, :448-463), from (g^, c^, xb, wt), per latent j:

    s_r = g^[r] . wt[j],  S_r = |g^[r]| . |wt[j]|,  gate_r = [c^[r][j] > 0]
    p_r = gate_r (s_r + inv_m)               tau_r = gate_r (R8 |p_r| + (d_p + 4) u (S_r + inv_m))
    L_j = #rows with gate_r = 1,   P_j = slab pieces of column j's 128-column tile (bal_pieces(tile, bal_m), or `splits`)
    dW_ref[i][j] = scale sum_r (g^[r][i] c^[r][j] + xb[r][i] p_r)
        tol_dW = scale [ sum_r tau_r |xb[r][i]|  +  (2 L_j + P_j + 3) u sum_r (|g^ c^| + |xb| (|p_r| + tau_r)) ]
    db_ref[j] = scale sum_r p_r
        tol_db = scale [ sum_r gate_r (d_p + 4) u (S_r + inv_m)  +  (L_j + P_j + 3) u sum_r |p_r| ]

  * p^ = bf16(fp32 accumulator that STARTED at inv_m) (:305-307, :389): d_p products and the start value in any order, (d_p + 1) u
    (S_r + inv_m); inv_m itself comes out of two float divisions (alpha / (float)count, then (1 / M) / that, :173-181) that need not be
    correctly rounded: with 4 u instead of 1 u there is room for them and for the second order.  The pack rounds once: R8 |p_r| (:421).
    A gated-off element is exactly 0 (:419).
  * dW: the products g^ c^ and xb p^ are exact.  Rows with c^ = 0 add exact zeros to both chains (c^ = 0 implies p^ = 0), so the chain
    of one element has 2 L_j real additions in a piece, whatever the segment boundaries; the pieces are added in fp32 by
    reduce_grads_kernel: P_j - 1; each piece is multiplied by the float scale (:458): one rounding of the product and one of the division
    that formed scale.  (2 L_j + P_j + 3) u of the sum of the magnitudes covers them in any association.
  * db adds the UNROUNDED fp32 gated accumulator (:420): no R8 term; 16 registers per lane, one cross-lane add (:462), L_j real terms.
  * A dead latent (L_j = 0) has tol = 0: its dW column and db must be +0.0 to the bit (the slab pieces are acc = 0.f times scale).

Nothing in a bound is measured on the code under test.  tests/test_l1_step_bound_cpu.py keeps the bounds honest: a float32 emulation of
the backward (emulate) violates them nowhere, each failure mode of the partition, the piece indexing, the reduction and the gate violates
them (or an exact check of the GPU test) on the latents it hits.

The partition (partition): the Python mirror of bwd_fused.h:318-335 with bal_first_wg / bal_pieces of common.h: every workgroup's
segments (tile, step_begin, step_end, piece) in 32-row steps.

Planted inputs (make_case): the random low-rank recipe of tests/test_engine_gpu.py::test_l1_step_matches_oracle with 50 masked entries,
plus planted latents: latent p owns input column c_p; W[:, p] = e_{c_p} (unit norm: the engine's normalisation leaves it exactly), every
other latent is 0 in row c_p, b_p = -1, x[r][c_p] = 8 on p's row set and 0 elsewhere: c^ = 7 on the row set and relu(-1) = 0 off it,
exactly.  The row sets come from the partition (ROW_KINDS), the latents sit at the column positions where the kernels change owner
(column_positions).  The dead latent has b = -100 (L = 0), the hot latent a zero column and b = +6 (c^ = 6 on every row, L = M)."""
import numpy as np
import torch

from tests.decode_reference import as_f32, bf16, bits, round_up

U = 2.0 ** -23
R8 = 2.0 ** -8
D_P = 384
BM = 32                        # rows per step (BF_BM)
BN = 128                       # columns per tile (BF_BN)
FWD_ROWS = 128                 # rows per forward workgroup (FF_BM)
DW_FUSED = 0                   # DwForm of the one-launch fused backward
ALPHA = 1e4
PLANT_BIAS, HOT_BIAS, DEAD_BIAS, PLANT_X = -1.0, 6.0, -100.0, 8.0
N_MASKED = 50
ROW_KINDS = ("row0", "row_last", "ragged", "seg_ends", "clamped_step", "each_piece")


# ---- the partition -------------------------------------------------------------------------------------------------------------------
def bal_first_wg(j, m):
    return (32 * j) // m


def bal_pieces(j, m):
    return (32 * j + 31) // m - (32 * j) // m + 1


def make_plan(splits, steps, ntiles, bal_m=0):
    """A plan dict as SaeEngine.l1_backward_plan reports it (form DW_FUSED)."""
    if bal_m:
        return {"form": DW_FUSED, "splits": splits, "balanced": 1, "bal_m": bal_m, "bal_q": (steps + 31) // 32,
                "grid": (32 * ntiles + bal_m - 1) // bal_m, "steps": steps, "ntiles": ntiles}
    return {"form": DW_FUSED, "splits": splits, "balanced": 0, "bal_m": 0, "bal_q": 0, "grid": ntiles * splits, "steps": steps, "ntiles": ntiles}


# name -> (d, n, max_rows, M, x dtype, debug_flags, seed, plan): the batches of tests/test_l1_step_gpu.py and the plan sae_create's cost
# model (engine.hip: fused_bwd_splits, l1_create) and dw_plan give them -- hard-coded here, asserted against SaeEngine.l1_backward_plan
# on the GPU.  The balanced form is chosen at max_rows >= 31 744 (n = 3072, m = 3), >= 25 600 (n = 5000, m = 5), >= 4096 (n = 12 288,
# m = 12), never for n_p <= 4224 otherwise, and runs for batches of at least 64 steps.
CASES = {
    "uniform": (384, 3072, 1000, 1000, "bfloat16", 0, 11, make_plan(4, 32, 24)),
    "alias": (384, 1024, 2048, 2048, "bfloat16", 0, 12, make_plan(11, 64, 8)),
    "pad_d": (380, 200, 1500, 1500, "float16", 0, 13, make_plan(16, 48, 2)),
    "fp32_x": (384, 3072, 1024, 1024, "float32", 0, 14, make_plan(4, 32, 24)),
    "bal_m3": (384, 3072, 31744, 2100, "bfloat16", 0, 15, make_plan(10, 68, 24, 3)),
    "bal_m5": (384, 5000, 25600, 3000, "float32", 0, 16, make_plan(6, 96, 40, 5)),
    "bal_m12": (384, 12288, 4096, 2048, "bfloat16", 0, 17, make_plan(2, 64, 96, 12)),
    "bal_as_uniform": (384, 3072, 31744, 2100, "bfloat16", 83, 15, make_plan(10, 68, 24)),
    "bal_scal": (384, 3072, 31744, 2100, "bfloat16", 78, 15, make_plan(10, 68, 24, 3)),
    "second_step_700": (384, 3072, 31744, 700, "bfloat16", 0, 18, make_plan(10, 24, 24)),
    "second_step_2048": (384, 3072, 31744, 2048, "bfloat16", 0, 19, make_plan(10, 64, 24, 3)),
    "after_update": (384, 3072, 1000, 1000, "bfloat16", 0, 11, make_plan(4, 32, 24)),
}


INPUTS_OF = {"bal_as_uniform": "bal_m3", "bal_scal": "bal_m3", "after_update": "uniform"}     # cases that run another case's batch


def case_of(name):
    """The inputs of a case (planted for the partition of the case whose batch it runs)."""
    d, n, _, M, dtype, _, seed, plan = CASES[INPUTS_OF.get(name, name)]
    return make_case(d, n, M, plan, getattr(torch, dtype), seed)


def pieces_per_tile(plan):
    """P_j: the slab pieces reduce_grads_kernel adds for column tile j."""
    if plan["balanced"]:
        return np.array([bal_pieces(j, plan["bal_m"]) for j in range(plan["ntiles"])], np.int64)
    return np.full(plan["ntiles"], plan["splits"], np.int64)


def partition_arrays(plan):
    """Every segment of every workgroup as int64 arrays (wg, tile, step_begin, step_end, piece), workgroup-major, a workgroup's
    segments in the order it walks them.  Empty step ranges included: the kernel writes their zero slab piece all the same.
    Balanced (bwd_fused.h:158-162, :318-326): workgroup k takes the quanta [k m, min((k + 1) m, 32 ntiles)); a segment is their part
    inside one tile j: quanta qa .. qb -> steps min((qa - 32 j) q, steps) .. min((qb - 32 j) q, steps), piece k - bal_first_wg(j, m).
    Uniform (:327-335): workgroup i -> split i / ntiles, tile i % ntiles, steps floor(steps split / splits) .. floor(steps (split + 1) /
    splits) (the kernel's xcd_remap permutes the block numbers, not the set of workgroups)."""
    steps, ntiles = plan["steps"], plan["ntiles"]
    if plan["balanced"]:
        m, q = plan["bal_m"], plan["bal_q"]
        k = np.arange(plan["grid"], dtype=np.int64)
        qa0, qe = k * m, np.minimum(k * m + m, 32 * ntiles)
        nseg = np.where(qa0 < qe, ((qe - 1) >> 5) - (qa0 >> 5) + 1, 0)
        wg = np.repeat(k, nseg)
        first = np.cumsum(nseg) - nseg
        tile = np.repeat(qa0 >> 5, nseg) + (np.arange(nseg.sum()) - np.repeat(first, nseg))
        qa, qb = np.maximum(qa0[wg], 32 * tile), np.minimum(qe[wg], 32 * (tile + 1))
        s0, s1 = np.minimum((qa - 32 * tile) * q, steps), np.minimum((qb - 32 * tile) * q, steps)
        return wg, tile, s0, s1, wg - (32 * tile) // m
    sp = plan["splits"]
    i = np.arange(ntiles * sp, dtype=np.int64)
    split = i // ntiles
    return i, i - split * ntiles, steps * split // sp, steps * (split + 1) // sp, split


def check_partition(plan, arrays=None):
    """Each (tile, step) is covered exactly once; every piece 0 .. P_j - 1 of every tile is written exactly once and no other."""
    steps, ntiles = plan["steps"], plan["ntiles"]
    wg, tile, s0, s1, piece = partition_arrays(plan) if arrays is None else arrays
    assert ((tile >= 0) & (tile < ntiles) & (s0 >= 0) & (s0 <= s1) & (s1 <= steps)).all(), "a segment lies outside the launch"
    size = ntiles * (steps + 1)
    diff = np.bincount(tile * (steps + 1) + s0, minlength=size) - np.bincount(tile * (steps + 1) + s1, minlength=size)
    cover = np.cumsum(diff.reshape(ntiles, steps + 1), 1)[:, :steps]
    assert (cover == 1).all(), f"{int((cover != 1).sum())} (tile, step) pairs are not covered exactly once"
    P = pieces_per_tile(plan)
    assert (piece >= 0).all() and (piece < P[tile]).all(), "a piece is written that the reduction does not add"
    width = int(P.max())
    written = np.bincount(tile * width + piece, minlength=ntiles * width).reshape(ntiles, width)
    assert (written == (np.arange(width)[None, :] < P[:, None])).all(), "the pieces of a tile are not 0 .. P_j - 1, once each"


def partition(plan, check=True):
    """-> [workgroup] -> [(tile, step_begin, step_end, piece)] of partition_arrays; check: check_partition."""
    arrays = partition_arrays(plan)
    if check:
        check_partition(plan, arrays)
    wgs = [[] for _ in range(plan["grid"])]
    for k, j, s0, s1, piece in zip(*(a.tolist() for a in arrays)):
        wgs[k].append((j, s0, s1, piece))
    return wgs


def tile_segments(wgs, ntiles):
    """-> [tile] -> [(step_begin, step_end, piece, workgroup)] sorted by piece."""
    out = [[] for _ in range(ntiles)]
    for k, segs in enumerate(wgs):
        for j, s0, s1, piece in segs:
            out[j].append((s0, s1, piece, k))
    return [sorted(v, key=lambda t: t[2]) for v in out]


def straddled_tiles(wgs):
    """Tiles that are the SECOND (or later) segment of a workgroup with a non-empty first one."""
    return sorted({segs[i][0] for segs in wgs for i in range(1, len(segs))})


def clamped_steps(plan):
    """The steps of the quantum that the clamp at steps_total cuts short (balanced form, steps no multiple of bal_q); else none."""
    if not plan["balanced"] or plan["steps"] % plan["bal_q"] == 0:
        return []
    q, steps = plan["bal_q"], plan["steps"]
    return list(range(steps // q * q, steps))


# ---- planted inputs ------------------------------------------------------------------------------------------------------------------
def to_bf16_loader(x32):
    """fp32 -> bf16 by the loader's rule (csrc/bf16_guard.h: bg_f32_bits_to_bf16), as float32 numpy."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    b = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    b = np.where(nan, (u >> 16) | 0x40, b)
    guard = (b == 0xBF80) & (u != 0xBF800000)
    b = np.where(guard, np.where(u > 0xBF800000, 0xBF81, 0xBF7F), b)
    return (b.astype(np.uint32) << 16).view(np.float32)


def _real_rows(s0, s1, M):
    return np.arange(s0 * BM, min(s1 * BM, M), dtype=np.int64)


def row_sets(kind, M, plan, segs):
    """The row set of one ROW_KIND for a latent whose tile has the segments segs [(step_begin, step_end, piece, wg)]."""
    live = [(s0, s1) for s0, s1, _, _ in segs if len(_real_rows(s0, s1, M))]
    if kind == "row0":
        return np.array([0])
    if kind == "row_last":
        return np.array([M - 1])
    if kind == "ragged":          # one row of the ragged last 128-row block of the forward (M a multiple of 128: of the last block)
        return np.array([M // FWD_ROWS * FWD_ROWS + (M % FWD_ROWS) // 2 if M % FWD_ROWS else M - FWD_ROWS // 2])
    if kind == "seg_ends":        # first and last row of a segment in the middle of the tile's rows
        rows = _real_rows(*live[len(live) // 2], M)
        return np.unique([rows[0], rows[-1]])
    if kind == "clamped_step":    # every row of the last step of the clamped quantum that holds real rows; without a clamp: of the last step
        cl = [s for s in clamped_steps(plan) if s * BM < M] or [(M - 1) // BM]
        return _real_rows(cl[-1], cl[-1] + 1, M)
    if kind == "each_piece":      # one row in every piece of the tile (the middle one)
        return np.array([_real_rows(s0, s1, M)[len(_real_rows(s0, s1, M)) // 2] for s0, s1 in live])
    raise AssertionError(kind)


def column_positions(n, plan, wgs):
    """{name: latent} at the columns where the kernels change owner."""
    ntiles = plan["ntiles"]
    t = min(1, n // BN - 1) if n >= BN else 0
    pos = {"tile_first": BN * t, "wave_end": BN * t + 31, "wave_begin": BN * t + 32, "tile_last": BN * t + 127,
           "last_tile": BN * (ntiles - 1) + min(3, n - 1 - BN * (ntiles - 1)), "column_last": n - 1}
    st = [j for j in straddled_tiles(wgs) if BN * j + 40 < n]
    if st:
        j = st[len(st) // 2]
        pos["straddle_second"] = BN * j + 40
        pos["straddle_first"] = BN * (j - 1) + 90
    out, seen = {}, set()
    for name, p in pos.items():
        if 0 <= p < n and p not in seen:
            out[name] = p
            seen.add(p)
    return out


def make_case(d, n, M, plan, x_dtype, seed):
    """-> case dict: W [d][n], b [n] (fp32 torch), x [M][d] (torch, x_dtype), planted {latent: (column kind, row kind, rows, c_p)},
    dead, hot, masked (the number of -1 entries), plan."""
    assert round_up(d, 128) == D_P and plan["ntiles"] == round_up(n, BN) // BN and plan["steps"] == round_up(M, FWD_ROWS) // BM
    wgs = partition(plan)
    tsegs = tile_segments(wgs, plan["ntiles"])
    g = torch.Generator().manual_seed(seed)
    if n <= 8192:
        W = torch.empty(d, n)
        torch.nn.init.orthogonal_(W, generator=g)
    else:
        W = torch.randn(d, n, generator=g) / d ** 0.5
    b = 0.01 * torch.randn(n, generator=g)
    x = (torch.relu(torch.randn(M, 64, generator=g)) * 0.1) @ torch.randn(64, d, generator=g)
    cols = column_positions(n, plan, wgs)
    taken = set(cols.values())
    free = [j for j in range(min(n, BN) - 1, -1, -1) if j not in taken]
    dead, hot = free[0], free[1]
    names = list(cols)
    kinds = [ROW_KINDS[i % len(ROW_KINDS)] for i in range(len(names))]
    own = np.linspace(1, d - 2, len(names)).round().astype(np.int64)
    assert len(set(own)) == len(names)
    # masked entries: anywhere but the planted input columns
    others = np.setdiff1d(np.arange(d), own)
    mr = torch.randint(0, M, (N_MASKED,), generator=g).numpy()
    mc = others[torch.randint(0, len(others), (N_MASKED,), generator=g).numpy()]
    x[mr, mc] = -1.0
    W[own, :] = 0
    x[:, own] = 0
    planted = {}
    for name, kind, c_p in zip(names, kinds, own):
        p = cols[name]
        rows = np.asarray(row_sets(kind, M, plan, tsegs[p // BN]), np.int64)
        W[:, p] = 0
        W[c_p, p] = 1.0
        b[p] = PLANT_BIAS
        x[rows, c_p] = PLANT_X
        planted[p] = (name, kind, rows, int(c_p))
    W[:, hot] = 0
    b[hot] = HOT_BIAS
    b[dead] = DEAD_BIAS
    x = x.to(x_dtype)
    masked = int((x == -1.0).sum())
    return {"d": d, "n": n, "M": M, "W": W, "b": b, "x": x, "planted": planted, "dead": dead, "hot": hot, "masked": masked,
            "plan": dict(plan), "alpha": ALPHA}


def assert_coverage(case, c_hat, exact=True):
    """The planted structure holds on a latent (the oracle's, or the engine's own): a condition on the INPUTS of the backward, raised as
    an AssertionError -- never a skip.  exact=False (weights that an optimizer step has moved): the row sets must hold, the
    activations need not be exactly 7 and 6."""
    M, plan = case["M"], case["plan"]
    c_hat = np.asarray(c_hat, np.float32)
    wgs = partition(plan)
    tsegs = tile_segments(wgs, plan["ntiles"])
    for p, (name, kind, rows, _) in case["planted"].items():
        on = np.flatnonzero(c_hat[:, p])
        assert np.array_equal(on, np.sort(rows)), f"planted latent {p} ({name}, {kind}) fires on rows {on[:8]}..., planted {np.sort(rows)[:8]}..."
        assert not exact or (c_hat[rows, p] == PLANT_X + PLANT_BIAS).all(), f"planted latent {p}: activations {np.unique(c_hat[rows, p])}, wanted 7"
    # (an optimizer step turns the hot latent's zero column into a unit vector: it fires on every row only before the first update)
    assert not exact or (c_hat[:, case["hot"]] == HOT_BIAS).all(), "the hot latent does not fire with 6 on every row"
    assert not c_hat[:, case["dead"]].any(), "the dead latent fires"
    kinds = {kind for _, kind, _, _ in case["planted"].values()}
    assert kinds == set(ROW_KINDS), f"row kinds not planted: {sorted(set(ROW_KINDS) - kinds)}"
    names = {name for name, _, _, _ in case["planted"].values()}
    need = {"tile_first", "tile_last", "last_tile", "column_last"} | ({"wave_end", "wave_begin"} if case["n"] >= BN else set())
    if straddled_tiles(wgs):
        need |= {"straddle_first", "straddle_second"}
    assert need <= names, f"column positions not planted: {sorted(need - names)}"
    for p, (name, kind, rows, _) in case["planted"].items():
        segs = tsegs[p // BN]
        if kind == "each_piece":
            for s0, s1, piece, _ in segs:
                real = _real_rows(s0, s1, M)
                assert len(real) == 0 or np.isin(rows, real).sum() == 1, f"latent {p}: piece {piece} holds {np.isin(rows, real).sum()} planted rows"
        if kind == "seg_ends":
            assert any(len(r) and r[0] in rows and r[-1] in rows for r in (_real_rows(s0, s1, M) for s0, s1, _, _ in segs))
        if kind == "clamped_step":
            assert len(rows) == min(BM, M - rows[0]) and rows[0] % BM == 0
            cl = [s for s in clamped_steps(plan) if s * BM < M]
            assert not cl or rows[0] // BM == cl[-1]
        if kind == "ragged":
            assert rows[0] >= (M - 1) // FWD_ROWS * FWD_ROWS
    for name in ("straddle_first", "straddle_second"):
        if name in names:
            p = next(q for q, v in case["planted"].items() if v[0] == name)
            k2 = [k for k, segs in enumerate(wgs) if len(segs) > 1 and p // BN in (segs[0][0], segs[1][0])]
            assert k2, f"latent {p}: its tile belongs to no straddling workgroup"


# ---- operands and references ---------------------------------------------------------------------------------------------------------
def _is_bf16(a):
    return not (bits(a) & 0xFFFF).any()


def operands(x, wt, b, c_hat, g_hat, alpha):
    """x: [M][d] as the engine received it (torch); wt [n][d], c_hat [M][n], g_hat [M][d]: bf16 values as float32; b [n] fp32."""
    xT = as_f32(x)
    M, d = xT.shape
    xb = xT if x.dtype == torch.bfloat16 else bf16(xT)
    guard_moved = int((bits(to_bf16_loader(xT)) != bits(xb)).sum())
    wt, c_hat, g_hat = as_f32(wt), as_f32(c_hat), as_f32(g_hat)
    assert wt.shape[1] == d and c_hat.shape == (M, wt.shape[0]) and g_hat.shape == (M, d)
    assert _is_bf16(wt) and _is_bf16(c_hat) and _is_bf16(g_hat), "operands of the fused step are bf16 values"
    count = M * d - int((xT == -1.0).sum())
    scale = alpha / count
    return {"M": M, "d": d, "n": wt.shape[0], "xb": xb, "xT": xT, "wt": wt, "b": as_f32(b), "c": c_hat, "g": g_hat, "count": count,
            "alpha": alpha, "scale": scale, "inv_m": (1.0 / M) / scale, "guard_moved": guard_moved}


CHUNK = 2048                   # latents per block of the float64 products


def forward_reference(ops):
    """-> {"c": (ref, tol) [M][n], "g": (ref, tol) [M][d]} in float64."""
    M, d, n = ops["M"], ops["d"], ops["n"]
    xb, xT = ops["xb"].astype(np.float64), ops["xT"].astype(np.float64)
    axb = np.abs(xb)
    c_ref, c_tol = np.empty((M, n)), np.empty((M, n))
    xh, xh_abs = np.zeros((M, d)), np.zeros((M, d))
    for j0 in range(0, n, CHUNK):
        wt = ops["wt"][j0:j0 + CHUNK].astype(np.float64)
        bj = ops["b"][j0:j0 + CHUNK].astype(np.float64)[None, :]
        s, S = xb @ wt.T, axb @ np.abs(wt).T
        ref = np.maximum(s + bj, 0.0)
        before = R8 * np.abs(s) + (D_P + 2) * U * (S + np.abs(bj))
        c_ref[:, j0:j0 + CHUNK] = ref
        c_tol[:, j0:j0 + CHUNK] = before + R8 * ref + R8 * before
        ch = ops["c"][:, j0:j0 + CHUNK].astype(np.float64)
        xh += ch @ wt
        xh_abs += np.abs(ch) @ np.abs(wt)
    L_r = (ops["c"] != 0).sum(1).astype(np.float64)[:, None]
    tol_xh = R8 * np.abs(xh) + (1 + R8) * (L_r + 2) * U * xh_abs
    keep = xT != -1.0
    g_ref = np.where(keep, 2.0 * (xh - xT), 0.0)
    g_tol = np.where(keep, (1 + R8) * (2 * tol_xh + 4 * U * (np.abs(xh) + np.abs(xT))) + R8 * np.abs(g_ref), 0.0)
    return {"c": (c_ref, c_tol), "g": (g_ref, g_tol)}


def backward_sums(ops):
    """The plan-independent float64 sums of the backward: {"dW", "dW_tau", "dW_abs" [d][n], "db", "db_acc", "db_abs", "L" [n]}, all
    in units of 1 / scale."""
    M, d, n, inv_m = ops["M"], ops["d"], ops["n"], ops["inv_m"]
    g, xb = ops["g"].astype(np.float64), ops["xb"].astype(np.float64)
    ag, axb = np.abs(g), np.abs(xb)
    out = {k: np.empty((d, n)) for k in ("dW", "dW_tau", "dW_abs")}
    out.update({k: np.empty(n) for k in ("db", "db_acc", "db_abs")})
    out["L"] = (ops["c"] > 0).sum(0).astype(np.int64)
    for j0 in range(0, n, CHUNK):
        sl = slice(j0, j0 + CHUNK)
        wt = ops["wt"][sl].astype(np.float64)
        ch = ops["c"][:, sl].astype(np.float64)
        gate = ch > 0
        s, S = g @ wt.T, ag @ np.abs(wt).T
        p = np.where(gate, s + inv_m, 0.0)
        acc = np.where(gate, (D_P + 4) * U * (S + inv_m), 0.0)
        tau = np.where(gate, R8 * np.abs(p), 0.0) + acc
        out["dW"][:, sl] = g.T @ ch + xb.T @ p
        out["dW_tau"][:, sl] = axb.T @ tau
        out["dW_abs"][:, sl] = ag.T @ np.abs(ch) + axb.T @ (np.abs(p) + tau)
        out["db"][sl], out["db_acc"][sl], out["db_abs"][sl] = p.sum(0), acc.sum(0), np.abs(p).sum(0)
    return out


def backward_reference(ops, plan, sums=None):
    """-> {"dW": (ref, tol) [d][n], "db": (ref, tol) [n], "L": [n]} in float64, for the piece counts of `plan`."""
    sums = backward_sums(ops) if sums is None else sums
    scale, n = ops["scale"], ops["n"]
    P = np.repeat(pieces_per_tile(plan), BN)[:n].astype(np.float64)
    L = sums["L"].astype(np.float64)
    live = L > 0
    tol_dW = scale * (sums["dW_tau"] + ((2 * L + P + 3) * U)[None, :] * sums["dW_abs"])
    tol_db = scale * (sums["db_acc"] + (L + P + 3) * U * sums["db_abs"])
    return {"dW": (scale * sums["dW"], np.where(live[None, :], tol_dW, 0.0)), "db": (scale * sums["db"], np.where(live, tol_db, 0.0)),
            "L": sums["L"]}


def violations(out, ref, tol):
    """Boolean, shaped like out: not finite, or further than tol from ref."""
    o = np.asarray(as_f32(out), np.float64)
    return ~np.isfinite(o) | ~(np.abs(o - ref) <= tol)


def worst_ratio(out, ref, tol):
    """|difference| / tol per element (0 where the difference is 0, inf for a difference where tol is 0 or a non-finite element)."""
    o = np.asarray(as_f32(out), np.float64)
    diff = np.abs(o - ref)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(o), np.where(diff == 0, 0.0, diff / np.maximum(tol, 1e-300)), np.inf)


def report(name, out, ref, tol, L=None, plan=None):
    """The violating share and the worst element with its place (row / latent, tile, wave, list length, pieces), for an assertion
    message.  name: "c", "g" ([M][.]), "dW" ([d][n]) or "db" ([n])."""
    bad = violations(out, ref, tol)
    o = np.asarray(as_f32(out), np.float64)
    ratio = worst_ratio(out, ref, tol)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    if name in ("dW", "db", "c"):
        j = int(at[-1])
        where = f"latent {j} (tile {j // BN}, wave {j % BN // 32}"
        where += f", L = {int(L[j])}" if L is not None else ""
        where += f", {int(pieces_per_tile(plan)[j // BN])} pieces" if plan is not None else ""
        where += ")" + (f", input column {at[0]}" if name == "dW" else f", row {at[0]} (step {at[0] // BM})" if name == "c" else "")
    else:
        where = f"row {at[0]} (step {at[0] // BM}), column {at[1]}"
    cols = ""
    if name in ("dW", "db") and bad.any():
        lat = np.flatnonzero(bad.reshape(-1, bad.shape[-1]).any(0))
        cols = f"; latents hit: {lat[:12].tolist()}{'...' if len(lat) > 12 else ''} ({len(lat)})"
    return (f"{name}: {int(bad.sum())} of {bad.size} elements ({bad.mean():.2%}) violate; worst at {where}: got {o[at]!r}, "
            f"reference {ref[at]!r}, |difference| / tol = {ratio[at]:.3g}{cols}")


def bad_latents(ref, dW, db):
    """Sorted latents with a violating element of dW or db."""
    return np.flatnonzero(violations(dW, *ref["dW"]).any(0) | violations(db, *ref["db"]))


# ---- float32 emulation of the backward (and of its failure modes) --------------------------------------------------------------------
MUTATIONS = ("drop_step", "drop_last_quantum", "piece_twice", "piece_missing", "wrong_piece_count", "stale_pad_rows", "no_gate",
             "no_inv_m", "dc_rounded_first", "neighbour_tile")


def emulate(ops, plan, mutation=None, tile=None):
    """bwd_fused_d384_kernel + reduce_grads_kernel in float32 numpy -> (dW [d][n], db [n]): p^ = bf16(fp32 dot + inv_m), gated; every
    segment's slab piece accumulated step by step in fp32 (32 rows per step, the rows of a step in one float32 product) and multiplied
    by the float scale; the pieces of a tile added in piece order; db from the unrounded p.
    mutation: one failure mode, on column tile `tile` where it is local (default: the middle tile) --
      drop_step          the last step with real rows of one segment of the tile is not walked
      drop_last_quantum  every tile loses the rows of its last non-empty quantum (1/32 of the rows, or the last uniform row range)
      piece_twice        the tile's last piece that holds real rows is added twice
      piece_missing      ... is not added
      wrong_piece_count  the reduction adds the NEXT tile's number of pieces everywhere (uniform: splits - 1); a piece that was
                         not written holds the slab of the tile's piece 0 (a stale slab of an earlier step)
      stale_pad_rows     the rows M .. M_p of c^, g^ and xb hold the first rows of the batch (what a larger batch left) instead of zeros
      no_gate            p^ is not gated by c^ > 0
      no_inv_m           the accumulator starts at 0
      dc_rounded_first   dc is rounded to bf16 before 1 / M is added in fp32 (CPU autocast's order): db sums that, dW its bf16
      neighbour_tile     one segment of the tile reads the latent of the tile before it"""
    assert mutation is None or mutation in MUTATIONS
    M, d, n = ops["M"], ops["d"], ops["n"]
    steps, ntiles = plan["steps"], plan["ntiles"]
    Mp, n_p = steps * BM, ntiles * BN
    tile = ntiles // 2 if tile is None else tile
    f32 = np.float32
    scale = f32(f32(ops["alpha"]) / f32(ops["count"]))
    inv_m = f32(0) if mutation == "no_inv_m" else f32(f32(f32(1.0) / f32(M)) / scale)

    def padded(a, cols):
        out = np.zeros((Mp, cols), f32)
        out[:a.shape[0], :a.shape[1]] = a
        if mutation == "stale_pad_rows":
            out[M:Mp, :a.shape[1]] = a[:Mp - M]
        return out
    g, xb, c = padded(ops["g"], d), padded(ops["xb"], d), padded(ops["c"], n_p)
    wt = np.zeros((n_p, d), f32)
    wt[:n] = ops["wt"]
    dc = g @ wt.T
    p = bf16(dc) + inv_m if mutation == "dc_rounded_first" else dc + inv_m
    if mutation != "no_gate":
        p = np.where(c > 0, p, f32(0))
    ph = bf16(p)
    wgs = partition(plan)
    tsegs = tile_segments(wgs, ntiles)
    P = pieces_per_tile(plan)
    dW, db = np.zeros((d, n_p), f32), np.zeros(n_p, f32)
    for j in range(ntiles):
        cs = slice(BN * j, BN * (j + 1))
        live = [i for i, (s0, s1, _, _) in enumerate(tsegs[j]) if len(_real_rows(s0, s1, M))]
        last_q = None
        if mutation == "drop_last_quantum":
            q = plan["bal_q"] if plan["balanced"] else tsegs[j][live[-1]][1] - tsegs[j][live[-1]][0]
            last_q = ((min(steps, (M + BM - 1) // BM) - 1) // q * q) if plan["balanced"] else tsegs[j][live[-1]][0]
        slabs, dbs = [], []
        for i, (s0, s1, piece, _) in enumerate(tsegs[j]):
            acc, dacc = np.zeros((d, BN), f32), np.zeros(BN, f32)
            csrc = slice(BN * (j - 1), BN * j) if mutation == "neighbour_tile" and j == tile and i == live[len(live) // 2] else cs
            for st in range(s0, s1):
                if mutation == "drop_step" and j == tile and i == live[len(live) // 2] and st == (min(s1 * BM, M) - 1) // BM:
                    continue
                if last_q is not None and st >= last_q:
                    continue
                rs = slice(BM * st, BM * (st + 1))
                acc = acc + (g[rs].T @ c[rs, csrc] + xb[rs].T @ ph[rs, cs])
                dacc = dacc + p[rs, cs].sum(0, dtype=f32)
            slabs.append(acc * scale)
            dbs.append(dacc * scale)
        cnt = int(P[j])
        order = list(range(cnt))
        if j == tile and mutation == "piece_twice":
            order.append(live[-1])
        if j == tile and mutation == "piece_missing":
            order.remove(live[-1])
        if mutation == "wrong_piece_count":
            want = int(P[(j + 1) % ntiles]) if plan["balanced"] else cnt - 1
            order = [i if i < cnt else 0 for i in range(want)]
        a, bsum = np.zeros((d, BN), f32), np.zeros(BN, f32)
        for i in order:
            a, bsum = a + slabs[i], bsum + dbs[i]
        dW[:, cs], db[cs] = a, bsum
    return dW[:, :n], db[:n]


def oracle_operands(case):
    """Operands of the step from the CPU oracle's forward (fp32-defined bf16 matmuls) on a case of make_case."""
    from oracle import sae_oracle as O
    mode, O.MATMUL_MODE = O.MATMUL_MODE, "fp32"
    try:
        Wn = O.normalize_columns(case["W"].clone())
        f = O.l1_forward(case["x"].float(), Wn, case["b"], case["alpha"])
    finally:
        O.MATMUL_MODE = mode
    return operands(case["x"], bf16(Wn.numpy().T), case["b"].numpy(), bf16(f["c"].numpy()), bf16(2.0 * f["diff"].numpy()), case["alpha"])
