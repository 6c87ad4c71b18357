"""Dictionary comparison throughput (freud_amd/dictionary_match.py; include/freud_sae.h sae_dict_pack / sae_dict_sim_keys) -- one JSON
line, also written to profiles/dict_match_bench.json.

Per shape (d, n_a, n_b; K = 8 neighbours), device-resident Gaussian dictionaries:
  pack_ms      both operand packs (HIP events around the kernels);
  keys_ms      the similarity-key GEMMs of all row blocks, select_ms the radix selects of all row blocks, the same blocks as the
               whole call uses (coactivation.select_top_rows: at most 2^25 keys each, begun at multiples of 256);
  call_ms      the whole compare_dictionaries call: packs, keys, selects, and the read-back of the tables;
  torch_ms     the route a user has without it, on the same box: torch fp32 normalize(A) @ normalize(B).T and topk in row blocks of
               the same size (self mode: the diagonal filled with -inf), tables read back;
  pflops       effective bf16 PFLOP/s of the key GEMMs over 2 x 3 d x n_a x n_b;
  torch_over_pass   torch_ms / call_ms: >= 1 means the pass is at least as fast as the generic route.
Every time is the median of alternating rounds, with the smallest and the largest round beside it.

    python tools/bench_dict_match.py [--iters 3] [--rounds 5] [--out profiles/dict_match_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freud_amd import coactivation as CO                            # noqa: E402
from freud_amd import dictionary_match as DM                        # noqa: E402
from freud_amd import engine as E                                   # noqa: E402
from bench_pass_common import timed                                 # noqa: E402

K = 8


def blocks(n_a, n_b):
    rows = max(1, min(n_a, CO.KEY_BLOCK // n_b))
    if DM.ROW_ALIGN <= rows < n_a:
        rows -= rows % DM.ROW_ALIGN
    return rows, [(r0, min(rows, n_a - r0)) for r0 in range(0, n_a, rows)]


def torch_route(A, B, self_mode, rows):
    ua, ub = torch.nn.functional.normalize(A, dim=1), torch.nn.functional.normalize(B, dim=1)
    out = []
    for r0 in range(0, A.shape[0], rows):
        S = ua[r0:r0 + rows] @ ub.T
        if self_mode:
            S.diagonal(r0).fill_(float("-inf"))
        v, i = torch.topk(S, K, dim=1)
        out.append((v.cpu(), i.cpu()))
    return out


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def shape(d, n_a, n_b, self_mode, iters, rounds):
    g = torch.Generator().manual_seed(0)
    A = torch.randn(n_a, d, generator=g).cuda()
    B = A if self_mode else torch.randn(n_b, d, generator=g).cuda()
    rows, blks = blocks(n_a, n_b)
    da = DM.decoder_directions(A)
    db = da if self_mode else DM.decoder_directions(B)
    pa, _ = DM.pack_directions(da, E.DICT_LEFT)
    pb, _ = DM.pack_directions(db, E.DICT_RIGHT)
    keys = torch.empty(rows * n_b, dtype=torch.int64, device="cuda")
    lat = torch.empty(rows * K, dtype=torch.int32, device="cuda")
    out = torch.empty(rows * K, dtype=torch.int64, device="cuda")

    def f_pack():
        DM.pack_directions(da, E.DICT_LEFT)
        DM.pack_directions(db, E.DICT_RIGHT)

    def f_keys():
        for r0, nr in blks:
            E.dict_sim_keys(pa, n_a, pb, n_b, d, r0, nr, self_mode, keys)

    def f_select():
        for _r0, nr in blks:
            E.file_top_features(keys, nr, n_b, K, 0, lat, out)

    f_call = lambda: DM.compare_dictionaries(A, None if self_mode else B, n_neighbors=K)
    f_torch = lambda: torch_route(A, B, self_mode, rows)
    fns = {"pack_ms": f_pack, "keys_ms": f_keys, "select_ms": f_select, "call_ms": f_call, "torch_ms": f_torch}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    res = {"n_a": n_a, "n_b": n_b, "d": d, "self_mode": self_mode, "n_neighbors": K, "row_blocks": len(blks), "rows_per_block": rows}
    res.update({k: spread(v) for k, v in times.items()})
    res["pflops"] = 2.0 * 3 * d * n_a * n_b / res["keys_ms"]["median"] / 1e12
    res["torch_over_pass"] = res["torch_ms"]["median"] / res["call_ms"]["median"]
    name = f"d{d}_n{n_a}" + ("_self" if self_mode else f"_vs_n{n_b}")
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_match_bench.json"))
    a = ap.parse_args()
    res = {"tool": "bench_dict_match", "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}
    res.update(shape(384, 3072, 3072, True, a.iters, a.rounds))
    res.update(shape(384, 3072, 12288, False, a.iters, a.rounds))
    res.update(shape(1280, 40960, 40960, True, a.iters, a.rounds))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
