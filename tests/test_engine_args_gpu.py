"""GPU: the host-side tensor checks of freud_amd/engine.py, one table.  Every output or auxiliary device tensor of every *_files method and
of every free function is handed over wrong in each way the binding checks -- on the CPU, of another dtype, one element short,
non-contiguous and, where the size rule is exact, one element long -- and the call must end in an EngineError raised in Python, before
the C call: a short buffer that passed would be a device over-write.  The rows are the record of which size rules are exact (EXACT)
and which are "at least" (AT_LEAST); SHAPE rows have a shape rule next to the call that refuses both a shorter and a longer tensor,
UNSIZED rows give their own size to the call.  Afterwards both contexts still evaluate: nothing was enqueued."""
import numpy as np
import pytest
import torch

from freud_amd import engine as E

pytestmark = pytest.mark.gpu

EXACT = ("cpu", "dtype", "short", "noncontig", "long")
SHAPE = EXACT
AT_LEAST = ("cpu", "dtype", "short", "noncontig")
UNSIZED = ("cpu", "dtype", "noncontig")
BYTES = ("cpu", "short", "noncontig")             # packed operands: any dtype, at least so many bytes
STRIDED = ("cpu", "dtype", "short")               # dict_pack's directions: strided on purpose, inside their storage
OTHER = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int64: torch.int32, torch.int32: torch.int16,
         torch.uint8: torch.int8}                 # (int16: collect_files and the feature index take int32 or int64 indices)


def wrong(t, case):
    if case == "cpu":
        return t.cpu()
    if case == "dtype":
        return t.to(OTHER[t.dtype])
    if case == "short":
        return t.flatten()[:-1].clone()
    if case == "long":
        return torch.cat([t.flatten(), t.flatten()[:1]])
    assert case == "noncontig"
    return torch.stack([t, t], -1)[..., 0]          # the shape of t over doubled strides


def dev(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def context_rows(eng, x):
    """(call, its good keyword arguments, {argument: cases}) for every *_files method: x is 2 files x 8 frames."""
    B, T, d = x.shape
    n, M, Cn, K, nsel = eng.n, B * T, 4, 4, 3
    i32, i64, f32, f64, u8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8
    lengths = torch.full((B,), T, dtype=i32, device="cuda")
    labels = dev(i32, B, T, 2)
    spec = (-4, 4, 1)
    hb, tb = E.hist_nbins(spec), E.timing_nbins(2, T)
    return [
        (eng.search_files, dict(x=x, file_keys=dev(i64, B, n), lengths=lengths), {"file_keys": AT_LEAST, "lengths": EXACT}),
        (eng.stats_files, dict(x=x, stats_block=dev(u8, E.stats_layout(n)["bytes"]), lengths=lengths),
         {"stats_block": AT_LEAST, "lengths": EXACT}),
        (eng.coact_files, dict(x=x, counts=dev(i32, n, n), lengths=lengths), {"counts": EXACT, "lengths": EXACT}),
        (eng.label_files, dict(x=x, labels=labels, n_classes=Cn, counts=dev(i32, Cn + 1, n), label_count=dev(i64, Cn + 1), lengths=lengths),
         {"labels": SHAPE, "counts": EXACT, "label_count": EXACT, "lengths": EXACT}),
        (eng.hist_files, dict(x=x, spec=spec, frame_hist=dev(i64, n, hb), file_max_hist=dev(i64, n, hb), n_frames=dev(i64, 1),
                              lengths=lengths, labels=labels, n_classes=Cn, sel_latents=dev(i32, nsel),
                              label_hist=dev(i64, nsel, Cn + 1, hb), label_count=dev(i64, Cn + 1)),
         {"frame_hist": EXACT, "file_max_hist": EXACT, "n_frames": EXACT, "lengths": EXACT, "labels": SHAPE, "sel_latents": UNSIZED,
          "label_hist": EXACT, "label_count": EXACT}),
        (eng.timing_files, dict(x=x, sub_bits=2, bridge=0, threshold_bits=0, run_hist=dev(i64, n, tb), gap_hist=dev(i64, n, tb),
                                totals=dev(i64, n, E.TIMING_NTOTALS), n_frames=dev(i64, 1), lengths=lengths),
         {"run_hist": EXACT, "gap_hist": EXACT, "totals": EXACT, "n_frames": EXACT, "lengths": EXACT}),
        (eng.manipulate_files, dict(x=x, latents=[3, 5], ops=[0, 1], values=[[2.0, 0.5]], standard=dev(f32, M, d),
                                    manipulated=dev(f32, 1, M, d), series=dev(f32, 2, M)),
         {"standard": EXACT, "manipulated": EXACT, "series": EXACT}),
        (eng.recon_files, dict(x=x, block=dev(u8, E.recon_layout(n, d)["bytes"]), file_out=dev(f64, B, 2), lengths=lengths,
                               resid=dev(f32, M, d)),
         {"block": AT_LEAST, "file_out": EXACT, "lengths": EXACT, "resid": EXACT}),
        (eng.collect_files, dict(x=x, K=K, values=dev(f32, M, K), indices=dev(i64, M, K), stats=dev(i64, 8)),
         {"values": EXACT, "stats": EXACT}),
        (eng.collect_files, dict(x=x, K=K, values=dev(f32, M, K), indices=dev(i32, M, K), stats=dev(i64, 8)), {"indices": EXACT}),
    ]


def free_rows(x):
    """The same for the free functions that take device tensors."""
    B, T, d = x.shape
    i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8
    F, ncols, n_top, n, Cn, rows = 2, 32, 4, 32, 4, 2
    lengths = torch.full((B,), T, dtype=i32, device="cuda")
    keys, aux = dev(i64, F, ncols), dev(i64, F, ncols)
    nd, dd = 8, 16
    packed = dev(u8, E.dict_pack_bytes(nd, dd))
    vals, idx, n_dict = dev(f32, 4, 3), dev(i32, 4, 3), 32
    return [
        (E.search_raw_files, dict(x=x, file_keys=dev(i64, B, d), aux=dev(i64, B, d), lengths=lengths, absolute=True),
         {"file_keys": AT_LEAST, "aux": AT_LEAST, "lengths": EXACT}),
        (E.search_merge, dict(file_keys=keys, aux=aux, n_files=F, ncols=ncols, file0=0, n_top=n_top, flags=0, min_val=0.0, max_val=1.0,
                              top_keys=dev(i64, n_top, ncols), top_frames=dev(i32, n_top, ncols)),
         {"file_keys": AT_LEAST, "aux": AT_LEAST, "top_keys": AT_LEAST, "top_frames": AT_LEAST}),
        (E.search_file_values, dict(file_keys=keys, aux=aux, n_files=F, ncols=ncols, flags=0, latents=dev(i32, 3), file0=0,
                                    out=dev(f32, 3, F)),
         {"file_keys": AT_LEAST, "aux": AT_LEAST, "latents": UNSIZED, "out": AT_LEAST}),
        (E.file_top_features, dict(file_keys=keys, n_files=F, ncols=ncols, n_top=n_top, flags=0, top_latents=dev(i32, F, n_top),
                                   top_keys=dev(i64, F, n_top)),
         {"file_keys": AT_LEAST, "top_latents": AT_LEAST, "top_keys": AT_LEAST}),
        (E.coact_neighbor_keys, dict(counts=dev(i32, n, n), n=n, row0=0, n_rows=rows, measure=0, keys=dev(i64, rows, n)),
         {"counts": EXACT, "keys": AT_LEAST}),
        (E.label_keys, dict(counts=dev(i32, Cn + 1, n), label_count=dev(i64, Cn + 1), n_classes=Cn, n=n, measure=0, by_latent=0, row0=0,
                            n_rows=rows, keys=dev(i64, rows, n)),
         {"counts": EXACT, "label_count": EXACT, "keys": AT_LEAST}),
        (E.label_keys, dict(counts=dev(i32, Cn + 1, n), label_count=dev(i64, Cn + 1), n_classes=Cn, n=n, measure=0, by_latent=1, row0=0,
                            n_rows=rows, keys=dev(i64, rows, Cn)),
         {"keys": AT_LEAST}),
        (E.dict_pack, dict(w=dev(f32, nd, dd), n=nd, d=dd, dir_stride=dd, elem_stride=1, side=E.DICT_LEFT, packed=packed,
                           norms=dev(f32, nd)),
         {"w": STRIDED, "packed": BYTES, "norms": AT_LEAST}),
        (E.dict_sim_keys, dict(packed_a=packed, n_a=nd, packed_b=packed.clone(), n_b=nd, d=dd, row0=0, n_rows=rows, self_mode=False,
                               keys=dev(i64, rows, nd)),
         {"packed_a": BYTES, "packed_b": BYTES, "keys": AT_LEAST}),
        (E.findex_count, dict(values=vals, indices=idx, n_dict=n_dict, totals=dev(i64, n_dict), stats=dev(i64, E.FINDEX_NSTATS)),
         {"values": SHAPE, "indices": SHAPE, "totals": EXACT, "stats": EXACT}),
        (E.findex_fill, dict(values=vals, indices=idx, n_dict=n_dict, j0=0, j1=n_dict, pos0=0, cursor=dev(i64, n_dict), out_base=0,
                             positions_out=dev(i32, 12), values_out=dev(f32, 12), workspace=dev(u8, E.findex_workspace_bytes(4, n_dict)),
                             err=dev(i64, 2)),
         {"values": SHAPE, "indices": SHAPE, "cursor": EXACT, "positions_out": UNSIZED, "values_out": EXACT, "workspace": AT_LEAST,
          "err": EXACT}),
        (E.findex_verify, dict(starts=dev(i64, 2), j0=0, j1=1, out_base=0, positions=dev(i32, 12), limit=12, err=dev(i64, 2)),
         {"starts": AT_LEAST, "positions": UNSIZED, "err": EXACT}),
    ]


def make_contexts(d, n):
    g = np.random.default_rng(1)
    W = np.zeros((d, n), np.float32)
    for j in range(n):
        W[g.permutation(d)[:256], j] = np.where(g.random(256) < 0.5, -1 / 16, 1 / 16)
    l1 = E.SaeEngine("l1", d, n, 512)
    l1.set_params({"decoder.weight": W, "encoder_bias": g.normal(-1.5, 0.3, n).astype(np.float32)})
    topk = E.SaeEngine("topk", d, n, 512, k=16, optimizer="adam")
    We = (g.normal(0, 1, (n, d)) / 16).astype(np.float32)
    topk.set_params({"encoder.weight": We, "encoder.bias": np.zeros(n, np.float32), "W_dec": We.copy(), "b_dec": np.zeros(d, np.float32)})
    return l1, topk


def test_every_wrong_device_tensor_is_refused_in_python():
    d, n = 256, 1024
    x = torch.randn(2, 8, d, generator=torch.Generator().manual_seed(0)).cuda()
    l1, topk = make_contexts(d, n)
    table = context_rows(l1, x) + context_rows(topk, x) + free_rows(x)
    tried, missed = 0, []
    for call, good, checks in table:
        assert set(checks) <= set(good)
        for arg, cases in checks.items():
            for case in cases:
                if case == "noncontig" and good[arg].numel() < 2:       # (a one-element tensor is contiguous whatever its strides)
                    continue
                bad = wrong(good[arg], case)
                assert case != "noncontig" or (not bad.is_contiguous() and bad.shape == good[arg].shape)
                tried += 1
                try:
                    call(**{**good, arg: bad})
                    missed.append((call.__name__, arg, case, "no error"))
                except E.EngineError as e:
                    if "libfreud_sae error" in str(e):                  # (the C side's refusal: the Python check let it through)
                        missed.append((call.__name__, arg, case, str(e)))
    assert not missed, missed
    assert tried > 400
    torch.cuda.synchronize()
    for eng in (l1, topk):
        eng.eval(x.reshape(-1, d))
        m = eng.metrics()
        assert np.isfinite(m).all(), (eng.variant, m)
        eng.close()
