"""Dead-latent resampling for L1 training: revive latents that never fire from the frames the dictionary reconstructs worst
(Bricken et al. 2023, "Towards Monosemanticity", neuron resampling) -- one pass over a prefix of the training shards, a selection on
the device, and a rewrite of the chosen columns inside the engine.

The rule (include/freud_sae.h, sae_resample_*; the arithmetic: freud_amd/csrc/resample_draw.h).  Over the first `files` files of a
shard directory, in file order (rows i = file * T + frame; with `lengths` only the first min(L[f], T) frames of file f count): a latent
is dead iff it fires on no counted frame; every dead latent, in ascending order, draws a row with probability proportional to the
squared reconstruction loss of the row (integer weights, a counter-based hash of (seed, round, rank): no dependence on the batching
or on a rank); a row drawn more than once goes to the lowest latent and the others stay dead this round.  The drawn frame x becomes
the latent's unit column W[:, j] = x / |x|, its bias b_j = -(1 - activation_scale) |x| -- so that the frame activates it at
activation_scale * |x| -- and both Adam moments of the column and of the bias are zeroed.  L1 dictionaries in bf16 contexts only: a
TopK dictionary has AuxK (auxk_alpha).

    python -m freud_amd.resample --sae CKPT --data_path DIR --layer_name L [--files 512] [--seed 0] [--round 0]
        [--activation_scale 0.2] [--lengths f.npy] [--batch_files B] --out CKPT_OUT [--report report.npz]
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional

import numpy as np

from .file_pass import FilePass, add_pass_arguments, is_raw, keep_rng, run_pass_cli

_ARRAYS = ("latents", "files", "frames")


@dataclasses.dataclass
class ResampleReport:
    """What one round did.  latents / files / frames: the revived latents (ascending) and the (file, frame) each was seeded from."""
    dead: int
    revived: int
    skipped_duplicate: int
    skipped_degenerate: int
    l_max: float
    mean_row_loss: float
    n_frames: int
    latents: np.ndarray         # int32 [revived]
    files: np.ndarray           # int64 [revived]
    frames: np.ndarray          # int64 [revived]

    def summary(self) -> dict:
        return {"dead": int(self.dead), "revived": int(self.revived), "skipped_duplicate": int(self.skipped_duplicate),
                "skipped_degenerate": int(self.skipped_degenerate), "l_max": float(self.l_max),
                "mean_row_loss": float(self.mean_row_loss), "n_frames": int(self.n_frames)}

    def to_npz(self, path: str) -> None:
        s = self.summary()
        np.savez(path, **{k: np.asarray(v) for k, v in s.items()}, **{k: getattr(self, k) for k in _ARRAYS})

    @classmethod
    def from_npz(cls, path: str) -> "ResampleReport":
        z = np.load(path)
        return cls(int(z["dead"]), int(z["revived"]), int(z["skipped_duplicate"]), int(z["skipped_degenerate"]), float(z["l_max"]),
                   float(z["mean_row_loss"]), int(z["n_frames"]), *(z[k] for k in _ARRAYS))


def check_resample_args(files, activation_scale) -> None:
    """The argument rules that need no device."""
    if int(files) < 1:
        raise ValueError(f"files={files} must be >= 1")
    if not 0.0 <= float(activation_scale) <= 1.0:
        raise ValueError(f"activation_scale={activation_scale} outside [0, 1]")


@keep_rng
def resample_dead_latents(sae, data_path: str, layer_name: str, *, files: int = 512, seed: int, round: int = 0,
                          activation_scale: float = 0.2, lengths=None, batch_files: Optional[int] = None) -> ResampleReport:
    """One resampling round of `sae` (a freud_amd.models L1 SAE or an L1 SaeEngine in bf16 precision -- its parameters and Adam
    moments are rewritten in place) over the first `files` files of a shard directory (512 files of 1500 frames: the paper's order of
    8e5 inputs).  seed / round: the counters of the draw (train() passes the run's seed and step // every).  lengths: frames per
    file for those files.  batch_files: files per engine call (default: file_pass.default_batch_files).  The caller's global torch
    RNG is left as it was."""
    import torch
    from . import engine as E
    from .loader import MemoryMappedActivationsDataset, require_directory

    require_directory(data_path)                # (the chosen frames are read from the files below)
    if is_raw(sae) or isinstance(sae, str):
        raise ValueError("resampling rewrites a live SAE: pass a freud_amd.models L1 SAE or an L1 SaeEngine (for a checkpoint, the "
                         "command line reads one and writes one)")
    check_resample_args(files, activation_scale)
    topk_advice = "resampling serves L1 dictionaries; a TopK dictionary revives its dead latents with AuxK (auxk_alpha)"
    if getattr(sae, "variant", None) == "topk" or getattr(sae, "_variant", None) == "topk":
        raise ValueError(topk_advice)
    fp = FilePass(sae, data_path, layer_name, what="resampling pass", lengths=lengths, subset_size=int(files), batch_files=batch_files,
                  max_frames=2 ** 31 - 1)
    eng = fp.eng
    if eng.variant != "l1":
        raise ValueError(topk_advice)
    n, T, d, rows = eng.n, fp.T, fp.d, fp.n_total * fp.T
    with torch.cuda.device(fp.device):
        row_loss = torch.zeros(rows, dtype=torch.float32, device=fp.device)
        fire = torch.zeros(n, dtype=torch.int64, device=fp.device)
        for x, file0, _nb, lb in fp:
            eng.resample_files(x, row_loss, file0 * T, fire, lb)
        lat_out = torch.zeros(n, dtype=torch.int32, device=fp.device)
        rows_out = torch.zeros(n, dtype=torch.int64, device=fp.device)
        counts = torch.zeros(E.RESAMPLE_NCOUNTS, dtype=torch.int64, device=fp.device)
        ws = torch.empty(E.resample_workspace_bytes(rows, n), dtype=torch.uint8, device=fp.device)
        E.resample_select(row_loss, rows, fire, n, seed, round, lat_out, rows_out, counts, ws)
        cnt = counts.cpu().numpy()                                  # the read-back of the selection
        pairs = int(cnt[E.RESAMPLE_PAIRS])
        lat = lat_out[:pairs].cpu().numpy()
        chosen = rows_out[:pairs].cpu().numpy()
        mean_loss = float(row_loss.double().sum().item() / max(fp.n_frames, 1))
        l_max = float(np.array([int(cnt[E.RESAMPLE_LMAX_BITS])], dtype=np.uint32).view(np.float32)[0])
        applied = np.zeros(pairs, dtype=bool)
        degenerate = 0
        if pairs:
            # the chosen frames from the shard memory map, widened exactly to fp32
            ds = MemoryMappedActivationsDataset(data_path, layer_name, int(files))
            x_rows = np.empty((pairs, d), dtype=np.float32)
            for i, r in enumerate(chosen):
                t = int(r) % T          # (a view of the file's row of the map: only the frame's d elements are read)
                x_rows[i] = ds.mmap[int(r) // T].reshape(-1)[t * d:(t + 1) * d]
            out_stats = torch.zeros(2 + pairs, dtype=torch.int64, device=fp.device)
            x_dev = torch.from_numpy(x_rows).to(fp.device)
            eng.resample_apply(lat_out[:pairs].contiguous(), x_dev, float(activation_scale), out_stats)
            st = out_stats.cpu().numpy()
            degenerate = int(st[1])
            applied = st[2:] != 0
            if int(st[0]) != int(applied.sum()) or int(st[0]) + degenerate != pairs:
                raise RuntimeError(f"the engine applied {int(st[0])} and skipped {degenerate} of {pairs} pairs")
    return ResampleReport(dead=int(cnt[E.RESAMPLE_DEAD]), revived=int(applied.sum()),
                          skipped_duplicate=int(cnt[E.RESAMPLE_SKIPPED_DUPLICATE]), skipped_degenerate=degenerate, l_max=l_max,
                          mean_row_loss=mean_loss, n_frames=int(fp.n_frames), latents=lat[applied].astype(np.int32),
                          files=(chosen[applied] // T).astype(np.int64), frames=(chosen[applied] % T).astype(np.int64))


def resample_checkpoint(checkpoint: dict, report: ResampleReport, params: dict) -> dict:
    """A copy of a train_sae checkpoint dict with the model of `params` (the engine's parameters after the round) and the Adam
    moments of the revived columns reset; every other entry is the checkpoint's own."""
    import torch
    out = dict(checkpoint)
    out["model"] = {k: torch.from_numpy(np.ascontiguousarray(params[k]).copy()) for k in checkpoint["model"]}
    opt = dict(checkpoint["optimizer"])
    state = {}
    for pid, st in checkpoint["optimizer"].get("state", {}).items():
        st = dict(st)
        for mk in ("exp_avg", "exp_avg_sq"):
            if mk in st and report.revived:
                t = st[mk].clone()
                t[..., torch.from_numpy(report.latents.astype(np.int64))] = 0    # (bias [n] and decoder.weight [d, n]: the latent is the last axis)
                st[mk] = t
        state[pid] = st
    opt["state"] = state
    out["optimizer"] = opt
    return out


def main(argv=None) -> None:
    import torch
    from .models import init_sae_from_checkpoint

    ap = argparse.ArgumentParser(description="One dead-latent resampling round of an L1 checkpoint over a shard directory.")
    add_pass_arguments(ap, sae_help="checkpoint path (train_sae.py format); --out is the checkpoint written")
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--activation_scale", type=float, default=0.2)
    ap.add_argument("--report", default=None, help="optional .npz of the ResampleReport")
    a = ap.parse_args(argv)
    ck = torch.load(a.sae, map_location="cpu")
    if ck["hparams"]["autoencoder_variant"] != "l1":
        raise ValueError("resampling serves L1 dictionaries; a TopK dictionary revives its dead latents with AuxK (auxk_alpha)")
    model = init_sae_from_checkpoint(a.sae)

    class _Written:
        """What run_pass_cli stores as --out: the checkpoint with the revived model (and the report beside it, if asked for)."""

        def __init__(self, report):
            self.report = report

        def to_npz(self, path):
            torch.save(resample_checkpoint(ck, self.report, model._eng.get_params()), path)
            if a.report:
                self.report.to_npz(a.report)

        def summary(self):
            return self.report.summary()

    run_pass_cli(a, lambda lengths: _Written(resample_dead_latents(
        model, a.data_path, a.layer_name, files=a.files, seed=a.seed, round=a.round, activation_scale=a.activation_scale,
        lengths=lengths, batch_files=a.batch_files)))


if __name__ == "__main__":
    main()
