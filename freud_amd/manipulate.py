"""Feature manipulation: edit latents of an SAE and decode both ways -- the reference's manipulate_latent (utils/activations.py:
212-296, served as /manipulate_feature) between the cached Whisper activations and the tensors handed to whisper_subbed.forward,
for a batch of files, several edited latents and a sweep of values in ONE engine call (without it: forward + decode(edited) +
decode(standard) per factor, three dense decoder GEMMs of which two differ in one column of the latent).

Semantics (include/freud_sae.h, sae_manipulate_files; freud_amd/csrc/manip.h).  Per frame and edited latent, a is the value
freud_amd.models encode() returns (L1: the bf16 latent; TopK: the selected activation, 0 where the latent is not among the frame's
k).  An edit is (latent, op): "scale" -> new = a * value (the reference's manipulation_factor), "set" -> new = value on every
frame.  A variant is one row of `values` [V, E].  standard_decoded is the decode of the unedited latent; manipulated_decoded[v] is
standard + sum_e (new - a) * w_e in fp32, w_e the bf16 decoder row of the latent: the decode of the edited latent without rounding
the edited value back to bf16.  ALL T frames are edited and decoded, as the reference does; only the returned series are trimmed
to `lengths`.  Two runs give bitwise identical results.

    python -m freud_amd.manipulate --sae CKPT --shards DIR --layer NAME --file I --feat J --factor F [--factor ...] --out FILE.npz
"""
from __future__ import annotations

import argparse
import json
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .engine import MANIP_MAX_EDITS, MANIP_MAX_VARIANTS, MANIP_OPS
from .file_pass import check_lengths, keep_rng, resolve_sae

_OP_NAMES = {v: k for k, v in MANIP_OPS.items()}


class Manipulation(NamedTuple):
    """What manipulate_features returns (see the module docstring)."""
    standard_decoded: torch.Tensor            # fp32 [B, T, d], on the device
    manipulated_decoded: torch.Tensor         # fp32 [V, B, T, d], on the device
    standard_activations: list                # [E][B] fp32 CPU series, trimmed to the file's length
    manipulated_activations: list             # [V][E][B] the same after the edit
    latents: list                             # [E] int
    ops: list                                 # [E] "scale" | "set"
    values: np.ndarray                        # float32 [V, E]

    def save(self, path: str) -> None:
        B, T = int(self.standard_decoded.shape[0]), int(self.standard_decoded.shape[1])
        lens = np.array([len(s) for s in self.standard_activations[0]], np.int64)
        std = np.zeros((len(self.latents), B, T), np.float32)
        man = np.zeros((self.values.shape[0], len(self.latents), B, T), np.float32)
        for e, per_file in enumerate(self.standard_activations):
            for f, s in enumerate(per_file):
                std[e, f, :len(s)] = s.numpy()
        for v, per_edit in enumerate(self.manipulated_activations):
            for e, per_file in enumerate(per_edit):
                for f, s in enumerate(per_file):
                    man[v, e, f, :len(s)] = s.numpy()
        np.savez(path, standard_decoded=self.standard_decoded.cpu().numpy(), manipulated_decoded=self.manipulated_decoded.cpu().numpy(),
                 standard_activations=std, manipulated_activations=man, lengths=lens, latents=np.array(self.latents, np.int64),
                 ops=np.array(self.ops), values=self.values)

    @classmethod
    def load(cls, path: str) -> "Manipulation":
        """The saved result with CPU tensors."""
        with np.load(path) as z:
            lens = z["lengths"]
            std = [[torch.from_numpy(z["standard_activations"][e, f, :L].copy()) for f, L in enumerate(lens)]
                   for e in range(len(z["latents"]))]
            man = [[[torch.from_numpy(z["manipulated_activations"][v, e, f, :L].copy()) for f, L in enumerate(lens)]
                    for e in range(len(z["latents"]))] for v in range(z["values"].shape[0])]
            return cls(torch.from_numpy(z["standard_decoded"]), torch.from_numpy(z["manipulated_decoded"]), std, man,
                       [int(j) for j in z["latents"]], [str(o) for o in z["ops"]], z["values"].astype(np.float32))


def check_edits(n: int, edits, values=None):
    """edits: [(latent, op)] or, without `values`, [(latent, op, value)] (one variant); op: "scale" | "set" or its code.
    -> (latents [E] int32, ops [E] int32, values [V, E] float32), or ValueError: no edit or more than 16, more than 16 variants, a
    latent outside [0, n) or named twice, an unknown op, a value that is not finite, a `values` that is not [V, E]."""
    edits = list(edits)
    E = len(edits)
    if E < 1 or E > MANIP_MAX_EDITS:
        raise ValueError(f"{E} edits: one call takes 1 to {MANIP_MAX_EDITS}")
    latents, ops, own = [], [], []
    for i, ed in enumerate(edits):
        ed = tuple(ed)
        if len(ed) != (2 if values is not None else 3):
            raise ValueError(f"edit {i} must be (latent, op{'' if values is not None else ', value'}), got {ed!r}")
        j, op = int(ed[0]), ed[1]
        if not 0 <= j < n:
            raise ValueError(f"edit {i}: latent {j} outside [0, {n})")
        if j in latents:
            raise ValueError(f"edit {i}: latent {j} is named twice")
        code = MANIP_OPS.get(op) if isinstance(op, str) else (int(op) if int(op) in _OP_NAMES else None)
        if code is None:
            raise ValueError(f"edit {i}: op={op!r} is not one of {sorted(MANIP_OPS)}")
        latents.append(j)
        ops.append(code)
        if values is None:
            own.append(float(ed[2]))
    val = np.asarray([own] if values is None else values, dtype=np.float64)
    if val.ndim != 2 or val.shape[1] != E:
        raise ValueError(f"values must be [V, {E}] (one row per variant, one column per edit), got shape {val.shape}")
    V = int(val.shape[0])
    if V < 1 or V > MANIP_MAX_VARIANTS:
        raise ValueError(f"{V} variants: one call takes 1 to {MANIP_MAX_VARIANTS}")
    with np.errstate(over="ignore"):
        val32 = val.astype(np.float32)                 # (a double beyond fp32 becomes inf and is refused below)
    if not np.isfinite(val32).all():
        v, e = np.argwhere(~np.isfinite(val32))[0]
        raise ValueError(f"values[{v}][{e}]={val[v, e]} is not a finite float32")
    return np.array(latents, np.int32), np.array(ops, np.int32), val32


def edited_series(series: torch.Tensor, op: int, value: float) -> torch.Tensor:
    """manip.h's sm_new on a CPU fp32 series: one fp32 multiplication, or the value itself."""
    v = torch.tensor(value, dtype=torch.float32)
    return torch.full_like(series, float(v)) if op == MANIP_OPS["set"] else series * v


def _as_batch(x):
    x = torch.as_tensor(x)
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        x = x.float()
    if x.dim() == 2:
        x = x[None]
    if x.dim() != 3:
        raise ValueError(f"x must be [B, T, d] or [T, d], got {tuple(x.shape)}")
    return x


@keep_rng
def manipulate_features(sae, x, edits, values=None, lengths=None) -> Manipulation:
    """Edit latents of `sae` (a checkpoint path, a freud_amd.models SAE or a SaeEngine; bf16 contexts) on the activations x
    [B, T, d] or [T, d] and decode both ways, all variants in one engine call.  lengths: frames per file, file_pass.check_lengths
    rules (the series are trimmed to them; the decoded tensors keep all T frames)."""
    model, eng = resolve_sae(sae)
    if model is None and eng is None:
        raise ValueError("manipulate_features needs an SAE (manipulate_latent(None, ...) is the raw-activation branch)")
    x = _as_batch(x)
    B, T, d = (int(v) for v in x.shape)
    sae_d, n = (eng.d, eng.n) if eng is not None else (model.activation_size, model.n_dict_components)
    if sae_d != d:
        raise ValueError(f"the SAE expects d_model={sae_d}, x holds d={d}")
    latents, ops, val = check_edits(n, edits, values)
    lens = check_lengths(lengths, B, T)
    if not torch.cuda.is_available():
        raise RuntimeError("the feature manipulation runs on the GPU (HIP engine); there is no CPU path")
    if model is not None:
        eng, dev = model._ensure(B * T), model.device
    else:
        dev = torch.device("cuda", eng.device_id)
        if B * T > eng.max_rows:
            raise ValueError(f"{B} files x {T} frames exceed the engine's max_rows={eng.max_rows}")
    if eng.precision != "bf16":
        raise ValueError("the feature manipulation runs in bf16 contexts only")
    E, V = len(latents), int(val.shape[0])
    with torch.cuda.device(dev):
        x = x.to(dev).contiguous()
        standard = torch.empty(B, T, d, dtype=torch.float32, device=dev)
        manipulated = torch.empty(V, B, T, d, dtype=torch.float32, device=dev)
        series = torch.empty(E, B, T, dtype=torch.float32, device=dev)
        eng.manipulate_files(x, latents, ops, val, standard, manipulated, series)
        host = series.cpu()                                        # the one read-back (it synchronises)
    L = [T] * B if lens is None else [int(v) for v in lens]
    std = [[host[e, f, :L[f]].clone() for f in range(B)] for e in range(E)]
    man = [[[edited_series(std[e][f], int(ops[e]), float(val[v, e])) for f in range(B)] for e in range(E)] for v in range(V)]
    return Manipulation(standard, manipulated, std, man, [int(j) for j in latents], [_OP_NAMES[int(o)] for o in ops], val)


def manipulate_latent(sae, activations, feat_idx: int, manipulation_factor: float, length: Optional[int] = None):
    """activations.py:243-289 for one file's Whisper activations [1, T, d] or [T, d] (this project does not run Whisper):
    (standard_decoded, manipulated_decoded, standard_activations, manipulated_activations) -- the two tensors the reference hands to
    whisper_subbed.forward, shaped like `activations`, and its two series trimmed to `length` frames (1-D fp32 CPU).  sae=None is
    the reference's raw branch: the feature is a column of the activations, "decoded" is the activations with that column scaled."""
    a = torch.as_tensor(activations)
    if a.dim() == 3 and a.shape[0] != 1:
        raise ValueError(f"manipulate_latent takes one file, got {tuple(a.shape)}")
    if a.dim() not in (2, 3):
        raise ValueError(f"activations must be [1, T, d] or [T, d], got {tuple(a.shape)}")
    T = int(a.shape[-2])
    L = T if length is None else min(int(length), T)
    if L < 0:
        raise ValueError(f"length={length} must be >= 0")
    if not math.isfinite(float(manipulation_factor)):
        raise ValueError(f"manipulation_factor={manipulation_factor} is not finite")
    model, eng = resolve_sae(sae)
    if model is None and eng is None:
        j = int(feat_idx)
        if not 0 <= j < int(a.shape[-1]):
            raise ValueError(f"feat_idx={j} outside [0, {int(a.shape[-1])})")
        pre = a[..., j]
        new = pre * manipulation_factor
        manipulated = a.clone()
        manipulated[..., j] = new
        return a, manipulated, pre.reshape(-1)[:L].cpu(), new.reshape(-1)[:L].cpu()
    m = manipulate_features(sae, a, [(int(feat_idx), "scale")], [[float(manipulation_factor)]])
    shape = tuple(a.shape)
    return (m.standard_decoded.reshape(shape), m.manipulated_decoded[0].reshape(shape), m.standard_activations[0][0][:L],
            m.manipulated_activations[0][0][0][:L])


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="Scale one latent of an SAE on one file and decode both ways (the reference's manipulate_latent).")
    ap.add_argument("--sae", required=True, help="checkpoint path")
    ap.add_argument("--shards", required=True, help="shard directory")
    ap.add_argument("--layer", required=True, help="layer name")
    ap.add_argument("--file", type=int, required=True, help="index of the file in the shard directory")
    ap.add_argument("--feat", type=int, required=True, help="the latent to edit")
    ap.add_argument("--factor", type=float, action="append", required=True, help="manipulation factor (repeat for a sweep)")
    ap.add_argument("--length", type=int, default=None, help="frames of the file; default: the full T")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    from .loader import MemoryMappedActivationsDataset

    ds = MemoryMappedActivationsDataset(a.shards, a.layer, None)
    if not 0 <= a.file < len(ds):
        raise SystemExit(f"--file {a.file} outside [0, {len(ds)})")
    x = torch.as_tensor(ds[a.file][0])
    m = manipulate_features(a.sae, x, [(a.feat, "scale")], [[f] for f in a.factor], None if a.length is None else [a.length])
    m.save(a.out)
    diff = (m.manipulated_decoded - m.standard_decoded[None]).flatten(1).norm(dim=1)
    print(json.dumps({"out": a.out, "latent": a.feat, "factors": a.factor, "frames": int(x.shape[-2]),
                      "max_activation": float(m.standard_activations[0][0].max()), "moved_l2": [float(v) for v in diff.cpu()]}))


if __name__ == "__main__":
    main()
