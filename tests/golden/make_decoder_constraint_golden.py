"""Golden vectors of the decoder-norm constraint: the REAL reference model's remove_gradient_parallel_to_decoder_directions() and
set_decoder_norm_to_unit_norm() (src/models/topkautoencoder.py:153-175) inside three fp32 training steps in the order of the trainer
the model file was taken from:

    backward -> remove_gradient_parallel_to_decoder_directions -> clip_grad_norm_(1.0) -> Adam.step -> set_decoder_norm_to_unit_norm

Run where a checkout of the reference is present (its path as the first argument, default make_golden.REF); only the .npz it writes
is kept:

    python tests/golden/make_decoder_constraint_golden.py [path/to/reference]

It reuses make_golden.py's stubs of the absent third-party imports.  Written (decoder_constraint.npz) for a tiny TopKAutoEncoder
(d = 16, n = 64, k = 4; 40 rows of random input per step; no autocast, fp32 on CPU; Adam lr 1e-2, betas (0.9, 0.999), eps 1e-8), for
every step s = 0, 1, 2:

  s<s>_W_before                  W_dec at the start of the step (unit rows: the constructor / the previous step normalised them)
  s<s>_grad_<name>               the gradients the backward left, all four parameters (name: W_dec, b_dec, encoder.weight, encoder.bias)
  s<s>_grad_W_dec_projected      W_dec.grad after the projection
  s<s>_total_norm                what clip_grad_norm_ returned (torch's fp32 norm of the projected gradients)
  s<s>_m_<name> / s<s>_v_<name>  Adam's moments BEFORE the step (zeros at s = 0)
  s<s>_p_<name>                  the parameters before the step
  s<s>_W_updated                 W_dec after Adam.step, before the renorm
  s<s>_W_renormed                W_dec after set_decoder_norm_to_unit_norm

Data only."""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
D, N, K, ROWS, STEPS, LR = 16, 64, 4, 40, 3, 1e-2
NAMES = ("W_dec", "b_dec", "encoder.weight", "encoder.bias")


def main():
    sys.path.insert(0, OUT)
    import make_golden
    make_golden.install_stubs()
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else make_golden.REF)
    from src.models.config import TopKAutoEncoderConfig
    from src.models.topkautoencoder import TopKAutoEncoder
    torch.manual_seed(31)
    sae = TopKAutoEncoder(D, TopKAutoEncoderConfig(n_dict_components=N, k=K))
    params = dict(sae.named_parameters())
    assert tuple(params) == NAMES
    opt = torch.optim.Adam(sae.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    out = {}
    for s in range(STEPS):
        x = torch.randn(ROWS, D)
        out[f"s{s}_W_before"] = sae.W_dec.detach().numpy().copy()
        for k, p in params.items():
            out[f"s{s}_p_{k}"] = p.detach().numpy().copy()
            st = opt.state.get(p, {})
            out[f"s{s}_m_{k}"] = st["exp_avg"].numpy().copy() if st else np.zeros(p.shape, np.float32)
            out[f"s{s}_v_{k}"] = st["exp_avg_sq"].numpy().copy() if st else np.zeros(p.shape, np.float32)
        opt.zero_grad()
        fo = sae(x)
        (fo.fvu + fo.auxk_loss + fo.multi_topk_fvu / 8).backward()
        for k, p in params.items():
            out[f"s{s}_grad_{k}"] = p.grad.numpy().copy()
        sae.remove_gradient_parallel_to_decoder_directions()
        out[f"s{s}_grad_W_dec_projected"] = sae.W_dec.grad.numpy().copy()
        out[f"s{s}_total_norm"] = np.float64(torch.nn.utils.clip_grad_norm_(sae.parameters(), 1.0).item())
        opt.step()
        out[f"s{s}_W_updated"] = sae.W_dec.detach().numpy().copy()
        sae.set_decoder_norm_to_unit_norm()
        out[f"s{s}_W_renormed"] = sae.W_dec.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, "decoder_constraint.npz"), **out)
    print("decoder_constraint.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
