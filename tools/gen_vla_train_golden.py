"""Golden vector for the differentiable cross-modal layer: builds the reference's own `InterModuleAttnLayer`
(models/transformer/transformer.py:209-221) through the import shims of oracle/ref_shims.py, in eval mode and float64, and writes
tests/golden/vla_train_L5_Lk16.npz -- data only: its state dict (under "sd/<key>"), the two inputs, the output, and the autograd gradients of
the inputs ("grad/input_1", "grad/input_2") and of every parameter ("grad/<key>") for a fixed cotangent.  Needs the reference checkout; runs
on the build machine, never on the GPU box.

    python tools/gen_vla_train_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vla_train_L5_Lk16.npz")
B, L, LK = 2, 5, 16
D, H, DK, D_FF = 16, 4, 4, 32          # small widths keep the fixture at tens of kilobytes; the restatement is width-agnostic


def main():
    ref_shims.install()
    from robo_vln_baselines.models.transformer.transformer import InterModuleAttnLayer
    torch.manual_seed(20)
    layer = InterModuleAttnLayer(d_model=D, d_k=DK, d_v=DK, h=H, d_ff=D_FF, dropout=0.25).double().eval()
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        for n, p in layer.named_parameters():             # biases and LayerNorm parameters off their trivial initial values
            if n.endswith("bias") or "layer_norm" in n:
                p.add_((torch.rand(p.shape, generator=g, dtype=torch.float64) - 0.5) * 0.4)
    x1 = (torch.rand(B, L, D, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    x2 = (torch.rand(B, LK, D, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    cot = torch.rand(B, L, D, generator=g, dtype=torch.float64) * 2 - 1
    out = layer(x1, x2, None, None)
    params = dict(layer.named_parameters())
    grads = torch.autograd.grad(out, [x1, x2, *params.values()], cot)
    data = {"dims": np.array([D, DK, DK, H, D_FF]), "input_1": x1.detach().numpy(), "input_2": x2.detach().numpy(), "cotangent": cot.numpy(), "out": out.detach().numpy(),
            "grad/input_1": grads[0].numpy(), "grad/input_2": grads[1].numpy()}
    for k, v in layer.state_dict().items():
        data["sd/" + k] = v.numpy()
    for k, gr in zip(params, grads[2:]):
        data["grad/" + k] = gr.numpy()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(layer.state_dict())} state-dict keys")


if __name__ == "__main__":
    main()
