"""Golden vector for the differentiable Visual_Ling_Attn: builds the reference's own `Visual_Ling_Attn` (models/transformer/transformer.py:250-282)
through the import shims of oracle/ref_shims.py, in eval mode and float64, and writes tests/golden/vla_encoder_train_N2_L5_Lk6.npz -- data only:
its state dict (under "sd/<key>"), the two inputs, the output, and the autograd gradients of the inputs ("grad/input", "grad/input_2") and of
every parameter ("grad/<key>") for a fixed cotangent.  The reference moves its float32 sinusoid table with `.to(input.get_device())`, which is -1
for a CPU tensor; for the duration of the forward get_device answers with the tensor's device instead.  Needs the reference checkout; runs on
the build machine, never on the GPU box.

    python tools/gen_vla_encoder_train_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vla_encoder_train_N2_L5_Lk6.npz")
B, L, LK = 2, 5, 6
CFG = dict(d_model=16, h=4, d_ff=32, vis_in_features=8, ins_in_features=24, N=2, dropout=0.25)   # small widths: the restatement is width-agnostic


def main():
    ref_shims.install()
    from robo_vln_baselines.models.transformer.transformer import Visual_Ling_Attn
    torch.manual_seed(30)
    enc = Visual_Ling_Attn(types.SimpleNamespace(**CFG)).double().eval()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for n, p in enc.named_parameters():               # biases and LayerNorm parameters off their trivial initial values
            if n.endswith("bias") or "layer_norm" in n:
                p.add_((torch.rand(p.shape, generator=g, dtype=torch.float64) - 0.5) * 0.4)
    x = (torch.rand(B, L, CFG["ins_in_features"], generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    x2 = (torch.rand(B, LK, CFG["vis_in_features"], generator=g, dtype=torch.float64) * 2 - 1).requires_grad_()
    cot = torch.rand(B, L, CFG["d_model"], generator=g, dtype=torch.float64) * 2 - 1
    get_device = torch.Tensor.get_device
    torch.Tensor.get_device = lambda t: t.device
    try:
        out = enc(x, x2, None, None)
    finally:
        torch.Tensor.get_device = get_device
    params = dict(enc.named_parameters())
    grads = torch.autograd.grad(out, [x, x2, *params.values()], cot)
    data = {"dims": np.array([CFG[k] for k in ("N", "vis_in_features", "ins_in_features", "d_model", "h", "d_ff")]), "input": x.detach().numpy(),
            "input_2": x2.detach().numpy(), "cotangent": cot.numpy(), "out": out.detach().numpy(), "grad/input": grads[0].numpy(),
            "grad/input_2": grads[1].numpy()}
    for k, v in enc.state_dict().items():
        data["sd/" + k] = v.numpy()
    for k, gr in zip(params, grads[2:]):
        data["grad/" + k] = gr.numpy()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(enc.state_dict())} state-dict keys")


if __name__ == "__main__":
    main()
