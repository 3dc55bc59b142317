"""Forward plus backward of the whole cross-modal encoder, robo_vln_amd.train.Visual_Ling_Attn (both prologue halves on hcm_op_embed_ln_train /
hcm_op_embed_ln_bwd, the layer on hcm_op_vla_layer_train / _bwd), against what a user had before it: the reference-shaped torch prologue
(transformer.py:262-274 -- Linear, ReLU, dropout, LayerNorm, the sinusoid table built on the CPU and copied to the device in every forward) in
front of the same device InterModuleAttnLayer.  Same GPU, same rows, same weights, same keep masks: (B, L, Lk) = (64, 80, 16), N = 1, ins_in 768,
vis_in 256, d_ff 1024, float32; p = 0.25 and p = 0, the vis input with and without requires_grad (without, the vis half's d_x product is skipped;
the instruction input never requires a gradient, as it comes out of torch.no_grad() BERT).  Also the two prologue halves alone, embed_ln against
embed_ln_ref in torch eager on the device (vis: 1024 rows of 256 with d_x; ins: 5120 rows of 768 with the table, no d_x), and the bytes each side
keeps for the backward pass (distinct storages autograd holds between forward and backward; inputs, parameters, keep masks and table excluded).

Each variant runs `iters` forward+backward passes in a group that ends in one device synchronise; the sides alternate inside a round, at least
five rounds after a warm-up; median and range per variant, one JSON line per configuration, host clock, profiler off.  Run it at least twice and
report ranges.

    python tools/bench_vla_encoder_train.py [--rounds 5] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from robo_vln_amd import train                              # noqa: E402

B, L, LK, D, D_FF, VIS_IN, INS_IN = 64, 80, 16, 256, 1024, 256, 768
CFG = dict(N=1, vis_in_features=VIS_IN, ins_in_features=INS_IN, d_model=D, h=4, d_ff=D_FF)


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def saved_bytes(fn, exclude):
    """bytes of the distinct storages autograd keeps between forward and backward of fn(), without those of `exclude`"""
    skip = {t.untyped_storage().data_ptr() for t in exclude if t is not None}
    seen = {}

    def pack(t):
        s = t.untyped_storage()
        if s.data_ptr() not in skip:
            seen[s.data_ptr()] = s.nbytes()
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    return sum(seen.values())


class ParentEncoder(train.Visual_Ling_Attn):
    """the same parameters with the prologue as the reference writes it, in torch ops on the device; the layers are the device InterModuleAttnLayer.
    Dropout takes the injected keep masks (train.mask_dropout: three element-wise kernels and a saved float copy of the mask, where nn.Dropout is
    one fused kernel that saves a byte mask), so that both sides run the same arithmetic."""

    def forward(self, input, input_2, self_att_mask, enc_att_mask, _keep=None):
        F = torch.nn.functional
        p = self.p if _keep[0] is not None else 0.0
        out = self.layer_norm(train.mask_dropout(F.relu(self.vis_fc(input_2)), _keep[0], p))
        inp = self.layer_norm(train.mask_dropout(F.relu(self.ins_fc(input)), _keep[1], p))
        pe = train.sinusoid_table(inp.shape[1], inp.shape[2])
        inp = inp + pe.expand(inp.shape[0], pe.shape[0], pe.shape[1]).to(inp.device)
        for layer, k in zip(self.layers, _keep[2:]):
            out = layer(inp, out, None, None, _keep=k)
        return out


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def interleave(variants, a):
    for fn in variants.values():                                   # warm-up: code objects, allocator, the BLAS library's choices
        for _ in range(3):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.iters))
    return {k: stats(v) for k, v in times.items()}


def rel_diff(x, y):
    return ((x - y).abs().max() / y.abs().max()).item()


def bench_encoder(p, vis_grad, a):
    torch.manual_seed(0)
    m = train.Visual_Ling_Attn(dropout=p, **CFG).cuda().train()
    ref = ParentEncoder(dropout=p, **CFG).cuda().train()
    ref.load_state_dict(m.state_dict())
    g = torch.Generator().manual_seed(1)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    ins, vis, cot = u(B, L, INS_IN), u(B, LK, VIS_IN).requires_grad_(vis_grad), u(B, L, D)
    keep = m.draw_keep(B, L, LK, "cuda") if p > 0 else (None, None, None)
    run = lambda mod: torch.autograd.backward(mod(ins, vis, None, None, _keep=keep), cot)

    def grads(mod):
        for t in [vis] + list(mod.parameters()):
            t.grad = None
        run(mod)
        return [q.grad.clone() for q in mod.parameters()] + ([vis.grad.clone()] if vis_grad else [])

    with torch.no_grad():
        out_diff = rel_diff(m(ins, vis, None, None, _keep=keep), ref(ins, vis, None, None, _keep=keep))
    names = [n for n, _ in m.named_parameters()] + ["d_input_2"]
    # fc_k.bias is left out of the ratio: its exact gradient is zero (a key bias shifts a row's scores alike), both sides return float32 noise
    per = {n: rel_diff(o, t) for n, o, t in zip(names, grads(m), grads(ref)) if not n.endswith("fc_k.bias")}
    worst = max(per, key=per.get)
    excl = [ins, vis, m.table(L, ins.device)] + [k for k in (keep[0], keep[1], *(keep[2] or ())) if k is not None]
    kept = {"hip": saved_bytes(lambda: m(ins, vis, None, None, _keep=keep), excl + list(m.parameters())),
            "parent": saved_bytes(lambda: ref(ins, vis, None, None, _keep=keep), excl + list(ref.parameters()))}
    res = {"what": "encoder", "p": p, "vis_requires_grad": vis_grad, "B": B, "L": L, "Lk": LK, "iters": a.iters, "rounds": a.rounds,
           "out_rel_difference": float(f"{out_diff:.3e}"), "max_rel_grad_difference": float(f"{per[worst]:.3e}"), "worst_tensor": worst, "saved_bytes": kept}
    res.update(interleave({"hip": lambda: run(m), "parent": lambda: run(ref)}, a))
    res["ratio_parent_over_hip"] = round(res["parent"]["median_ms"] / res["hip"]["median_ms"], 3)
    res["ranges_disjoint"] = res["hip"]["max_ms"] < res["parent"]["min_ms"] or res["parent"]["max_ms"] < res["hip"]["min_ms"]
    print(json.dumps(res), flush=True)
    return res


def bench_half(which, p, a):
    rows, K, want_dx = (B * LK, VIS_IN, True) if which == "vis" else (B * L, INS_IN, False)
    g = torch.Generator().manual_seed(2)
    u = lambda *s, scale=1.0: ((torch.rand(*s, generator=g) * 2 - 1) * scale).cuda()
    x = u(rows, K).requires_grad_(want_dx)
    w, b = u(D, K, scale=K ** -0.5).requires_grad_(), u(D, scale=K ** -0.5).requires_grad_()
    gamma, beta = (1 + u(D, scale=0.5)).requires_grad_(), u(D, scale=0.5).requires_grad_()
    keep = (torch.rand(rows, D, device="cuda") >= p).to(torch.uint8) if p > 0 else None
    post = train.sinusoid_table(L, D).cuda() if which == "ins" else None
    cot = u(rows, D)
    leaves = [x, w, b, gamma, beta]
    hip = lambda: train.embed_ln(*leaves, keep=keep, p=p, post=post)
    eager = lambda: train.embed_ln_ref(*leaves, keep=keep, p=p, post=post)

    def grads(fn):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(fn(), cot)
        return [t.grad.clone() for t in leaves if t.grad is not None]

    per = [rel_diff(o, t) for o, t in zip(grads(hip), grads(eager))]
    excl = leaves + [keep, post]
    res = {"what": which + "_half", "p": p, "rows": rows, "K": K, "d_x": want_dx, "iters": a.iters, "rounds": a.rounds,
           "max_rel_grad_difference": float(f"{max(per):.3e}"), "saved_bytes": {"hip": saved_bytes(hip, excl), "torch": saved_bytes(eager, excl)}}
    res.update(interleave({"hip": lambda: torch.autograd.backward(hip(), cot), "torch": lambda: torch.autograd.backward(eager(), cot)}, a))
    res["ratio_torch_over_hip"] = round(res["torch"]["median_ms"] / res["hip"]["median_ms"], 3)
    res["ranges_disjoint"] = res["hip"]["max_ms"] < res["torch"]["min_ms"] or res["torch"]["max_ms"] < res["hip"]["min_ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vla_encoder_train.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    for p in (0.25, 0.0):
        for vis_grad in (True, False):
            bench_encoder(p, vis_grad, a)
    for p in (0.25, 0.0):
        for which in ("vis", "ins"):
            bench_half(which, p, a)


if __name__ == "__main__":
    main()
