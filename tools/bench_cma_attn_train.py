"""Forward plus backward of CMANet's three attention stages (cma.py:271-311) at the trainer's shape -- 64 rows; text L = 80 with 512 channels; RGB
(2048 + 64, 16); depth (128 + 64, 16); hidden 512, float32 -- over three routes on the same GPU, inputs and cotangents:

    hip     qt = q W_k, robo_vln_amd.train.attn1q (hcm_op_attn1q_train / _bwd), and for RGB / depth xbar W_v^T + b_v
    ref     torch eager autograd of the reference's own formulation: cat([x, spatial]), conv1d, split, _attn
    folded  torch eager autograd of train.attn1q_ref with the same two projections: what the algebra buys without the kernel

and the whole train.CMANet step (forward, loss, backward) from cached features at (T, N) = (16, 4) and (8, 8) against the same module with its
attention stages forced onto attn1q_ref.  Also the attention op alone (no projections), forward and backward, with the bytes it streams (the
sample is read twice in each direction), as the figure behind the read-twice-from-L2 decision (DESIGN_LOG CMAT.1).

Each variant runs `iters` passes in a group that ends in one device synchronise; the variants alternate inside a round, at least five rounds after
a warm-up; the whole measurement runs twice; median and range per variant and run, host clock, profiler off.  One JSON line per configuration, and
the table as markdown to --out.

    python tools/bench_cma_attn_train.py [--rounds 5] [--iters 50] [--out profiles/cma_attn_train.md]
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
from robo_vln_amd import synth, train                      # noqa: E402
from robo_vln_amd.config import CMAConfig                  # noqa: E402

ROWS, HH, SCALE = 64, 256, 1.0 / 16.0
# stage -> (layout, C0, Ce, I, masked, value width or None)
STAGES = {"text": (train.TOKEN_MAJOR, 512, 0, 80, True, None), "rgb": (train.CHANNEL_MAJOR, 2048, 64, 16, False, 256),
          "depth": (train.CHANNEL_MAJOR, 128, 64, 16, False, 128)}


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


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
    runs = []
    for _ in range(2):
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.iters))
        runs.append({k: stats(v) for k, v in times.items()})
    return runs


def rel_diff(x, y):
    return ((x - y).abs().max() / y.abs().max()).item()


def reference_attn(q, k, v, mask=None):
    """CMANet._attn, cma.py:201-209"""
    logits = torch.einsum("nc, nci -> ni", q, k)
    if mask is not None:
        logits = logits - mask.float() * 1e8
    attn = torch.softmax(logits * SCALE, dim=1)
    return torch.einsum("ni, nci -> nc", attn, v)


def stage_routes(name):
    """the stage's leaves and its three routes as functions of nothing that return the stage's output"""
    layout, C0, Ce, I, masked, n_out = STAGES[name]
    g = torch.Generator().manual_seed(3)
    u = lambda *s, scale=1.0: ((torch.rand(*s, generator=g) * 2 - 1) * scale).cuda()
    C = C0 + Ce
    q = u(ROWS, HH).requires_grad_()
    if name == "text":
        x = u(ROWS, I, C0)
        for b in range(ROWS):                                      # lengths between I / 2 and I, as the trainer's padded instructions
            x[b, I // 2 + (b * 7) % (I // 2 + 1):] = 0
        x.requires_grad_()                                         # the instruction encoder trains
        w, bias = u(HH, C, 1, scale=2 * (3 / C) ** 0.5).requires_grad_(), u(HH, scale=0.1).requires_grad_()
        e = None
        leaves = [q, x, w]
    else:
        x = torch.relu(u(ROWS, C0, I))                             # a frozen trunk's feature: no gradient
        emb = u(I, 64, scale=0.5).requires_grad_()                 # spatial_embeddings.weight
        w, bias = u(HH + n_out, C, 1, scale=(3 / C) ** 0.5).requires_grad_(), u(HH + n_out, scale=0.1).requires_grad_()
        leaves = [q, emb, w, bias]
    cot = u(ROWS, n_out or C)

    def folded(fn):
        def run():
            if name == "text":
                return fn(q @ w[:, :, 0], x, None, True, SCALE, layout)
            xbar = fn(q @ w[:HH, :, 0], x, emb.view(64, I).t().contiguous(), False, SCALE, layout)
            return torch.nn.functional.linear(xbar, w[HH:, :, 0], bias[HH:])
        return run

    def ref():
        if name == "text":
            X = x.permute(0, 2, 1)                                 # (rows, D, L) as the instruction encoder returns it
            k = torch.nn.functional.conv1d(X, w, bias)
            return reference_attn(q, k, X, (X == 0.0).all(dim=1))
        X = torch.cat([x, emb.view(1, 64, I).expand(ROWS, 64, I)], dim=1)
        k, v = torch.split(torch.nn.functional.conv1d(X, w, bias), HH, dim=1)
        return reference_attn(q, k, v)

    return leaves, cot, {"hip": folded(train.attn1q), "ref": ref, "folded": folded(train.attn1q_ref)}


def bench_stage(name, a):
    leaves, cot, routes = stage_routes(name)

    def grads(fn):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(fn(), cot)
        return [t.grad.clone() for t in leaves]

    gr = {k: grads(fn) for k, fn in routes.items()}
    diff = {k: max(rel_diff(o, t) for o, t in zip(gr[k], gr["ref"])) for k in ("hip", "folded")}
    with torch.no_grad():
        out_diff = {k: rel_diff(routes[k](), routes["ref"]()) for k in ("hip", "folded")}
    runs = interleave({k: (lambda fn=fn: torch.autograd.backward(fn(), cot)) for k, fn in routes.items()}, a)
    res = {"what": "stage", "stage": name, "rows": ROWS, "shape": STAGES[name][1:4], "iters": a.iters, "rounds": a.rounds,
           "out_rel_difference_to_ref": {k: float(f"{v:.3e}") for k, v in out_diff.items()},
           "max_rel_grad_difference_to_ref": {k: float(f"{v:.3e}") for k, v in diff.items()}, "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def bench_op(name, a):
    """the attention op alone: forward, and forward + backward, with the bytes of x it streams (two reads per direction)"""
    layout, C0, Ce, I, masked, _ = STAGES[name]
    g = torch.Generator().manual_seed(4)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    qt = u(ROWS, C0 + Ce).requires_grad_()
    x = u(ROWS, I, C0) if layout == train.TOKEN_MAJOR else u(ROWS, C0, I)
    e = u(I, Ce).requires_grad_() if Ce else None
    cot = u(ROWS, C0 + Ce)

    def fwd():
        with torch.no_grad():
            return train.attn1q(qt, x, e, masked, SCALE, layout)

    runs = interleave({"forward": fwd, "forward_backward": lambda: torch.autograd.backward(train.attn1q(qt, x, e, masked, SCALE, layout), cot)}, a)
    res = {"what": "op", "stage": name, "rows": ROWS, "x_bytes": ROWS * C0 * I * 4, "reads_per_direction": 2, "iters": a.iters, "rounds": a.rounds, "runs": runs}
    print(json.dumps(res), flush=True)
    return res


class FoldedTorchCMANet(train.CMANet):
    """the same module with its attention stages on attn1q_ref (torch eager on the device); everything else unchanged"""

    def _attend(self, q, w_k, x, e, mask_zero, layout, kernel=True):
        return train.attn1q_ref(q @ w_k, x, e, mask_zero, self.scale, layout)


def bench_step(T, N, a):
    cfg = CMAConfig().validate()                                   # 256 x 256 frames: depth (128, 4, 4); L = 80
    sd = synth.make_cma_weights(cfg, 0)
    mods = {}
    for k, cls in (("hip", train.CMANet), ("torch_attention", FoldedTorchCMANet)):
        m = cls(cfg)
        m.load_reference_state_dict(sd)
        mods[k] = m.cuda().train()
    rows = T * N
    g = torch.Generator().manual_seed(5)
    ids = torch.from_numpy(synth.make_cma_observations(cfg, N, step=0, seed=0)["instruction"]).repeat(T, 1).cuda()
    obs = {"rgb_features": torch.relu(torch.rand(rows, 2048, 4, 4, generator=g) * 2 - 0.5).cuda(),
           "depth_features": torch.relu(torch.rand(rows, 128, 4, 4, generator=g) * 2 - 0.5).cuda(), "instruction": ids}
    h0 = torch.zeros(cfg.num_recurrent_layers, N, cfg.hidden, device="cuda")
    masks = torch.ones(rows, 1, device="cuda")
    masks[:N] = 0
    target = (torch.rand(rows, cfg.num_actions, generator=g) * 2 - 1).cuda()

    def step(m):
        def run():
            for p in m.parameters():
                p.grad = None
            out, stop, _ = m((obs, h0, None, masks))
            (torch.nn.functional.mse_loss(out, target) + stop.square().mean()).backward()
        return run

    with torch.no_grad():
        outs = {k: m((obs, h0, None, masks))[0] for k, m in mods.items()}
    runs = interleave({k: step(m) for k, m in mods.items()}, a)
    res = {"what": "step", "T": T, "N": N, "rows": rows, "iters": a.iters, "rounds": a.rounds,
           "out_rel_difference": float(f"{rel_diff(outs['hip'], outs['torch_attention']):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def cell(r):
    return f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f})"


def markdown(device, stages, ops, steps, a):
    o = ["# CMANet attention stages, forward + backward: device op against torch", "",
         f"`tools/bench_cma_attn_train.py --rounds {a.rounds} --iters {a.iters}` on {device}; float32; milliseconds per forward + backward, median",
         "(min-max) over the interleaved rounds, two runs in one process; host clock around groups that end in a device synchronise.", "",
         "## The three stages at the trainer's shape (64 rows)", "",
         "`hip`: q W_k, `train.attn1q`, value projection.  `ref`: the reference's formulation (`cat`, `conv1d`, `split`, `_attn`) in torch eager.",
         "`folded`: `train.attn1q_ref` with the same projections in torch eager.", "",
         "| stage | (C0, Ce, I) | route | run 1 | run 2 | ref / route (medians, run 1; run 2) |", "|---|---|---|---|---|---|"]
    for s in stages:
        for k in ("hip", "ref", "folded"):
            ratio = "; ".join(f"{r['ref']['median_ms'] / r[k]['median_ms']:.2f}" for r in s["runs"])
            o.append(f"| {s['stage']} | {tuple(s['shape'])} | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio} |")
    o += ["", "Largest relative difference to `ref` (output; gradients): " +
          "; ".join(f"{s['stage']}: hip {s['out_rel_difference_to_ref']['hip']:.1e}, {s['max_rel_grad_difference_to_ref']['hip']:.1e} / folded "
                    f"{s['out_rel_difference_to_ref']['folded']:.1e}, {s['max_rel_grad_difference_to_ref']['folded']:.1e}" for s in stages) + ".", "",
          "## The op alone (no projections)", "",
          "x is read twice forward (logits, weighted sum) and twice backward (da, d_qt); the second read of each pair comes from L2.", "",
          "| stage | x bytes | forward, run 1 | run 2 | forward + backward, run 1 | run 2 | x bytes read / forward time (run 1 median) |", "|---|---|---|---|---|---|---|"]
    for s in ops:
        r1, r2 = s["runs"]
        rate = 2 * s["x_bytes"] / (r1["forward"]["median_ms"] * 1e-3) / 1e9
        o.append(f"| {s['stage']} | {s['x_bytes']} | {cell(r1['forward'])} | {cell(r2['forward'])} | {cell(r1['forward_backward'])} | "
                 f"{cell(r2['forward_backward'])} | {rate:.0f} GB/s |")
    fw = [r["forward"]["median_ms"] * 1e3 for s in ops for r in s["runs"]]
    per_sample = ", ".join(f"{s['stage']} {s['x_bytes'] // ROWS // 1024} KiB" for s in ops)
    o += ["", "These times include the host's launch path (allocations and one launch forward, two backward); they bound the kernel from above.", "",
          "### Read twice from L2, or keep the sample in LDS", "",
          f"The forward call takes {min(fw):.1f}-{max(fw):.1f} us (medians, both runs) whether a sample is {per_sample}: at 64 rows the call's time is",
          "the launch path, and the second read of x is not visible in it.  Keeping the sample in LDS between the two passes could only shorten the",
          "kernel below that floor, would not fit a text sample from L = 80 with 512 channels upwards (160 KiB and more beside the staged query), and",
          "would need a second code path for the sizes that do fit.  The kernels therefore read x twice and stage nothing but the query, the",
          "cotangent and the I-vectors; an LDS-resident variant was not built, so there is no A/B figure for it (DESIGN_LOG CMAT.1).  The same floor",
          "answers the question of several workgroups per sample for few rows: the call does not get shorter with less work per workgroup.", "",
          "## The whole train.CMANet step from cached features", "",
          "`hip`: the module as it is.  `torch_attention`: the same module with its three attention stages on `attn1q_ref`.", "",
          "| (T, N) | route | run 1 | run 2 | torch_attention / hip (medians, run 1; run 2) |", "|---|---|---|---|---|"]
    for s in steps:
        ratio = "; ".join(f"{r['torch_attention']['median_ms'] / r['hip']['median_ms']:.3f}" for r in s["runs"])
        for k in ("hip", "torch_attention"):
            o.append(f"| ({s['T']}, {s['N']}) | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k == 'hip' else ''} |")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cma_attn_train.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cma_attn_train.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    stages = [bench_stage(n, a) for n in STAGES]
    ops = [bench_op(n, a) for n in STAGES]
    a_step = argparse.Namespace(rounds=a.rounds, iters=a.step_iters)
    steps = [bench_step(T, N, a_step) for T, N in ((16, 4), (8, 8))]
    text = markdown(device, stages, ops, steps, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
