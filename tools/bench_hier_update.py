"""The end of the hierarchical trainer's high-level update step -- the head of Seq2Seq_HighLevel_CMA and the cross-entropy of `_update_agent`
(hierarchical_trainer.py:506-511), forward plus backward, float32 -- over two routes on the same GPU, inputs and cotangents:

    hip    robo_vln_amd.train.subtask_ce (hcm_op_subtask_ce_train / _bwd: two launches each way)
    torch  torch eager autograd of the reference's statements (train.subtask_ce_ref on the device)

at 64, 256 and 1024 rows, and the whole train.hier_update step (zero_grad, both models' forward, criterion, backward and Adam) of train.HighLevel /
train.LowLevel from cached features and a cached instruction stream at (T, N) = (16, 4) and (8, 8), L = 80, against the same pair with both
models' heads and criteria in torch (subtask_ce_ref, flat_heads_loss_ref).

Each variant runs `iters` passes in a group that ends in one device synchronise; the variants alternate inside a round, at least five rounds after
a warm-up; the whole measurement runs twice; median and range per variant and run, host clock, profiler off.  One JSON line per configuration, and
the table as markdown to --out.

    python tools/bench_hier_update.py [--rounds 5] [--iters 50] [--out profiles/hier_update.md]
"""
import argparse
import json
import math
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
from robo_vln_amd.config import HCMConfig                  # noqa: E402

H, A = 512, 4
OP_ROWS = (64, 256, 1024)


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


def labels(rows):
    """the oracle sub-task as the collate function carries it, (rows, 1) float: the classes 1..4 in turn, every seventh row padded"""
    o = (torch.arange(rows) % A + 1).float().reshape(rows, 1)
    o[4::7] = 0.0
    return o


def bench_op(rows, a):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows, H, generator=g).cuda().requires_grad_()              # the state encoder's output: it needs d_x
    w = (torch.randn(A, H, generator=g) / math.sqrt(H)).cuda().requires_grad_()
    b = (torch.randn(A, generator=g) * 0.1).cuda().requires_grad_()
    oracle = labels(rows).cuda()
    leaves = [x, w, b]
    cot = torch.tensor([1.0, 0, 0, 0, 0, 0, 0, 0], device="cuda")              # the trainer's loss is result[0]

    def route(fn):
        return lambda: fn(x, w, b, oracle, A)[0]

    routes = {"hip": route(train.subtask_ce), "torch": route(train.subtask_ce_ref)}

    def grads(fn):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(fn(), cot)
        return [t.grad.clone() for t in leaves]

    gr = {k: grads(fn) for k, fn in routes.items()}
    with torch.no_grad():
        out_diff = rel_diff(routes["hip"]()[:1], routes["torch"]()[:1])
    runs = interleave({k: (lambda fn=fn: torch.autograd.backward(fn(), cot)) for k, fn in routes.items()}, a)
    res = {"what": "op", "rows": rows, "iters": a.iters, "rounds": a.rounds, "loss_rel_difference": float(f"{out_diff:.3e}"),
           "max_rel_grad_difference": float(f"{max(rel_diff(o, t) for o, t in zip(gr['hip'], gr['torch'])):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


class TorchHigh(train.HighLevel):
    """the same module with its head and criterion on subtask_ce_ref (torch eager on the device); everything else unchanged"""
    _subtask_ce = staticmethod(train.subtask_ce_ref)


class TorchLow(train.LowLevel):
    _flat_heads = staticmethod(train.flat_heads_loss_ref)


def bench_step(T, N, a):
    """train.hier_update of the pair from cached features at the full frame size (depth feature (128, 4, 4)) and a cached stream of L = 80"""
    cfg = HCMConfig().validate()
    spec_hi = [s for s in synth.high_level_spec(cfg) if not s[0].startswith(train.HCM_HIGH_FROZEN_PREFIXES)]
    spec_lo = [s for s in synth.low_level_spec(cfg) if not s[0].startswith(train.HCM_LOW_FROZEN_PREFIXES)]
    hi_sd, lo_sd = synth.materialize(spec_hi, "hi", 0), synth.materialize(spec_lo, "lo", 0)
    rows = T * N
    g = torch.Generator().manual_seed(5)
    fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()

    def feat(*shape):
        return torch.relu(torch.rand(rows, *shape, generator=g) * 2 - 0.5).cuda()

    obs = {"rgb_features": (feat(2048, 4, 4), feat(2048, 1, 1)), "depth_features": (feat(cc, fs, fs), feat(cc, fs, fs)),
           "instruction_features": torch.randn(N, cfg.instr_len, cfg.ins_in, generator=g).repeat(T, 1, 1).cuda(),
           "vln_oracle_action_sensor": labels(rows).cuda()}
    corrected = torch.randn(rows, cfg.lo_actions, generator=g)
    stop = (torch.rand(rows, 1, generator=g) < 0.5).float()
    corrected[4::7], stop[4::7] = 0.0, -1.0
    corrected, stop = corrected.cuda(), stop.cuda()
    R = cfg.num_recurrent_layers
    h_hi, h_lo = (torch.zeros(R, N, cfg.hidden, device="cuda") for _ in range(2))
    masks = torch.ones(rows, 2, device="cuda")
    masks[:N] = 0
    prev = torch.zeros(rows, 2, device="cuda")
    steps, first = {}, {}
    for k, (ch, cl) in (("hip", (train.HighLevel, train.LowLevel)), ("torch_heads", (TorchHigh, TorchLow))):
        high, low = ch(cfg), cl(cfg)
        high.load_reference_state_dict(hi_sd)
        low.load_reference_state_dict(lo_sd)
        high, low = high.cuda().train(), low.cuda().train()
        with torch.no_grad():
            first[k] = high.eval().update_loss((obs, h_hi, prev, masks), obs["vln_oracle_action_sensor"])[0][:1]
        high.train()
        opts = (torch.optim.Adam(high.parameters(), lr=1e-4), torch.optim.Adam(low.parameters(), lr=1e-4))
        steps[k] = lambda high=high, low=low, opts=opts: train.hier_update(high, low, *opts, obs, prev, masks, corrected, stop, h_hi, h_lo)
    runs = interleave(steps, a)
    res = {"what": "step", "T": T, "N": N, "rows": rows, "L": cfg.instr_len, "iters": a.iters, "rounds": a.rounds,
           "loss_rel_difference": float(f"{rel_diff(first['hip'], first['torch_heads']):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def cell(r):
    return f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f})"


def markdown(device, ops, steps, a):
    o = ["# The hierarchical trainer's update step: fused sub-task head and cross-entropy against torch", "",
         f"`tools/bench_hier_update.py --rounds {a.rounds} --iters {a.iters} --step-iters {a.step_iters}` on {device}; float32; milliseconds, median",
         "(min-max) over the interleaved rounds, two runs in one process; host clock around groups that end in a device synchronise.", "",
         "## The op, forward + backward", "",
         "`hip`: `train.subtask_ce` (the head launch, the criterion launch, the backward's row-block launch, the ordered reduce).  `torch`: torch eager",
         f"autograd of the reference's statements (`train.subtask_ce_ref`) on the device.  hidden 512, {A} classes; x requires a gradient.", "",
         "| rows | route | run 1 | run 2 | torch / hip (medians, run 1; run 2) | hip's range below torch's in both runs |", "|---|---|---|---|---|---|"]
    for s in ops:
        ratio = "; ".join(f"{r['torch']['median_ms'] / r['hip']['median_ms']:.2f}" for r in s["runs"])
        below = all(r["hip"]["max_ms"] < r["torch"]["min_ms"] for r in s["runs"])
        for k in ("hip", "torch"):
            o.append(f"| {s['rows']} | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k == 'hip' else ''} | "
                     f"{('yes' if below else 'NO') if k == 'hip' else ''} |")
    o += ["", "Largest relative difference between the routes (the loss; gradients): " +
          "; ".join(f"{s['rows']} rows: {s['loss_rel_difference']:.1e}, {s['max_rel_grad_difference']:.1e}" for s in ops) + ".", "",
          "These times include the host's launch path (allocations, two launches each way, autograd's bookkeeping); they bound the kernels from above.", "",
          "## The whole `train.hier_update` step from cached features and a cached instruction stream (L = 80, dropout 0.25, Adam)", "",
          "`hip`: the pair as it is.  `torch_heads`: the same pair with both models' heads and criteria in torch (`subtask_ce_ref`, `flat_heads_loss_ref`).", "",
          "| (T, N) | route | run 1 | run 2 | torch_heads / hip (medians, run 1; run 2) |", "|---|---|---|---|---|"]
    for s in steps:
        ratio = "; ".join(f"{r['torch_heads']['median_ms'] / r['hip']['median_ms']:.3f}" for r in s["runs"])
        for k in ("hip", "torch_heads"):
            o.append(f"| ({s['T']}, {s['N']}) | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k == 'hip' else ''} |")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hier_update.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hier_update.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    ops = [bench_op(rows, a) for rows in OP_ROWS]
    a_step = argparse.Namespace(rounds=a.rounds, iters=a.step_iters)
    steps = [bench_step(T, N, a_step) for T, N in ((16, 4), (8, 8))]
    text = markdown(device, ops, steps, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
