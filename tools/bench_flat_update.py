"""The end of the flat trainer's update step -- the heads of CMANet / Seq2SeqNet and the criterion of `_update_agent` (robo_vln_trainer.py:521-533),
forward plus backward, float32 -- over two routes on the same GPU, inputs and cotangents:

    hip    robo_vln_amd.train.flat_heads_loss (hcm_op_flat_heads_loss_train / _bwd: two launches each way)
    torch  torch eager autograd of the reference's statements (train.flat_heads_loss_ref on the device)

at 64, 256 and 1024 rows with and without the progress monitor, and the whole train.flat_update step (zero_grad, forward, criterion, backward, Adam)
of train.Seq2SeqNet and train.CMANet from cached features at (T, N) = (16, 4) and (8, 8) against the same module with its heads and criterion on
flat_heads_loss_ref.

Each variant runs `iters` passes in a group that ends in one device synchronise; the variants alternate inside a round, at least five rounds after
a warm-up; the whole measurement runs twice; median and range per variant and run, host clock, profiler off.  One JSON line per configuration, and
the table as markdown to --out.

    python tools/bench_flat_update.py [--rounds 5] [--iters 50] [--out profiles/flat_update.md]
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
from robo_vln_amd.config import CMAConfig, S2SConfig       # noqa: E402

H, A = 512, 2
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


def labels(rows, g):
    """corrected_actions and oracle_stop with every seventh row padded and a few exact zeros in valid rows, progress uniform in [0, 1]"""
    corrected = torch.randn(rows, A, generator=g)
    stop = (torch.rand(rows, 1, generator=g) < 0.5).float()
    corrected[4::7], stop[4::7] = 0.0, -1.0
    corrected[1::5, 0] = 0.0
    return corrected, stop, torch.rand(rows, generator=g)


def bench_op(rows, monitor, a):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows, H, generator=g).cuda().requires_grad_()              # the state encoder's output: it needs d_x
    params = []
    for n in (A, 1, 1):
        params += [(torch.randn(n, H, generator=g) / math.sqrt(H)).cuda().requires_grad_(), (torch.randn(n, generator=g) * 0.1).cuda().requires_grad_()]
    corrected, stop, progress = (t.cuda() for t in labels(rows, g))
    if not monitor:
        params[4:], progress = [None, None], None
    leaves = [x] + [p for p in params if p is not None]
    cot = torch.tensor([1.0, 1.0, 1.0, 0, 0, 0, 0, 0], device="cuda")          # the trainer's loss is the sum of the three

    def route(fn):
        return lambda: fn(x, *params, corrected, stop, progress)[0]

    routes = {"hip": route(train.flat_heads_loss), "torch": route(train.flat_heads_loss_ref)}

    def grads(fn):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(fn(), cot)
        return [t.grad.clone() for t in leaves]

    gr = {k: grads(fn) for k, fn in routes.items()}
    with torch.no_grad():
        out_diff = rel_diff(routes["hip"]()[:3], routes["torch"]()[:3])
    runs = interleave({k: (lambda fn=fn: torch.autograd.backward(fn(), cot)) for k, fn in routes.items()}, a)
    res = {"what": "op", "rows": rows, "monitor": monitor, "iters": a.iters, "rounds": a.rounds, "loss_rel_difference": float(f"{out_diff:.3e}"),
           "max_rel_grad_difference": float(f"{max(rel_diff(o, t) for o, t in zip(gr['hip'], gr['torch'])):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def bench_step(kind, T, N, a):
    """train.flat_update of one module, progress monitor on, from cached features at the full frame size (depth feature (128, 4, 4), L = 80)"""
    if kind == "s2s":
        cfg = S2SConfig(progress_monitor=True).validate()
        sd, cls, rgb_shape = synth.make_s2s_weights(cfg, 0), train.Seq2SeqNet, (2048, 1, 1)
        ids = synth.make_s2s_observations(cfg, N, step=0, seed=0)["instruction"]
        make = lambda c: c(cfg)
    else:
        cfg = CMAConfig().validate()
        sd, cls, rgb_shape = synth.make_cma_weights(cfg, 0), train.CMANet, (2048, 4, 4)
        ids = synth.make_cma_observations(cfg, N, step=0, seed=0)["instruction"]
        make = lambda c: c(cfg, progress_monitor=True)

    class TorchHeads(cls):
        """the same module with its heads and criterion on flat_heads_loss_ref (torch eager on the device); everything else unchanged"""
        _flat_heads = staticmethod(train.flat_heads_loss_ref)

    rows = T * N
    g = torch.Generator().manual_seed(5)
    fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
    obs = {"rgb_features": torch.relu(torch.rand(rows, *rgb_shape, generator=g) * 2 - 0.5).cuda(),
           "depth_features": torch.relu(torch.rand(rows, cc, fs, fs, generator=g) * 2 - 0.5).cuda(),
           "instruction": torch.from_numpy(ids).repeat(T, 1).cuda(), "progress": torch.rand(rows, generator=g).cuda()}
    corrected, stop, _ = (t.cuda() for t in labels(rows, g))
    h0 = torch.zeros(cfg.num_recurrent_layers, N, cfg.hidden, device="cuda")
    masks = torch.ones(rows, 2, device="cuda")
    masks[:N] = 0
    prev = torch.zeros(rows, 2, device="cuda")
    mods, steps, first = {}, {}, {}
    for k, c in (("hip", cls), ("torch_heads", TorchHeads)):
        m = make(c)
        m.load_reference_state_dict(sd)
        mods[k] = m.cuda().train()
        with torch.no_grad():
            first[k] = mods[k].update_loss((obs, h0, prev, masks), corrected, stop)[0][:3]
        opt = torch.optim.Adam(mods[k].parameters(), lr=1e-4)
        steps[k] = lambda m=mods[k], opt=opt: train.flat_update(m, opt, obs, prev, masks, corrected, stop, h0)
    runs = interleave(steps, a)
    res = {"what": "step", "model": kind, "T": T, "N": N, "rows": rows, "iters": a.iters, "rounds": a.rounds,
           "loss_rel_difference": float(f"{rel_diff(first['hip'], first['torch_heads']):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def cell(r):
    return f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f})"


def markdown(device, ops, steps, a):
    o = ["# The flat trainer's update step: fused heads and criterion against torch", "",
         f"`tools/bench_flat_update.py --rounds {a.rounds} --iters {a.iters} --step-iters {a.step_iters}` on {device}; float32; milliseconds, median",
         "(min-max) over the interleaved rounds, two runs in one process; host clock around groups that end in a device synchronise.", "",
         "## The op, forward + backward", "",
         "`hip`: `train.flat_heads_loss` (the heads launch, `flat_val_loss_kernel`, the backward's row-block launch, the ordered reduce).  `torch`: torch",
         f"eager autograd of the reference's statements (`train.flat_heads_loss_ref`) on the device.  hidden 512, {A} actions; x requires a gradient.", "",
         "| rows | monitor | route | run 1 | run 2 | torch / hip (medians, run 1; run 2) | hip's range below torch's in both runs |", "|---|---|---|---|---|---|---|"]
    for s in ops:
        ratio = "; ".join(f"{r['torch']['median_ms'] / r['hip']['median_ms']:.2f}" for r in s["runs"])
        below = all(r["hip"]["max_ms"] < r["torch"]["min_ms"] for r in s["runs"])
        for k in ("hip", "torch"):
            o.append(f"| {s['rows']} | {'on' if s['monitor'] else 'off'} | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | "
                     f"{ratio if k == 'hip' else ''} | {('yes' if below else 'NO') if k == 'hip' else ''} |")
    o += ["", "Largest relative difference between the routes (the three losses; gradients): " +
          "; ".join(f"{s['rows']} rows, monitor {'on' if s['monitor'] else 'off'}: {s['loss_rel_difference']:.1e}, {s['max_rel_grad_difference']:.1e}"
                    for s in ops) + ".", "",
          "These times include the host's launch path (allocations, two launches each way, autograd's bookkeeping); they bound the kernels from above.", "",
          "## The whole `train.flat_update` step from cached features (progress monitor on, Adam)", "",
          "`hip`: the module as it is.  `torch_heads`: the same module with its heads and criterion on `flat_heads_loss_ref`.", "",
          "| model | (T, N) | route | run 1 | run 2 | torch_heads / hip (medians, run 1; run 2) |", "|---|---|---|---|---|---|"]
    for s in steps:
        ratio = "; ".join(f"{r['torch_heads']['median_ms'] / r['hip']['median_ms']:.3f}" for r in s["runs"])
        for k in ("hip", "torch_heads"):
            o.append(f"| {s['model']} | ({s['T']}, {s['N']}) | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k == 'hip' else ''} |")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_update.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flat_update.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    ops = [bench_op(rows, monitor, a) for rows in OP_ROWS for monitor in (True, False)]
    a_step = argparse.Namespace(rounds=a.rounds, iters=a.step_iters)
    steps = [bench_step(kind, T, N, a_step) for kind in ("s2s", "cma") for T, N in ((16, 4), (8, 8))]
    text = markdown(device, ops, steps, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
