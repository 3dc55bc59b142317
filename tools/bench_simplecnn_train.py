"""The SimpleCNN encoders' three convolutions, forward plus backward to the six parameters, float32, over two routes on the same GPU, frames and
cotangent:

    hip    robo_vln_amd.train.simple_cnn (hcm_op_simplecnn_train / _bwd, csrc/simplecnn_train.hip)
    torch  torch eager autograd of train.simple_cnn_ref on the device (MIOpen, warmed outside the timed loop so its kernel search is not timed)

at 64 and 256 rows of 256 x 256, depth and RGB, and at two small calls (8 rows of 64 x 64 depth, 32 rows of 128 x 128 RGB); then the whole train.flat_update step of the SimpleCNN train.Seq2SeqNet at (T, N) = (16, 4) and
(8, 8), and the low-level half of train.hier_update (zero_grad, update_loss, backward, Adam of train.LowLevel), each with the encoders on either
route.

Each variant runs `iters` passes in a group that ends in one device synchronise; the variants alternate inside a round, at least five rounds after
a warm-up; the whole measurement runs twice; median and range per variant and run, host clock, profiler off.  One JSON line per configuration, and
the table as markdown to --out.

    python tools/bench_simplecnn_train.py [--rounds 5] [--iters 10] [--out profiles/simplecnn_train_table.md]
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
from robo_vln_amd.config import HCMConfig, S2SConfig       # noqa: E402

OP_SHAPES = [(64, 256, 256, 1), (256, 256, 256, 1), (64, 256, 256, 3), (256, 256, 256, 3), (8, 64, 64, 1), (32, 128, 128, 3)]


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def interleave(variants, rounds, iters):
    for fn in variants.values():                                   # warm-up: code objects, allocator, MIOpen's kernel search
        for _ in range(3):
            fn()
    runs = []
    for _ in range(2):
        times = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, iters))
        runs.append({k: stats(v) for k, v in times.items()})
    return runs


def rel_diff(x, y):
    return ((x - y).abs().max() / y.abs().max()).item()


def bench_op(shape, a):
    B, H, W, Cin = shape
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, shape, generator=g).float() if Cin == 3 else torch.rand(shape, generator=g)).cuda()
    scale = 1 / 255.0 if Cin == 3 else 1.0
    params = []
    for co, ci, k in ((32, Cin, 8), (64, 32, 4), (32, 64, 3)):
        params += [(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5).cuda().requires_grad_(),
                   (torch.randn(co, generator=g) * 0.1).cuda().requires_grad_()]
    d_y = torch.randn(B, 32, *train.simple_cnn_out_hw(H, W), generator=g).cuda()
    routes = {"hip": lambda: train.simple_cnn(x, *params, scale=scale), "torch": lambda: train.simple_cnn_ref(x, *params, scale=scale)}

    def grads(fn):
        return torch.autograd.grad(fn(), params, d_y)

    gr = {k: grads(fn) for k, fn in routes.items()}
    runs = interleave({k: (lambda fn=fn: grads(fn)) for k, fn in routes.items()}, a.rounds, a.iters)
    res = {"what": "op", "B": B, "H": H, "W": W, "Cin": Cin, "iters": a.iters, "rounds": a.rounds,
           "max_rel_grad_difference": float(f"{max(rel_diff(o, t) for o, t in zip(gr['hip'], gr['torch'])):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def _to_torch_route(net):
    """the same model with its SimpleCNN encoders' convolutions on simple_cnn_ref (torch eager on the device); everything else unchanged"""
    for enc in (net.depth_encoder, net.rgb_encoder):
        if isinstance(enc, (train.SimpleDepthCNN, train.SimpleRGBCNN)):
            enc.route = "torch"
    return net


def _to_hip_route(net):
    for enc in (net.depth_encoder, net.rgb_encoder):
        if isinstance(enc, (train.SimpleDepthCNN, train.SimpleRGBCNN)):
            enc.route = "hip"
    return net


def bench_step(kind, T, N, a):
    rows = T * N
    g = torch.Generator().manual_seed(5)
    simple = dict(rgb_encoder="SimpleRGBCNN", depth_encoder="SimpleDepthCNN")
    if kind == "s2s":
        cfg = S2SConfig(**simple).validate()
        sd = synth.make_s2s_weights(cfg, 0)
        ids = synth.make_s2s_observations(cfg, N, step=0, seed=0)["instruction"]
        make = lambda: train.Seq2SeqNet(cfg, trainable_trunks=True)
    else:
        cfg = HCMConfig(**simple).validate()
        sd = synth.materialize(synth.low_level_spec(cfg), "lo", 0)
        make = lambda: train.LowLevel(cfg, trainable_trunks=True)
    obs = {"rgb": torch.randint(0, 256, (rows, *cfg.rgb_shape, 3), generator=g, dtype=torch.uint8).cuda(),
           "depth": torch.rand(rows, *cfg.depth_shape, 1, generator=g).cuda()}
    if kind == "s2s":
        obs["instruction"] = torch.from_numpy(ids).repeat(T, 1).cuda()
    corrected = torch.randn(rows, 2, generator=g).cuda()
    stop = (torch.rand(rows, 1, generator=g) < 0.5).float().cuda()
    h0 = torch.zeros(cfg.num_recurrent_layers, N, cfg.hidden, device="cuda")
    masks = torch.ones(rows, 2, device="cuda")
    masks[:N] = 0
    prev = torch.zeros(rows, 2, device="cuda")
    sub = torch.randint(0, cfg.num_sub_tasks, (rows,), generator=g).cuda() if kind == "lo" else None
    steps, first = {}, {}
    for k in ("hip", "torch_convs"):
        m = make()
        m.load_reference_state_dict(sd)
        m = m.cuda().train()
        (_to_torch_route if k == "torch_convs" else _to_hip_route)(m)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        if kind == "s2s":
            with torch.no_grad():
                first[k] = m.update_loss((obs, h0, prev, masks), corrected, stop)[0][:2]
            steps[k] = lambda m=m, opt=opt: train.flat_update(m, opt, obs, prev, masks, corrected, stop, h0)
        else:
            with torch.no_grad():
                first[k] = m.update_loss((obs, h0, prev, masks, sub), corrected, stop)[0][:2]

            def low_half(m=m, opt=opt):
                opt.zero_grad()
                res, _ = m.update_loss((obs, h0, prev, masks, sub), corrected, stop)
                (res[0] + res[1]).backward()
                opt.step()
            steps[k] = low_half
    runs = interleave(steps, a.rounds, a.step_iters)
    res = {"what": "step", "model": kind, "T": T, "N": N, "rows": rows, "iters": a.step_iters, "rounds": a.rounds,
           "loss_rel_difference": float(f"{rel_diff(first['hip'], first['torch_convs']):.3e}"), "runs": runs}
    print(json.dumps(res), flush=True)
    return res


def cell(r):
    return f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f})"


def verdict(s, ours, theirs):
    """the decision rule: `torch` only where torch's range lies wholly below the op's in both runs"""
    return "torch" if all(r[theirs]["max_ms"] < r[ours]["min_ms"] for r in s["runs"]) else "hip"


def markdown(device, ops, steps, a):
    o = [f"`tools/bench_simplecnn_train.py --rounds {a.rounds} --iters {a.iters} --step-iters {a.step_iters}` on {device}; float32; milliseconds, median",
         "(min-max) over the interleaved rounds, two runs in one process; host clock around groups that end in a device synchronise.", "",
         "## The op, forward + backward to the six parameters", "",
         "| frames | route | run 1 | run 2 | torch / hip (medians, run 1; run 2) | faster in both runs by range |", "|---|---|---|---|---|---|"]
    for s in ops:
        ratio = "; ".join(f"{r['torch']['median_ms'] / r['hip']['median_ms']:.2f}" for r in s["runs"])
        for k in ("hip", "torch"):
            o.append(f"| {s['B']} x {s['H']} x {s['W']} x {s['Cin']} | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | "
                     f"{ratio if k == 'hip' else ''} | {verdict(s, 'hip', 'torch') if k == 'hip' else ''} |")
    o += ["", "Largest relative difference between the routes' gradients: " +
          "; ".join(f"{s['B']} x {s['H']} x {s['W']} x {s['Cin']}: {s['max_rel_grad_difference']:.1e}" for s in ops) + ".", "",
          "## Whole update steps of the SimpleCNN models (both encoders SimpleCNN, 256 x 256 frames, uint8 RGB, Adam)", "",
          "`hip`: the encoders' convolutions on `simple_cnn`.  `torch_convs`: the same model with them on `simple_cnn_ref`.  `s2s`: `train.flat_update` of",
          "`train.Seq2SeqNet`; `lo`: the low-level half of `train.hier_update` on `train.LowLevel`.", "",
          "| model | (T, N) | route | run 1 | run 2 | torch_convs / hip (medians, run 1; run 2) |", "|---|---|---|---|---|---|"]
    for s in steps:
        ratio = "; ".join(f"{r['torch_convs']['median_ms'] / r['hip']['median_ms']:.3f}" for r in s["runs"])
        for k in ("hip", "torch_convs"):
            o.append(f"| {s['model']} | ({s['T']}, {s['N']}) | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k == 'hip' else ''} |")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplecnn_train_table.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplecnn_train.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    ops = [bench_op(s, a) for s in OP_SHAPES]
    steps = [bench_step(kind, T, N, a) for kind in ("s2s", "lo") for T, N in ((16, 4), (8, 8))]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(markdown(device, ops, steps, a))


if __name__ == "__main__":
    main()
