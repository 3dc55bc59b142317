"""Forward plus backward of the differentiable state encoder (robo_vln_amd.train.state_scan: hcm_op_state_scan_train, hcm_op_state_scan_bwd
and the batched torch reductions) against torch.nn.LSTM / nn.GRU on the same GPU and the same rows, run the way the reference's seq_forward
runs them: split at the steps that have a zero mask, the state multiplied by that step's masks (state_encoder.py:99-126).  hidden 512, input
640, float32; masks are zero at t = 0 and at one interior step.  Each variant runs K forward+backward passes in a group that ends in one
device synchronise; the torch variant additionally reads its split points from the device once per pass, as the reference does
(state_encoder.py:101: `.nonzero().squeeze().cpu()`), which waits for the work enqueued before it -- that read is part of what the
reference's way costs and is in its column; `torch_rnn_presplit` is the same calls with the split points found once outside the timed
loop, so that it too only enqueues.  The variants are interleaved in one process over several rounds after a warm-up; median and
range per variant, one JSON line per (rnn, shape).

    python tools/bench_state_scan_bwd.py [--rounds 5] [--iters 20] [--shapes 16x4,8x8]
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

H, I = 512, 640


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def split_points(masks, T, N):
    """the split points as state_encoder.py:101-110 finds them: ONE device-to-host read"""
    return [0] + ((masks.view(T, N)[1:] == 0.0).any(dim=-1).nonzero().reshape(-1).cpu() + 1).tolist() + [T]


def torch_seq_forward(rnn, lstm, x, hidden, masks, T, N, zeros=None):
    """the reference's seq_forward (for LSTM too, which the reference's own raises for): one rnn call per run of steps without a zero mask;
    `zeros`: split points found beforehand (no device read in the call), else found here as the reference does"""
    x, masks = x.view(T, N, -1), masks.view(T, N)
    zeros = split_points(masks, T, N) if zeros is None else zeros
    hs = (hidden[0:1], hidden[1:2]) if lstm else hidden
    outs = []
    for a, b in zip(zeros[:-1], zeros[1:]):
        mk = masks[a].view(1, -1, 1)
        hs = tuple(v * mk for v in hs) if lstm else hs * mk
        o, hs = rnn(x[a:b], hs)
        outs.append(o)
    return torch.cat(outs, 0).view(T * N, -1)


def bench(rnn_type, T, N, a):
    lstm = rnn_type == "LSTM"
    g = torch.Generator().manual_seed(0)
    enc = train.RNNStateEncoder(I, H, rnn_type=rnn_type)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    enc = enc.cuda()
    ref = getattr(torch.nn, rnn_type)(I, H).cuda()
    ref.load_state_dict(enc.rnn.state_dict())
    x = (torch.rand(T * N, I, generator=g) * 2 - 1).cuda().requires_grad_()
    hidden = (torch.rand(2 if lstm else 1, N, H, generator=g) - 0.5).cuda()
    masks = torch.ones(T, N)
    masks[0] = 0
    masks[T // 2, N // 2] = 0
    masks = masks.reshape(-1).cuda()
    cot = (torch.rand(T * N, H, generator=g) * 2 - 1).cuda()

    def run_ours():
        for _ in range(a.iters):
            seq, _ = enc(x, hidden, masks)
            torch.autograd.backward(seq, cot)

    def run_torch():
        for _ in range(a.iters):
            torch.autograd.backward(torch_seq_forward(ref, lstm, x, hidden, masks, T, N), cot)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    zeros = split_points(masks, T, N)

    def run_torch_presplit():
        for _ in range(a.iters):
            torch.autograd.backward(torch_seq_forward(ref, lstm, x, hidden, masks, T, N, zeros), cot)

    variants = {"state_scan": run_ours, "torch_rnn": run_torch, "torch_rnn_presplit": run_torch_presplit}
    for fn in variants.values():                                   # warm-up: code objects, allocator, the BLAS library's choices
        fn()
    for p in list(enc.parameters()) + list(ref.parameters()) + [x]:
        p.grad = None
    run_ours()
    ours = [p.grad.clone() for p in enc.parameters()] + [x.grad.clone()]
    for p in list(enc.parameters()) + [x]:
        p.grad = None
    run_torch()
    theirs = [p.grad.clone() for p in ref.parameters()] + [x.grad.clone()]
    agree = max(((o - t).abs().max() / t.abs().max()).item() for o, t in zip(ours, theirs))     # same rows, same weights: the two must agree
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    ours_ms, torch_ms, pre_ms = (float(np.median(times[k])) for k in variants)
    print(json.dumps({"rnn": rnn_type, "T": T, "N": N, "hidden": H, "input": I, "iters": a.iters, "rounds": a.rounds,
                      "state_scan_fwd_bwd": stats(times["state_scan"]), "torch_rnn_fwd_bwd": stats(times["torch_rnn"]),
                      "torch_rnn_presplit_fwd_bwd": stats(times["torch_rnn_presplit"]),
                      "ratio_torch_over_state_scan": round(torch_ms / ours_ms, 3), "ratio_presplit_over_state_scan": round(pre_ms / ours_ms, 3),
                      "max_rel_grad_difference": float(f"{agree:.3e}")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="16x4,8x8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_state_scan_bwd.py measures on the GPU; none is visible")
    for rnn_type in ("LSTM", "GRU"):
        for T, N in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
            bench(rnn_type, T, N, a)


if __name__ == "__main__":
    main()
