"""Forward plus backward of the differentiable instruction encoder (robo_vln_amd.train.InstructionEncoder: embedding, torch.addmm,
hcm_op_instr_scan_train, hcm_op_instr_scan_bwd and the batched torch reductions) against the reference's own sequence on the same GPU, the same
rows and the same weights: embedding, `lengths.cpu()`, pack_padded_sequence(enforce_sorted=False), nn.LSTM / nn.GRU, then pad_packed_sequence
or the final state (instruction_encoder.py:80-92).  hidden 256, embedding 50, float32, frozen embeddings (the reference default); B rows with
ragged lengths in [L/2, L].  Each variant runs K forward+backward passes in a group that ends in one device synchronise.  The reference's
`lengths.cpu()` waits for the work enqueued before it; that read is part of what the reference's way costs and is in its column;
`torch_packed_hostlen` is the same calls with the lengths read once outside the timed loop, so that it too only enqueues.  The variants are
interleaved in one process over several rounds after a warm-up; median and range per variant, one JSON line per (setting, shape).

The clock is the host's around a group that ends in a device synchronise, not a pair of events on the stream: the reference's route blocks the
host in the middle of every pass, and that wait is part of what is compared -- events on the stream would time the device's share only and
leave it out.  A group is tens of milliseconds of device work, so the one synchronise at its end is a small part of it.

    python tools/bench_instr_scan_bwd.py [--rounds 5] [--iters 10] [--rows 64] [--lengths 80,200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from robo_vln_amd import train                              # noqa: E402

H, E, VOCAB = 256, 50, 2504
# (name, rnn_type, bidirectional, final_state_only): CMANet's encoder; Seq2SeqNet's with either cell
SETTINGS = [("cma_lstm_bidir_full", "LSTM", True, False), ("s2s_lstm_final", "LSTM", False, True), ("s2s_gru_final", "GRU", False, True)]


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def reference_forward(emb, rnn, final, instruction, lengths=None):
    """instruction_encoder.py:80-92; `lengths`: read beforehand (no device read in the call), else read here as the reference does"""
    if lengths is None:
        lengths = (instruction != 0.0).long().sum(dim=1).cpu()
    packed = pack_padded_sequence(emb(instruction), lengths, batch_first=True, enforce_sorted=False)
    output, final_state = rnn(packed)
    if final:
        return (final_state[0] if isinstance(final_state, tuple) else final_state).squeeze(0)
    return pad_packed_sequence(output, batch_first=True)[0].permute(0, 2, 1)


def bench(name, rnn_type, bidir, final, B, L, a):
    g = torch.Generator().manual_seed(0)
    table = torch.rand(VOCAB, E, generator=g) * 2 - 1
    table[0] = 0
    enc = train.InstructionEncoder(embeddings=table, hidden_size=H, rnn_type=rnn_type, bidirectional=bidir, final_state_only=final)
    with torch.no_grad():
        for p in enc.encoder_rnn.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    enc = enc.cuda()
    ref_emb = torch.nn.Embedding.from_pretrained(table.clone(), freeze=True).cuda()
    ref_rnn = getattr(torch.nn, rnn_type)(input_size=E, hidden_size=H, bidirectional=bidir).cuda()
    ref_rnn.load_state_dict(enc.encoder_rnn.state_dict())
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    lens[0] = L                                                    # one full row: both routes return L columns
    ids = torch.randint(1, VOCAB, (B, L), generator=g)
    ids[torch.arange(L)[None, :] >= lens[:, None]] = 0
    ids = ids.cuda()
    cot = (torch.rand((B, H) if final else (B, (2 if bidir else 1) * H, L), generator=g) * 2 - 1).cuda()

    def run_ours():
        for _ in range(a.iters):
            torch.autograd.backward(enc(ids), cot)

    def run_torch():
        for _ in range(a.iters):
            torch.autograd.backward(reference_forward(ref_emb, ref_rnn, final, ids), cot)

    def run_torch_hostlen():
        for _ in range(a.iters):
            torch.autograd.backward(reference_forward(ref_emb, ref_rnn, final, ids, lens), cot)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    variants = {"instr_scan": run_ours, "torch_packed": run_torch, "torch_packed_hostlen": run_torch_hostlen}
    for fn in variants.values():                                   # warm-up: code objects, allocator, the BLAS library's choices
        fn()
    for p in list(enc.parameters()) + list(ref_rnn.parameters()):
        p.grad = None
    run_ours()
    ours = [p.grad.clone() for p in enc.encoder_rnn.parameters()]
    run_torch()
    theirs = [p.grad.clone() for p in ref_rnn.parameters()]
    agree = max(((o - t).abs().max() / t.abs().max()).item() for o, t in zip(ours, theirs))     # same rows, same weights: the two must agree
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    ours_ms, torch_ms, host_ms = (float(np.median(times[k])) for k in variants)
    print(json.dumps({"setting": name, "B": B, "L": L, "hidden": H, "embedding": E, "iters": a.iters, "rounds": a.rounds,
                      "instr_scan_fwd_bwd": stats(times["instr_scan"]), "torch_packed_fwd_bwd": stats(times["torch_packed"]),
                      "torch_packed_hostlen_fwd_bwd": stats(times["torch_packed_hostlen"]),
                      "ratio_torch_over_instr_scan": round(torch_ms / ours_ms, 3), "ratio_hostlen_over_instr_scan": round(host_ms / ours_ms, 3),
                      "max_rel_grad_difference": float(f"{agree:.3e}")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--lengths", default="80,200")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instr_scan_bwd.py measures on the GPU; none is visible")
    for name, rnn_type, bidir, final in SETTINGS:
        for L in (int(v) for v in a.lengths.split(",")):
            bench(name, rnn_type, bidir, final, a.rows, L, a)


if __name__ == "__main__":
    main()
