"""Validation step: one hcm_val_step per chunk against what the same chunk cost before it existed -- hcm_high_forward_seq, then
hcm_low_forward_seq, then torch's criteria on the device.  Both run K chunks with ONE synchronise at the end, interleaved in one process
over several rounds; prints ms per chunk for both and the ratio, one JSON line per shape.

    python tools/bench_val.py [--rounds 3] [--chunks 20] [--shapes 32x3,32x2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from robo_vln_amd import synth                  # noqa: E402
from robo_vln_amd.config import HCMConfig       # noqa: E402
from robo_vln_amd.policy import HCMEngine       # noqa: E402


def baseline_chunk(eng, obs, oracle, corrected, stop_lab, hh, lh, masks, crit, select=False):
    """_update_agent_val (hierarchical_trainer.py:575-626) on top of the two sequence calls, everything on the device, nothing read back and no
    host wait: the stop loss is BCEWithLogitsLoss(reduction="none") * keep / keep.sum().  select=True: the reference's own torch.masked_select
    instead, which sizes its output on the host (one wait per chunk) -- a second, labelled column."""
    logits, hh = eng.high_forward_seq(obs, hh, masks)
    pad = oracle == 0
    high = crit[0](logits.masked_fill(pad.view(-1, 1), 0), oracle - 1)
    pred = torch.argmax(logits, 1)
    correct = ((pred == oracle - 1) & ~pad).sum()
    total = (~pad).sum()
    vel, stop, lh = eng.low_forward_seq(obs, lh, masks, (oracle - 1).masked_fill(pad, 4))
    action = crit[1](vel.masked_fill(corrected == 0, 0), corrected)
    keep = stop_lab != -1
    if select:
        st = crit[2](torch.masked_select(stop, keep), torch.masked_select(stop_lab, keep))
    else:
        st = (crit[3](stop, stop_lab.clamp(min=0)) * keep).sum() / keep.sum()
    return torch.stack([high, action, st, correct.float(), total.float()]), hh, lh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--shapes", default="32x3,32x2")
    a = ap.parse_args()
    cfg = HCMConfig().validate()                                  # 256 x 256 RGB-D, L = 80
    hi_sd, lo_sd = synth.make_weights(cfg, seed=0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    eng = HCMEngine(cfg, hi_sd, lo_sd, max_batch=max(T * N for T, N in shapes), precision="fp16")
    crit = (nn.CrossEntropyLoss(ignore_index=-1, reduction="mean"), nn.MSELoss(), nn.BCEWithLogitsLoss(), nn.BCEWithLogitsLoss(reduction="none"))
    print(json.dumps({"workspace_bytes": eng.query(4), "max_batch": eng.query(6)}), flush=True)
    for T, N in shapes:
        rows = T * N
        obs = {k: torch.from_numpy(v).cuda() for k, v in synth.make_observations(cfg, rows, step=0, seed=0, rgb_uint8=True).items()}
        rng = np.random.RandomState(0)
        oracle = torch.from_numpy(rng.randint(0, 5, rows)).cuda()
        obs["vln_oracle_action_sensor"] = oracle
        corrected = torch.from_numpy(rng.uniform(-1, 1, (rows, 2)).astype(np.float32)).cuda()
        stop_lab = torch.from_numpy(rng.randint(-1, 2, (rows, 1)).astype(np.float32)).cuda()
        masks = torch.ones(rows, device="cuda")
        masks[:N] = 0
        R = cfg.num_recurrent_layers
        table = torch.zeros(a.chunks, 8, device="cuda")

        def run_base(select=False):
            hh = torch.zeros(R, N, cfg.hidden, device="cuda"); lh = torch.zeros_like(hh)
            for _ in range(a.chunks):
                _, hh, lh = baseline_chunk(eng, obs, oracle, corrected, stop_lab, hh, lh, masks, crit, select)

        def run_calls_only():
            hh = torch.zeros(R, N, cfg.hidden, device="cuda"); lh = torch.zeros_like(hh)
            st = (oracle - 1).masked_fill(oracle == 0, 4)
            for _ in range(a.chunks):
                _, hh = eng.high_forward_seq(obs, hh, masks)
                _, _, lh = eng.low_forward_seq(obs, lh, masks, st)

        def run_cand():
            hh = torch.zeros(R, N, cfg.hidden, device="cuda"); lh = torch.zeros_like(hh)
            for i in range(a.chunks):
                _, hh, lh = eng.val_step(obs, corrected, stop_lab, hh, lh, masks, result=table[i])

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.chunks

        run_base(); run_base(True); run_calls_only(); run_cand()   # warm-up: kernel attribute setup, allocator
        base, sel, calls, cand = [], [], [], []
        for _ in range(a.rounds):
            base.append(timed(run_base))
            cand.append(timed(run_cand))
            sel.append(timed(lambda: run_base(True)))
            calls.append(timed(run_calls_only))
        b, c = float(np.median(base)), float(np.median(cand))
        print(json.dumps({"T": T, "N": N, "rows": rows, "chunks": a.chunks, "rounds": a.rounds, "baseline_ms_per_chunk": round(b, 4),
                          "val_step_ms_per_chunk": round(c, 4), "ratio_baseline_over_val_step": round(b / c, 4),
                          "baseline_all": [round(v, 4) for v in base], "val_step_all": [round(v, 4) for v in cand],
                          "baseline_masked_select_all": [round(v, 4) for v in sel], "two_seq_calls_only_all": [round(v, 4) for v in calls]}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
