"""Flat validation step: one hcm_flat_val_step per chunk against what the same chunk cost before it existed -- the kind's forward_seq, then
torch's criteria on the device tensors, then the reference's `.item()` reads (robo_vln_trainer.py:571-574: action, stop, and aux when it is
a tensor, i.e. with the progress monitor).  fp16, 256 x 256 frames, L = 80, T*N = 64 rows per chunk, CMANet and Seq2SeqNet (with
PROGRESS_MONITOR.use, so that all three criteria and all three reads are there).

Three routes per shape, each timed over an "epoch" of K chunks with the state carried, by a host clock around work that ends in a device
synchronise, the routes alternating inside every round (the order flips from round to round):

    parent      forward_seq + criteria + the reads, every chunk               (the route without this call)
    read_each   val_step + one read of its eight floats, every chunk         (the call used like the parent route: per-chunk cost, read included)
    epoch       val_step into a device table row, ONE read after K chunks    (FlatValidator's way)

Prints one JSON line per (kind, shape); --md FILE also writes the table of profiles/flat_val_step.md.

    python tools/bench_flat_val.py [--rounds 7] [--chunks 20] [--shapes 16x4,8x8] [--md FILE]
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
from robo_vln_amd import synth                        # noqa: E402
from robo_vln_amd.cma import CMAEngine                # noqa: E402
from robo_vln_amd.config import CMAConfig, S2SConfig  # noqa: E402
from robo_vln_amd.seq2seq import S2SEngine            # noqa: E402


def parent_chunk(kind, eng, obs, corrected, stop_lab, progress, h, masks, T, N, crit):
    """_update_agent_val (robo_vln_trainer.py:553-574) on top of the sequence forward: torch's criteria on the device tensors, then the reads."""
    if kind == "cma":
        out, stop, h = eng.forward_seq(obs, h, masks, T, N)
        prog = None
    else:
        out, stop, prog, h = eng.forward_seq(obs, h, masks, T, N)
    action_mask = corrected == 0
    action = crit[0](out.masked_fill_(action_mask, 0), corrected)
    keep = stop_lab != -1
    st = crit[1](torch.masked_select(stop, keep), torch.masked_select(stop_lab, keep))
    loss = [action.item(), st.item()]
    if prog is not None:
        per_row = nn.functional.mse_loss(prog.squeeze(1), progress, reduction="none")
        loss.append(torch.masked_select(per_row, ~action_mask[:, 0]).mean().item())
    return loss, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--shapes", default="16x4,8x8")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    max_rows = max(T * N for T, N in shapes)
    crit = (nn.MSELoss(), nn.BCEWithLogitsLoss())
    lines = []
    for kind in ("cma", "s2s"):
        if kind == "cma":
            cfg = CMAConfig().validate()                              # 256 x 256 RGB-D, L = 80 (paper_configs/cma_robo.yaml)
            eng = CMAEngine(cfg, synth.make_cma_weights(cfg, 0), max_batch=max_rows, precision="fp16")
            make = synth.make_cma_observations
        else:
            cfg = S2SConfig(progress_monitor=True).validate()         # paper_configs/seq2seq_robo_pm.yaml
            eng = S2SEngine(cfg, synth.make_s2s_weights(cfg, 0), max_batch=max_rows, precision="fp16")
            make = synth.make_s2s_observations
        R = eng.num_recurrent_layers
        for T, N in shapes:
            rows = T * N
            obs = make(cfg, rows, step=0, seed=0, rgb_uint8=True)
            obs["instruction"] = np.tile(make(cfg, N, step=0, seed=0)["instruction"], (T, 1))
            obs = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in obs.items()}
            rng = np.random.RandomState(0)
            corrected = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
            corrected[rng.uniform(size=(rows, 2)) < 0.1] = 0
            corrected = torch.from_numpy(corrected).cuda()
            stop_lab = torch.from_numpy(rng.randint(-1, 2, (rows, 1)).astype(np.float32)).cuda()
            progress = torch.from_numpy(rng.uniform(0, 1, rows).astype(np.float32)).cuda()
            vobs = dict(obs, progress=progress) if kind == "s2s" else obs
            masks = torch.ones(rows, device="cuda")
            masks[:N] = 0
            table = torch.zeros(a.chunks, 8, device="cuda")

            def run_parent():
                h = torch.zeros(R, N, cfg.hidden, device="cuda")
                for _ in range(a.chunks):
                    _, h = parent_chunk(kind, eng, obs, corrected, stop_lab, progress, h, masks, T, N, crit)

            def run_read_each():
                h = torch.zeros(R, N, cfg.hidden, device="cuda")
                for i in range(a.chunks):
                    r, h = eng.val_step(vobs, corrected, stop_lab, h, masks, result=table[i])
                    r.cpu()

            def run_epoch():
                h = torch.zeros(R, N, cfg.hidden, device="cuda")
                for i in range(a.chunks):
                    _, h = eng.val_step(vobs, corrected, stop_lab, h, masks, result=table[i])
                table.cpu()

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            routes = {"parent": run_parent, "read_each": run_read_each, "epoch": run_epoch}
            for fn in routes.values():                                # warm-up: kernel attribute setup, allocator
                fn()
            # same numbers from both routes on the shapes that are timed: faster and different is not faster
            ref, _ = parent_chunk(kind, eng, obs, corrected, stop_lab, progress, torch.zeros(R, N, cfg.hidden, device="cuda"), masks, T, N, crit)
            got = eng.val_step(vobs, corrected, stop_lab, torch.zeros(R, N, cfg.hidden, device="cuda"), masks)[0].cpu().numpy()
            agree = float(np.max(np.abs(got[:len(ref)] - np.asarray(ref)) / np.abs(np.asarray(ref))))
            ms = {k: [] for k in routes}
            for r in range(a.rounds):
                order = list(routes) if r % 2 == 0 else list(routes)[::-1]
                for k in order:
                    ms[k].append(timed(routes[k]))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rec = {"kind": kind, "T": T, "N": N, "rows": rows, "chunks": a.chunks, "rounds": a.rounds, "loss_max_rel_diff_vs_parent": agree,
                   "workspace_bytes": eng.query(4)}
            for k in routes:
                rec[k + "_ms_per_chunk"] = round(med[k] / a.chunks, 4)
                rec[k + "_epoch_ms"] = round(med[k], 3)
                rec[k + "_epoch_ms_min_max"] = [round(min(ms[k]), 3), round(max(ms[k]), 3)]
            rec["parent_over_read_each"] = round(med["parent"] / med["read_each"], 4)
            rec["parent_over_epoch"] = round(med["parent"] / med["epoch"], 4)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        eng.close()
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"| kind | T x N | parent ms/chunk (min-max) | val_step + read ms/chunk (min-max) | val_step, one read per epoch ms/chunk (min-max) | "
                    f"epoch of {a.chunks} chunks: parent / one read, ms | parent / epoch |\n|---|---|---|---|---|---|---|\n")
            for r in lines:
                c = r["chunks"]

                def cell(k):
                    lo, hi = r[k + "_epoch_ms_min_max"]
                    return f"{r[k + '_ms_per_chunk']:.3f} ({lo / c:.3f}-{hi / c:.3f})"
                f.write(f"| {r['kind']} | {r['T']} x {r['N']} | {cell('parent')} | {cell('read_each')} | {cell('epoch')} | "
                        f"{r['parent_epoch_ms']:.1f} / {r['epoch_epoch_ms']:.1f} | {r['parent_over_epoch']:.3f} |\n")


if __name__ == "__main__":
    main()
