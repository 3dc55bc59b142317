"""The precomputed instruction stream (hcm_instr_features / hcm_encode_instruction, observations["instruction_features"]): what it saves.
fp16, 256 x 256 RGB-D, L = 80, one engine (max_batch 64, graph mode for act()).

    val     hcm_val_step from cached trunk features at (T, N) = (16, 4) and (8, 8): with the chunk's T*N rows of ids (BERT on T*N rows: the code as
            it was, the baseline) against the (N, L, 768) stream encoded once
    encode  encode_instruction at 4, 8 and 64 rows
    act     act() at B = 64 and B = 1: with ids, with the stream, with reuse_instruction=True
    kernel  the ingest / export kernels alone at (64, 80, 768), hipEvent time, against the 6.1 TB/s streaming ceiling of profiles/r6_request_rate.md
            (over rotating buffers larger than the last-level cache, and over one cache-resident pair)

Each variant runs `iters` calls in a group that ends in one device synchronise; the variants alternate inside a round, at least five rounds after
a warm-up; the whole measurement runs twice; median and range per variant and run, host clock, profiler off.  One JSON line per configuration, and
the tables as markdown to --out (whatever stands below the line `<!-- notes -->` in an existing file is kept).

    python tools/bench_instr_features.py [--rounds 5] [--iters 10] [--out profiles/instruction_features.md]
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
from robo_vln_amd import _lib, synth                        # noqa: E402
from robo_vln_amd.config import HCMConfig                   # noqa: E402
from robo_vln_amd.policy import HCMEngine                   # noqa: E402

KEY = "instruction_features"
CEILING_GBS = 6100.0
NOTES = "<!-- notes -->"


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def interleave(variants, a):
    """variants: name -> (prime, fn); prime() runs outside the clock in front of every group (None: nothing)"""
    def timed(prime, fn):
        if prime is not None:
            prime()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.iters

    for prime, fn in variants.values():                            # warm-up: kernel attribute setup, allocator, graph capture
        if prime is not None:
            prime()
        for _ in range(4):
            fn()
    runs = []
    for _ in range(2):
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, (prime, fn) in variants.items():
                times[k].append(timed(prime, fn))
        runs.append({k: stats(v) for k, v in times.items()})
    return runs


def collate_ids(obs, T, N):
    """the trainer's collate: environment n's instruction at every one of the chunk's T steps (row t*N + n)"""
    return obs["instruction"][:N].repeat(T, 1).contiguous()


def bench_val(eng, cfg, T, N, a):
    rows = T * N
    obs = {k: torch.from_numpy(v).cuda() for k, v in synth.make_observations(cfg, rows, step=0, seed=0, rgb_uint8=True).items()}
    obs["instruction"] = collate_ids(obs, T, N)
    rng = np.random.RandomState(0)
    obs["vln_oracle_action_sensor"] = torch.from_numpy(rng.randint(0, 5, rows)).cuda()
    corrected = torch.from_numpy(rng.uniform(-1, 1, (rows, 2)).astype(np.float32)).cuda()
    stop_lab = torch.from_numpy(rng.randint(-1, 2, (rows, 1)).astype(np.float32)).cuda()
    masks = torch.ones(rows, device="cuda")
    masks[:N] = 0
    fobs = {k: v for k, v in obs.items() if k not in ("rgb", "depth")}
    fobs.update(eng.encode_features(obs))
    sobs = {k: v for k, v in fobs.items() if k != "instruction"}
    sobs[KEY] = eng.encode_instruction(obs["instruction"][:N])      # (N, L, 768), once
    h = torch.zeros(eng.num_recurrent_layers, N, cfg.hidden, device="cuda")
    res = {k: torch.zeros(8, device="cuda") for k in ("ids", "stream")}

    def run(o, k):
        return lambda: eng.val_step(o, corrected, stop_lab, h, h, masks, result=res[k])

    runs = interleave({"ids": (None, run(fobs, "ids")), "stream": (None, run(sobs, "stream"))}, a)
    torch.cuda.synchronize()
    out = {"what": "val_step", "T": T, "N": N, "rows": rows, "L": cfg.instr_len, "iters": a.iters, "rounds": a.rounds,
           "result_max_abs_difference": float(f"{float((res['ids'][:3] - res['stream'][:3]).abs().max()):.3e}"),
           "counts_equal": bool(torch.equal(res["ids"][3:], res["stream"][3:])), "runs": runs}
    print(json.dumps(out), flush=True)
    return out


def bench_encode(eng, cfg, rows, a):
    ids = torch.from_numpy(synth.make_observations(cfg, rows, step=0, seed=0)["instruction"]).cuda()
    runs = interleave({"encode": (None, lambda: eng.encode_instruction(ids))}, a)
    out = {"what": "encode_instruction", "rows": rows, "L": cfg.instr_len, "iters": a.iters, "rounds": a.rounds, "runs": runs}
    print(json.dumps(out), flush=True)
    return out


def bench_act(eng, cfg, B, a):
    obs = {k: torch.from_numpy(v).cuda() for k, v in synth.make_observations(cfg, B, step=0, seed=0, rgb_uint8=True).items()}
    sobs = {k: v for k, v in obs.items() if k != "instruction"}
    sobs[KEY] = eng.encode_instruction(obs["instruction"])
    hh = torch.zeros(eng.num_recurrent_layers, B, cfg.hidden, device="cuda")
    m = torch.ones(B, device="cuda")
    recs = {}

    def step(o, k, **kw):
        def f():
            recs[k] = eng.act(o, hh, hh, m, **kw)[0]
        return f

    variants = {"ids": (None, step(obs, "ids")), "stream": (None, step(sobs, "stream")),
                "reuse": (step(obs, "reuse"), step(obs, "reuse", reuse_instruction=True))}      # (an ordinary step in front: the cache it reuses)
    runs = interleave(variants, a)
    torch.cuda.synchronize()
    out = {"what": "act", "B": B, "L": cfg.instr_len, "iters": a.iters, "rounds": a.rounds,
           "stream_equals_ids": bool(torch.equal(recs["ids"], recs["stream"])), "reuse_equals_ids": bool(torch.equal(recs["ids"], recs["reuse"])),
           "graph_launches": eng.query(_lib.HCM_GRAPH_LAUNCHES), "runs": runs}
    print(json.dumps(out), flush=True)
    return out


def bench_kernels(rows, L, D, a):
    """hot: one buffer pair, back to back (23.6 MB: it stays in the 256 MB last-level cache between launches); rotating: 16 pairs in turn, 377 MB,
    so that every launch streams from and to HBM"""
    l = _lib.lib()
    pairs = [(torch.rand(rows, L, D, device="cuda"), torch.zeros(rows, L, D, device="cuda", dtype=torch.float16)) for _ in range(16)]
    moved = rows * L * D * (4 + 2)
    calls = {"ingest": lambda x, y: l.hcm_op_instr_feat_ingest(x.data_ptr(), y.data_ptr(), _lib.HCM_F16, None, rows, rows, L, D, None),
             "export": lambda x, y: l.hcm_op_instr_feat_export(y.data_ptr(), _lib.HCM_F16, x.data_ptr(), None, rows, L, D, None)}
    out = []
    for name, call in calls.items():
        for mode, n_pairs in (("rotating", len(pairs)), ("hot", 1)):
            assert call(*pairs[0]) == 0
            per = []
            for _ in range(2 * a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(48):
                    call(*pairs[i % n_pairs])
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) / 48)
            us = float(np.median(per)) * 1e3
            r = {"what": "kernel", "kernel": "instr_feat_" + name, "buffers": mode, "shape": [rows, L, D], "bytes": moved, "median_us": round(us, 2),
                 "min_us": round(min(per) * 1e3, 2), "max_us": round(max(per) * 1e3, 2), "GB_per_s": round(moved / us / 1e3, 1),
                 "of_ceiling": round(moved / us / 1e3 / CEILING_GBS, 3)}
            print(json.dumps(r), flush=True)
            out.append(r)
    return out


def cell(r):
    return f"{r['median_ms']:.3f} ({r['min_ms']:.3f}-{r['max_ms']:.3f})"


def markdown(device, vals, encs, acts, kernels, a, notes):
    o = ["# The precomputed instruction stream: what it saves", "",
         f"`tools/bench_instr_features.py --rounds {a.rounds} --iters {a.iters}` on {device}; fp16, 256 x 256 RGB-D, L = 80; milliseconds per call, median",
         "(min-max) over the interleaved rounds, two runs in one process; host clock around groups that end in a device synchronise.", "",
         "## `val_step` from cached trunk features: T*N rows of ids against the (N, L, 768) stream", "",
         "`ids`: BERT runs on the chunk's T*N rows (the code as it was: the baseline).  `stream`: the stream of the N trajectories, encoded once",
         "outside the clock, handed over as `instruction_features`; the call runs one conversion launch in BERT's place.", "",
         "| (T, N) | arm | run 1 | run 2 | ids / stream (medians, run 1; run 2) | ranges disjoint in both runs | largest loss difference |", "|---|---|---|---|---|---|---|"]
    for s in vals:
        ratio = "; ".join(f"{r['ids']['median_ms'] / r['stream']['median_ms']:.2f}" for r in s["runs"])
        below = all(r["stream"]["max_ms"] < r["ids"]["min_ms"] for r in s["runs"])
        for k in ("ids", "stream"):
            first = k == "ids"
            o.append(f"| ({s['T']}, {s['N']}) | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if first else ''} | "
                     f"{('yes' if below else 'NO') if first else ''} | {(format(s['result_max_abs_difference'], '.1e')) if first else ''} |")
    o += ["", "The stream of a validation epoch is encoded at N rows and the baseline runs BERT at T*N: where BERT's GEMM launch forms differ between the two row",
          "counts the losses agree to fp16 round-off (last column), not bit for bit (include/hcm.h, hcm_instr_features).", "",
          "## `encode_instruction`", "", "| rows | run 1 | run 2 |", "|---|---|---|"]
    for s in encs:
        o.append(f"| {s['rows']} | {cell(s['runs'][0]['encode'])} | {cell(s['runs'][1]['encode'])} |")
    o += ["", "## `act()` (graph mode)", "",
          "`ids`: the measured configuration.  `stream`: `instruction_features` at a fixed address.  `reuse`: `reuse_instruction=True`, which also skips the",
          "instruction side of the cross-modal block (it lives in the workspace and dies with any other call; the stream is the caller's tensor).", "",
          "| B | arm | run 1 | run 2 | ids / arm (medians, run 1; run 2) | record equals the ids arm's |", "|---|---|---|---|---|---|"]
    for s in acts:
        for k in ("ids", "stream", "reuse"):
            ratio = "; ".join(f"{r['ids']['median_ms'] / r[k]['median_ms']:.2f}" for r in s["runs"])
            eq = {"ids": "", "stream": str(s["stream_equals_ids"]), "reuse": str(s["reuse_equals_ids"])}[k]
            o.append(f"| {s['B']} | {k} | {cell(s['runs'][0][k])} | {cell(s['runs'][1][k])} | {ratio if k != 'ids' else ''} | {eq} |")
    o += ["", "## The two kernels alone, (64, 80, 768) in fp16 storage", "",
          f"hipEvent time over 48 back-to-back launches; bytes = f32 side + fp16 side; HBM streaming ceiling {CEILING_GBS / 1000:.1f} TB/s (profiles/r6_request_rate.md).",
          "`rotating`: 16 buffer pairs in turn (377 MB, more than the 256 MB last-level cache): every launch streams from and to HBM, the row to hold against",
          "the ceiling.  `hot`: one 23.6 MB pair again and again, which stays in that cache between launches -- cache bandwidth, it can exceed the ceiling.", "",
          "| kernel | buffers | MB moved | median us (min-max) | GB/s | of the HBM ceiling |", "|---|---|---|---|---|---|"]
    for r in kernels:
        o.append(f"| {r['kernel']} | {r['buffers']} | {r['bytes'] / 1e6:.1f} | {r['median_us']:.2f} ({r['min_us']:.2f}-{r['max_us']:.2f}) | {r['GB_per_s']:.0f} | "
                 f"{100 * r['of_ceiling']:.0f} % |")
    return "\n".join(o) + "\n\n" + NOTES + "\n" + notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instruction_features.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instr_features.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("at least five interleaved rounds")
    device = torch.cuda.get_device_name(0)
    print(json.dumps({"device": device}), flush=True)
    cfg = HCMConfig().validate()                                  # 256 x 256 RGB-D, L = 80
    eng = HCMEngine(cfg, *synth.make_weights(cfg, seed=0), max_batch=64, precision="fp16", graph=True, guard_every=0)
    vals = [bench_val(eng, cfg, T, N, a) for T, N in ((16, 4), (8, 8))]
    encs = [bench_encode(eng, cfg, rows, a) for rows in (4, 8, 64)]
    acts = [bench_act(eng, cfg, B, a) for B in (64, 1)]
    eng.close()
    kernels = bench_kernels(64, 80, 768, a)
    notes = ""
    if os.path.exists(a.out):
        old = open(a.out).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1].lstrip("\n")
    text = markdown(device, vals, encs, acts, kernels, a, notes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
