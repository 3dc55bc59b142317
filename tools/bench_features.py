"""Precomputed trunk features: what a validation chunk costs from frames, from cached features on the device, and what encode_features alone
costs -- hcm_val_step on the HCM pair, hcm_flat_val_step on CMANet and Seq2SeqNet.  fp16, 256 x 256 RGB-D, L = 80.  Each variant runs K chunks with
ONE synchronise at the end; the variants are interleaved in one process over several rounds after a warm-up; median and range per variant, one
JSON line per (engine, shape).  Then the two kernels of csrc/features.hip alone (hcm_op_feat_ingest / hcm_op_feat_export) on the step's tensors,
against the bytes they move.

    python tools/bench_features.py [--rounds 5] [--chunks 10] [--shapes 16x4,8x8]
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
from robo_vln_amd.cma import CMAEngine                      # noqa: E402
from robo_vln_amd.config import CMAConfig, HCMConfig, S2SConfig   # noqa: E402
from robo_vln_amd.policy import HCMEngine                   # noqa: E402
from robo_vln_amd.seq2seq import S2SEngine                  # noqa: E402


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def bench_engine(kind, eng, cfg, shapes, a):
    make = {"hcm": synth.make_observations, "cma": synth.make_cma_observations, "s2s": synth.make_s2s_observations}[kind]
    R = eng.num_recurrent_layers
    for T, N in shapes:
        rows = T * N
        obs = {k: torch.from_numpy(v).cuda() for k, v in make(cfg, rows, step=0, seed=0, rgb_uint8=True).items()}
        rng = np.random.RandomState(0)
        if kind == "hcm":
            obs["vln_oracle_action_sensor"] = torch.from_numpy(rng.randint(0, 5, rows)).cuda()
        corrected = torch.from_numpy(rng.uniform(-1, 1, (rows, 2)).astype(np.float32)).cuda()
        stop_lab = torch.from_numpy(rng.randint(-1, 2, (rows, 1)).astype(np.float32)).cuda()
        masks = torch.ones(rows, device="cuda")
        masks[:N] = 0
        feats = eng.encode_features(obs)
        fobs = {k: v for k, v in obs.items() if k not in ("rgb", "depth")}
        fobs.update(feats)
        table = torch.zeros(a.chunks, 8, device="cuda")

        def run_val(o):
            h = torch.zeros(R, N, cfg.hidden, device="cuda")
            hs = (h, torch.zeros_like(h)) if kind == "hcm" else (h,)
            for i in range(a.chunks):
                out = eng.val_step(o, corrected, stop_lab, *hs, masks, result=table[i])
                hs = out[1:]

        def run_encode():
            for _ in range(a.chunks):
                eng.encode_features(obs)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.chunks

        variants = {"frames": lambda: run_val(obs), "features": lambda: run_val(fobs), "encode": run_encode}
        for fn in variants.values():                               # warm-up: kernel attribute setup, allocator
            fn()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        fr, fe = float(np.median(times["frames"])), float(np.median(times["features"]))
        print(json.dumps({"engine": kind, "T": T, "N": N, "rows": rows, "chunks": a.chunks, "rounds": a.rounds,
                          "val_step_from_frames": stats(times["frames"]), "val_step_from_features": stats(times["features"]),
                          "encode_features": stats(times["encode"]), "ratio_frames_over_features": round(fr / fe, 3)}), flush=True)


def bench_kernels(rows, a):
    """ingest / export of the step's three tensors in fp16 storage, hipEvent time over `reps` back-to-back launches"""
    l = _lib.lib()
    for what, C_, S, ld in (("rgb tokens (2048,4,4)", 2048, 16, 2112), ("rgb pooled (2048,1,1)", 2048, 1, 2048), ("depth (128,4,4)", 128, 16, 192)):
        x = torch.rand(rows, C_, S, device="cuda")
        y = torch.zeros(rows, S, ld, device="cuda", dtype=torch.float16)
        moved = rows * C_ * S * (4 + 2)
        for name, call in (("ingest", lambda: l.hcm_op_feat_ingest(x.data_ptr(), y.data_ptr(), _lib.HCM_F16, rows, C_, S, ld, 1.0, None)),
                           ("export", lambda: l.hcm_op_feat_export(y.data_ptr(), _lib.HCM_F16, x.data_ptr(), rows, C_, S, ld, 1.0, None))):
            assert call() == 0
            per = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    call()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) / 50)
            us = float(np.median(per)) * 1e3
            print(json.dumps({"kernel": "feat_" + name, "tensor": what, "rows": rows, "bytes": moved, "median_us": round(us, 2),
                              "min_us": round(min(per) * 1e3, 2), "max_us": round(max(per) * 1e3, 2), "GB_per_s": round(moved / us / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=10)
    ap.add_argument("--shapes", default="16x4,8x8")
    ap.add_argument("--engines", default="hcm,cma,s2s")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    mb = max(T * N for T, N in shapes)
    for kind in a.engines.split(","):
        if kind == "hcm":
            cfg = HCMConfig().validate()                          # 256 x 256 RGB-D, L = 80
            eng = HCMEngine(cfg, *synth.make_weights(cfg, seed=0), max_batch=mb, precision="fp16")
        elif kind == "cma":
            cfg = CMAConfig().validate()
            eng = CMAEngine(cfg, synth.make_cma_weights(cfg, seed=0), max_batch=mb, precision="fp16")
        else:
            cfg = S2SConfig().validate()
            eng = S2SEngine(cfg, synth.make_s2s_weights(cfg, seed=0), max_batch=mb, precision="fp16")
        bench_engine(kind, eng, cfg, shapes, a)
        eng.close()
    bench_kernels(mb, a)


if __name__ == "__main__":
    main()
