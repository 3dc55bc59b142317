"""CMANet on a truncated-BPTT chunk at the BASELINE frame size (T*N = 64 frames, 256 x 256 RGB-D uint8 / f32, L = 80 with lengths drawn over
20..80, "fp16"): hcm_cma_forward_seq against T single-step hcm_cma_forward calls with the state carried (what the library offered before the
sequence call; timed eagerly and through the engine's hipGraph replay), alternating in one process.  One JSON line.

    python tools/bench_cma_seq.py [--T 16 --N 4] [--rnn LSTM|GRU] [--reps 5] [--calls 10]
    HCM_DEV_LIB=1 python tools/bench_cma_seq.py --seq-only                        # development build: the one-launch-per-step scan ...
    HCM_DEV_LIB=1 HCM_NO_STATE_SCAN=1 python tools/bench_cma_seq.py --seq-only    # ... against rnn_scan's per-step launches (run both, alternating)
"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import hcm_pkg; hcm_pkg.load()
from robo_vln_amd.config import CMAConfig
from robo_vln_amd import synth
from robo_vln_amd.cma import CMAEngine


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


T, N, L = arg("--T", 16), arg("--N", 4), 80
REPS, CALLS, RNN = arg("--reps", 5), arg("--calls", 10), arg("--rnn", "LSTM")
B = T * N
cfg = CMAConfig(instr_len=L, rnn_type=RNN).validate()
sd = synth.make_cma_weights(cfg, 0)
obs = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.make_cma_observations(cfg, B, rgb_uint8=True).items()}
lens = synth.randint("bench/cma_seq_len", N, 20, L + 1)
ids = synth.randint("bench/cma_seq_ids", N * L, 1, cfg.vocab_size).reshape(N, L)
for n in range(N):
    ids[n, lens[n]:] = 0
obs["instruction"] = torch.from_numpy(np.tile(ids, (T, 1))).cuda()
masks = torch.ones(T, N, device="cuda")
masks[0] = 0
masks[T // 2, 0] = 0
masks = masks.reshape(-1).contiguous()
h0 = torch.zeros(cfg.num_recurrent_layers, N, cfg.hidden, device="cuda")
steps = [({k: v[t * N:(t + 1) * N].contiguous() for k, v in obs.items()}, masks[t * N:(t + 1) * N].contiguous()) for t in range(T)]

seq_eng = CMAEngine(cfg, sd, max_batch=B, precision="fp16")
paths = {"seq": lambda: seq_eng.forward_seq(obs, h0, masks, T, N)}
if "--seq-only" not in sys.argv:
    step_eng = CMAEngine(cfg, sd, max_batch=N, precision="fp16")
    graph_eng = CMAEngine(cfg, sd, max_batch=N, precision="fp16", graph=True)

    def loop(eng):
        def run():
            h = h0
            outs = []
            for o, m in steps:
                out, stop, h = eng.forward(o, h, m)
                outs.append(out.clone())          # (the graph engine's outputs alias its static buffers)
            return torch.cat(outs), h
        return run
    paths["steps_eager"] = loop(step_eng)
    paths["steps_graph"] = loop(graph_eng)

for fn in paths.values():                         # warm-up: every shape, the graph capture included
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in paths}
for _ in range(REPS):                             # alternating: A B C A B C ...
    for k, fn in paths.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize(); ms[k].append((time.perf_counter() - t0) / CALLS * 1e3)
res = {"bench": "cma_seq", "T": T, "N": N, "L": L, "frames": 256, "precision": "fp16", "rnn_type": RNN, "reps": REPS, "calls": CALLS,
       "dev_lib": os.environ.get("HCM_DEV_LIB", "0"), "no_state_scan": os.environ.get("HCM_NO_STATE_SCAN", "0"),
       "workspace_bytes": seq_eng.query(4)}          # HCM_WORKSPACE_BYTES
for k, v in ms.items():
    res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
if "steps_eager" in ms:
    res["speedup_vs_steps_eager"] = round(res["steps_eager"]["median_ms"] / res["seq"]["median_ms"], 3)
    res["speedup_vs_steps_graph"] = round(res["steps_graph"]["median_ms"] / res["seq"]["median_ms"], 3)
    a = paths["seq"]()
    b = paths["steps_eager"]()
    torch.cuda.synchronize()
    res["seq_vs_steps_max_abs"] = float((a[0] - b[0]).abs().max())
print(json.dumps(res))
