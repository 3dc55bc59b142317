"""Where one hcm_val_step spends its time: wall-clock stamps of the marker kernels (`make DEV=1` library, HCM_MARKS=1; forward.cpp Fwd::mark) at the
start and end of each of the call's chains and tails, read after a run of eager calls.  rocprofv3's kernel trace serialises the streams, so this is
the in-call timeline there is.
usage: HCM_DEV_LIB=1 HCM_MARKS=1 python tools/val_marks.py [T N]     (prints a table: chain, milestone, us since the call's first stamp, segment)"""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, hcm_pkg
hcm_pkg.load()
from robo_vln_amd import synth, _lib
from robo_vln_amd.config import HCMConfig
from robo_vln_amd.policy import HCMEngine
T, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (32, 3)
rows = T * N
cfg = HCMConfig().validate()
eng = HCMEngine(cfg, *synth.make_weights(cfg, seed=0), max_batch=rows, precision="fp16")
obs = {k: torch.from_numpy(v).cuda() for k, v in synth.make_observations(cfg, rows, step=0, seed=0, rgb_uint8=True).items()}
rng = np.random.RandomState(0)
obs["vln_oracle_action_sensor"] = torch.from_numpy(rng.randint(0, 5, rows)).cuda()
corrected = torch.from_numpy(rng.uniform(-1, 1, (rows, 2)).astype(np.float32)).cuda()
stop_lab = torch.from_numpy(rng.randint(-1, 2, (rows, 1)).astype(np.float32)).cuda()
masks = torch.ones(rows, device="cuda"); masks[:N] = 0
hh = torch.zeros(cfg.num_recurrent_layers, N, cfg.hidden, device="cuda"); lh = torch.zeros_like(hh)
for _ in range(5):
    eng.val_step(obs, corrected, stop_lab, hh, lh, masks)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    eng.val_step(obs, corrected, stop_lab, hh, lh, masks)
torch.cuda.synchronize()
print(f"T {T} N {N}: {(time.perf_counter() - t0) * 100:.3f} ms per call (wall, with the marker launches)\n")
out = (C.c_uint64 * 256)()
names = C.create_string_buffer(16384)
n = _lib.lib().hcm_debug_marks(eng._h, out, names, 16384)
marks = [(nm, int(out[i])) for i, nm in enumerate(names.value.decode().split("\n")[:n]) if out[i]]
if not marks:
    sys.exit("no marks: needs HCM_DEV_LIB=1 HCM_MARKS=1")
z = min(t for _, t in marks)
print("| chain | milestone | reached at (us) | segment (us) |\n|---|---|---|---|")
chains = {}
for nm, t in marks:
    chains.setdefault(nm.split(".")[0], []).append((t, nm))
for ch, lst in chains.items():
    prev = None
    for t, nm in sorted(lst):
        us = (t - z) / 100.0
        print(f"| {ch} | {nm} | {us:8.1f} | {'' if prev is None else f'{us - prev:7.1f}'} |")
        prev = us
eng.close()
