"""The driver's multi-GPU command line -- `python bench.py --gpus N --steps K --warmup W` -- must launch itself: it re-executes under
torch.distributed.run (one rank per GPU on 127.0.0.1), and rank 0 prints ONE JSON line carrying the weak AND the strong leg, the ranks seen
by the rank-tagged all-gather and the host enqueue time.  Run here at world size 2 on CPU with the stand-in engine (HCM_BENCH_STUB=1: gloo,
no GPU, no libhcm) -- the launch plumbing, rendezvous, legs and the output contract are the product code's own."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.update({"HCM_BENCH_STUB": "1", "HCM_BENCH_STUB_BATCH": "2", "OMP_NUM_THREADS": "2"})
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    if env_extra:
        env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    return p


def test_gpus_2_spawns_its_own_ranks_and_prints_one_line():
    p = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--prewarm", "1", "--full"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["ranks_seen"] == [0, 1]
    assert out["scaling"] == "weak" and out["config"]["global_batch"] == 2 * out["config"]["per_gpu_batch"]
    assert out["weak"]["value"] == out["value"] and out["weak"]["per_gpu_batch"] == out["config"]["per_gpu_batch"]
    st = out["strong"]
    assert st["total_batch"] == 2 * st["per_gpu_batch"] and st["value"] > 0 and st["ranks_seen"] == [0, 1]
    assert out["host_us_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert "STUB" in out["metric"]           # a stub line can never be mistaken for a measurement


def test_gpus_1_stays_in_process():
    p = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--prewarm", "1"])
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.strip()][0])
    assert out["n_gpus"] == 1 and "strong" not in out and "ranks_seen" not in out


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full only the K timed steps run (no extra legs, probes or baselines in the line); --dump-outputs writes what the last
    timed step returned as float32 .npy files, the same on every run with the same arguments."""
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        p = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "1", "--dump-outputs", str(d)])
        assert p.returncode == 0, p.stderr[-3000:]
        out = json.loads([l for l in p.stdout.splitlines() if l.strip()][0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
        assert not {"sustained", "strong", "cpu_baseline", "bf16_mode", "h2d", "single_env_latency", "gather_world1", "host_8proc", "configs"} & set(out)
        assert sorted(os.listdir(d)) == ["hidden_hi.npy", "hidden_lo.npy", "records.npy"]
        dumps.append({f: np.load(d / f) for f in os.listdir(d)})
    B = 2
    assert dumps[0]["records.npy"].shape == (B, 7) and dumps[0]["hidden_hi.npy"].shape[1:] == (B, 512)
    for f, a in dumps[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, dumps[1][f]), f


def test_world_size_mismatch_is_refused():
    p = _run(["--gpus", "4", "--steps", "1", "--warmup", "0"], {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533"})
    assert p.returncode != 0 and "--gpus 4" in (p.stderr + p.stdout)
