"""Golden vectors for the teacher-forced validation step (hcm_val_step): tests/golden/val_*.npz, in two layers, named in each fixture's meta.

  layer 1 -- `logits`, `vel`, `stop`, `hi_hidden`, `lo_hidden`: the reference's own Seq2Seq_HighLevel_CMA / Seq2Seq_LowLevel, imported through
             oracle/ref_shims.py and called on the T*N frames as oracle/gen_golden.py does for seq_T4_N2_gru, the low-level model fed the
             remapped oracle sub-task (hierarchical_trainer.py:597-599).
  layer 2 -- `result` (mixed labels) and `result_padded` (every row padded): torch's nn.CrossEntropyLoss / nn.MSELoss / nn.BCEWithLogitsLoss
             applied to the layer-1 tensors by tests/val_ref.criteria.  The trainer module cannot be imported (habitat_sim, lmdb, tensorflow
             at import time), so `_update_agent_val` itself is not called.

Needs the reference checkout; runs on the build machine, never on the GPU box.

    python tools/gen_val_golden.py [case ...]
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims   # noqa: E402
from tests import val_ref      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed member timestamp, so that a re-run gives the same file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def run_case(name):
    cfg, T, N = val_ref.case(name)
    hi_sd, lo_sd = val_ref.weights(cfg)
    hi, lo = ref_shims.build_models(cfg, hi_sd, lo_sd)
    obs_np, corrected, oracle_stop, m = val_ref.observations(cfg, T, N)
    oracle = obs_np.pop("vln_oracle_action_sensor")
    obs = {k: torch.from_numpy(v.astype(np.float32)) for k, v in obs_np.items()}
    masks = torch.from_numpy(m).view(-1, 1).expand(-1, 2).contiguous()
    h0 = val_ref.h0(cfg, N)
    prev = torch.zeros(T * N, 2, dtype=torch.long)
    subtask = val_ref.remap(oracle, cfg.num_sub_tasks)
    with torch.no_grad():
        logits, hi_h = hi((dict(obs), h0.clone(), prev, masks))
        vel, stop, lo_h = lo((dict(obs), h0.clone(), prev, masks, subtask))
    result = val_ref.criteria(logits, vel, stop, oracle, corrected, oracle_stop, cfg.num_sub_tasks)
    o_p, c_p, s_p = val_ref.labels(T, N, "padded")
    result_padded = val_ref.criteria(logits, vel, stop, o_p, c_p, s_p, cfg.num_sub_tasks)
    gold = {"logits": logits.numpy(), "vel": vel.numpy(), "stop": stop.numpy(), "hi_hidden": hi_h.numpy(), "lo_hidden": lo_h.numpy(),
            "result": result.numpy(), "result_padded": result_padded.numpy(),
            "meta": np.array(repr(dict(case=name, T=T, N=N, config=repr(cfg.to_dict()),
                                       layer1="logits, vel, stop, hi_hidden, lo_hidden: imported reference models, T*N frames + (R,N,H) hidden "
                                              "state -> seq_forward, low-level model fed the remapped oracle sub-task",
                                       layer2="result, result_padded: torch nn.CrossEntropyLoss(ignore_index=-1) / nn.MSELoss / "
                                              "nn.BCEWithLogitsLoss applied to the layer-1 tensors by tests/val_ref.criteria")))}
    save_npz(os.path.join(OUT, name + ".npz"), **gold)     # (the initial hidden state is val_ref.h0: not stored)
    # restatement cross-check
    orc = val_ref.ValOracle(cfg, hi_sd, lo_sd)
    obs2, c2, s2, m2 = val_ref.observations(cfg, T, N)
    res2, hh2, lh2, (l2, v2, st2) = orc.val_step(obs2, c2, s2, h0.clone(), h0.clone(), m2, return_outputs=True)
    worst = max(np.abs(l2.numpy() - gold["logits"]).max(), np.abs(v2.numpy() - gold["vel"]).max(), np.abs(st2.numpy() - gold["stop"]).max(),
                np.abs(hh2.numpy() - gold["hi_hidden"]).max(), np.abs(lh2.numpy() - gold["lo_hidden"]).max())
    top2 = np.sort(gold["logits"], 1)[:, -2:]
    print(f"[{name}] T={T} N={N}: restatement-vs-reference worst max-abs {worst:.3e}; result {np.array2string(gold['result'], precision=6)}; "
          f"smallest logit gap {np.min(top2[:, 1] - top2[:, 0]):.4f}")
    return worst


if __name__ == "__main__":
    names = sys.argv[1:] or list(val_ref.VAL_GOLDEN)
    bad = 0
    for n in names:
        bad |= (run_case(n) > 1e-5)
    sys.exit(1 if bad else 0)
