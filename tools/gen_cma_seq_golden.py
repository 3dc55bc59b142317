"""Golden vectors for CMANet's sequence forward: builds the reference's own `CMANet` (models/cma.py) through oracle/ref_shims.py, loads the
synthetic weights with strict=True and calls it ONCE on T*N frames with an (R,N,H) hidden state, so that RNNStateEncoder.forward takes
seq_forward (state_encoder.py:83-133) for both state encoders, as the flat trainer's training and validation steps do
(robo_vln_trainer.py:516-518, :553-555).  Writes tests/golden/cma_seq_*.npz: outputs, final hidden, h0 and meta only -- the inputs are
rebuilt from the seed (tests/cma_seq_cases.py).  Needs the reference checkout; runs on the build machine, never on the GPU box.

    python tools/gen_cma_seq_golden.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import hcm_oracle, ref_shims  # noqa: E402
from robo_vln_amd import synth            # noqa: E402
from tests import cma_seq_cases as cs     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def run_case(name):
    cfg, T, N = cs.seq_case(name)
    sd = synth.make_cma_weights(cfg, cs.SEED)
    net = ref_shims.build_cma(cfg, sd)
    obs_np = cs.seq_observations(cfg, T, N)
    lens = (obs_np["instruction"][:N] != 0).sum(1)
    assert len(set(lens.tolist())) > 1, "the envs' instructions must differ in token count"
    obs = {k: torch.from_numpy(np.asarray(v).astype(np.float32)) for k, v in obs_np.items()}
    m = cs.seq_masks(T, N)
    masks = torch.from_numpy(m).view(-1, 1).expand(-1, 2).contiguous()      # cma.py:219 reads column 0
    h0 = cs.seq_h0(cfg, N)
    with torch.no_grad():
        out, stop, hid = net((obs, h0.clone(), torch.zeros(T * N, 1, dtype=torch.long), masks))
    gold = {"out": out.numpy(), "stop": stop.numpy(), "hidden": hid.numpy(), "h0": h0.numpy(),
            "meta": np.array(repr(dict(case=name, T=T, N=N, config=repr(cfg.to_dict()),
                                       note="reference CMANet.forward with T*N frames and an (R,N,H) hidden state -> seq_forward in both state encoders")))}
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **gold)
    o2, s2, h2 = hcm_oracle.CMAOracle(cfg, sd).forward(obs_np, h0.clone(), m)
    worst = max(np.abs(o2.numpy() - gold["out"]).max(), np.abs(s2.numpy() - gold["stop"]).max(), np.abs(h2.numpy() - gold["hidden"]).max())
    print(f"[{name}] CMANet seq_forward T={T} N={N}: restatement-vs-reference worst max-abs {worst:.3e}")
    return worst


if __name__ == "__main__":
    names = sys.argv[1:] or list(cs.CMA_SEQ_CASES)
    bad = 0
    for n in names:
        bad |= (run_case(n) > 1e-5)
    sys.exit(1 if bad else 0)
