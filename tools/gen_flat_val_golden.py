"""Golden vectors for the flat trainer's validation step (hcm_flat_val_step): tests/golden/flatval_*.npz, in two layers, named in each
fixture's meta.

  layer 1 -- `out`, `stop`, `hidden` (and `progress_hat`, `aux_reference` with the progress monitor): the reference's own CMANet / Seq2SeqNet,
             imported through oracle/ref_shims.py and called ONCE on the T*N frames with an (R,N,H) hidden state, as `_update_agent_val` calls
             it (robo_vln_trainer.py:553-555).  AuxLosses is active, so the reference model registers the progress loss itself
             (seq2seq.py:176-185) and AuxLosses.reduce(~action_mask[:,0]) reduces it (robo_vln_trainer.py:569-570).
  layer 2 -- `result` (mixed labels) and `result_padded` (every row padded): torch's nn.MSELoss / nn.BCEWithLogitsLoss and the masked mean
             applied to the layer-1 tensors by tests/flat_val_ref.criteria.  The trainer module cannot be imported (habitat_sim, lmdb,
             tensorflow at import time), so `_update_agent_val` itself is not called; its aux term is checked against the reference's own
             AuxLosses.reduce.

Needs the reference checkout; runs on the build machine, never on the GPU box.

    python tools/gen_flat_val_golden.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims                     # noqa: E402
from tests import flat_val_ref as fv             # noqa: E402
from tools.gen_s2s_golden import build_reference  # noqa: E402
from tools.gen_val_golden import save_npz        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def run_case(name):
    ref_shims.install()
    from robo_vln_baselines.common.aux_losses import AuxLosses
    kind, cfg, T, N, obs_np, corrected, oracle_stop, m, h0 = fv.inputs(name)
    sd = fv.weights(kind, cfg)
    net = ref_shims.build_cma(cfg, sd) if kind == "cma" else build_reference(cfg, sd)
    monitor = bool(getattr(cfg, "progress_monitor", False))
    hats = []
    if monitor:
        net.progress_monitor.register_forward_hook(lambda mod, i, o: hats.append(torch.tanh(o.detach()).clone()))
    obs = {k: torch.from_numpy(np.asarray(v).astype(np.float32)) for k, v in obs_np.items()}
    masks = torch.from_numpy(m).view(-1, 1).expand(-1, 2).contiguous()
    c_t = torch.from_numpy(corrected)
    c_p, s_p = fv.labels(T, N, "padded")
    AuxLosses.activate()                             # robo_vln_trainer.py:949-954: active for the whole train and val loop
    try:
        AuxLosses.clear()
        with torch.no_grad():
            out, stop, hid = net((dict(obs), h0.clone(), torch.zeros(T * N, 1, dtype=torch.long), masks))
        aux_ref = AuxLosses.reduce(~(c_t == 0)[:, 0])
        aux_ref_padded = AuxLosses.reduce(~(torch.from_numpy(c_p) == 0)[:, 0])
    finally:
        AuxLosses.deactivate()
        AuxLosses.clear()
    assert monitor == isinstance(aux_ref, torch.Tensor) and (monitor or aux_ref == 0.0) and len(hats) == int(monitor)
    hat = hats[0] if monitor else None
    prog = obs_np.get("progress")
    result = fv.criteria(out, stop, hat, corrected, oracle_stop, prog)
    result_padded = fv.criteria(out, stop, hat, c_p, s_p, prog)
    gold = {"out": out.numpy(), "stop": stop.numpy(), "hidden": hid.numpy(), "result": result.numpy(), "result_padded": result_padded.numpy(),
            "meta": np.array(repr(dict(case=name, T=T, N=N, config=repr(cfg.to_dict()),
                                       layer1="out, stop, hidden, progress_hat, aux_reference: imported reference model, T*N frames + (R,N,H) hidden "
                                              "state -> seq_forward; AuxLosses active, the model registers and AuxLosses.reduce reduces the progress loss",
                                       layer2="result, result_padded: torch nn.MSELoss / nn.BCEWithLogitsLoss / masked mean applied to the layer-1 "
                                              "tensors by tests/flat_val_ref.criteria")))}
    worst = 0.0
    if monitor:
        gold["progress_hat"] = hat.numpy()
        gold["aux_reference"] = np.array([float(aux_ref), float(aux_ref_padded)], np.float32)
        # the aux term of layer 2 is the reference's own reduction
        worst = abs(float(aux_ref) - float(result[2]))
        assert np.isnan(float(aux_ref_padded)) and np.isnan(float(result_padded[2]))
    save_npz(os.path.join(OUT, name + ".npz"), **gold)     # (inputs, labels and the initial state come from the seed: not stored)
    # restatement cross-check
    r2, h2, (o2, s2, p2) = fv.oracle(name).val_step(obs_np, corrected, oracle_stop, h0.clone(), m, return_outputs=True)
    worst = max(worst, np.abs(o2.numpy() - gold["out"]).max(), np.abs(s2.numpy() - gold["stop"]).max(), np.abs(h2.numpy() - gold["hidden"]).max(),
                np.abs(r2.numpy()[:3] - gold["result"][:3]).max())
    if monitor:
        worst = max(worst, np.abs(p2.numpy() - gold["progress_hat"]).max())
    print(f"[{name}] {kind} T={T} N={N}: restatement-vs-reference worst max-abs {worst:.3e}; result {np.array2string(gold['result'], precision=6)}; "
          f"padded {np.array2string(gold['result_padded'], precision=6)}")
    return worst


if __name__ == "__main__":
    names = sys.argv[1:] or list(fv.FLAT_VAL_GOLDEN)
    bad = 0
    for n in names:
        bad |= (run_case(n) > 1e-5)
    sys.exit(1 if bad else 0)
