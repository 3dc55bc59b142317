"""Golden vectors for the update steps (train.flat_update / train.hier_update): tests/golden/update_*.npz -- the losses, the outputs, the new
state and every parameter gradient of the reference's own models under torch autograd, in float64, and a two-step Adam trajectory.  The layers
are named in each fixture's meta.

  layer 1 -- `out/*`, `state/*`: the reference's own Seq2Seq_HighLevel_CMA / Seq2Seq_LowLevel, CMANet or Seq2SeqNet, imported through
             oracle/ref_shims.py, in float64 and eval mode (dropout is the identity; its placement is pinned by the vla_*train* goldens),
             called ONCE on the T*N rows with an (R, N, H) state as `_update_agent` calls it.  The trunks are frozen: both sides take
             observations["rgb_features"] / ["depth_features"] and the frozen BERT's output (a forward hook on the reference's embedding_layer)
             from tests/update_ref.frozen_outputs -- tests/features_ref.trunk_features and oracle/hcm_oracle.bert_encoder computed in float64 and
             rounded to 1/4096, the same bits on every machine.
  layer 2 -- `losses`, `counts`: the criterion as the trainer writes it, restated with torch's criterion classes because the trainer module
             cannot be imported (habitat_sim, lmdb, tensorflow at import time): robo_vln_trainer.py:521-533 -- masked_fill_, MSELoss,
             masked_select, BCEWithLogitsLoss, the reference's own AuxLosses.reduce(~action_mask[:, 0]) with AuxLosses active -- and
             hierarchical_trainer.py:508-511, :522-553 for the pair, the low-level model fed tests/val_ref.remap of the oracle.
  layer 3 -- `grad/*`, `nograd`, `frozen`, `buffer`: loss.backward() of layer 2.  Every parameter of the reference model has a `grad/<key>` entry
             or stands in exactly one of the string lists `nograd` (its gradient is None) and `frozen` (requires_grad false); `buffer` lists
             the state dict's other keys.  A gradient is stored whole up to `subsample` elements and as that many values at a fixed stride
             above, with [max|g|, sum|g|, elements] (`gstat/*`) and four seeded +-1 projections (`gproj/*`): tests/update_ref.encode.
             `subsample` is the largest of 1024, 512, ... that keeps the file under 300 KB.
  layer 4 -- `traj_*`, `final/*`, `fstat/*`, `fproj/*` (three fixtures): torch.optim.Adam(lr=1e-3, eps=1e-3) on the reference model, the same
             chunk twice with the state carried and detached (repackage_hidden) -- the pair's on the first two steps of its chunk
             (tests/update_ref.TRAJECTORY_T) -- : the losses of every step, the final state, and every final parameter encoded as the
             gradients are.

State encoders are GRU: the reference's in-tree RNNStateEncoder.seq_forward raises for LSTM (oracle/cases.py:96-100); the LSTM scan stays
pinned by nn.LSTM in its own tests.  No inputs are stored: they come from the seeds (tests/update_ref.inputs).

Needs the reference checkout; runs on the build machine, never on the GPU box.  Ends with the float64 CPU path of the train modules on the
same inputs and exits non-zero above 1e-9.

    python tools/gen_update_golden.py [case ...]
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims                      # noqa: E402
from tests import update_ref as ur                # noqa: E402
from tests import val_ref                         # noqa: E402
from tools.gen_s2s_golden import build_reference  # noqa: E402
from tools.gen_val_golden import save_npz         # noqa: E402

LIMIT = 300 * 1024
CHECK = 1e-9


def _d(t):
    return t.double()


def build(c):
    """{model: the imported reference model in float64 and eval mode}"""
    kind, cfg, sd = c["kind"], c["cfg"], c["sd"]
    if kind == "hier":
        hi, lo = ref_shims.build_models(cfg, sd["hi"], sd["lo"])
        nets = {"hi": hi, "lo": lo}
        stream = _d(c["obs"]["instruction_features"])
        # the frozen BERT: the stream the tests compute, not its own float64 run (the rows of the call: a trajectory may take the chunk's first steps)
        hi.embedding_layer.register_forward_hook(lambda mod, i, o: (stream[:i[0].shape[0]],))
    else:
        nets = {"net": ref_shims.build_cma(cfg, sd["net"]) if kind == "cma" else build_reference(cfg, sd["net"])}
    return {tag: net.double().eval() for tag, net in nets.items()}


def step(c, nets, state, aux_losses):
    """The forward and the criterion of one `_update_agent` on the reference models, backward included (each model's loss on its own, in the
    trainer's order) -> (losses [3], counts, outputs, new state)"""
    kind, rows = c["kind"], c["T"] * c["N"]
    masks, corrected, oracle_stop = _d(c["masks"]), c["corrected"].clone(), c["stop"].clone()
    outputs = {}
    if kind == "hier":
        sensor = c["obs"]["vln_oracle_action_sensor"].clone()
        prev = torch.zeros(rows, 2, dtype=torch.long)
        high_level_criterion = nn.CrossEntropyLoss(ignore_index=-1, reduction="mean")            # hierarchical_trainer.py:498-500
        low_level_criterion = nn.MSELoss()
        low_level_stop_criterion = nn.BCEWithLogitsLoss()
        obs = {"rgb_features": _d(c["obs"]["rgb_features"][0]), "depth_features": _d(c["obs"]["depth_features"][0]), "instruction": c["ids"].clone()}
        output, hi_state = nets["hi"]((obs, state["hi"].detach().clone(), prev, masks))          # :505-506
        outputs["logits"] = output.detach().clone()
        high_level_action_mask = sensor == 0                                                     # :508
        output = output.masked_fill_(high_level_action_mask, 0)                                  # :509
        sensor = sensor.squeeze(1).to(dtype=torch.int64)                                         # :510
        high_level_loss = high_level_criterion(output, (sensor - 1))                             # :511
        high_level_loss.backward()                                                               # :512
        valid = sensor != 0
        correct = int((torch.argmax(outputs["logits"], 1)[valid] == (sensor - 1)[valid]).sum())
        discrete_actions = val_ref.remap(sensor, c["cfg"].num_sub_tasks)                         # :522-524
        assert torch.equal(discrete_actions, (sensor - 1).masked_fill_(sensor == 0, 4))
        obs = {"rgb_features": _d(c["obs"]["rgb_features"][1]), "depth_features": _d(c["obs"]["depth_features"][1])}
        output, stop_out, lo_state = nets["lo"]((obs, state["lo"].detach().clone(), prev, masks, discrete_actions.view(-1)))     # :527-539
        outputs["vel"], outputs["stop"] = output.detach().clone(), stop_out.detach().clone()
        action_mask = corrected == 0                                                             # :543
        output = output.masked_fill_(action_mask, 0)                                             # :544
        low_level_action_loss = low_level_criterion(output, corrected.to(output.dtype))          # :545-547, in the model's precision
        mask = oracle_stop != -1                                                                 # :549
        low_level_stop_loss = low_level_stop_criterion(torch.masked_select(stop_out, mask), torch.masked_select(oracle_stop, mask).to(output.dtype))
        (low_level_action_loss + low_level_stop_loss).backward()                                 # :553-554
        losses = [high_level_loss, low_level_action_loss, low_level_stop_loss]
        counts = [correct, int(valid.sum()), 0, int(mask.sum())]
        new_state = {"hi": hi_state.detach().clone(), "lo": lo_state.detach().clone()}
    else:
        criterion, stop_criterion = nn.MSELoss(), nn.BCEWithLogitsLoss()                         # robo_vln_trainer.py:510-512
        aux_losses.clear()                                                                       # :513
        obs = {"rgb_features": _d(c["obs"]["rgb_features"]), "depth_features": _d(c["obs"]["depth_features"]), "instruction": c["ids"].clone()}
        monitor = "progress" in c["obs"]
        if monitor:
            obs["progress"] = _d(c["obs"]["progress"])
        output, stop_out, new = nets["net"]((obs, state["net"].detach().clone(), torch.zeros(rows, 1, dtype=torch.long), masks))     # :516-518
        outputs["out"], outputs["stop"] = output.detach().clone(), stop_out.detach().clone()
        action_mask = corrected == 0                                                             # :521
        output = output.masked_fill_(action_mask, 0)                                             # :522
        action_loss = criterion(output, corrected.to(output.dtype))                              # :523-525, in the model's precision
        mask = oracle_stop != -1                                                                 # :527
        stop_loss = stop_criterion(torch.masked_select(stop_out, mask), torch.masked_select(oracle_stop, mask).to(output.dtype))    # :528-530
        aux_mask = ~action_mask[:, 0]                                                            # :531
        aux_loss = aux_losses.reduce(aux_mask)                                                   # :532
        assert monitor == isinstance(aux_loss, torch.Tensor) and (monitor or aux_loss == 0.0)
        (action_loss + stop_loss + aux_loss).backward()                                          # :533-535
        losses = [action_loss, stop_loss, aux_loss]
        counts = [int(mask.sum()), int(aux_mask.sum()) if monitor else 0]
        new_state = {"net": new.detach().clone()}
    return np.array([float(x.detach() if torch.is_tensor(x) else x) for x in losses], np.float64), np.array(counts, np.float64), outputs, new_state


def zero_grad(nets):
    for net in nets.values():
        for p in net.parameters():
            p.grad = None


def gold_of(name, c, nets, aux_losses, sub):
    kind, trajectory = c["kind"], ur.case(name)[4]
    gold = {"subsample": np.array(sub, np.int64)}
    state0 = {tag: _d(c["h0"]) for tag in nets}
    zero_grad(nets)
    gold["losses"], gold["counts"], outputs, state = step(c, nets, state0, aux_losses)
    for k, t in outputs.items():
        gold["out/" + k] = t.numpy()
    for tag, t in state.items():
        gold["state/" + tag] = t.numpy()
    lists = {"nograd": [], "frozen": [], "buffer": []}
    for tag, net in nets.items():
        params = dict(net.named_parameters())
        for k in net.state_dict():
            key = f"{tag}/{k}"
            p = params.get(k)
            if p is None:
                lists["buffer"].append(key)
            elif not p.requires_grad:
                lists["frozen"].append(key)
            elif p.grad is None:
                lists["nograd"].append(key)
            else:
                gold["grad/" + key], gold["gstat/" + key], gold["gproj/" + key] = ur.encode(key, p.grad.numpy(), sub)
    for k, v in lists.items():
        gold[k] = np.array(v, dtype=np.str_)
    if trajectory:
        before = {tag: {k: v.detach().clone() for k, v in net.state_dict().items()} for tag, net in nets.items()}
        opts = {tag: torch.optim.Adam(net.parameters(), **ur.ADAM) for tag, net in nets.items()}
        state, losses, counts, ct = state0, [], [], ur.trajectory_inputs(name)
        for _ in range(ur.STEPS):
            zero_grad(nets)                                   # optimizer.zero_grad() of both models first, as both trainers do
            l, n, _, state = step(ct, nets, state, aux_losses)
            for tag in ur.MODELS[kind]:                       # each model's step follows its own backward; the models share no parameter
                opts[tag].step()
            losses.append(l)
            counts.append(n)
        gold["traj_losses"], gold["traj_counts"] = np.stack(losses), np.stack(counts)
        for tag, t in state.items():
            gold["traj_state/" + tag] = t.numpy()
        for tag, net in nets.items():
            for k, p in net.named_parameters():
                if p.requires_grad:
                    key = f"{tag}/{k}"
                    gold["final/" + key], gold["fstat/" + key], gold["fproj/" + key] = ur.encode("final/" + key, p.detach().numpy(), sub)
            net.load_state_dict(before[tag])
    gold["meta"] = np.array(repr(dict(
        case=name, T=c["T"], N=c["N"], config=repr(c["cfg"].to_dict()),
        layer1="out/*, state/*: imported reference models in float64 and eval mode, T*N rows + (R,N,H) state -> seq_forward; trunk features and "
               "the BERT stream (hooked onto embedding_layer) from tests/update_ref.frozen_outputs: float64, rounded to 1/4096",
        layer2="losses, counts: torch nn.CrossEntropyLoss(ignore_index=-1) / nn.MSELoss / nn.BCEWithLogitsLoss and the reference's AuxLosses.reduce "
               "as robo_vln_trainer.py:521-533 and hierarchical_trainer.py:508-511, :522-553 apply them",
        layer3="grad/*, gstat/*, gproj/*, nograd, frozen, buffer: loss.backward() of layer 2; tests/update_ref.encode",
        layer4="traj_*, final/*, fstat/*, fproj/*: torch.optim.Adam(lr=1e-3, eps=1e-3), the chunk twice, the state carried and detached")))
    return gold


def run_case(name):
    ref_shims.install()
    from robo_vln_baselines.common.aux_losses import AuxLosses
    c = ur.inputs(name)
    nets = build(c)
    path = os.path.join(ur.GOLD, name + ".npz")
    AuxLosses.activate()                                      # robo_vln_trainer.py:949-954: active for the whole train loop
    try:
        for sub in (1024, 512, 256, 128, 64):                 # the largest subsample that keeps the file under the limit
            save_npz(path, **gold_of(name, c, nets, AuxLosses, sub))
            if os.path.getsize(path) <= LIMIT:
                break
        else:
            raise SystemExit(f"{name}: {os.path.getsize(path)} bytes with the smallest subsample")
    finally:
        AuxLosses.deactivate()
        AuxLosses.clear()
    # restatement cross-check: the float64 CPU path of the train modules
    gold = ur.load(name)
    ours = ur.modules(name, _d)
    worst = ur.compare(name, gold, ours, ur.forward_backward(name, ours, _d), None, "float64 CPU path")
    if name in ur.TRAJECTORY:
        ours = ur.modules(name, _d)
        worst.update(ur.compare(name, gold, ours, None, ur.trajectory(name, ours, _d), "float64 CPU path, trajectory"))
    w = ur.worse(*worst.values())
    grad, nograd, frozen, buffers = ur.partition(gold)
    print(f"[{name}] {os.path.getsize(path)} bytes, subsample {int(gold['subsample'])}; {len(grad)} gradients, {len(nograd)} None, {len(frozen)} frozen; "
          f"losses {np.array2string(gold['losses'], precision=6)}; restatement-vs-reference worst {w:.3e}")
    return w


if __name__ == "__main__":
    names = sys.argv[1:] or list(ur.UPDATE_CASES)
    bad = 0
    for n in names:
        bad |= not run_case(n) <= CHECK
    sys.exit(1 if bad else 0)
