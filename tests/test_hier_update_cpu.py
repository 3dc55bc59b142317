"""The hierarchical trainer's update step without a GPU: the declaration, export and argument errors of the sub-task cross-entropy op,
train.subtask_ce_ref against nn.CrossEntropyLoss as the trainer writes it, train.HighLevel and train.LowLevel against the golden captured from
the imported reference models (tests/golden/val_T4_N2_gru.npz), their state dicts, gradients, ablations and refusals, train.hier_update, what the
case list of tests/subtask_ce_cases.py reaches, and whether the GPU tests' bound means anything on those cases."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import hcm_oracle
from robo_vln_amd import _lib, synth, train
from robo_vln_amd.config import HCMConfig
from tests import features_ref, val_ref
from tests import subtask_ce_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5          # the project's module-against-golden bound (tests/test_flat_update_cpu.py)
HALF = 0.5 * 1e-5


# ---------------------------------------------------------------- declaration, export, binding
def test_header_declares_and_library_exports_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for sym, n, res in (("hcm_op_subtask_ce_work_floats", 3, C.c_int64), ("hcm_op_subtask_ce_train", 11, C.c_int),
                        ("hcm_op_subtask_ce_bwd", 15, C.c_int)):
        m = re.search(r"(?:int|int64_t) %s\(([^;]*)\);" % sym, text)
        assert m, f"include/hcm.h does not declare {sym}"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        got, args = _lib.EXPORTS[sym]
        assert got is res and len(args) == n_args == n, sym
        assert hasattr(_lib.lib(), sym)
    l = _lib.lib()
    assert l.hcm_op_subtask_ce_work_floats(64, 512, 4) == 2 * (4 * 512 + 8) and l.hcm_op_subtask_ce_work_floats(33, 512, 6) == 2 * (6 * 512 + 8)
    assert l.hcm_op_subtask_ce_work_floats(0, 512, 4) == 0
    for bad in ((64, 256, 4), (64, 512, 0), (64, 512, 7), (-1, 512, 4)):
        assert l.hcm_op_subtask_ce_work_floats(*bad) == 0, bad


def test_argument_errors_without_a_device():
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                         # 16-byte aligned, as the ops require of x and the weights
    l = _lib.lib()

    def fwd(rows=4, hidden=512, A=4, nst=4, **null):
        a = dict.fromkeys(("x", "w", "b", "oracle", "logits", "result"), p)
        a.update(null)
        return l.hcm_op_subtask_ce_train(*a.values(), rows, hidden, A, nst, None)

    def bwd(rows=4, hidden=512, A=4, nst=4, **null):
        a = dict.fromkeys(("d_result", "x", "w", "logits", "oracle", "result", "d_x", "d_w", "d_b", "work"), p)
        a.update(null)
        return l.hcm_op_subtask_ce_bwd(*a.values(), rows, hidden, A, nst, None)

    for call in (fwd, bwd):
        assert call(hidden=256) == -1 and _lib.last_error().startswith("subtask_ce:")
        assert call(A=0) == -1 and call(A=7) == -1 and call(rows=-1) == -1
        assert call(nst=0) == -1 and call(nst=5) == -1 and "num_sub_tasks" in _lib.last_error()
        assert call(x=None) == -1 and call(w=None) == -1 and call(oracle=None) == -1 and call(result=None) == -1
        assert call(x=C.c_void_p(p.value + 4)) == -1 and "aligned" in _lib.last_error()
        assert call(oracle=C.c_void_p(p.value + 4)) == -1 and "aligned" in _lib.last_error()
        assert call(rows=0) == 0 and call(rows=0, x=None, oracle=None) == 0          # nothing to do, nothing read, nothing written
    assert fwd(logits=None) == -1 and fwd(b=None) == -1
    assert bwd(d_result=None) == -1 and bwd(d_w=None) == -1 and bwd(d_b=None) == -1 and bwd(work=None) == -1 and bwd(logits=None) == -1
    assert bwd(d_w=C.c_void_p(p.value + 8)) == -1 and "aligned" in _lib.last_error()
    assert bwd() == -1 and "overlaps work" in _lib.last_error()                       # every pointer is the same buffer: d_x lies in work
    assert all(v == 0 for v in buf)


# ---------------------------------------------------------------- restatement against nn.CrossEntropyLoss
REF_CASES = [(5, 4, 4, True, True), (33, 4, 4, False, False), (64, 6, 6, True, True), (63, 1, 1, False, False), (17, 6, 4, True, True),
             (300, 4, 4, True, True)]


@pytest.mark.parametrize("rows,A,nst,dx,bad", REF_CASES)
def test_ref_matches_the_trainer_s_cross_entropy(rows, A, nst, dx, bad):
    args = sc.make_inputs(rows, A, nst, bad)
    a, named = sc.leaves_of(args, True, lambda t: t.double())
    result, logits = train.subtask_ce_ref(*a, nst)
    b, named_t = sc.leaves_of(args, True, lambda t: t.double())
    loss, correct, total, n_bad = sc.torch_criterion(*b, nst)
    assert abs(float(result[0].detach()) - float(loss.detach())) <= 1e-12
    assert result[1:].tolist() == [0, 0, correct, total, 0, n_bad, 0] and 0 < total < rows and n_bad == int(bad)
    assert torch.equal(logits.detach(), torch.nn.functional.linear(a[0], a[1], a[2]).detach())       # the raw output: no row zeroed
    got = torch.autograd.grad(result, list(named.values()), sc.cotangent(torch.float64))
    ref = torch.autograd.grad(sc.COT * loss, list(named_t.values()))
    for name, g, r in zip(named, got, ref):
        assert (g - r).abs().max().item() <= 1e-12 * max(1.0, r.abs().max().item()), name
    # tests/val_ref.criteria (float32) on the float32 run's own logits, with dummy low-level tensors
    r32, l32 = train.subtask_ce_ref(*args, nst)
    crit = val_ref.criteria(l32, torch.zeros(rows, 2), torch.zeros(rows, 1), args[3], torch.zeros(rows, 2), torch.zeros(rows, 1), nst)
    assert [crit[k].item() for k in (3, 4, 6)] == [r32[k].item() for k in (3, 4, 6)]
    assert abs(float(r32[0]) - float(crit[0])) <= 1e-6 * max(1.0, abs(float(crit[0])))
    # integer labels of any shape mean the same
    r_int = train.subtask_ce_ref(*args[:3], args[3].reshape(-1).to(torch.int32), nst)[0]
    assert torch.equal(r_int, r32)


def test_label_edges():
    rows, A = 6, 4
    x, w, b, _ = sc.make_inputs(rows, A, A, False, seed=3)
    result, logits, grads = sc.run(train.subtask_ce_ref, (x, w, b, torch.zeros(rows, 1)), A, True, lambda t: t.double())
    assert math.isnan(float(result[0])) and result[1:].tolist() == [0] * 7 and torch.isfinite(logits).all()
    for name, g in grads.items():
        assert (g == 0).all(), name                                                   # the all-padded case: NaN loss, zero gradients
    result, _, grads = sc.run(train.subtask_ce_ref, (x, w, b, torch.tensor([[-1.0], [5], [9], [0], [-3], [7]])), A, True, lambda t: t.double())
    assert math.isnan(float(result[0])) and result[1:].tolist() == [0, 0, 0, 0, 0, 5, 0] and all((g == 0).all() for g in grads.values())
    # a padded and an out-of-range row get exact zero rows of d_x; the valid rows do not
    oracle = torch.tensor([[1.0], [0], [4], [9], [2], [3]])
    result, _, grads = sc.run(train.subtask_ce_ref, (x, w, b, oracle), A, True, lambda t: t.double())
    assert result[4] == 4 and result[6] == 1
    assert (grads["d_x"][[1, 3]] == 0).all() and (grads["d_x"][[0, 2, 4, 5]] != 0).any(1).all()
    # num_sub_tasks below A: label 4 is out of range, the fourth class is never a target but stays in the softmax
    r3 = train.subtask_ce_ref(x, w, b, oracle, 3)[0]
    assert r3[4] == 3 and r3[6] == 2
    with pytest.raises(ValueError, match="num_sub_tasks"):
        train.subtask_ce_ref(x, w, b, oracle, 5)
    with pytest.raises(ValueError, match="one sub-task label per row"):
        train.subtask_ce(x, w, b, oracle[:5])
    # the CPU route of subtask_ce is the restatement, default num_sub_tasks = A
    assert torch.equal(train.subtask_ce(x, w, b, oracle)[0], train.subtask_ce_ref(x, w, b, oracle, A)[0])


# ---------------------------------------------------------------- the modules against the reference golden
def _golden_case():
    name = "val_T4_N2_gru"
    cfg, T, N = val_ref.case(name)
    hi_sd, lo_sd = val_ref.weights(cfg)
    obs, corrected, stop, masks = val_ref.observations(cfg, T, N)
    return name, cfg, T, N, hi_sd, lo_sd, obs, corrected, stop, masks


def test_the_pair_matches_the_reference_golden():
    name, cfg, T, N, hi_sd, lo_sd, obs, corrected, stop, masks = _golden_case()
    rows = T * N
    hi_rgb, hi_depth = features_ref.trunk_features(cfg, hi_sd, obs, spatial=True)
    lo_rgb, lo_depth = features_ref.trunk_features(cfg, lo_sd, obs, spatial=False)
    ids = torch.as_tensor(np.asarray(obs["instruction"])).long()
    with torch.no_grad():
        stream = hcm_oracle.bert_encoder(ids, hcm_oracle.Weights(hi_sd).sub("embedding_layer."), cfg.bert_layers, cfg.bert_heads)
    assert stream.shape[0] in (1, rows) and stream.shape[2] == cfg.ins_in
    high, low = train.HighLevel(cfg).eval(), train.LowLevel(cfg).eval()
    high.load_reference_state_dict(hi_sd)
    low.load_reference_state_dict(lo_sd)
    oracle = torch.as_tensor(obs["vln_oracle_action_sensor"])
    assert tuple(oracle.shape) == (rows, 1) and oracle.dtype == torch.float32
    o = {"rgb_features": (hi_rgb, lo_rgb), "depth_features": (hi_depth, lo_depth), "instruction_features": stream}
    m = torch.as_tensor(np.asarray(masks, np.float32)).reshape(rows, -1)
    h0 = val_ref.h0(cfg, N)
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    with torch.no_grad():
        logits, hi_hidden = high((o, h0.clone(), None, m))
        res_hi, hi_hidden_u = high.update_loss((o, h0.clone(), None, m), oracle)
        sub = val_ref.remap(oracle, cfg.num_sub_tasks)
        vel, stop_out, lo_hidden = low((o, h0.clone(), None, m, sub))
        res_lo, lo_hidden_u = low.update_loss((o, h0.clone(), None, m, sub), torch.from_numpy(corrected), torch.from_numpy(stop))
    assert torch.equal(hi_hidden, hi_hidden_u) and torch.equal(lo_hidden, lo_hidden_u)
    errs = {}
    for got, key in ((logits, "logits"), (vel, "vel"), (stop_out, "stop"), (hi_hidden, "hi_hidden"), (lo_hidden, "lo_hidden")):
        errs[key] = float(np.abs(got.numpy() - gold[key]).max())
    result = [float(res_hi[0]), float(res_lo[0]), float(res_lo[1])]
    errs["result"] = float(np.abs(np.array(result) - gold["result"][:3]).max())
    print(f"{name}: modules vs golden {errs}")
    assert max(errs.values()) <= TOL, errs
    assert [float(res_hi[3]), float(res_hi[4]), float(res_lo[3]), float(res_hi[6])] == gold["result"][3:7].tolist()
    # one stream for all rows is expanded (seq2seq_highlevel_cma.py:190): the golden's instruction is the same in every row
    if stream.shape[0] == rows and bool((ids == ids[:1]).all()):
        with torch.no_grad():
            one = high((dict(o, instruction_features=stream[:1]), h0.clone(), None, m))[0]
        assert (one - logits).abs().max().item() <= TOL            # (a product over one row may round differently from one over all rows)
    # the embedder route gives the stream's result
    def embedder(tokens):
        return hcm_oracle.bert_encoder(tokens, hcm_oracle.Weights(hi_sd).sub("embedding_layer."), cfg.bert_layers, cfg.bert_heads)
    high_e = train.HighLevel(cfg, embedder=embedder).eval()
    high_e.load_reference_state_dict(hi_sd)
    assert set(high_e.state_dict()) == set(high.state_dict())
    with torch.no_grad():
        via = high_e(({k: v for k, v in o.items() if k != "instruction_features"} | {"instruction": ids}, h0.clone(), None, m))[0]
    assert torch.equal(via, logits)


# ---------------------------------------------------------------- state dicts
def test_state_dict_keys_are_the_reference_s_outside_the_frozen_parts():
    cfg = sc.module_cfg()
    for spec, sd_tag, net, prefixes in ((synth.high_level_spec(cfg), "hi", train.HighLevel(cfg), train.HCM_HIGH_FROZEN_PREFIXES),
                                        (synth.low_level_spec(cfg), "lo", train.LowLevel(cfg), train.HCM_LOW_FROZEN_PREFIXES)):
        sd = synth.materialize(spec, sd_tag, 3)
        rest = [k for k, *_ in spec if not k.startswith(prefixes)]
        own = net.state_dict()
        assert set(own) == set(rest) and len(rest) < len(spec)
        assert all(tuple(own[k].shape) == tuple(np.shape(sd[k])) for k in rest)
        net.load_reference_state_dict(sd)                                     # the full reference dict, frozen parts included
        assert all(np.array_equal(net.state_dict()[k].numpy(), sd[k]) for k in rest)
        net.load_reference_state_dict({k: sd[k] for k in rest})               # ... and without them
        for k in ("progress_monitor.weight", "linear.bias", "state_encoder.rnn.weight_hh_l0"):
            with pytest.raises((RuntimeError, KeyError)):
                net.load_reference_state_dict({j: v for j, v in sd.items() if j != k})
        with pytest.raises((RuntimeError, ValueError)):
            net.load_reference_state_dict(dict(sd, **{"linear.weight": sd["linear.weight"][:, :-1]}))
        with pytest.raises((RuntimeError, KeyError)):
            net.load_reference_state_dict(dict(sd, **{"no_such.weight": sd["linear.bias"]}))
        assert net.num_recurrent_layers == cfg.num_recurrent_layers and net.output_size == cfg.hidden
    assert train.HCM_HIGH_FROZEN_PREFIXES == ("rgb_encoder.cnn.", "depth_encoder.visual_encoder.", "embedding_layer.")
    low = train.LowLevel(cfg)
    assert low.sub_task_embedding.padding_idx == cfg.num_sub_tasks and (low.sub_task_embedding.weight[cfg.num_sub_tasks] == 0).all()


# ---------------------------------------------------------------- gradients
def _losses(high, low, obs, h_hi, h_lo, prev, masks, corrected, stop, cfg):
    res_hi, _ = high.update_loss((obs, h_hi, prev, masks), obs["vln_oracle_action_sensor"])
    sub = val_ref.remap(obs["vln_oracle_action_sensor"], cfg.num_sub_tasks)
    res_lo, _ = low.update_loss((obs, h_lo, prev, masks, sub), corrected, stop)
    return res_hi, res_lo


def test_every_trainable_parameter_gets_a_gradient_and_the_monitors_none():
    cfg, high, low, obs, h_hi, h_lo, prev, masks, corrected, stop = sc.module_case()
    res_hi, res_lo = _losses(high, low, obs, h_hi, h_lo, prev, masks, corrected, stop, cfg)
    assert res_hi[4] == 4 and res_hi[6] == 1 and res_lo[3] == 5
    res_hi[0].backward()
    (res_lo[0] + res_lo[1]).backward()
    for net in (high, low):
        for n, p in net.named_parameters():
            if n.startswith(("progress_monitor.", "ins_fc.")):
                assert p.grad is None, n                                       # parameters only
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any(), n
    g = low.sub_task_embedding.weight.grad
    assert (g[cfg.num_sub_tasks] == 0).all() and (g[:cfg.num_sub_tasks] != 0).any(1).all()      # the padding row gets no gradient


# ---------------------------------------------------------------- ablations and refusals
def test_ablation_flags_and_refusals():
    cfg, high, low, obs, h_hi, h_lo, prev, masks, corrected, stop = sc.module_case(T=1)
    rows = masks.shape[0]
    for flag, key in (("ablate_rgb", "rgb_features"), ("ablate_depth", "depth_features")):
        acfg = sc.module_cfg(**{flag: True})
        a_hi, a_lo = train.HighLevel(acfg, dropout=0.0), train.LowLevel(acfg)
        a_hi.load_state_dict(high.state_dict())
        a_lo.load_state_dict(low.state_dict())
        without = {k: v for k, v in obs.items() if k != key}
        zeroed = dict(obs, **{key: tuple(torch.zeros_like(t) for t in obs[key])})
        sub = val_ref.remap(obs["vln_oracle_action_sensor"], cfg.num_sub_tasks)
        with torch.no_grad():
            # an ablated modality needs no key, and the key is not read when it is there
            assert all(torch.equal(u, v) for u, v in zip(a_hi((without, h_hi, prev, masks)), a_hi((obs, h_hi, prev, masks))))
            assert all(torch.equal(u, v) for u, v in zip(a_lo((without, h_lo, prev, masks, sub)), a_lo((obs, h_lo, prev, masks, sub))))
            # the low-level embedding is times 0: the model fed zero features with the visual bias removed; the high-level one zeroes the whole
            # embedding, the spatial tail included, which differs from zero features
            assert not torch.equal(a_hi((obs, h_hi, prev, masks))[0], high((zeroed, h_hi, prev, masks))[0])
            assert not torch.equal(a_lo((obs, h_lo, prev, masks, sub))[0], low((obs, h_lo, prev, masks, sub))[0])
    with pytest.raises(ValueError, match="ablate_instruction"):
        train.HighLevel(HCMConfig(rgb_hw=128, depth_hw=128, ablate_instruction=True))
    for kw in (dict(depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN"), dict(rgb_encoder="SimpleRGBCNN")):
        with pytest.raises(ValueError, match="trainable trunk"):
            train.LowLevel(HCMConfig(rgb_hw=128, depth_hw=128, **kw).validate())
        with pytest.raises(ValueError, match="trainable trunk"):
            train.HighLevel(HCMConfig(rgb_hw=128, depth_hw=128, **kw).validate())
    with pytest.raises(ValueError, match="instruction_features"):
        high(({k: v for k, v in obs.items() if k != "instruction_features"}, h_hi, prev, masks))
    with pytest.raises(ValueError, match="instruction_features"):
        high((dict(obs, instruction_features=obs["instruction_features"][:, :, :64]), h_hi, prev, masks))
    with pytest.raises(ValueError, match="encode_features"):
        high(({k: v for k, v in obs.items() if k != "rgb_features"}, h_hi, prev, masks))
    with pytest.raises(ValueError, match="rgb_features"):
        high((dict(obs, rgb_features=obs["rgb_features"][1]), h_hi, prev, masks))             # the low entry: (rows, 2048, 1, 1)
    with pytest.raises(ValueError, match="depth_features"):
        low(({k: v for k, v in obs.items() if k != "depth_features"}, h_lo, prev, masks, torch.zeros(rows, dtype=torch.int64)))
    with pytest.raises(ValueError, match="discrete_actions"):
        low((obs, h_lo, prev, masks, torch.zeros(rows)))
    with pytest.raises(ValueError, match="oracle_subtask"):
        high.update_loss((obs, h_hi, prev, masks), obs["vln_oracle_action_sensor"][:1])
    # a tensor in place of a pair is taken as it is
    with torch.no_grad():
        a = high((dict(obs, rgb_features=obs["rgb_features"][0], depth_features=obs["depth_features"][0]), h_hi, prev, masks))
        b = high((obs, h_hi, prev, masks))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------- hier_update
def test_hier_update_steps_both_parameter_sets_and_returns_detached_states():
    cfg, high, low, obs, h_hi, h_lo, prev, masks, corrected, stop = sc.module_case()
    before = {id(net): {n: p.detach().clone() for n, p in net.named_parameters()} for net in (high, low)}
    opt_hi, opt_lo = torch.optim.Adam(high.parameters(), lr=1e-4), torch.optim.Adam(low.parameters(), lr=1e-4)
    hi_in, lo_in = (h_hi * 1.0).requires_grad_(), (h_lo * 1.0).requires_grad_()     # states that carry a graph: hier_update must cut it
    keys = set(obs)
    res_hi, res_lo, hi_h, lo_h = train.hier_update(high, low, opt_hi, opt_lo, obs, prev, masks, corrected, stop, hi_in, lo_in)
    assert set(obs) == keys                                                       # the observations are left as they were
    for t, shape in ((res_hi, (8,)), (res_lo, (8,)), (hi_h, h_hi.shape), (lo_h, h_lo.shape)):
        assert t.shape == shape and not t.requires_grad and t.grad_fn is None and torch.isfinite(t).all()
    assert hi_in.grad is None and lo_in.grad is None
    assert res_hi.tolist()[1:] == [0, 0, float(res_hi[3]), 4, 0, 1, 0] and res_lo[3] == 5 and res_lo[2] == 0
    for net in (high, low):
        for n, p in net.named_parameters():
            same = torch.equal(p, before[id(net)][n])
            assert same == n.startswith(("progress_monitor.", "ins_fc.")), n
    assert (low.sub_task_embedding.weight[cfg.num_sub_tasks] == before[id(low)]["sub_task_embedding.weight"][cfg.num_sub_tasks]).all()
    res_hi2, res_lo2, _, _ = train.hier_update(high, low, opt_hi, opt_lo, obs, prev, masks, corrected, stop, hi_h, lo_h)
    assert float(res_hi2[0]) < float(res_hi[0]) and float(res_lo2[:2].sum()) < float(res_lo[:2].sum())      # the same batch again
    with pytest.raises(ValueError, match="vln_oracle_action_sensor"):
        train.hier_update(high, low, opt_hi, opt_lo, {k: v for k, v in obs.items() if k != "vln_oracle_action_sensor"}, prev, masks, corrected,
                          stop, hi_h, lo_h)


# ---------------------------------------------------------------- coverage
def test_cases_reach_every_launch_rule_edge():
    assert (train.SUBTASK_CE_FWD_ROWS, train.SUBTASK_CE_BWD_ROWS, train.SUBTASK_CE_BWD_HALF, train.SUBTASK_CE_LOSS_THREADS) == (4, 32, 16, 256)
    src = open(os.path.join(ROOT, "robo-vln_amd", "csrc", "subtask_ce_train.hip")).read()
    assert "kFwdRows = kT / 64, kBwdRows = 32, kHalfRows = kBwdRows / 2, kMaxA = 6, kBiasSlot = 8, kLossT = 256" in src and "constexpr int kT = 256" in src
    assert "constexpr int kValLossThreads = 256" in open(os.path.join(ROOT, "robo-vln_amd", "csrc", "elementwise.hip")).read()
    assert train.SUBTASK_CE_MAX_CLASSES == 6 and train.SUBTASK_CE_HIDDEN == 512
    assert [sc.fwd_workgroups(r) for r in (1, 4, 5, 8, 9)] == [1, 1, 2, 2, 3]
    assert [sc.bwd_blocks(r) for r in (1, 16, 17, 32, 33, 300)] == [(1, 1, 1, 0), (1, 16, 16, 0), (1, 17, 16, 1), (1, 32, 16, 16), (2, 1, 1, 0), (10, 12, 12, 0)]
    assert [sc.criterion_rows_per_thread(r) for r in (1, 256, 257, 512, 513)] == [1, 1, 2, 2, 3]
    rows = {c[0] for c in sc.CASES}
    assert rows == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 600}
    for edge in (train.SUBTASK_CE_FWD_ROWS, train.SUBTASK_CE_BWD_HALF, train.SUBTASK_CE_BWD_ROWS, 2 * train.SUBTASK_CE_BWD_ROWS,
                 train.SUBTASK_CE_LOSS_THREADS):
        assert {edge - 1, edge, edge + 1} <= rows, edge                           # one below, at, one above
    assert any(sc.bwd_blocks(r)[0] > 2 and 0 < sc.bwd_blocks(r)[1] < train.SUBTASK_CE_BWD_ROWS for r in rows)         # a ragged last block
    assert any(sc.bwd_blocks(r)[0] > 1 and sc.bwd_blocks(r)[3] == 0 for r in rows)                                    # ... whose second half is idle
    assert any(sc.fwd_workgroups(r) > 1 and r % train.SUBTASK_CE_FWD_ROWS for r in rows)                              # idle waves in the last workgroup
    assert max(sc.criterion_rows_per_thread(r) for r in rows) > 2
    assert {c[1] for c in sc.CASES} == {1, 2, 4, 6} and all(1 <= c[2] <= c[1] for c in sc.CASES)
    assert any(c[2] < c[1] for c in sc.CASES if c[0] > 32) and any(c[2] < c[1] for c in sc.CASES if c[0] <= 32)
    for small in (True, False):
        part = [c for c in sc.CASES if (c[0] <= 32) == small]
        assert {c[3] for c in part} == {False, True} and {c[4] for c in part} == {False, True}
    assert len(set(sc.CASES)) == len(sc.CASES) and set(sc.SEEDS) <= set(sc.CASES)
    assert all(sc.first_seed(*c) == sc.SEEDS.get(c, 0) for c in sc.CASES)
    for rows_, A, nst, dx, bad in sc.CASES:                                       # the scripted labels are present wherever the rows allow
        o = sc.case(rows_, A, nst, dx, bad)["args"][3][:, 0]
        assert o.shape == (rows_,) and ((o == sc.BAD_LABEL).sum() == int(bad)) and sc.BAD_LABEL > A
        if rows_ >= 5:
            assert (o[4::7] == 0).all() and (o == 0).sum() == len(range(4, rows_, 7))
        if rows_ >= nst + 3:
            assert set(range(1, nst + 1)) <= set(o.long().tolist())               # every class occurs


# ---------------------------------------------------------------- a condition on the cases, not a tolerance on the code
@pytest.mark.parametrize("rows,A,nst,dx,bad", sc.CASES)
def test_float32_restatement_stays_within_half_the_bound(rows, A, nst, dx, bad):
    c = sc.case(rows, A, nst, dx, bad)
    result, logits, grads = sc.run(train.subtask_ce_ref, c["args"], nst, dx, lambda t: t)
    worst = {"logits": sc._rel(logits, c["logits64"])}
    if c["result64"][4] > 0:
        worst["loss"] = sc._rel(result[:1], c["result64"][:1])
    else:
        assert math.isnan(float(result[0])) and math.isnan(float(c["result64"][0]))
    for name, g in grads.items():
        worst[name] = sc._rel(g, c["ref"][name])
    print(f"{(rows, A, nst, dx, bad)}: float32 restatement vs float64, worst {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
    assert result[1:].tolist() == c["result64"][1:].tolist()
    assert max(worst.values()) <= HALF, worst
    assert set(grads) == set(sc.NAMES[0 if dx else 1:])
