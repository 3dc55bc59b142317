"""Teacher-forced validation step without a GPU: the C ABI's declaration, export and argument checks, the torch-CPU restatement
(tests/val_ref.py) against the golden captured from the imported reference models (tests/golden/val_*.npz, tools/gen_val_golden.py), the
logit-gap condition that keeps the accuracy count well defined, and HCMValidator's chunking against a direct loop."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robo_vln_amd import _lib
from robo_vln_amd.cma import _to_struct as cma_struct
from robo_vln_amd.config import CMAConfig, HCMConfig, S2SConfig
from robo_vln_amd.policy import HCMEngine, _to_struct
from robo_vln_amd.seq2seq import _to_struct as s2s_struct
from robo_vln_amd.validate import HCMValidator
from tests import val_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5      # fp32 CPU restatement vs fp32 CPU reference (different op order only), as tests/test_s2s_cpu.py


# ---------------------------------------------------------------- declaration, export, binding
def test_header_declares_and_library_exports_val_step():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    m = re.search(r"int hcm_val_step\(([^;]*)\);", text)
    assert m, "include/hcm.h does not declare hcm_val_step"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = _lib.EXPORTS["hcm_val_step"]
    assert res is C.c_int and len(args) == n_args == 23
    assert hasattr(_lib.lib(), "hcm_val_step")
    m2 = re.search(r"int hcm_op_val_loss\(([^;]*)\);", text)
    assert m2 and len(m2.group(1).split(",")) == len(_lib.EXPORTS["hcm_op_val_loss"][1]) == 11 and hasattr(_lib.lib(), "hcm_op_val_loss")
    for line in ("562-631", "597-599", "617-621", "623-626", "NaN"):
        assert line in text[text.index("hierarchical_trainer.py:562-631"):m.end()], line


# ---------------------------------------------------------------- argument checks (no device work)
def _hcm_handle(max_batch=4):
    l = _lib.lib()
    st = _to_struct(HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2).validate(), max_batch, "fp32", True, True)
    h = C.c_void_p()
    assert l.hcm_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    return l, h


def _args(h, p, T=2, N=2, L=20, rgb_dt=_lib.HCM_F32, ids_dt=_lib.HCM_I64, result="p"):
    return (h, p, rgb_dt, p, p, ids_dt, None, T, N, L, p, p, p, p, p, p, p if result == "p" else result, p, p, None, None, None, None)


def test_val_step_argument_errors():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    l = _lib.lib()
    assert l.hcm_val_step(*_args(None, p)) == -1                                    # null handle
    l, h = _hcm_handle(max_batch=4)
    try:
        assert l.hcm_val_step(*_args(h, p, result=None)) == -1 and b"result" in l.hcm_last_error(h)
        assert l.hcm_val_step(*_args(h, p, T=3, N=2)) == -1 and b"max_batch" in l.hcm_last_error(h)      # T*N = 6 > 4
        assert l.hcm_val_step(*_args(h, p, T=0)) == -1
        assert l.hcm_val_step(*_args(h, p, rgb_dt=_lib.HCM_I64)) == -1 and b"dtype" in l.hcm_last_error(h)
        assert l.hcm_val_step(*_args(h, p, ids_dt=_lib.HCM_U8)) == -1 and b"dtype" in l.hcm_last_error(h)
        assert l.hcm_val_step(*_args(h, p)) == -2                                   # well-formed, but the handle is not finalized
    finally:
        l.hcm_destroy(h)


@pytest.mark.parametrize("kind", ["cma", "s2s"])
def test_val_step_refuses_flat_baseline_handles(kind):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    l = _lib.lib()
    h = C.c_void_p()
    if kind == "cma":
        st = cma_struct(CMAConfig(rgb_hw=128, depth_hw=128, instr_len=12).validate(), 4, "fp32")
        assert l.hcm_cma_create(C.byref(st), C.byref(h)) == 0
    else:
        st = s2s_struct(S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12).validate(), 4, "fp32")
        assert l.hcm_s2s_create(C.byref(st), C.byref(h)) == 0
    try:
        assert l.hcm_val_step(*_args(h, p, L=12)) == -2 and b"HCM handle" in l.hcm_last_error(h)
    finally:
        l.hcm_destroy(h)


# ---------------------------------------------------------------- restatement vs golden
@pytest.fixture(scope="module")
def restated():
    """name -> (cfg, T, N, ValOracle, result, hi_hidden, lo_hidden, (logits, vel, stop)) on the mixed labels"""
    out = {}
    for name in val_ref.VAL_CASES:
        cfg, T, N = val_ref.case(name)
        orc = val_ref.ValOracle(cfg, *val_ref.weights(cfg))
        obs, corrected, stop, m = val_ref.observations(cfg, T, N)
        h0 = val_ref.h0(cfg, N)
        out[name] = (cfg, T, N, orc) + tuple(orc.val_step(obs, corrected, stop, h0.clone(), h0.clone(), m, return_outputs=True))
    return out


def test_labels_exercise_every_branch():
    oracle, corrected, stop = val_ref.labels(4, 2)
    assert oracle.shape == (8, 1) and oracle.dtype == np.float32 and corrected.shape == (8, 2) and stop.shape == (8, 1)
    pad = oracle[:, 0] == 0
    assert pad.sum() >= 1 and (stop[pad] == -1).all() and (corrected[pad] == 0).all()
    assert any((corrected[r] == 0).sum() == 1 for r in np.nonzero(~pad)[0])          # a valid row with an exact 0 in one component
    assert set(oracle[:, 0].tolist()) >= {1.0, 2.0, 3.0, 4.0}
    assert {0.0, 1.0} <= set(stop[:, 0].tolist())
    o_p, c_p, s_p = val_ref.labels(4, 2, "padded")
    assert (o_p == 0).all() and (c_p == 0).all() and (s_p == -1).all()


@pytest.mark.parametrize("name", list(val_ref.VAL_GOLDEN))
def test_restatement_matches_reference_golden(name, restated):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    meta = str(gold["meta"])
    assert "layer1" in meta and "layer2" in meta and "imported reference models" in meta and "nn.CrossEntropyLoss" in meta
    cfg, T, N, orc, res, hh, lh, (logits, vel, stop) = restated[name]
    for got, key in ((logits, "logits"), (vel, "vel"), (stop, "stop"), (hh, "hi_hidden"), (lh, "lo_hidden")):
        np.testing.assert_allclose(got.numpy(), gold[key], atol=TOL, rtol=0, err_msg=key)
    np.testing.assert_allclose(res.numpy()[:3], gold["result"][:3], rtol=1e-6, atol=0)
    assert res.numpy()[3:].tolist() == gold["result"][3:].tolist()
    assert gold["result"][4] == 7 and gold["result"][5] == 7 and 0 < gold["result"][3] < 7 and gold["result"][6] == 0
    # the golden's own five numbers are torch's criteria of the golden's tensors
    oracle, corrected, ostop = val_ref.labels(T, N)
    again = val_ref.criteria(gold["logits"], gold["vel"], gold["stop"], oracle, corrected, ostop)
    assert np.array_equal(again.numpy(), gold["result"])


@pytest.mark.parametrize("name", list(val_ref.VAL_CASES))
def test_all_padded_labels_give_nan_losses_and_zero_counts(name, restated):
    cfg, T, N, orc, res, hh, lh, (logits, vel, stop) = restated[name]
    r = val_ref.criteria(logits, vel, stop, *val_ref.labels(T, N, "padded")).numpy()
    assert math.isnan(r[0]) and math.isnan(r[2])
    assert r[1] == 0.0                                                                 # every vel element masked: NaN-free, exactly 0
    assert r[3:].tolist() == [0, 0, 0, 0, 0]
    if name in val_ref.VAL_GOLDEN:
        g = np.load(os.path.join(GOLD, name + ".npz"))["result_padded"]
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.nan_to_num(g), np.nan_to_num(r))


@pytest.mark.parametrize("name", list(val_ref.VAL_CASES))
def test_valid_rows_have_a_clear_argmax(name, restated):
    """Accuracy is a count over an argmax: every valid row's two largest logits are further apart than twice the 16-bit output
    tolerance, so the GPU tests may demand the exact count in every precision mode."""
    cfg, T, N, orc, res, hh, lh, (logits, vel, stop) = restated[name]
    oracle, _, _ = val_ref.labels(T, N)
    top2 = torch.sort(logits[torch.from_numpy(oracle[:, 0] != 0)], dim=1).values[:, -2:]
    gap = (top2[:, 1] - top2[:, 0]).min().item()
    print(f"{name}: smallest top-2 logit gap over the valid rows {gap:.4f} (required > {val_ref.LOGIT_GAP})")
    assert gap > val_ref.LOGIT_GAP


def test_out_of_range_labels_are_counted_and_padded(restated):
    cfg, T, N, orc, res, hh, lh, (logits, vel, stop) = restated["val_T4_N2_gru"]
    r = val_ref.criteria(logits, vel, stop, *val_ref.labels(T, N, "bad")).numpy()
    assert r[6] == 1 and r[4] == 6
    assert val_ref.remap(val_ref.labels(T, N, "bad")[0]).tolist() == [0, 1, 4, 1, 4, 3, 0, 2]
    with pytest.raises(ValueError, match="outside"):
        HCMEngine.check_val_result(torch.from_numpy(r))
    assert HCMEngine.check_val_result(res).shape == (1, 8)


# ---------------------------------------------------------------- HCMValidator
def _batches(cfg, n_batches, T_total, N):
    """Batches as the trainer's collate_fn returns them: T_total*N rows, masks / prev_actions (rows, 2), one instruction per trajectory."""
    from oracle import cases
    from robo_vln_amd import synth
    out = []
    for b in range(n_batches):
        rows = T_total * N
        obs = synth.make_observations(cfg, rows, step=20 + b, seed=val_ref.SEED)
        obs["instruction"] = synth.make_observations(cfg, N, step=b, seed=val_ref.SEED)["instruction"]
        oracle, corrected, stop = val_ref.labels(T_total, N)
        oracle = np.roll(oracle, b, 0)
        obs["vln_oracle_action_sensor"] = oracle
        masks = np.ones((rows, 2), np.float32)
        masks[:N] = 0                                                                  # not_done_masks[0] = 0 (hierarchical_trainer.py:137-138)
        out.append(({k: torch.from_numpy(np.asarray(v)) for k, v in obs.items()}, torch.zeros(rows, 2), torch.from_numpy(masks),
                    torch.from_numpy(corrected), torch.from_numpy(stop)))
    return out


def test_validator_chunks_carries_and_accumulates_like_a_direct_loop():
    cfg, _, N = val_ref.case("val_T4_N2_gru")
    orc = val_ref.ValOracle(cfg, *val_ref.weights(cfg))
    steps, T_total = 2 * N, 5                                   # chunks of 2 time steps; 5 steps -> chunks of 4, 4 and 2 rows
    batches = _batches(cfg, 2, T_total, N)
    got = HCMValidator(orc, tbptt_steps=steps, batch_size=N).run(batches)
    assert got["chunks"] == 6 and got["table"].shape == (6, 8)
    assert [c["rows"] for c in orc.calls] == [4, 4, 2, 4, 4, 2]

    # the direct loop: val_epoch (:759-830) written out with torch's split
    direct = val_ref.ValOracle(cfg, *val_ref.weights(cfg))
    R = cfg.num_recurrent_layers
    highs, lows, correct, total, carried = [], [], 0, 0, []
    for obs, prev, masks, corrected, stop in batches:
        hh = torch.zeros(R, N, cfg.hidden)
        lh = torch.zeros(R, N, cfg.hidden)
        split = {k: v.split(steps, 0) for k, v in obs.items() if k != "instruction"}
        for i, (c, s, m) in enumerate(zip(corrected.split(steps, 0), stop.split(steps, 0), masks.split(steps, 0))):
            o = {k: v[i] for k, v in split.items()}
            o["instruction"] = obs["instruction"].repeat(c.shape[0] // N, 1)
            carried.append((hh.clone(), lh.clone()))
            r, hh, lh = direct.val_step(o, c, s, hh, lh, m)
            highs.append(float(r[0])); lows.append(float(r[1]) + float(r[2]))
            correct += int(r[3]); total += int(r[4])
    assert got["high_loss"] == pytest.approx(np.mean(highs), rel=1e-6)
    assert got["low_loss"] == pytest.approx(np.mean(lows), rel=1e-6)
    assert got["accuracy"] == pytest.approx(100 * correct / total, rel=1e-12) and total > 0
    # hidden states: zero at the start of each batch, carried inside it
    for call, (hh, lh) in zip(orc.calls, carried):
        assert torch.equal(call["hi_hidden"], hh) and torch.equal(call["lo_hidden"], lh)
    assert not orc.calls[0]["hi_hidden"].any() and not orc.calls[3]["lo_hidden"].any() and orc.calls[1]["hi_hidden"].any()


class _Recorder:
    """A val_step that computes nothing: for the refusals, which must come before any model work."""
    device = "cpu"
    num_recurrent_layers = 1
    cfg = HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2, rnn_type="GRU").validate()
    check_val_result = staticmethod(HCMEngine.check_val_result)

    def __init__(self, bad_at=None):
        self.n, self.bad_at = 0, bad_at

    def val_step(self, observations, corrected_actions, oracle_stop, hi_hidden, lo_hidden, masks, result=None, return_outputs=False):
        result.copy_(torch.tensor([1.0, 0.5, 0.25, 1, 2, 2, 1.0 if self.n == self.bad_at else 0.0, 0]))
        self.n += 1
        return result, hi_hidden, lo_hidden


def _label_batch(rows):
    obs = {"rgb": torch.zeros(rows, 1), "depth": torch.zeros(rows, 1), "instruction": torch.zeros(1, 5), "vln_oracle_action_sensor": torch.ones(rows, 1)}
    return obs, torch.zeros(rows, 2), torch.ones(rows, 2), torch.zeros(rows, 2), torch.zeros(rows, 1)


def test_validator_refuses_a_ragged_chunk_and_out_of_range_labels():
    rec = _Recorder()
    with pytest.raises(ValueError, match=r"state_encoder\.py:96.*view"):
        HCMValidator(rec, tbptt_steps=4, batch_size=2).run([_label_batch(7)])         # chunks of 4 and 3 rows
    assert rec.n == 0
    with pytest.raises(ValueError, match="outside"):
        HCMValidator(_Recorder(bad_at=1), tbptt_steps=4, batch_size=2).run([_label_batch(8)])
    ok = HCMValidator(_Recorder(), tbptt_steps=4, batch_size=2).run([_label_batch(8), _label_batch(4)])
    assert ok["chunks"] == 3 and ok["high_loss"] == 1.0 and ok["low_loss"] == 0.75 and ok["accuracy"] == 50.0
