"""The flat trainer's validation step without a GPU: the torch-CPU restatement (tests/flat_val_ref.py) against the goldens captured from the
imported reference models (tests/golden/flatval_*.npz, tools/gen_flat_val_golden.py), torch's criteria on hand-made rows, FlatValidator's
chunking against a direct loop, and the C ABI's declaration, binding and argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robo_vln_amd import _lib
from robo_vln_amd.cma import _to_struct as cma_struct
from robo_vln_amd.config import HCMConfig
from robo_vln_amd.policy import _to_struct
from robo_vln_amd.seq2seq import _to_struct as s2s_struct
from robo_vln_amd.validate import FlatValidator
from tests import flat_val_ref as fv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5      # fp32 CPU restatement vs fp32 CPU reference (different op order only): the generators' bound


# ---------------------------------------------------------------- declaration, export, binding
def test_header_declares_and_library_exports_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for sym, n in (("hcm_flat_val_step", 21), ("hcm_op_flat_val_loss", 10)):
        m = re.search(r"int %s\(([^;]*)\);" % sym, text)
        assert m, f"include/hcm.h does not declare {sym}"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = _lib.EXPORTS[sym]
        assert res is C.c_int and len(args) == n_args == n, sym
        assert hasattr(_lib.lib(), sym)
    doc = text[text.index("robo_vln_trainer.py:544-575"):text.index("int hcm_flat_val_step(")]
    for cite in (":726-813", "aux_losses.py", "alpha", "NaN", "HCM_STEP_NONFINITE", "bit-identical"):
        assert cite in doc, cite


# ---------------------------------------------------------------- argument checks (no device work)
def _handle(kind, max_batch=4, **kw):
    l = _lib.lib()
    h = C.c_void_p()
    if kind == "cma":
        st = cma_struct(fv.case("flatval_cma_T4_N2")[1], max_batch, "fp32")
        assert l.hcm_cma_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    elif kind == "s2s":
        st = s2s_struct(fv.case("flatval_s2s_T4_N2_gru")[1], max_batch, "fp32")
        assert l.hcm_s2s_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    elif kind == "s2s_pm":
        st = s2s_struct(fv.case("flatval_s2s_pm_T3_N2_gru")[1], max_batch, "fp32")
        assert l.hcm_s2s_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    else:
        st = _to_struct(HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2).validate(), max_batch, "fp32", True, True)
        assert l.hcm_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    return l, h


def _call(l, h, p, T=2, N=2, B_instr=None, L=12, progress=None, progress_hat=None, result="p"):
    return l.hcm_flat_val_step(h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, T, N, T * N if B_instr is None else B_instr, L, p, p, progress, p, p,
                               p if result == "p" else result, p, None, None, progress_hat, None)


def test_flat_val_step_argument_errors_without_a_device():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    l = _lib.lib()
    assert _call(l, None, p) == -1                                                          # null handle
    l, h = _handle("hcm")
    try:
        assert _call(l, h, p, L=20) == -2 and b"hcm_val_step" in l.hcm_last_error(h)         # HCM_ERR_STATE, and where to go instead
    finally:
        l.hcm_destroy(h)
    l, h = _handle("cma")
    try:
        assert _call(l, h, p, B_instr=1) == -1 and b"B_instr" in l.hcm_last_error(h)         # CMANet: one instruction row per frame
        assert _call(l, h, p, progress=p) == -1 and b"progress" in l.hcm_last_error(h)
        assert _call(l, h, p, progress_hat=p) == -1 and b"progress" in l.hcm_last_error(h)
        assert _call(l, h, p, T=3, N=2) == -1 and b"max_batch" in l.hcm_last_error(h)        # T*N = 6 > 4
        assert _call(l, h, p, T=1 << 16, N=1 << 16) == -1                                    # (no 32-bit wrap of the product)
        assert _call(l, h, p, T=0) == -1 and _call(l, h, p, N=0) == -1
        assert _call(l, h, p, result=None) == -1 and b"result" in l.hcm_last_error(h)
        assert _call(l, h, p) == -2                                                          # well-formed, but the handle is not finalized
    finally:
        l.hcm_destroy(h)
    l, h = _handle("s2s")
    try:
        assert _call(l, h, p, progress=p) == -1 and b"progress" in l.hcm_last_error(h)       # no monitor on this handle
        assert _call(l, h, p, progress_hat=p) == -1 and b"progress" in l.hcm_last_error(h)
        assert _call(l, h, p, B_instr=3) == -1 and b"B_instr" in l.hcm_last_error(h)
        assert _call(l, h, p, T=3, N=2) == -1 and b"max_batch" in l.hcm_last_error(h)
        assert _call(l, h, p, B_instr=1) == -2 and _call(l, h, p) == -2                      # both legal: the handle is not finalized
    finally:
        l.hcm_destroy(h)
    l, h = _handle("s2s_pm")
    try:
        assert _call(l, h, p) == -1 and b"progress" in l.hcm_last_error(h)                   # the monitor's target is missing
        assert _call(l, h, p, progress_hat=p) == -1 and b"progress" in l.hcm_last_error(h)
        assert _call(l, h, p, progress=p) == -2 and _call(l, h, p, progress=p, progress_hat=p) == -2
    finally:
        l.hcm_destroy(h)
    assert l.hcm_op_flat_val_loss(p, p, p, p, p, None, p, 4, 2, None) == -1                  # progress_hat without progress
    assert l.hcm_op_flat_val_loss(p, p, None, p, p, None, p, 0, 2, None) == -1               # no rows


# ---------------------------------------------------------------- restatement vs golden
@pytest.fixture(scope="module")
def restated():
    """name -> (kind, cfg, T, N, result, hidden, (out, stop, progress_hat)) on the mixed labels, golden cases only"""
    made = {}

    def get(name):
        if name not in made:
            kind, cfg, T, N, obs, corrected, stop, m, h0 = fv.inputs(name)
            made[name] = (kind, cfg, T, N) + tuple(fv.oracle(name).val_step(obs, corrected, stop, h0.clone(), m, return_outputs=True))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(fv.FLAT_VAL_GOLDEN))
def test_restatement_matches_reference_golden(name, restated):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    meta = str(gold["meta"])
    assert "layer1" in meta and "layer2" in meta and "imported reference model" in meta and "nn.MSELoss" in meta and "AuxLosses" in meta
    kind, cfg, T, N, res, hid, (out, stop, prog) = restated(name)
    monitor = bool(getattr(cfg, "progress_monitor", False))
    assert set(gold.files) == {"out", "stop", "hidden", "result", "result_padded", "meta"} | ({"progress_hat", "aux_reference"} if monitor else set())
    for got, key in ((out, "out"), (stop, "stop"), (hid, "hidden")) + (((prog, "progress_hat"),) if monitor else ()):
        err = np.abs(got.numpy() - gold[key]).max()
        print(f"{name}: restatement vs golden {key} {err:.3e}")
        assert err <= TOL, key
    np.testing.assert_allclose(res.numpy()[:3], gold["result"][:3], rtol=0, atol=TOL)
    assert res.numpy()[3:].tolist() == gold["result"][3:].tolist()
    rows = T * N
    n_pad = 1 if rows >= 5 else 0                                      # row 4 of tests/val_ref.labels
    assert gold["result"][3] == rows - n_pad and gold["result"][4] == ((rows - n_pad - 1) if monitor else 0)    # row 1: corrected[1, 0] == 0
    assert (gold["result"][2] > 0) == monitor and np.array_equal(gold["result"][5:], np.zeros(3, np.float32))
    # the golden's own numbers are torch's criteria of the golden's tensors, and its aux term is what the reference's AuxLosses.reduce returned
    corrected, ostop = fv.labels(T, N)
    p_hat, p = (gold["progress_hat"], fv.progress_targets(rows)) if monitor else (None, None)
    again = fv.criteria(gold["out"], gold["stop"], p_hat, corrected, ostop, p)
    assert np.array_equal(again.numpy(), gold["result"])
    if monitor:
        assert gold["aux_reference"][0] == pytest.approx(gold["result"][2], rel=1e-6) and math.isnan(gold["aux_reference"][1])


@pytest.mark.parametrize("name", list(fv.FLAT_VAL_GOLDEN))
def test_all_padded_labels_give_nan_losses_and_zero_counts(name, restated):
    kind, cfg, T, N, res, hid, (out, stop, prog) = restated(name)
    c_p, s_p = fv.labels(T, N, "padded")
    r = fv.criteria(out, stop, prog, c_p, s_p, fv.progress_targets(T * N) if prog is not None else None).numpy()
    assert r[0] == 0.0 and math.isnan(r[1]) and r[3:].tolist() == [0, 0, 0, 0, 0]          # every output element masked: exactly 0
    assert math.isnan(r[2]) if prog is not None else r[2] == 0.0
    g = np.load(os.path.join(GOLD, name + ".npz"))["result_padded"]
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.nan_to_num(g), np.nan_to_num(r))


# ---------------------------------------------------------------- criteria on hand-made rows
def test_criteria_on_hand_made_rows():
    out = torch.tensor([[0.5, -1.0], [2.0, 3.0], [7.0, 7.0], [-0.25, 0.75]])
    stop = torch.tensor([[0.0], [2.0], [50.0], [-1.0]])
    p_hat = torch.tensor([[0.5], [-0.5], [0.9], [0.0]])
    corrected = torch.tensor([[1.0, -1.0], [0.0, 2.0], [0.0, 0.0], [0.25, 0.0]])            # row 1: a valid row with an exact 0 in column 0
    ostop = torch.tensor([[1.0], [0.0], [-1.0], [1.0]])                                     # row 2 padded
    prog = torch.tensor([0.25, 0.5, 0.1, 1.0])
    r = fv.criteria(out, stop, p_hat, corrected, ostop, prog).numpy()
    # action: elements (0.5-1)^2, 0, 0, (3-2)^2, 0, 0, (-0.25-0.25)^2, 0 over ALL 8 elements
    assert r[0] == pytest.approx((0.25 + 1.0 + 0.25) / 8, rel=1e-6)
    bce = [math.log(2.0), 2.0 + math.log1p(math.exp(-2.0)), 1.0 + math.log1p(math.exp(-1.0))]
    assert r[1] == pytest.approx(sum(bce) / 3, rel=1e-6) and r[3] == 3
    # aux: rows with corrected[:, 0] != 0 are 0 and 3 -- row 1 is valid for the stop loss but NOT for the aux mean
    assert r[2] == pytest.approx(((0.5 - 0.25) ** 2 + (0.0 - 1.0) ** 2) / 2, rel=1e-6) and r[4] == 2
    assert r[5:].tolist() == [0, 0, 0]
    # monitor off: aux is exactly 0, and so is its count
    r0 = fv.criteria(out, stop, None, corrected, ostop, None).numpy()
    assert r0[2] == 0.0 and r0[4] == 0 and np.array_equal(r0[[0, 1, 3]], r[[0, 1, 3]])
    assert math.copysign(1.0, float(r0[2])) == 1.0
    # all padded
    rp = fv.criteria(out, stop, p_hat, torch.zeros(4, 2), torch.full((4, 1), -1.0), prog).numpy()
    assert rp[0] == 0.0 and math.isnan(rp[1]) and math.isnan(rp[2]) and rp[3:].tolist() == [0, 0, 0, 0, 0]
    # a NaN in a selected row's output propagates; in a masked element it does not
    o2 = out.clone(); o2[2, 0] = float("nan")
    assert np.isfinite(fv.criteria(o2, stop, None, corrected, ostop, None).numpy()[0])
    o2[0, 0] = float("nan")
    assert math.isnan(fv.criteria(o2, stop, None, corrected, ostop, None).numpy()[0])


def test_labels_exercise_every_branch():
    corrected, stop = fv.labels(4, 2)
    assert corrected.shape == (8, 2) and stop.shape == (8, 1) and corrected.dtype == np.float32
    pad = stop[:, 0] == -1
    assert pad.sum() == 1 and (corrected[pad] == 0).all() and {0.0, 1.0} <= set(stop[:, 0].tolist())
    assert corrected[1, 0] == 0 and corrected[1, 1] != 0 and not pad[1]
    p = fv.progress_targets(8)
    assert p.shape == (8,) and p.dtype == np.float32 and (p >= 0).all() and (p <= 1).all() and np.array_equal(p, fv.progress_targets(8))
    for name in fv.FLAT_VAL_CASES:
        kind, cfg, T, N = fv.case(name)
        assert cfg.rgb_shape == (128, 128) and cfg.instr_len <= 12
        assert ("_pm_" in name) == bool(getattr(cfg, "progress_monitor", False)) and ("lstm" in name) == (cfg.rnn_type == "LSTM")
        assert (name in fv.FLAT_VAL_GOLDEN) == (cfg.rnn_type == "GRU")


# ---------------------------------------------------------------- FlatValidator
def test_validator_chunks_carries_and_accumulates_like_a_direct_loop():
    name = "flatval_s2s_pm_T3_N2_gru"
    kind, cfg, _, N = fv.case(name)
    orc = fv.oracle(name)
    steps, T_total = N, 3                                        # one time step per chunk: 3 steps -> 3 chunks of N rows
    batches = fv.epoch_batches(name, 2, T_total)
    got = FlatValidator(orc, tbptt_steps=steps, batch_size=N).run(batches)
    assert got["chunks"] == 6 and got["table"].shape == (6, 8)
    assert [c["rows"] for c in orc.calls] == [N] * 6

    # the direct loop: val_epoch (robo_vln_trainer.py:726-813) written out with torch's split
    direct = fv.oracle(name)
    R = cfg.num_recurrent_layers
    terms, carried = [], []
    for obs, prev, masks, corrected, stop in batches:
        h = torch.zeros(R, N, cfg.hidden)
        split = {k: v.split(steps, 0) for k, v in obs.items() if k != "instruction"}
        assert "progress" in split
        for i, (c, s, m) in enumerate(zip(corrected.split(steps, 0), stop.split(steps, 0), masks.split(steps, 0))):
            o = {k: v[i] for k, v in split.items()}
            o["instruction"] = obs["instruction"].repeat(c.shape[0] // N, 1)
            carried.append(h.clone())
            r, h = direct.val_step(o, c, s, h, m)
            terms.append([float(r[0]), float(r[1]), float(r[2])])
    terms = np.asarray(terms, np.float64)
    assert np.isfinite(terms).all() and (terms[:, 2] > 0).all()
    for k, key in enumerate(("action_loss", "stop_loss", "aux_loss")):
        assert got[key] == pytest.approx(terms[:, k].mean(), rel=1e-6)
    assert got["val_loss"] == pytest.approx(terms.sum(1).mean(), rel=1e-6)          # "Val Loss Epoch": the mean over chunks of the sum
    # hidden state: zero at the start of each batch, carried inside it
    for call, h in zip(orc.calls, carried):
        assert torch.equal(call["hidden"], h)
    assert not orc.calls[0]["hidden"].any() and not orc.calls[3]["hidden"].any() and orc.calls[1]["hidden"].any() and orc.calls[5]["hidden"].any()


class _Recorder:
    """A val_step that computes nothing: for the refusal, which must come before any model work."""
    device = "cpu"
    num_recurrent_layers = 1
    cfg = fv.case("flatval_s2s_T4_N2_gru")[1]

    def __init__(self):
        self.n = 0

    def val_step(self, observations, corrected_actions, oracle_stop, hidden, masks, result=None, return_outputs=False):
        result.copy_(torch.tensor([0.5, 0.25, 0.125, 2, 0, 0, 0, 0]))
        self.n += 1
        return result, hidden


def _label_batch(rows):
    obs = {"rgb": torch.zeros(rows, 1), "depth": torch.zeros(rows, 1), "instruction": torch.zeros(1, 5)}
    return obs, torch.zeros(rows, 2), torch.ones(rows, 2), torch.zeros(rows, 2), torch.zeros(rows, 1)


def test_validator_refuses_a_ragged_chunk():
    rec = _Recorder()
    with pytest.raises(ValueError, match=r"state_encoder\.py:96.*view"):
        FlatValidator(rec, tbptt_steps=4, batch_size=2).run([_label_batch(7)])          # chunks of 4 and 3 rows
    assert rec.n == 0
    with pytest.raises(ValueError, match="no batches"):
        FlatValidator(rec, tbptt_steps=4, batch_size=2).run([])
    ok = FlatValidator(_Recorder(), tbptt_steps=4, batch_size=2).run([_label_batch(8), _label_batch(4)])
    assert ok["chunks"] == 3 and ok["action_loss"] == 0.5 and ok["stop_loss"] == 0.25 and ok["aux_loss"] == 0.125 and ok["val_loss"] == 0.875
