"""CMANet sequence forward without a GPU: the goldens captured from the imported reference (tests/golden/cma_seq_*.npz,
tools/gen_cma_seq_golden.py) against the torch-CPU restatement's sequence branch, the restatement's LSTM sequence branch against its own
single steps (the reference's seq_forward raises for LSTM, so there is no golden), and the C ABI's declaration, binding and argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import hcm_oracle
from robo_vln_amd import _lib, synth
from robo_vln_amd.config import HCMConfig
from robo_vln_amd.cma import _to_struct as cma_struct
from robo_vln_amd.policy import _to_struct
from tests import cma_seq_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", list(cs.CMA_SEQ_CASES))
def test_restatement_matches_reference_golden(name):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, T, N = cs.seq_case(name)
    assert set(gold.files) == {"out", "stop", "hidden", "h0", "meta"}                 # outputs and h0 only: inputs come from the seed
    R = cfg.num_recurrent_layers
    assert gold["out"].shape == (T * N, cfg.num_actions) and gold["stop"].shape == (T * N, 1) and gold["hidden"].shape == (R, N, cfg.hidden)
    h0 = cs.seq_h0(cfg, N)
    assert np.array_equal(gold["h0"], h0.numpy())
    obs = cs.seq_observations(cfg, T, N)
    m = cs.seq_masks(T, N).reshape(T, N)
    lens = (obs["instruction"][:N] != 0).sum(1)
    assert len(set(lens.tolist())) > 1                                                 # instructions of different token counts
    assert (m[0] == 1).any() and np.abs(gold["h0"]).max() > 0 and (m[1:] == 0).any()   # a continuing episode at t = 0 and a reset at t > 0
    out, stop, hid = hcm_oracle.CMAOracle(cfg, synth.make_cma_weights(cfg, cs.SEED)).forward(obs, h0, m.reshape(-1))
    errs = [np.abs(out.numpy() - gold["out"]).max(), np.abs(stop.numpy() - gold["stop"]).max(), np.abs(hid.numpy() - gold["hidden"]).max()]
    print(f"{name}: restatement vs golden out {errs[0]:.3e} stop {errs[1]:.3e} hidden {errs[2]:.3e}")
    assert max(errs) <= 1e-5


@pytest.mark.parametrize("name", list(cs.CMA_SEQ_CASES_ORACLE_ONLY))
def test_restatement_lstm_sequence_equals_single_steps(name):
    """One CPU thread: torch's multi-threaded GroupNorm / convolution kernels split their reductions by the batch they are given, so the depth
    trunk's features of the SAME frame differ by ~2e-5 between a 12-row and a 3-row call (measured: state 3e-6, hidden 5e-6) -- noise of the
    encoders, not of the sequence branch this test pins.  Single-threaded the trunks are row-independent and the two routes agree to 3e-7."""
    cfg, T, N = cs.seq_case(name)
    assert cfg.rnn_type == "LSTM"
    orc = hcm_oracle.CMAOracle(cfg, synth.make_cma_weights(cfg, cs.SEED))
    obs, m, h0 = cs.seq_observations(cfg, T, N), cs.seq_masks(T, N), cs.seq_h0(cfg, N)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out, stop, hid = orc.forward(obs, h0, m)
        h = h0
        for t in range(T):
            sl = slice(t * N, (t + 1) * N)
            o, s, h = orc.forward({k: v[sl] for k, v in obs.items()}, h, m[sl])
            e_o, e_s = (out[sl] - o).abs().max().item(), (stop[sl] - s).abs().max().item()
            print(f"{name} step {t}: out {e_o:.3e} stop {e_s:.3e}")
            assert e_o <= 1e-6 and e_s <= 1e-6, t
    finally:
        torch.set_num_threads(threads)
    e_h = (hid - h).abs().max().item()
    print(f"{name}: hidden {e_h:.3e}")
    assert e_h <= 1e-6


def test_header_declares_and_library_exports_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for sym, n in (("hcm_cma_forward_seq", 15), ("hcm_op_state_scan", 12)):
        m = re.search(r"int %s\(([^;]*)\);" % sym, text)
        assert m, f"include/hcm.h does not declare {sym}"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = _lib.EXPORTS[sym]
        assert res is C.c_int and len(args) == n_args == n, sym
        assert hasattr(_lib.lib(), sym)
    doc = text[text.index("robo_vln_trainer.py:516-518"):text.index("int hcm_cma_forward_seq(")]
    for cite in (":553-555", "state_encoder.py:83-133"):
        assert cite in doc, cite


def test_forward_seq_argument_errors_without_a_device():
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    l = _lib.lib()

    def call(h, T=2, N=2, L=12):
        return l.hcm_cma_forward_seq(h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, T, N, L, p, p, p, p, p, None)

    assert call(None) == -1                                                           # null handle
    cfg, _, _ = cs.seq_case("cma_seq_T4_N2_L12")
    st = cma_struct(cfg, 4, "fp32")
    h = C.c_void_p()
    assert l.hcm_cma_create(C.byref(st), C.byref(h)) == 0, l.hcm_last_error(None)
    try:
        assert call(h, T=0) == -1 and call(h, N=0) == -1
        assert call(h, T=3, N=2) == -1 and b"max_batch" in l.hcm_last_error(h)        # T*N = 6 > 4
        assert call(h, T=1 << 16, N=1 << 16) == -1                                    # (no 32-bit wrap of the product)
        assert call(h) == -2                                                          # well-formed, but the handle is not finalized
    finally:
        l.hcm_destroy(h)
    st2 = _to_struct(HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2).validate(), 4, "fp32", True, True)
    h2 = C.c_void_p()
    assert l.hcm_create(C.byref(st2), C.byref(h2)) == 0
    try:
        assert call(h2) == -2 and b"CMANet" in l.hcm_last_error(h2)                   # not a CMA handle
    finally:
        l.hcm_destroy(h2)
    assert l.hcm_op_state_scan(p, p, None, p, p, p, p, 2, 2, 500, _lib.HCM_LSTM, None) == -1     # a hidden size the kernel does not serve
