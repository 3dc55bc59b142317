"""CMANet sequence forward (hcm_cma_forward_seq) on the GPU through the C ABI: parity against the goldens captured from the imported reference
(tests/golden/cma_seq_*.npz) and, for LSTM state encoders, against the CPU restatement; the one-launch-per-step scan (hcm_op_state_scan)
against torch's own cells; and the call's invariants -- sequence = single steps, T = 1, aliasing, run-to-run bits, the overflow guard, argument
errors.  128 x 128 frames, T*N <= 12; the engines are built once per module (max_batch 12)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import hcm_oracle
from robo_vln_amd import _lib, synth
from robo_vln_amd.config import HCMConfig
from tests import cma_seq_cases as cs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"fp32": 1e-3, "fp16": 1e-2}           # the project's standing tolerance on the outputs (tests/test_cma_gpu.py, tests/test_s2s_gpu.py)
HID = {"fp32": 1e-4, "fp16": 1e-2}           # ... and on the final hidden state (relative L2)
MAXB = 12
LSTM = "cma_seq_T4_N3_lstm"
GRU = "cma_seq_T4_N2_L12"

_ENG, _SD, _ORC = {}, {}, {}


def _sd(name):
    if name not in _SD:
        _SD[name] = synth.make_cma_weights(cs.seq_case(name)[0], cs.SEED)
    return _SD[name]


def _net(name, prec):
    from robo_vln_amd.cma import CMAEngine, CMANet
    if (name, prec) not in _ENG:
        _ENG[name, prec] = CMANet(CMAEngine(cs.seq_case(name)[0], _sd(name), max_batch=MAXB, precision=prec))
    return _ENG[name, prec]


def _t(obs):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in obs.items()}


def _inputs(name, T, N):
    cfg = cs.seq_case(name)[0]
    return cs.seq_observations(cfg, T, N), cs.seq_masks(T, N), cs.seq_h0(cfg, N)


def _check(tag, got, ref, prec):
    out, stop, hid = (x.cpu().numpy() for x in got)
    e_o, e_s = np.abs(out - ref[0]).max(), np.abs(stop - ref[1]).max()
    rel = np.linalg.norm(hid - ref[2]) / max(1e-12, np.linalg.norm(ref[2]))
    print(f"{tag} [{prec}]: out {e_o:.3e} stop {e_s:.3e} hidden rel {rel:.3e}")
    assert e_o <= TOL[prec] and e_s <= TOL[prec], tag
    assert rel <= HID[prec], (tag, rel)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(cs.CMA_SEQ_CASES))
def test_cma_seq_matches_reference_golden(name, prec):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, T, N = cs.seq_case(name)
    net = _net(name, prec)
    obs, m, _ = _inputs(name, T, N)
    obs = _t(obs)
    got = net.seq_forward((obs, torch.from_numpy(gold["h0"]), None, torch.from_numpy(m)), T, N)
    assert "instruction" not in obs                                # cma.py:228
    torch.cuda.synchronize()
    assert got[0].shape == (T * N, cfg.num_actions) and got[1].shape == (T * N, 1) and got[2].shape == (cfg.num_recurrent_layers, N, cfg.hidden)
    _check(name, got, (gold["out"], gold["stop"], gold["hidden"]), prec)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_cma_seq_lstm_vs_restatement(prec):
    cfg, T, N = cs.seq_case(LSTM)
    obs, m, h0 = _inputs(LSTM, T, N)
    if LSTM not in _ORC:
        _ORC[LSTM] = [x.numpy() for x in hcm_oracle.CMAOracle(cfg, _sd(LSTM)).forward(obs, h0, m)]
    net = _net(LSTM, prec)
    assert net.num_recurrent_layers == 4
    got = net.seq_forward((_t(obs), h0, None, torch.from_numpy(m)), T, N)
    torch.cuda.synchronize()
    _check(LSTM, got, _ORC[LSTM], prec)


@pytest.mark.parametrize("name", [LSTM, GRU])
def test_cma_seq_forward_equals_single_steps(name):
    """forward_seq over T*N frames = T single forward calls of the SAME engine with the state carried; masks with a continuing episode at
    t = 0 and mid-sequence resets.  Bound 2e-5: the bound of test_s2s_seq_forward_equals_single_steps / test_cma_batch_split_consistency (the
    same fp32 kernels, but the GEMM tile / split-K choice depends on the row count, and the scan sums h . W_hh in its own fixed order)."""
    T, N = 4, 3
    net = _net(name, "fp32")
    obs, m, h0 = _inputs(name, T, N)
    assert m.reshape(T, N)[0].max() == 1 and (m.reshape(T, N)[1:] == 0).any()
    out, stop, hid = net.engine.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)
    h = h0.cuda()
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        o, s, h = net.engine.forward({k: torch.from_numpy(np.ascontiguousarray(v[sl])) for k, v in obs.items()}, h, torch.from_numpy(m[sl]))
        torch.cuda.synchronize()
        e_o, e_s = (out[sl] - o).abs().max().item(), (stop[sl] - s).abs().max().item()
        print(f"{name} step {t}: out {e_o:.3e} stop {e_s:.3e}")
        assert e_o <= 2e-5 and e_s <= 2e-5, t
    e_h = (hid - h).abs().max().item()
    print(f"{name}: hidden {e_h:.3e}")
    assert e_h <= 2e-5


@pytest.mark.parametrize("rnn_type", ["LSTM", "GRU"])
def test_cma_seq_other_hidden_size_takes_the_per_step_launches(rnn_type):
    """STATE_ENCODER.hidden_size = 1024 is not one of the scan kernel's sizes: the call falls back to the per-step launches of the single-step
    path and still equals T single steps (same bound as above)."""
    from robo_vln_amd.cma import CMAEngine
    from robo_vln_amd.config import CMAConfig
    T, N = 3, 2
    cfg = CMAConfig(rgb_hw=128, depth_hw=128, instr_len=9, hidden=1024, rnn_type=rnn_type).validate()
    eng = CMAEngine(cfg, synth.make_cma_weights(cfg, 5), max_batch=T * N, precision="fp32")
    obs, m, h0 = cs.seq_observations(cfg, T, N), cs.seq_masks(T, N), cs.seq_h0(cfg, N)
    out, stop, hid = eng.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)
    h = h0.cuda()
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        o, s, h = eng.forward({k: torch.from_numpy(np.ascontiguousarray(v[sl])) for k, v in obs.items()}, h, torch.from_numpy(m[sl]))
        torch.cuda.synchronize()
        e_o, e_s = (out[sl] - o).abs().max().item(), (stop[sl] - s).abs().max().item()
        print(f"hidden 1024 [{rnn_type}] step {t}: out {e_o:.3e} stop {e_s:.3e}")
        assert e_o <= 2e-5 and e_s <= 2e-5, t
    e_h = (hid - h).abs().max().item()
    print(f"hidden 1024 [{rnn_type}]: hidden {e_h:.3e}")
    assert e_h <= 2e-5
    eng.close()


def _scan(pre, w_hh, b_hh, h_in, masks, T, N, H, rnn, h_out=None):
    lib = _lib.lib()
    seq = torch.empty(T * N, H, device="cuda")
    h_out = torch.empty_like(h_in) if h_out is None else h_out
    rc = lib.hcm_op_state_scan(pre.data_ptr(), w_hh.data_ptr(), b_hh.data_ptr() if b_hh is not None else None, h_in.data_ptr(), masks.data_ptr(),
                               seq.data_ptr(), h_out.data_ptr(), T, N, H, _lib.HCM_LSTM if rnn == "LSTM" else _lib.HCM_GRU,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return seq, h_out


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("N", [1, 3, 9])
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_state_scan_operator_vs_torch_cell(rnn, N, T):
    _operator_case(rnn, N, T, 512)


def _operator_case(rnn, N, T, H):
    """hcm_op_state_scan against a torch.nn.LSTMCell / GRUCell loop on the CPU with h * mask (and c * mask) in front of every step; 1e-5 is
    the bound the instruction scans are held to against torch (tests/test_s2s_gpu.py).  N = 1, 3: a partial register block; 9: a full block
    plus one sample.  Two runs give the same bits; h_out aliasing h_in gives them again."""
    I = 32
    g = torch.Generator().manual_seed(100 * T + N)
    cell = (torch.nn.LSTMCell if rnn == "LSTM" else torch.nn.GRUCell)(I, H)
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    x = torch.rand(T * N, I, generator=g) * 2 - 1
    R = 2 if rnn == "LSTM" else 1
    h0 = torch.rand(R, N, H, generator=g) - 0.5
    masks = (torch.rand(T, N, generator=g) > 0.4).float()
    masks[0, 0] = 0
    masks[T - 1, N - 1] = 0
    masks[0, N // 2] = 1 if N > 1 else 0
    with torch.no_grad():
        bias = cell.bias_ih + cell.bias_hh if rnn == "LSTM" else cell.bias_ih
        pre = torch.nn.functional.linear(x, cell.weight_ih, bias)
        h, c = h0[0], (h0[1] if rnn == "LSTM" else None)
        ref = []
        for t in range(T):
            mk = masks[t].view(N, 1)
            if rnn == "LSTM":
                h, c = cell(x[t * N:(t + 1) * N], (h * mk, c * mk))
            else:
                h = cell(x[t * N:(t + 1) * N], h * mk)
            ref.append(h)
        ref_seq = torch.cat(ref, 0)
        ref_h = torch.stack([h, c], 0) if rnn == "LSTM" else h[None]
    dev = dict(pre=pre.cuda(), w_hh=cell.weight_hh.detach().cuda(), b_hh=None if rnn == "LSTM" else cell.bias_hh.detach().cuda(), h_in=h0.cuda(),
               masks=masks.reshape(-1).cuda())
    seq, h_out = _scan(T=T, N=N, H=H, rnn=rnn, **dev)
    e_s, e_h = (seq.cpu() - ref_seq).abs().max().item(), (h_out.cpu() - ref_h).abs().max().item()
    print(f"state scan [{rnn}] H={H} T={T} N={N}: seq {e_s:.3e} h_out {e_h:.3e}")
    assert e_s <= 1e-5 and e_h <= 1e-5
    seq2, h_out2 = _scan(T=T, N=N, H=H, rnn=rnn, **dev)
    assert torch.equal(seq, seq2) and torch.equal(h_out, h_out2)
    h_alias = dev["h_in"].clone()
    seq3, _ = _scan(T=T, N=N, H=H, rnn=rnn, h_out=h_alias, **dict(dev, h_in=h_alias))
    assert torch.equal(seq, seq3) and torch.equal(h_out, h_alias)


def test_state_scan_operator_refuses_other_hidden_sizes():
    z = torch.zeros(4 * 96 * 96, device="cuda")
    rc = _lib.lib().hcm_op_state_scan(z.data_ptr(), z.data_ptr(), None, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 2, 96, _lib.HCM_LSTM, None)
    assert rc == -1                                                # HCM_ERR_ARG


def test_cma_seq_T1_is_the_step_call_bitwise():
    net = _net(LSTM, "fp32")
    obs, m, h0 = _inputs(LSTM, 1, 3)
    a = [x.clone() for x in net.engine.forward_seq(_t(obs), h0, torch.from_numpy(m), 1, 3)]
    b = [x.clone() for x in net.engine.forward(_t(obs), h0, torch.from_numpy(m))]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", [LSTM, GRU])
def test_cma_seq_aliasing_and_determinism(name):
    """Two calls give the same bits, and so does h_out aliasing h_in (the C call directly: the engine always hands out a fresh h_out)."""
    T, N = 4, 3
    net = _net(name, "fp32")
    eng = net.engine
    cfg = eng.cfg
    obs, m, h0 = _inputs(name, T, N)
    a = [x.clone() for x in eng.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)]
    b = [x.clone() for x in eng.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    d = {k: v.cuda().contiguous() for k, v in _t(obs).items()}
    h = h0.cuda().contiguous()
    mk = torch.from_numpy(m).cuda()
    out, stop = torch.empty(T * N, cfg.num_actions, device="cuda"), torch.empty(T * N, 1, device="cuda")
    _lib.check(eng._lib.hcm_cma_forward_seq(eng._h, d["rgb"].data_ptr(), _lib.HCM_F32, d["depth"].data_ptr(), d["instruction"].data_ptr(), _lib.HCM_I64,
                                            T, N, d["instruction"].shape[1], h.data_ptr(), mk.data_ptr(), out.data_ptr(), stop.data_ptr(), h.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), eng._h)
    torch.cuda.synchronize()
    assert torch.equal(out, a[0]) and torch.equal(stop, a[1]) and torch.equal(h, a[2])


def test_cma_seq_overflow_guard_counts_like_single_steps():
    """A healthy call leaves the guard alone.  One NaN depth frame at (t0, n0): the sample's state is NaN from t0 on in both encoders (NaN * mask
    stays NaN), and the guard's increase equals what T single-step calls on the same inputs count on a fresh engine -- a (sample, step) pair is
    counted once, not once per unit-slice workgroup.  The other samples' outputs keep their bits."""
    from robo_vln_amd.cma import CMAEngine
    T, N, t0, n0 = 4, 3, 1, 1
    eng = _net(LSTM, "fp32").engine
    obs, m, h0 = _inputs(LSTM, T, N)
    before = eng.nonfinite_steps()
    good = [x.clone() for x in eng.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)]
    assert eng.nonfinite_steps() == before
    bad_obs = dict(obs, depth=obs["depth"].copy())
    bad_obs["depth"][t0 * N + n0] = np.nan
    out, stop, hid = eng.forward_seq(_t(bad_obs), h0, torch.from_numpy(m), T, N)
    inc_seq = eng.nonfinite_steps() - before
    fresh = CMAEngine(eng.cfg, _sd(LSTM), max_batch=N, precision="fp32")
    base = fresh.nonfinite_steps()
    h = h0.cuda()
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        _, _, h = fresh.forward({k: torch.from_numpy(np.ascontiguousarray(v[sl])) for k, v in bad_obs.items()}, h, torch.from_numpy(m[sl]))
    inc_steps = fresh.nonfinite_steps() - base
    fresh.close()
    print(f"overflow guard: sequence call +{inc_seq}, {T} single steps +{inc_steps}")
    assert inc_seq == inc_steps == 2 * (T - t0)                    # both encoders, steps t0 .. T-1 of one sample
    keep = [t * N + n for t in range(T) for n in range(N) if n != n0]
    assert torch.equal(out[keep], good[0][keep]) and torch.equal(stop[keep], good[1][keep])
    others = [n for n in range(N) if n != n0]
    assert torch.equal(hid[:, others], good[2][:, others])
    assert not torch.isfinite(out[t0 * N + n0]).all()


def test_cma_seq_argument_errors():
    net = _net(LSTM, "fp32")
    eng, cfg = net.engine, net.engine.cfg
    T, N = 4, 3
    obs, m, h0 = _inputs(LSTM, T, N)
    big = cs.seq_observations(cfg, 4, 4)                           # T*N = 16 > max_batch = 12: refused by the library
    with pytest.raises(ValueError, match="max_batch"):
        eng.forward_seq(_t(big), cs.seq_h0(cfg, 4), torch.ones(16), 4, 4)
    d = {k: v.cuda().contiguous() for k, v in _t(obs).items()}
    h, mk = h0.cuda().contiguous(), torch.from_numpy(m).cuda()
    out, stop = torch.empty(T * N, cfg.num_actions, device="cuda"), torch.empty(T * N, 1, device="cuda")

    def call(handle, T=T, N=N, L=cfg.instr_len):
        return eng._lib.hcm_cma_forward_seq(handle, d["rgb"].data_ptr(), _lib.HCM_F32, d["depth"].data_ptr(), d["instruction"].data_ptr(), _lib.HCM_I64,
                                            T, N, L, h.data_ptr(), mk.data_ptr(), out.data_ptr(), stop.data_ptr(), h.data_ptr(), None)

    with pytest.raises(ValueError):
        _lib.check(call(eng._h, T=0), eng._h)
    with pytest.raises(ValueError, match="instruction length"):
        _lib.check(call(eng._h, L=cfg.instr_len + 1), eng._h)
    from robo_vln_amd.policy import _to_struct
    st = _to_struct(HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2).validate(), 4, "fp32", True, True)
    other = C.c_void_p()
    assert eng._lib.hcm_create(C.byref(st), C.byref(other)) == 0
    try:
        with pytest.raises(RuntimeError, match="CMANet"):
            _lib.check(call(other), other)
    finally:
        eng._lib.hcm_destroy(other)
    good = eng.forward_seq(_t(obs), h0, torch.from_numpy(m), T, N)  # the engine still works
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in good)
