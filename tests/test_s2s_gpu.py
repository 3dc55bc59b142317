"""Seq2SeqNet flat baseline on the GPU through the C ABI: parity against the goldens captured from the imported reference
(tests/golden/s2s_*.npz), the final-state instruction scan against torch's own nn.LSTM / nn.GRU, a large batch against the CPU restatement
(tests/s2s_ref.py), and the path's invariants (sequence path = single steps, graph replay, run-to-run bits, one instruction for B frames)."""
import os

import numpy as np
import pytest
import torch

from oracle import cases
from robo_vln_amd import synth
from robo_vln_amd.config import S2SConfig
from tests import s2s_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"fp32": 1e-3, "fp16": 1e-2}           # the project's standing tolerance on the outputs (tests/test_cma_gpu.py)
HID = {"fp32": 1e-4, "fp16": 1e-2}           # ... and on the final hidden state (relative L2)
SMALL = dict(rgb_hw=128, depth_hw=128, depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN")     # cheap encoders where the test is about the text side


def _net(cfg, sd, B, prec, graph=False):
    from robo_vln_amd.seq2seq import S2SEngine, Seq2SeqNet
    return Seq2SeqNet(S2SEngine(cfg, sd, max_batch=B, precision=prec, graph=graph))


def _t(obs):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in obs.items()}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(s2s_ref.S2S_CASES))
def test_s2s_matches_reference_golden(name, prec):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, B, T, n_instr = s2s_ref.case_config(name)
    net = _net(cfg, synth.make_s2s_weights(cfg, s2s_ref.SEED), B, prec)
    assert net.num_recurrent_layers == cfg.num_recurrent_layers and net.output_size == cfg.hidden and not net.is_blind
    hid = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden, device="cuda")
    for t in range(T):
        obs = _t(synth.make_s2s_observations(cfg, B, step=t, seed=s2s_ref.SEED, n_instr=n_instr))
        net.engine.enable_taps(t == 0 and prec == "fp32")
        out, stop, hid = net((obs, hid, torch.zeros(B, 1), torch.from_numpy(cases.step_masks(B, t))))
        assert "instruction" in obs                                    # seq2seq.py:150-151: not deleted
        torch.cuda.synchronize()
        e_out, e_stop = np.abs(out.cpu().numpy() - gold["out"][t]).max(), np.abs(stop.cpu().numpy() - gold["stop"][t]).max()
        print(f"{name} [{prec}] step {t}: out {e_out:.3e} stop {e_stop:.3e}")
        assert e_out <= TOL[prec] and e_stop <= TOL[prec], (name, t)
        if cfg.progress_monitor:
            e_p = np.abs(net.progress_hat.cpu().numpy() - gold["progress"][t]).max()
            print(f"   progress {e_p:.3e}")
            assert e_p <= TOL[prec]
        else:
            assert net.progress_hat is None
        if t == 0 and prec == "fp32":
            ins = net.engine.get_tap("s2s.instruction")
            ref = np.broadcast_to(gold["tap.instruction"], ins.shape)                     # (1, H) for the one-instruction case
            e_i = np.abs(ins - (0 if cfg.ablate_instruction else ref)).max()
            e_x = np.abs(net.engine.get_tap("s2s.rnn_in")[:, :gold["tap.rnn_in"].shape[1]] - gold["tap.rnn_in"]).max()
            print(f"   taps: instruction {e_i:.3e} rnn_in {e_x:.3e}")
            assert e_i <= 1e-5 and e_x <= TOL[prec]
    rel = np.linalg.norm(hid.cpu().numpy() - gold["hidden"]) / max(1e-12, np.linalg.norm(gold["hidden"]))
    print(f"{name} [{prec}] hidden rel {rel:.3e}")
    assert rel <= HID[prec], rel
    net.engine.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", list(s2s_ref.S2S_SEQ_CASES))
def test_s2s_seq_forward_matches_reference_golden(name, prec):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, T, N = s2s_ref.seq_case(name)
    net = _net(cfg, synth.make_s2s_weights(cfg, s2s_ref.SEED), T * N, prec)
    out, stop, hid = net.seq_forward((_t(s2s_ref.seq_observations(cfg, T, N)), torch.from_numpy(gold["h0"]), None, torch.from_numpy(cases.seq_masks(T, N))), T, N)
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy() - gold["out"]).max() <= TOL[prec]
    assert np.abs(stop.cpu().numpy() - gold["stop"]).max() <= TOL[prec]
    rel = np.linalg.norm(hid.cpu().numpy() - gold["hidden"]) / np.linalg.norm(gold["hidden"])
    assert rel <= HID[prec], rel
    net.engine.close()


def _spread_ids(cfg, B, L):
    """(B, L) ids with lengths spread over 1..L, both ends included."""
    lens = np.linspace(1, L, B).round().astype(np.int64)
    lens[0], lens[-1] = 1, L
    ids = synth.randint("obs/s2s_spread", B * L, 1, cfg.vocab_size, 5).reshape(B, L)
    for b in range(B):
        ids[b, lens[b]:] = 0
    return ids, lens


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_s2s_instruction_tap_vs_torch_final_state(rnn):
    """The final-state scan at B = 64, L = 80, lengths 1..80, against torch's own nn.LSTM / nn.GRU over the packed sequence (the module the
    reference's InstructionEncoder wraps, instruction_encoder.py:42-47,:83-90); two calls give the same bits."""
    B, L = 64, 80
    cfg = S2SConfig(instr_len=L, instr_rnn=rnn, **SMALL).validate()
    sd = synth.make_s2s_weights(cfg, 2)
    net = _net(cfg, sd, B, "fp32")
    ids, lens = _spread_ids(cfg, B, L)
    obs = _t(synth.make_s2s_observations(cfg, B, seed=2))
    obs["instruction"] = torch.from_numpy(ids)
    net.engine.enable_taps(True)
    hid = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden, device="cuda")
    got = []
    for _ in range(2):
        net((obs, hid, None, torch.zeros(B)))
        torch.cuda.synchronize()
        got.append(net.engine.get_tap("s2s.instruction").copy())
    mod = getattr(torch.nn, rnn)(cfg.embedding_size, cfg.instr_hidden, batch_first=True)
    p = "instruction_encoder.encoder_rnn."
    mod.load_state_dict({k: torch.from_numpy(sd[p + k]) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
    emb = torch.from_numpy(sd["instruction_encoder.embedding_layer.weight"])[torch.from_numpy(ids)]
    with torch.no_grad():
        _, fin = mod(torch.nn.utils.rnn.pack_padded_sequence(emb, torch.from_numpy(lens), batch_first=True, enforce_sorted=False))
    ref = (fin[0] if rnn == "LSTM" else fin).squeeze(0).numpy()
    err = np.abs(got[0] - ref).max()
    print(f"s2s.instruction [{rnn}] B={B} L={L}: max-abs vs torch {err:.3e}")
    assert got[0].shape == (B, cfg.instr_hidden) and err <= 1e-5
    assert np.array_equal(got[0], got[1])
    net.engine.close()


_B64 = {}


def _b64_reference():
    """B = 64 at 128 x 128 with both ResNet encoders, three steps with an episode reset, uint8 frames: the CPU restatement, computed once."""
    if not _B64:
        cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=24, progress_monitor=True).validate()
        sd = synth.make_s2s_weights(cfg, 3)
        orc = s2s_ref.S2SOracle(cfg, sd)
        hid = torch.zeros(cfg.num_recurrent_layers, 64, cfg.hidden)
        steps = []
        for t in range(3):
            obs = synth.make_s2s_observations(cfg, 64, step=t, seed=3, rgb_uint8=True)
            out, stop, prog, hid = orc.forward(obs, hid, cases.step_masks(64, t))
            steps.append((out, stop, prog))
        _B64.update(cfg=cfg, sd=sd, steps=steps, hid=hid)
    return _B64


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_s2s_batch64_vs_restatement(prec):
    r = _b64_reference()
    cfg, B = r["cfg"], 64
    net = _net(cfg, r["sd"], B, prec)
    hid = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden, device="cuda")
    for t in range(3):
        obs = _t(synth.make_s2s_observations(cfg, B, step=t, seed=3, rgb_uint8=True))
        out, stop, hid = net((obs, hid, None, torch.from_numpy(cases.step_masks(B, t))))
        torch.cuda.synchronize()
        o2, s2, p2 = r["steps"][t]
        errs = [(out.cpu() - o2).abs().max().item(), (stop.cpu() - s2).abs().max().item(), (net.progress_hat.cpu() - p2).abs().max().item()]
        print(f"B=64 [{prec}] step {t}: out {errs[0]:.3e} stop {errs[1]:.3e} progress {errs[2]:.3e}")
        assert max(errs) <= TOL[prec]
    rel = (hid.cpu() - r["hid"]).norm().item() / r["hid"].norm().item()
    assert rel <= HID[prec], rel
    assert net.engine.nonfinite_steps() == 0
    net.engine.close()


@pytest.mark.parametrize("rnn_type", ["LSTM", "GRU"])
def test_s2s_seq_forward_equals_single_steps(rnn_type):
    """seq_forward over T*N frames = T single steps of the SAME engine on the N frames of each step, state carried.  Bound: both paths run the
    same fp32 kernels, but the encoders see T*N rows instead of N, and the GEMM tile / split-K choice (hence the f32 summation order) depends on
    the row count: 2e-5, the bound tests/test_cma_gpu.py::test_cma_batch_split_consistency holds a batch against its sub-batches to."""
    T, N = 4, 3
    cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, rnn_type=rnn_type, progress_monitor=True).validate()
    net = _net(cfg, synth.make_s2s_weights(cfg, 4), T * N, "fp32")
    obs = s2s_ref.seq_observations(cfg, T, N)
    m = cases.seq_masks(T, N)
    h0 = s2s_ref.seq_h0(cfg, N)
    out, stop, hid = net.seq_forward((_t(obs), h0, None, torch.from_numpy(m)), T, N)
    prog = net.progress_hat.clone()
    h = h0.cuda()
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        o, s, h = net(({k: torch.from_numpy(np.ascontiguousarray(v[sl])) for k, v in obs.items()}, h, None, torch.from_numpy(m[sl])))
        torch.cuda.synchronize()
        assert (out[sl] - o).abs().max().item() <= 2e-5 and (stop[sl] - s).abs().max().item() <= 2e-5
        assert (prog[sl] - net.progress_hat).abs().max().item() <= 2e-5
    assert (hid - h).abs().max().item() <= 2e-5
    net.engine.close()


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_s2s_hipgraph_replay_equals_eager(rnn):
    """Engine graph mode: the first call of a key runs eagerly, the second is captured, later ones replay -- every call's outputs equal an
    eager engine's bit for bit, the first (eager) one included."""
    from robo_vln_amd.seq2seq import S2SEngine
    cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=20, instr_rnn=rnn, progress_monitor=True).validate()
    B = 2
    sd = synth.make_s2s_weights(cfg, s2s_ref.SEED)
    eager = S2SEngine(cfg, sd, max_batch=B, precision="fp16")
    graph = S2SEngine(cfg, sd, max_batch=B, precision="fp16", graph=True)
    he = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden, device="cuda")
    hg = he.clone()
    for t in range(5):
        obs = {k: v.cuda() for k, v in _t(synth.make_s2s_observations(cfg, B, step=t % 3, seed=s2s_ref.SEED)).items()}
        m = torch.from_numpy(cases.step_masks(B, t % 3)).cuda()
        oe, se, pe, he = eager.forward(obs, he, m)
        og, sg, pg, hg = graph.forward(obs, hg, m)
        torch.cuda.synchronize()
        assert torch.equal(oe, og) and torch.equal(se, sg) and torch.equal(pe, pg) and torch.equal(he, hg), t
        hg = hg.clone()
    assert graph.query(7) >= 3        # HCM_GRAPH_LAUNCHES: steps served by graph replay
    eager.close()
    graph.close()


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_s2s_one_instruction_equals_repeated_rows_bitwise(rnn):
    """B_instr = 1 (one sample scanned, the vector written to all B rows) gives the bits of the same instruction repeated B times."""
    from robo_vln_amd.seq2seq import S2SEngine
    B = 5
    cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=16, instr_rnn=rnn).validate()
    eng = S2SEngine(cfg, synth.make_s2s_weights(cfg, 6), max_batch=B, precision="fp16")
    obs = {k: v.cuda() for k, v in _t(synth.make_s2s_observations(cfg, B, step=1, seed=6, n_instr=1)).items()}
    assert obs["instruction"].shape == (1, 16)
    h = ((torch.rand(cfg.num_recurrent_layers, B, cfg.hidden, generator=torch.Generator().manual_seed(9)) - 0.5) * 0.2).cuda()
    m = torch.ones(B, device="cuda")
    one = [t.clone() for t in eng.forward(obs, h, m) if t is not None]
    rep = dict(obs, instruction=obs["instruction"].expand(B, 16).contiguous())
    many = [t.clone() for t in eng.forward(rep, h, m) if t is not None]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(one, many))
    eng.close()


def test_s2s_rejects_bad_input():
    from robo_vln_amd.seq2seq import S2SEngine
    cfg = S2SConfig(instr_len=12, **SMALL).validate()
    sd = synth.make_s2s_weights(cfg, s2s_ref.SEED)
    bad = dict(sd)
    bad.pop("sub_goal_linear.bias")
    with pytest.raises(KeyError):
        S2SEngine(cfg, bad, max_batch=2, precision="fp32")
    eng = S2SEngine(cfg, sd, max_batch=4, precision="fp32")
    obs = _t(synth.make_s2s_observations(cfg, 4))
    with pytest.raises(ValueError):
        eng.forward(obs, torch.zeros(1, 4, cfg.hidden), torch.zeros(4))                   # LSTM: R = 2
    with pytest.raises(ValueError):
        eng.forward(dict(obs, instruction=obs["instruction"][:2]), torch.zeros(2, 4, cfg.hidden), torch.zeros(4))     # 2 instructions, 4 frames
    # hcm_s2s_forward_seq: T*N beyond max_batch = 4 is refused before anything is launched, the product taken in 64 bits (2^16 * 2^16 wraps to 0 in 32)
    import ctypes as C
    from robo_vln_amd import _lib
    lib = _lib.lib()
    buf = torch.full((64,), 7.0, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    for T, N in ((3, 2), (1 << 16, 1 << 16)):
        assert lib.hcm_s2s_forward_seq(eng._h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, T, N, 1, 12, p, p, p, p, None, p, None) == -1, (T, N)
        assert b"max_batch" in lib.hcm_last_error(eng._h), (T, N)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    eng.close()
