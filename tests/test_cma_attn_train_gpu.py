"""CMANet's differentiable attention on the GPU: robo_vln_amd.train.attn1q (hcm_op_attn1q_train + hcm_op_attn1q_bwd) against float64 on the CPU on
the cases of tests/cma_attn_cases.py, the raw C ABI (determinism, sentinel pre-fill with guard elements, NULL d_x, B = 0, a non-default stream),
the refusals, the train.CMANet module against its own float64 CPU path (one chunk and one single step), an optimizer step between two calls, and
the module from CMAEngine.encode_features against the goldens captured from the reference.

Bound, the project's rule (vla_train_cases.rel): per tensor max|g - g64| / max|g64| <= 1e-5, a reference that is identically zero matched exactly."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from robo_vln_amd import _lib, synth, train
from robo_vln_amd.config import CMAConfig
from tests import cma_attn_cases as ac
from tests import cma_seq_cases as cs
from tests.vla_train_cases import rel

pytestmark = pytest.mark.gpu

BOUND = 1e-5
GUARD = 64
NAN = float("nan")
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _cu(t):
    return None if t is None else t.cuda()


class _Buf:
    """n floats pre-filled with NaN, with GUARD more behind them"""

    def __init__(self, n):
        self.n = n
        self.all = torch.full((n + GUARD,), NAN, device="cuda")
        self.t = self.all[:n]

    def untouched(self):
        return bool(torch.isnan(self.all).all())

    def guard_ok(self):
        return bool(torch.isnan(self.all[self.n:]).all())

    def written(self):
        return bool(torch.isfinite(self.t).all())


def _dims(case):
    layout, B, C0, Ce, I = case[:5]
    return layout, B, C0, Ce, I


def _raw_forward(t, case, stream=None, **over):
    """t: dict(qt, x, e) on the device; `over` replaces dims or pointers"""
    layout, B, C0, Ce, I = _dims(case)
    d = dict(layout=layout, B=B, C0=C0, Ce=Ce, I=I, mask_zero=int(case[5]), scale=1.0 / 16.0, work=None)
    o = dict(a=_Buf(B * I), xbar=_Buf(B * (C0 + Ce)))
    ptr = dict(qt=_p(t["qt"]), x=_p(t["x"]), e=_p(t["e"]), a=_p(o["a"].t), xbar=_p(o["xbar"].t))
    for k, v in over.items():
        (ptr if k in ptr else d)[k] = v
    rc = _lib.lib().hcm_op_attn1q_train(ptr["qt"], ptr["x"], ptr["e"], d["layout"], d["mask_zero"], d["scale"], ptr["a"], ptr["xbar"], _p(d["work"]),
                                        d["B"], d["C0"], d["Ce"], d["I"], stream)
    return rc, o


def _raw_backward(t, case, saved_a, cot, want_dx=True, stream=None, **over):
    layout, B, C0, Ce, I = _dims(case)
    d = dict(layout=layout, B=B, C0=C0, Ce=Ce, I=I, scale=1.0 / 16.0)
    o = dict(d_qt=_Buf(B * (C0 + Ce)), d_x=_Buf(B * C0 * I), d_e=_Buf(I * Ce))
    n = _lib.lib().hcm_op_attn1q_work_floats(B, C0, Ce, I)
    work = torch.empty(n, device="cuda") if n else None
    ptr = dict(d_xbar=_p(cot), qt=_p(t["qt"]), x=_p(t["x"]), e=_p(t["e"]), a=_p(saved_a), d_qt=_p(o["d_qt"].t), d_x=_p(o["d_x"].t) if want_dx else None,
               d_e=_p(o["d_e"].t) if Ce else None, work=_p(work))
    for k, v in over.items():
        (ptr if k in ptr else d)[k] = v
    rc = _lib.lib().hcm_op_attn1q_bwd(ptr["d_xbar"], ptr["qt"], ptr["x"], ptr["e"], ptr["a"], d["layout"], d["scale"], ptr["d_qt"], ptr["d_x"],
                                      ptr["d_e"], ptr["work"], d["B"], d["C0"], d["Ce"], d["I"], stream)
    return rc, o


def _dev(case):
    c = ac.case(*case)
    return c, dict(qt=c["qt"].cuda(), x=c["x"].cuda(), e=_cu(c["e"]))


@functools.lru_cache(maxsize=None)
def _gpu(case):
    """the case through the raw forward (a, xbar) and through the autograd function (gradients), once"""
    layout, B, C0, Ce, I, mask_zero, want_dx, _ = case
    c, t = _dev(case)
    rc, fw = _raw_forward(t, case)
    assert rc == 0, _lib.last_error()
    leaves = dict(qt=t["qt"].clone().requires_grad_(), x=t["x"].clone().requires_grad_(want_dx), e=None if Ce == 0 else t["e"].clone().requires_grad_())
    y = train.attn1q(leaves["qt"], leaves["x"], leaves["e"], mask_zero, c["scale"], layout)
    names = [n for n, k in zip(ac.NAMES, ("qt", "x", "e")) if leaves[k] is not None and leaves[k].requires_grad]
    grads = torch.autograd.grad(y, [leaves[k] for k in ("qt", "x", "e") if leaves[k] is not None and leaves[k].requires_grad], c["cot"].cuda())
    torch.cuda.synchronize()
    assert all(b.guard_ok() and b.written() for b in fw.values())
    return {k: b.t.cpu() for k, b in fw.items()}, y.detach().cpu(), dict(zip(names, [g.cpu() for g in grads]))


@pytest.mark.parametrize("case", ac.ALL_CASES)
def test_forward_matches_float64(case):
    layout, B, C0, Ce, I = _dims(case)
    c = ac.case(*case)
    fw, y, _ = _gpu(case)
    assert torch.equal(fw["xbar"].reshape(B, C0 + Ce), y)                 # the autograd function returns the raw call's bits
    worst = dict(a=rel(fw["a"].reshape(B, I), c["a64"], f"{case} a"), xbar=rel(y, c["out64"], f"{case} xbar"))
    assert max(worst.values()) <= BOUND, worst
    full = (c["out64"] == 0).all(1)                                       # fully masked samples: uniform weights, exact zeros
    assert (y[full] == 0).all() and (fw["a"].reshape(B, I)[full] == 1.0 / I).all()
    if I == 1:
        assert (fw["a"] == 1).all()


@pytest.mark.parametrize("case", ac.ALL_CASES)
def test_gradients_match_float64_autograd(case):
    c = ac.case(*case)
    _, _, grads = _gpu(case)
    assert ("d_x" in grads) == case[6] and ("d_e" in grads) == (case[3] > 0)
    assert all(torch.isfinite(g).all() for g in grads.values())
    worst = {n: rel(g, c["ref"][n], f"{case} {n}") for n, g in grads.items()}
    assert max(worst.values()) <= BOUND, worst


# ---- raw C ABI ----
RAW_CASES = [ac.CASES[1], ac.CASES[5], ac.CASES[6], ac.CASES[7], ac.CASES[10]] + ac.EXTRA_CASES


@pytest.mark.parametrize("case", RAW_CASES)
def test_raw_abi_bitwise_fully_written_and_guards(case):
    """two forward and two backward calls on the same inputs are bitwise equal; every output is fully written and the GUARD elements behind each
    buffer keep the sentinel; with a NULL d_x, d_qt and d_e carry the bits of the call that computes it and d_x is not touched"""
    layout, B, C0, Ce, I = _dims(case)
    c, t = _dev(case)
    cot = c["cot"].cuda()
    rc1, f1 = _raw_forward(t, case)
    rc2, f2 = _raw_forward(t, case)
    assert rc1 == 0 and rc2 == 0
    rc1, b1 = _raw_backward(t, case, f1["a"].t, cot)
    rc2, b2 = _raw_backward(t, case, f2["a"].t, cot)
    rc3, b3 = _raw_backward(t, case, f1["a"].t, cot, want_dx=False)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0, _lib.last_error()
    torch.cuda.synchronize()
    for n in f1:
        assert f1[n].written() and f1[n].guard_ok() and torch.equal(f1[n].t, f2[n].t), n
    for n in b1:
        assert b1[n].written() and b1[n].guard_ok() and torch.equal(b1[n].t, b2[n].t), n
    assert torch.equal(b3["d_qt"].t, b1["d_qt"].t) and torch.equal(b3["d_e"].t, b1["d_e"].t)
    assert b3["d_x"].untouched() and b3["d_qt"].guard_ok() and b3["d_e"].guard_ok()
    ref = c["ref"]
    assert rel(b1["d_x"].t.cpu().reshape(ref["d_x"].shape), ref["d_x"], f"{case} raw d_x") <= BOUND
    assert rel(b1["d_qt"].t.cpu().reshape(ref["d_qt"].shape), ref["d_qt"], f"{case} raw d_qt") <= BOUND
    if Ce:
        assert rel(b1["d_e"].t.cpu().reshape(ref["d_e"].shape), ref["d_e"], f"{case} raw d_e") <= BOUND


def test_zero_samples():
    """B = 0: HCM_OK, the backward writes zeros to d_e, nothing else is touched and the per-sample pointers may be NULL"""
    case = (ac.CM, 0, 128, 64, 16, False, True, 1.0)
    e = torch.rand(16, 64, device="cuda")
    t = dict(qt=None, x=None, e=e)
    rc, fw = _raw_forward(t, case, a=None, xbar=None)
    assert rc == 0
    rc, bw = _raw_backward(t, case, None, None, d_qt=None, d_x=None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert all(b.untouched() for b in fw.values()) and bw["d_qt"].untouched() and bw["d_x"].untouched()
    assert bw["d_e"].guard_ok() and torch.equal(bw["d_e"].t, torch.zeros(16 * 64, device="cuda"))
    assert _lib.lib().hcm_op_attn1q_work_floats(0, 128, 64, 16) == 0


# ---- refusals: an error code or ValueError, and no launch ----
def _nothing_written(*outs):
    torch.cuda.synchronize()
    return all(b.untouched() for o in outs for b in o.values())


REFUSAL_CASE = (ac.CM, 2, 128, 64, 16, False, True, 1.0)
REFUSALS = {
    "I = 0": dict(I=0), "I = 257": dict(I=257), "C above 4096": dict(C0=4096), "Ce % 4": dict(Ce=62), "C0 = 0": dict(C0=0), "B < 0": dict(B=-1),
    "unknown layout": dict(layout=2), "e without Ce": dict(Ce=0), "Ce without e": dict(e=None), "NULL qt": dict(qt=None), "NULL x": dict(x=None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_return_err_arg_with_a_message_and_write_nothing(what):
    c, t = _dev(REFUSAL_CASE)
    cot = c["cot"].cuda()
    rc, ok = _raw_forward(t, REFUSAL_CASE)
    assert rc == 0
    over = REFUSALS[what]
    rc, fw = _raw_forward(t, REFUSAL_CASE, **over)
    assert rc == -1 and _lib.last_error().startswith("attn1q:"), what
    rc, bw = _raw_backward(t, REFUSAL_CASE, ok["a"].t, cot, **over)
    assert rc == -1 and _lib.last_error().startswith("attn1q:"), what
    assert _nothing_written(fw, bw)
    if what in ("I = 0", "I = 257", "C above 4096", "Ce % 4", "C0 = 0", "B < 0"):
        d = {**dict(B=2, C0=128, Ce=64, I=16), **over}
        assert _lib.lib().hcm_op_attn1q_work_floats(d["B"], d["C0"], d["Ce"], d["I"]) == 0


def test_null_outputs_misalignment_and_work_overlap_are_refused():
    c, t = _dev(REFUSAL_CASE)
    layout, B, C0, Ce, I = _dims(REFUSAL_CASE)
    cot = c["cot"].cuda()
    rc, ok = _raw_forward(t, REFUSAL_CASE)
    assert rc == 0
    outs = []
    for k in ("a", "xbar"):
        rc, fw = _raw_forward(t, REFUSAL_CASE, **{k: None})
        assert rc == -1, k
        outs.append(fw)
    for k in ("d_xbar", "a", "d_qt", "d_e", "work"):
        rc, bw = _raw_backward(t, REFUSAL_CASE, ok["a"].t, cot, **{k: None})
        assert rc == -1, k
        outs.append(bw)
    rc, bw = _raw_backward(dict(t, e=None), (ac.CM, B, C0, 0, I, False, True, 1.0), ok["a"].t, cot, d_e=_p(torch.empty(64, device="cuda")))
    assert rc == -1                                                       # d_e without e
    outs.append(bw)
    off = lambda src: torch.cat([src.reshape(-1), src.new_zeros(4)])[1:1 + src.numel()]     # four bytes off a 16-byte boundary
    for k in ("qt", "x", "e"):
        rc, fw = _raw_forward(t, REFUSAL_CASE, **{k: _p(off(t[k]))})
        assert rc == -1 and "aligned" in _lib.last_error(), k
        outs.append(fw)
    for k, src in (("d_xbar", cot), ("a", ok["a"].t), ("d_qt", torch.empty(B * (C0 + Ce), device="cuda")), ("d_x", torch.empty(B * C0 * I, device="cuda")),
                   ("d_e", torch.empty(I * Ce, device="cuda"))):
        rc, bw = _raw_backward(t, REFUSAL_CASE, ok["a"].t, cot, **{k: _p(off(src))})
        assert rc == -1 and "aligned" in _lib.last_error(), k
        outs.append(bw)
    n = _lib.lib().hcm_op_attn1q_work_floats(B, C0, Ce, I)
    assert n == B * I * Ce
    big = torch.full((n + B * C0 * I,), NAN, device="cuda")
    inside = big[n - 4:]                                                  # starts in the work buffer's last 16 bytes
    for k in ("a", "xbar"):
        rc, fw = _raw_forward(t, REFUSAL_CASE, work=big, **{k: _p(inside)})
        assert rc == -1 and "overlaps" in _lib.last_error(), k
        outs.append(fw)
    for k in ("d_qt", "d_x", "d_e"):
        rc, bw = _raw_backward(t, REFUSAL_CASE, ok["a"].t, cot, work=_p(big), **{k: _p(inside)})
        assert rc == -1 and "overlaps" in _lib.last_error(), k
        outs.append(bw)
    assert _nothing_written(*outs) and torch.isnan(big).all()


def test_python_level_refusals():
    c, t = _dev(REFUSAL_CASE)
    with pytest.raises(ValueError):
        train.attn1q(c["qt"], c["x"], c["e"], False, c["scale"], ac.CM)            # host tensors
    with pytest.raises(ValueError):
        train.attn1q(t["qt"], c["x"], t["e"], False, c["scale"], ac.CM)
    with pytest.raises(ValueError):
        train.attn1q(t["qt"], t["x"], c["e"], False, c["scale"], ac.CM)
    with pytest.raises(ValueError):
        train.attn1q(t["qt"], t["x"], t["e"][:, :62], False, c["scale"], ac.CM)    # Ce % 4
    with pytest.raises(ValueError):
        train.attn1q(t["qt"], t["x"], None, False, c["scale"], ac.CM)              # qt's width against C0 + Ce
    with pytest.raises(ValueError):
        train.attn1q(torch.zeros(1, 8, device="cuda"), torch.zeros(1, 257, 8, device="cuda"), None, False, 1.0, ac.TM)
    with pytest.raises(ValueError):
        train.attn1q(t["qt"], t["x"], t["e"], False, c["scale"], 2)


# ---- non-default stream ----
@pytest.mark.parametrize("case", [ac.CASES[2], ac.EXTRA_CASES[0]])
def test_non_default_stream_bitwise(case):
    layout, B, C0, Ce, I, mask_zero, want_dx, _ = case
    c, t = _dev(case)
    fw0, y0, grads0 = _gpu(case)
    s = torch.cuda.Stream()
    leaves = [t[k].clone().requires_grad_() for k in ("qt", "x", "e") if t[k] is not None]
    cot = c["cot"].cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rc, fw = _raw_forward(t, case, stream=C.c_void_p(s.cuda_stream))
        y = train.attn1q(leaves[0], leaves[1], leaves[2] if Ce else None, mask_zero, c["scale"], layout)
        grads = torch.autograd.grad(y, leaves, cot)
    s.synchronize()
    assert rc == 0 and torch.equal(fw["a"].t.cpu(), fw0["a"]) and torch.equal(y.detach().cpu(), y0)
    for n, gt in zip(ac.NAMES, grads):
        assert torch.equal(gt.cpu(), grads0[n]), n


# ---- module ----
MOD_CFG = dict(rgb_hw=128, depth_hw=128, instr_len=9)


def _module_pair(name):
    """train.CMANet in float64 on the CPU and in float32 on the device with one state dict, and the case's inputs"""
    if name == "chunk":
        cfg, T, N = CMAConfig(**MOD_CFG).validate(), 3, 2
    else:
        cfg, T, N = CMAConfig(rnn_type="GRU", instr_rnn="GRU", bidirectional=False, **MOD_CFG).validate(), 1, 3
    sd = synth.make_cma_weights(cfg, cs.SEED)
    g = torch.Generator().manual_seed(23)
    s = cfg.depth_final_spatial()
    obs = dict(instruction=cs.seq_observations(cfg, T, N)["instruction"],
               rgb_features=torch.relu(torch.rand(T * N, 2048, 4, 4, generator=g) * 2 - 0.5).numpy(),
               depth_features=torch.relu(torch.rand(T * N, cfg.depth_compress_channels(), s, s, generator=g) * 2 - 0.5).numpy())
    m_cpu, m_gpu = train.CMANet(cfg), train.CMANet(cfg)
    m_cpu.load_reference_state_dict(sd)
    m_gpu.load_reference_state_dict(sd)
    cots = (torch.rand(T * N, cfg.num_actions, generator=g) * 2 - 1, torch.rand(T * N, 1, generator=g) * 2 - 1)
    return cfg, m_cpu.double(), m_gpu.cuda(), obs, cs.seq_masks(T, N), cs.seq_h0(cfg, N), cots


def _to64(t):
    return t.double() if t.is_floating_point() else t


def _to_dev(t):
    return t.cuda()


def _assert_grads_close(m_gpu, m_cpu, cfg, what):
    hh = cfg.hidden // 2
    worst = {}
    gc = {n: p.grad for n, p in m_cpu.named_parameters()}
    for n, pg in m_gpu.named_parameters():
        if n.startswith("progress_monitor."):
            assert pg.grad is None and gc[n] is None
            continue
        worst[n] = rel(pg.grad.cpu(), gc[n], f"{what} {n}")
        if n == "text_k.bias":
            assert (pg.grad == 0).all()
        if n in ("rgb_kv.bias", "depth_kv.bias"):
            assert (pg.grad[:hh] == 0).all() and (pg.grad[hh:] != 0).any(), n
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("name", ["chunk", "single_step"])
def test_module_matches_its_cpu_path(name):
    """train.CMANet on the device against its own float64 CPU path: outputs, state and every parameter gradient; the cancelled key biases
    come back as exact zeros"""
    cfg, m_cpu, m_gpu, obs, m, h0, cots = _module_pair(name)
    out_c, stop_c, hid_c = m_cpu(ac.module_batch(obs, h0, m, _to64))
    ((out_c * cots[0].double()).sum() + (stop_c * cots[1].double()).sum()).backward()
    out_g, stop_g, hid_g = m_gpu(ac.module_batch(obs, h0, m, _to_dev))
    ((out_g * cots[0].cuda()).sum() + (stop_g * cots[1].cuda()).sum()).backward()
    torch.cuda.synchronize()
    worst = dict(out=rel(out_g.detach().cpu(), out_c.detach(), f"{name} out"), stop=rel(stop_g.detach().cpu(), stop_c.detach(), f"{name} stop"),
                 hidden=rel(hid_g.detach().cpu(), hid_c.detach(), f"{name} hidden"))
    assert max(worst.values()) <= BOUND, worst
    _assert_grads_close(m_gpu, m_cpu, cfg, name)


def test_adam_step_between_two_calls():
    """Adam (eps 1e-3, lr 1e-3, the loss a mean: the construction of tests/test_embed_train_gpu.py) between two calls: the second forward sees the
    updated weights, nothing is cached; outputs before and after the step match the float64 CPU run"""
    cfg, m_cpu, m_gpu, obs, m, h0, cots = _module_pair("chunk")
    outs = {}
    for name, mod, cv in (("cpu", m_cpu, _to64), ("gpu", m_gpu, _to_dev)):
        opt = torch.optim.Adam([p for n, p in mod.named_parameters() if not n.startswith("progress_monitor.")], lr=1e-3, eps=1e-3)
        outs[name] = []
        for _ in range(2):
            opt.zero_grad()
            out, stop, _ = mod(ac.module_batch(obs, h0, m, cv))
            ((out * cv(cots[0])).mean() + (stop * cv(cots[1])).mean()).backward()
            opt.step()
            outs[name].append(torch.cat([out, stop], 1).detach().cpu().double())
    torch.cuda.synchronize()
    moved = (outs["cpu"][1] - outs["cpu"][0]).abs().max().item()
    off = [(outs["gpu"][i] - outs["cpu"][i]).abs().max().item() / outs["cpu"][i].abs().max().item() for i in range(2)]
    print(f"adam: the step moved the output by {moved:.3e}; device against float64 before / after the step {off[0]:.3e} / {off[1]:.3e} (relative)")
    assert off[0] <= BOUND and off[1] <= BOUND
    assert moved >= 50 * off[1] * outs["cpu"][1].abs().max().item()       # the step's own effect exceeds the error many times: the device saw the new weights


@pytest.mark.parametrize("name", ["cma_seq_T4_N2_L12", "cma_seq_gru_instr_T3_N3_L9"])
def test_module_from_encoded_features_matches_reference_golden(name):
    """frames -> CMAEngine("fp32").encode_features -> train.CMANet in eval mode with the same weights: the golden's out, stop and hidden to 1e-3,
    the project's fp32 parity bound"""
    from robo_vln_amd.cma import CMAEngine
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, T, N = cs.seq_case(name)
    sd = synth.make_cma_weights(cfg, cs.SEED)
    obs = cs.seq_observations(cfg, T, N)
    eng = CMAEngine(cfg, sd, max_batch=T * N, precision="fp32")
    try:
        feats = eng.encode_features({k: torch.from_numpy(np.asarray(v)).cuda() for k, v in obs.items()})
        net = train.CMANet(cfg)
        net.load_reference_state_dict(sd)
        net.cuda().eval()
        with torch.no_grad():
            out, stop, hid = net((dict(feats, instruction=torch.from_numpy(obs["instruction"]).cuda()), torch.from_numpy(gold["h0"]).cuda(), None,
                                  torch.from_numpy(cs.seq_masks(T, N)).cuda().reshape(-1, 1)))
        torch.cuda.synchronize()
    finally:
        eng.close()
    errs = [np.abs(out.cpu().numpy() - gold["out"]).max(), np.abs(stop.cpu().numpy() - gold["stop"]).max(), np.abs(hid.cpu().numpy() - gold["hidden"]).max()]
    print(f"{name}: module from encoded features vs golden out {errs[0]:.3e} stop {errs[1]:.3e} hidden {errs[2]:.3e}")
    assert max(errs) <= 1e-3
