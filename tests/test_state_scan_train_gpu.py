"""The differentiable state-encoder scan on the GPU: robo_vln_amd.train.state_scan (hcm_op_state_scan_train + hcm_op_state_scan_bwd) against
float64 CPU autograd through the cell loop, the training forward against hcm_op_state_scan bit for bit, determinism, the RNNStateEncoder
module against its CPU path, an optimizer step between two calls, and a non-default stream.

Gradient bound: per tensor max|g - g64| / max|g64| <= 1e-5, the bound the forward scans are held to against torch (tests/test_cma_seq_gpu.py);
torch's own float32 CPU backward lands at 1e-7 .. 6e-7 on these cases.  Where g64 is identically zero the result must be exactly zero.
The cases and their float64 references live in tests/state_scan_train_cases.py."""
import ctypes as C

import pytest
import torch

from robo_vln_amd import _lib, train
from tests import state_scan_train_cases as sc
from tests.state_scan_train_cases import BOUND, CASES, H, I, NAMES, SHAPES
from tests.state_scan_train_cases import case as _case
from tests.state_scan_train_cases import masks as _masks

pytestmark = pytest.mark.gpu

RAW_SHAPES = SHAPES + [(33, 5), (6, 13)]           # through the C ABI as well: the horizon, and the sample blocks 8 + 5 / 4 + 4 + 4 + 1


def _gpu_grads(rnn, T, N, kind, ih_scale=1.0):
    c = _case(rnn, T, N, kind, ih_scale)
    leaves = [t.cuda().requires_grad_() for t in (c["x"], *c["p"], c["h0"])]
    seq, hid = train.state_scan(*leaves, c["m"].reshape(-1).cuda())
    assert not hid.requires_grad
    grads = torch.autograd.grad(seq, leaves, c["cot"].cuda())
    torch.cuda.synchronize()
    return seq.detach().cpu(), hid.cpu(), dict(zip(NAMES, [t.cpu() for t in grads]))


def _rel(g, g64, what):
    """max|g - g64| / max|g64|, or exactly-zero where the reference is identically zero"""
    scale = g64.abs().max().item()
    if scale == 0:
        worst = g.abs().max().item()
        print(f"{what}: reference identically zero, result max {worst:.3e}")
        assert worst == 0, what
        return 0.0
    e = (g.double() - g64).abs().max().item() / scale
    print(f"{what}: {e:.3e}")
    return e


@pytest.mark.parametrize("T,N,kind", CASES)
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_gradients_match_float64_autograd(rnn, T, N, kind):
    c = _case(rnn, T, N, kind)
    seq, hid, grads = _gpu_grads(rnn, T, N, kind)
    e_s, e_h = (seq.double() - c["seq64"]).abs().max().item(), (hid.double() - c["hid64"]).abs().max().item()
    print(f"[{rnn} T={T} N={N} {kind}] seq {e_s:.3e} hidden {e_h:.3e}")
    assert e_s <= 1e-5 and e_h <= 1e-5
    errs = {k: _rel(grads[k], c["ref"][k], f"[{rnn} T={T} N={N} {kind}] {k}") for k in NAMES}
    # rows of d_h_in whose first mask is 0 receive nothing
    dead = c["m"][0] == 0
    assert dead.any() == (kind != "ones")
    if dead.any():
        assert c["ref"]["d_h_in"][:, dead].abs().max().item() == 0 and grads["d_h_in"][:, dead].abs().max().item() == 0
    if kind == "zero0" and T == 1:
        assert c["ref"]["dW_hh"].abs().max().item() == 0 and grads["dW_hh"].abs().max().item() == 0
    if kind == "cut":
        # every sample is reset in front of step T // 2 and the cotangent in front of it is zero: the first half receives nothing
        n = (T // 2) * N
        assert c["ref"]["dx"][:n].abs().max().item() == 0 and grads["dx"][:n].abs().max().item() == 0
        assert c["ref"]["dx"][n:].abs().max().item() > 0
        assert c["ref"]["d_h_in"].abs().max().item() == 0 and grads["d_h_in"].abs().max().item() == 0
    assert max(errs.values()) <= BOUND, errs


@pytest.mark.parametrize("T,N,kind", sc.SATURATED_CASES)
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_gradients_match_float64_autograd_with_saturated_gates(rnn, T, N, kind):
    """weight_ih times 20: about a fifth of the input-side pre-activations pass +-6, so g (1 - g) and 1 - n^2 round towards zero.  The bound is the
    one above; tests/test_train_coverage_cpu.py holds the float32 CPU restatement to half of it on the same inputs."""
    c = _case(rnn, T, N, kind, sc.SATURATED_IH_SCALE)
    seq, hid, grads = _gpu_grads(rnn, T, N, kind, sc.SATURATED_IH_SCALE)
    e_s, e_h = (seq.double() - c["seq64"]).abs().max().item(), (hid.double() - c["hid64"]).abs().max().item()
    print(f"[{rnn} T={T} N={N} {kind} saturated] seq {e_s:.3e} hidden {e_h:.3e}")
    assert e_s <= 1e-5 and e_h <= 1e-5
    errs = {k: _rel(grads[k], c["ref"][k], f"[{rnn} T={T} N={N} {kind} saturated] {k}") for k in NAMES}
    assert max(errs.values()) <= BOUND, errs


def _raw(rnn, T, N, kind, ih_scale=1.0, fill=None):
    """hcm_op_state_scan_train and hcm_op_state_scan_bwd through the C ABI on one case's inputs; every output starts as `fill` where one is given"""
    c = _case(rnn, T, N, kind, ih_scale)
    lstm = rnn == "LSTM"
    G = 4 if lstm else 3
    w_ih, w_hh, b_ih, b_hh = (t.cuda() for t in c["p"])
    pre = torch.addmm(b_ih + b_hh if lstm else b_ih, c["x"].cuda(), w_ih.t())
    h_in, m, cot = c["h0"].cuda(), c["m"].reshape(-1).cuda(), c["cot"].cuda()
    kind_id = _lib.HCM_LSTM if lstm else _lib.HCM_GRU
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pt = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib = _lib.lib()
    new = (lambda *s: torch.empty(*s, device="cuda")) if fill is None else (lambda *s: torch.full(s, fill, device="cuda"))
    o = dict(seq=new(T * N, H), h_out=new(*h_in.shape), gates=torch.full((T * N, 4 * H), float("nan"), device="cuda"),
             c_seq=new(T * N, H) if lstm else None, d_pre=new(T * N, G * H), d_gh=None if lstm else new(T * N, G * H), d_h_in=new(*h_in.shape))
    work = torch.empty(4 * H * H + 4 * N * H, device="cuda")
    bh = None if lstm else b_hh
    assert lib.hcm_op_state_scan_train(pt(pre), pt(w_hh), pt(bh), pt(h_in), pt(m), pt(o["seq"]), pt(o["h_out"]), pt(o["gates"]), pt(o["c_seq"]), pt(work),
                                       T, N, H, kind_id, st) == 0, _lib.last_error()
    assert lib.hcm_op_state_scan_bwd(pt(cot), pt(o["gates"]), pt(o["c_seq"]), pt(o["seq"]), pt(h_in), pt(m), pt(w_hh), pt(work), pt(o["d_pre"]),
                                     pt(o["d_gh"]), pt(o["d_h_in"]), T, N, H, kind_id, st) == 0, _lib.last_error()
    seq0, h_out0 = torch.empty_like(o["seq"]), torch.empty_like(h_in)
    assert lib.hcm_op_state_scan(pt(pre), pt(w_hh), pt(bh), pt(h_in), pt(m), pt(seq0), pt(h_out0), T, N, H, kind_id, st) == 0, _lib.last_error()
    torch.cuda.synchronize()
    return o, seq0, h_out0


def _saved64(rnn, T, N, kind):
    """gates / c_seq of the cell loop in float64: LSTM i,f,g,o and c_t; GRU r,z,n and hn = W_hn h' + b_hn"""
    c = _case(rnn, T, N, kind)
    w_ih, w_hh, b_ih, b_hh = (t.double() for t in c["p"])
    x, m = c["x"].double(), c["m"].double()
    h = c["h0"][0].double()
    cc = c["h0"][1].double() if rnn == "LSTM" else None
    gates, cs = [], []
    for t in range(T):
        hp = h * m[t][:, None]
        gi, gh = x[t * N:(t + 1) * N] @ w_ih.t() + b_ih, hp @ w_hh.t() + b_hh
        if rnn == "LSTM":
            i, f, g, o = (gi + gh).chunk(4, 1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            cc = f * (cc * m[t][:, None]) + i * g
            h = o * torch.tanh(cc)
            gates.append(torch.cat([i, f, g, o], 1))
            cs.append(cc)
        else:
            (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3, 1), gh.chunk(3, 1)
            r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
            n = torch.tanh(i_n + r * h_n)
            h = (1 - z) * n + z * hp
            gates.append(torch.cat([r, z, n, h_n], 1))
    return torch.cat(gates, 0), (torch.cat(cs, 0) if cs else None)


@pytest.mark.parametrize("T,N", RAW_SHAPES)
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_training_forward_is_the_forward_scan_bitwise_and_saves_the_gates(rnn, T, N):
    o, seq0, h_out0 = _raw(rnn, T, N, "random")
    assert torch.equal(o["seq"], seq0) and torch.equal(o["h_out"], h_out0)
    g64, c64 = _saved64(rnn, T, N, "random")
    e_g = (o["gates"].cpu().double() - g64).abs().max().item()
    e_c = (o["c_seq"].cpu().double() - c64).abs().max().item() if c64 is not None else 0.0
    print(f"[{rnn} T={T} N={N}] saved gates {e_g:.3e} c_seq {e_c:.3e}")
    assert e_g <= 1e-5 and e_c <= 1e-5              # (gates start as NaN: every element was written)


@pytest.mark.parametrize("T,N,kind,ih_scale", [(33, 5, "random", 1.0), (6, 13, "random", 1.0), (8, 5, "cut", 1.0), (12, 5, "random", sc.SATURATED_IH_SCALE)])
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_two_runs_give_the_same_bits_at_the_horizon_and_the_edges(rnn, T, N, kind, ih_scale):
    """outputs pre-filled with NaN: fully written, and the same bits on a second run"""
    nan = float("nan")
    a, _, _ = _raw(rnn, T, N, kind, ih_scale, fill=nan)
    b, _, _ = _raw(rnn, T, N, kind, ih_scale, fill=nan)
    for k, t in a.items():
        if t is not None:
            assert not t.isnan().any(), k
            assert torch.equal(t, b[k]), k


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_two_runs_give_the_same_bits(rnn):
    a, _, _ = _raw(rnn, 5, 9, "random")
    b, _, _ = _raw(rnn, 5, 9, "random")
    for k in ("d_pre", "d_gh", "d_h_in"):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


def _modules(rnn, seed):
    g = torch.Generator().manual_seed(seed)
    cpu = train.RNNStateEncoder(I, H, rnn_type=rnn)
    with torch.no_grad():
        for p in cpu.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    dev = train.RNNStateEncoder(I, H, rnn_type=rnn)
    dev.load_state_dict(cpu.state_dict())
    return cpu.double(), dev.cuda(), g


def _module_inputs(rnn, T, N, g):
    R = 2 if rnn == "LSTM" else 1
    x = torch.rand(T * N, I, generator=g) * 2 - 1
    h0 = torch.rand(R, N, H, generator=g) - 0.5
    m = _masks(T, N, "random", g)
    cot = torch.rand(T * N, H, generator=g) * 2 - 1
    return x, h0, m, cot


@pytest.mark.parametrize("T,N,call", [(5, 9, "seq_forward"), (1, 3, "single_forward")])
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_module_matches_its_cpu_path(rnn, T, N, call):
    cpu, dev, g = _modules(rnn, 5)
    x, h0, m, cot = _module_inputs(rnn, T, N, g)
    masks = m.reshape(-1, 1)                                             # the (T*N, 1) form the trainers pass
    s64, h64 = getattr(cpu, call)(x.double(), h0.double(), masks.double())
    (s64 * cot.double()).sum().backward()
    s, h = getattr(dev, call)(x.cuda(), h0.cuda(), masks.cuda())
    (s * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    e_s, e_h = (s.detach().cpu().double() - s64.detach()).abs().max().item(), (h.cpu().double() - h64).abs().max().item()
    print(f"module [{rnn}] {call}: seq {e_s:.3e} hidden {e_h:.3e}")
    assert e_s <= 1e-5 and e_h <= 1e-5 and not h.requires_grad
    errs = [_rel(pd.grad.cpu(), pc.grad, f"module [{rnn}] {call} {n}") for (n, pc), pd in zip(cpu.named_parameters(), dev.parameters())]
    assert max(errs) <= BOUND


def test_device_module_names_its_limits():
    h0 = torch.zeros(1, 2, 256, device="cuda")
    with pytest.raises(ValueError, match="512"):
        train.RNNStateEncoder(I, 256).cuda()(torch.zeros(2, I, device="cuda"), h0, torch.ones(2, 1, device="cuda"))
    with pytest.raises(ValueError, match="one layer"):
        train.RNNStateEncoder(I, H, num_layers=2).cuda()(torch.zeros(2, I, device="cuda"), torch.zeros(2, 2, H, device="cuda"), torch.ones(2, 1, device="cuda"))


@pytest.mark.parametrize("host", ["weight_hh", "hidden_states", "masks"])
def test_a_host_tensor_beside_device_rows_is_refused(host):
    """the kernels take raw pointers: a tensor left on the CPU must raise before any launch"""
    c = _case("GRU", 1, 3, "random")
    args = dict(zip(("x", "weight_ih", "weight_hh", "bias_ih", "bias_hh", "hidden_states"), (t.cuda() for t in (c["x"], *c["p"], c["h0"]))))
    args["masks"] = c["m"].reshape(-1).cuda()
    args[host] = args[host].cpu()
    with pytest.raises(ValueError, match=host):
        train.state_scan(*args.values())


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_an_optimizer_step_is_seen_by_the_next_call(rnn):
    """Adam with eps = 1e-3: with the default 1e-8 the first update is lr * sign(g) for every element, so an element whose float64 gradient
    is below float32 rounding noise could move by +lr on one side and -lr on the other; 1e-3 makes the update continuous in g."""
    cpu, dev, g = _modules(rnn, 9)
    T, N = 3, 8
    x, h0, m, cot = _module_inputs(rnn, T, N, g)
    outs = []
    for mod, to in ((cpu, lambda t: t.double()), (dev, lambda t: t.cuda())):
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3, eps=1e-3)
        s1, _ = mod(to(x), to(h0), to(m.reshape(-1)))
        (s1 * to(cot)).sum().backward()
        opt.step()
        with torch.no_grad():
            s2, _ = mod(to(x), to(h0), to(m.reshape(-1)))
        outs.append((s1.detach().cpu().double(), s2.cpu().double()))
    (c1, c2), (d1, d2) = outs
    moved, e1, e2 = (d2 - d1).abs().max().item(), (d1 - c1).abs().max().item(), (d2 - c2).abs().max().item()
    print(f"optimizer step [{rnn}]: output moved by {moved:.3e}; vs CPU before {e1:.3e} after {e2:.3e}")
    assert moved > 1e-4 and e1 <= 1e-5 and e2 <= 1e-5


@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_calls_enqueue_on_the_current_stream(rnn):
    T, N = 5, 9
    _, _, want = _gpu_grads(rnn, T, N, "random")
    c = _case(rnn, T, N, "random")
    leaves = [t.cuda().requires_grad_() for t in (c["x"], *c["p"], c["h0"])]
    m, cot = c["m"].reshape(-1).cuda(), c["cot"].cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    before, after = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s):
        before.record()
        seq, _ = train.state_scan(*leaves, m)
        grads = torch.autograd.grad(seq, leaves, cot)
        after.record()
    after.synchronize()                                                  # only the side stream's work is waited for
    assert before.query() and after.query()
    # d_h_in is the kernels' alone: the same bits.  The others end in a torch GEMM or sum, whose reduction order is the BLAS library's: float32 rounding
    for k, gk in zip(NAMES, grads):
        if k == "d_h_in":
            assert torch.equal(gk.cpu(), want[k])
        else:
            assert _rel(gk.cpu(), want[k].double(), f"side stream [{rnn}] {k}") <= 1e-6
