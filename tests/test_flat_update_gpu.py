"""The flat trainer's fused heads and criterion on the GPU: robo_vln_amd.train.flat_heads_loss (hcm_op_flat_heads_loss_train + hcm_op_flat_heads_loss_bwd)
against float64 on the CPU on every case of tests/flat_update_cases.py, the bit identities the header promises, the raw C ABI with guarded outputs,
the label edges, train.Seq2SeqNet / train.CMANet update_loss against their own float64 CPU path, and two flat_update steps with Adam.

The bound is the project's rule for the training ops (tests/vla_train_cases.rel): per tensor max|g - g64| / max|g64| <= 1e-5, a reference that is
identically zero matched exactly.  Each of the three losses is held to it on its own."""
import math

import pytest
import torch

from robo_vln_amd import _lib, train
from tests import flat_update_cases as fc
from tests.vla_train_cases import rel

pytestmark = pytest.mark.gpu
BOUND = 1e-5


def _cuda(t):
    return t.cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _val_loss(out, stop, p_hat, corrected, oracle_stop, progress):
    """hcm_op_flat_val_loss on device tensors -> result (8,)"""
    res = torch.full((8,), float("nan"), device="cuda")
    args = [None if t is None else t.data_ptr() for t in (out, stop, p_hat, corrected, oracle_stop, progress)]
    _lib.check(_lib.lib().hcm_op_flat_val_loss(*args, res.data_ptr(), out.shape[0], out.shape[1], torch.cuda.current_stream().cuda_stream))
    return res


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("rows,A,monitor,dx", fc.CASES)
def test_matches_float64_and_the_validation_criterion_bit_for_bit(rows, A, monitor, dx):
    c = fc.case(rows, A, monitor, dx)
    result, out, stop, p_hat, grads = fc.run(train.flat_heads_loss, c["args"], dx, _cuda)
    torch.cuda.synchronize()
    what = f"{(rows, A, monitor, dx)}"
    worst = {f"loss{k}": rel(result[k:k + 1].cpu(), c["result64"][k:k + 1], f"{what} result[{k}]") for k in range(3)}
    worst["out"] = rel(out.cpu(), c["out64"], what + " out")
    worst["stop"] = rel(stop.cpu(), c["stop64"], what + " stop")
    if monitor:
        worst["progress_hat"] = rel(p_hat.cpu(), c["progress_hat64"], what + " progress_hat")
    else:
        assert p_hat is None and float(result[2]) == 0.0
    assert set(grads) == set(c["ref"])
    for name, g in grads.items():
        worst[name] = rel(g.cpu(), c["ref"][name], f"{what} {name}")
    assert result[3:].tolist() == c["result64"][3:].tolist()
    assert max(worst.values()) <= BOUND, worst
    # the criterion is the validation step's: the same bits from hcm_op_flat_val_loss on this call's own outputs
    labels = [None if t is None else t.cuda() for t in c["args"][7:10]]
    assert _same_bits(result, _val_loss(out, stop, p_hat, *labels))


def test_a_row_has_the_bits_of_the_same_row_run_alone():
    args = fc.case(300, 2, True, True)["args"]
    dev = [t.cuda() for t in args]
    with torch.no_grad():
        _, out, stop, p_hat = train.flat_heads_loss(*dev)
        for r in (0, 3, 37, 255, 299):
            one = [dev[0][r:r + 1]] + dev[1:7] + [dev[7][r:r + 1], dev[8][r:r + 1], dev[9][r:r + 1]]
            _, o1, s1, p1 = train.flat_heads_loss(*one)
            assert _same_bits(o1, out[r:r + 1]) and _same_bits(s1, stop[r:r + 1]) and _same_bits(p1, p_hat[r:r + 1]), r
        # ... and of a 65-row call that holds it at another position
        part = [dev[0][235:300]] + dev[1:7] + [dev[7][235:300], dev[8][235:300], dev[9][235:300]]
        _, o2, s2, p2 = train.flat_heads_loss(*part)
        assert _same_bits(o2, out[235:300]) and _same_bits(s2, stop[235:300]) and _same_bits(p2, p_hat[235:300])


@pytest.mark.parametrize("rows,A,monitor,dx", [(300, 2, True, True), (600, 4, False, False), (33, 2, True, False)])
def test_two_calls_give_the_same_bits(rows, A, monitor, dx):
    args = fc.case(rows, A, monitor, dx)["args"]
    a = fc.run(train.flat_heads_loss, args, dx, _cuda)
    b = fc.run(train.flat_heads_loss, args, dx, _cuda)
    for u, v in zip(a[:4], b[:4]):
        assert (u is None and v is None) or _same_bits(u, v)
    for name in a[4]:
        assert _same_bits(a[4][name], b[4][name]), name


# ---------------------------------------------------------------- raw C ABI
GUARD, MARK = 16, 12345.0


class _Guarded:
    """an output of n floats pre-filled with NaN between two guards of 16 floats (which keep it 16-byte aligned)"""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), MARK, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(float("nan"))

    def guards_intact(self):
        return bool((self.buf[:GUARD] == MARK).all() and (self.buf[GUARD + self.t.numel():] == MARK).all())

    def written(self):
        return not torch.isnan(self.t).any()

    def untouched(self):
        return bool(torch.isnan(self.t).all())


def _raw(args, rows, A, monitor, dx, stream=None, hidden=512, null=(), A_arg=None, rows_arg=None):
    """both ops through the C ABI on guarded outputs -> (rc forward, rc backward, forward outputs, backward outputs)"""
    dev = [None if t is None else t.cuda() for t in args]
    x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected, ostop, progress = dev
    n = max(rows, 1)
    fo = dict(out=_Guarded(n * A), stop=_Guarded(n), result=_Guarded(8))
    bo = dict(d_w_lin=_Guarded(A * 512), d_b_lin=_Guarded(A), d_w_stop=_Guarded(512), d_b_stop=_Guarded(1))
    if monitor:
        fo["progress_hat"] = _Guarded(n)
        bo.update(d_w_pm=_Guarded(512), d_b_pm=_Guarded(1))
    if dx:
        bo["d_x"] = _Guarded(n * 512)
    work = _Guarded(max(1, _lib.lib().hcm_op_flat_heads_work_floats(rows, 512, A)))
    d_result = fc.cotangent(device="cuda")
    torch.cuda.synchronize()

    def p(t, name=None):
        if name in null or t is None:
            return None
        return (t.t if isinstance(t, _Guarded) else t).data_ptr()

    st = stream.cuda_stream if stream is not None else None
    A_, rows_ = A if A_arg is None else A_arg, rows if rows_arg is None else rows_arg
    l = _lib.lib()
    rc_f = l.hcm_op_flat_heads_loss_train(p(x, "x"), p(w_lin), p(b_lin), p(w_stop), p(b_stop), p(w_pm), p(b_pm), p(corrected), p(ostop), p(progress),
                                          p(fo["out"], "out"), p(fo["stop"]), p(fo.get("progress_hat")), p(fo["result"]), rows_, hidden, A_, st)
    rc_b = l.hcm_op_flat_heads_loss_bwd(p(d_result), p(x, "x"), p(w_lin), p(w_stop), p(w_pm), p(fo["out"]), p(fo["stop"]), p(fo.get("progress_hat")),
                                        p(corrected), p(ostop), p(progress), p(fo["result"]), p(bo.get("d_x")), p(bo["d_w_lin"], "d_w_lin"),
                                        p(bo["d_b_lin"]), p(bo["d_w_stop"]), p(bo["d_b_stop"]), p(bo.get("d_w_pm")), p(bo.get("d_b_pm")), p(work),
                                        rows_, hidden, A_, st)
    torch.cuda.synchronize()
    assert work.guards_intact()
    return rc_f, rc_b, fo, bo


@pytest.mark.parametrize("rows,A,monitor,dx,own_stream", [(33, 2, True, True, False), (65, 4, False, False, True), (5, 1, True, False, True),
                                                           (300, 2, False, True, False)])
def test_raw_abi_writes_every_output_and_nothing_else(rows, A, monitor, dx, own_stream):
    """NaN-filled outputs between guards: every output element is written and no guard is touched; NULL d_x, NULL monitor and a stream of the
    caller's own; the results are the autograd wrapper's, bit for bit"""
    args = fc.case(rows, A, monitor, dx)["args"]
    stream = torch.cuda.Stream() if own_stream else None
    rc_f, rc_b, fo, bo = _raw(args, rows, A, monitor, dx, stream)
    assert rc_f == 0 and rc_b == 0, _lib.last_error()
    for name, g in {**fo, **bo}.items():
        assert g.guards_intact(), name
        assert g.written(), name
    result, out, stop, p_hat, grads = fc.run(train.flat_heads_loss, args, dx, _cuda)
    assert _same_bits(fo["result"].t, result) and _same_bits(fo["out"].t.view(rows, A), out) and _same_bits(fo["stop"].t.view(rows, 1), stop)
    if monitor:
        assert _same_bits(fo["progress_hat"].t.view(rows, 1), p_hat)
    for name, g in grads.items():
        assert _same_bits(bo[name].t.view(g.shape), g), name


def test_raw_abi_zero_rows_and_refusals_write_nothing():
    args = fc.case(5, 2, True, True)["args"]
    empty = tuple(None if t is None else t[:0] if i in (0, 7, 8, 9) else t for i, t in enumerate(args))
    rc_f, rc_b, fo, bo = _raw(empty, 0, 2, True, True)
    assert rc_f == 0 and rc_b == 0, _lib.last_error()
    for name, g in {**fo, **bo}.items():
        assert g.guards_intact() and g.untouched(), name
    for what, kw in (("hidden", dict(hidden=256)), ("no actions", dict(A_arg=0)), ("five actions", dict(A_arg=5)), ("rows", dict(rows_arg=-1)),
                     ("x NULL", dict(null=("x",)))):
        rc_f, rc_b, fo, bo = _raw(args, 5, 2, True, True, **kw)
        assert rc_f == -1 and rc_b == -1 and _lib.last_error().startswith("flat_heads:"), what
        for name, g in {**fo, **bo}.items():
            assert g.guards_intact() and g.untouched(), (what, name)
    rc_f, rc_b, fo, bo = _raw(args, 5, 2, True, True, null=("out", "d_w_lin"))
    assert rc_f == -1 and rc_b == -1
    assert all(g.guards_intact() and g.untouched() for g in {**fo, **bo}.values())


def test_wrapper_refusals_and_restatement_routes():
    args = [t.cuda() for t in fc.case(5, 2, True, True)["args"]]
    with pytest.raises(ValueError, match="w_lin is on cpu"):
        train.flat_heads_loss(args[0], args[1].cpu(), *args[2:])
    with pytest.raises(ValueError, match="together"):
        train.flat_heads_loss(*args[:6], None, *args[7:])
    with pytest.raises(ValueError, match="corrected_actions"):
        train.flat_heads_loss(*args[:7], args[7][:4], *args[8:])
    # float64 on the device and a hidden size the kernels do not serve go through the restatement
    r64 = train.flat_heads_loss(*[t.double() for t in args])[0]
    assert r64.dtype == torch.float64 and rel(r64[:3].cpu(), fc.case(5, 2, True, True)["result64"][:3], "float64 on the device") <= 1e-12
    small = [args[0][:, :256].contiguous(), args[1][:, :256].contiguous(), args[2], args[3][:, :256].contiguous(), args[4],
             args[5][:, :256].contiguous(), args[6]] + args[7:]
    want = train.flat_heads_loss_ref(*[t.cpu().double() for t in small])[0]
    assert rel(train.flat_heads_loss(*small)[0][:3].cpu(), want[:3], "hidden 256 on the device") <= BOUND


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("monitor", [False, True])
def test_all_padded_labels_give_nan_losses_and_exact_zero_gradients(monitor):
    rows, A = 70, 2
    args = list(fc.make_inputs(rows, A, monitor))
    padded = args[:7] + [torch.zeros(rows, A), torch.full((rows, 1), -1.0), args[9]]
    result, out, stop, p_hat, grads = fc.run(train.flat_heads_loss, padded, True, _cuda)
    torch.cuda.synchronize()
    assert float(result[0]) == 0.0 and math.isnan(float(result[1])) and result[3:].tolist() == [0, 0, 0, 0, 0]
    assert math.isnan(float(result[2])) if monitor else float(result[2]) == 0.0
    assert torch.isfinite(out).all() and torch.isfinite(stop).all()
    for name, g in grads.items():
        assert (g == 0).all(), name
    assert (grads["d_x"] == 0).all()


def test_padded_rows_of_a_mixed_batch_get_exact_zero_d_x_rows():
    c = fc.case(300, 2, True, True)
    corrected, stop = c["args"][7], c["args"][8]
    pad = (stop[:, 0] == -1) & (corrected == 0).all(1)
    assert 30 < int(pad.sum()) < 60
    _, _, _, _, grads = fc.run(train.flat_heads_loss, c["args"], True, _cuda)
    d_x = grads["d_x"].cpu()
    assert (d_x[pad] == 0).all() and (d_x[~pad] != 0).any(1).all()
    assert (c["ref"]["d_x"][pad] == 0).all()


# ---------------------------------------------------------------- modules on the device
def _to64(t):
    return t.double()


def _module_pair(kind, monitor, T, N):
    cfg, m_cpu, batch, corrected, stop = fc.module_case(kind, monitor, T, N)
    _, m_gpu, _, _, _ = fc.module_case(kind, monitor, T, N)
    return cfg, m_cpu.double(), m_gpu.cuda(), batch, corrected, stop


def _assert_grads_close(m_gpu, m_cpu, cfg, monitor, what):
    hh = cfg.hidden // 2
    worst = {}
    gc = {n: p.grad for n, p in m_cpu.named_parameters()}
    for n, pg in m_gpu.named_parameters():
        if n.startswith("sub_goal_linear.") or (n.startswith("progress_monitor.") and not monitor):
            assert pg.grad is None and gc[n] is None, n
            continue
        worst[n] = rel(pg.grad.cpu(), gc[n], f"{what} {n}")
        if n == "text_k.bias":
            assert (pg.grad == 0).all()
        if n in ("rgb_kv.bias", "depth_kv.bias"):
            assert (pg.grad[:hh] == 0).all() and (pg.grad[hh:] != 0).any(), n
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("kind,monitor,T,N", [("s2s", True, 3, 2), ("s2s", False, 1, 2), ("cma", True, 3, 2), ("cma", False, 1, 2)])
def test_update_loss_matches_its_cpu_path(kind, monitor, T, N):
    """update_loss on the device against the same module's float64 CPU path: the three losses, the counts, the state and every parameter gradient"""
    cfg, m_cpu, m_gpu, batch, corrected, stop = _module_pair(kind, monitor, T, N)
    res_c, hid_c = m_cpu.update_loss(fc.convert_batch(batch, _to64), corrected, stop)
    (res_c[0] + res_c[1] + res_c[2]).backward()
    res_g, hid_g = m_gpu.update_loss(fc.convert_batch(batch, _cuda), corrected, stop)
    (res_g[0] + res_g[1] + res_g[2]).backward()
    torch.cuda.synchronize()
    what = f"{kind} monitor {monitor} ({T}, {N})"
    worst = {f"loss{k}": rel(res_g[k:k + 1].detach().cpu(), res_c[k:k + 1].detach(), f"{what} result[{k}]") for k in range(3)}
    worst["hidden"] = rel(hid_g.cpu(), hid_c, what + " hidden")
    assert res_g[3:].tolist() == res_c[3:].tolist() and (float(res_g[2]) > 0) == monitor
    assert max(worst.values()) <= BOUND, worst
    _assert_grads_close(m_gpu, m_cpu, cfg, monitor, what)


@pytest.mark.parametrize("kind", ["s2s", "cma"])
def test_two_flat_update_steps_match_the_cpu_path(kind):
    """Two flat_update steps with Adam (lr 1e-3, eps 1e-3: the construction of tests/test_embed_train_gpu.py -- with the default eps a parameter
    whose gradient is round-off takes a full step of either sign) on the device and on the float64 CPU path: every parameter within 1e-5 of its
    largest element, the results of both steps within the bound, and the second step saw the first one's weights"""
    cfg, m_cpu, m_gpu, batch, corrected, stop = _module_pair(kind, True, 3, 2)
    before = {n: p.detach().clone() for n, p in m_cpu.named_parameters()}
    results = {}
    for name, mod, conv in (("cpu", m_cpu, _to64), ("gpu", m_gpu, _cuda)):
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3, eps=1e-3)
        obs, h, prev, masks = fc.convert_batch(batch, conv)
        results[name] = []
        for _ in range(2):
            res, h = train.flat_update(mod, opt, obs, prev, masks, corrected, stop, h)
            assert not res.requires_grad and not h.requires_grad and res.device == h.device
            results[name].append(res.cpu().double())
    torch.cuda.synchronize()
    for i in range(2):
        for k in range(3):
            assert rel(results["gpu"][i][k:k + 1], results["cpu"][i][k:k + 1], f"{kind} step {i} result[{k}]") <= BOUND
    assert float(results["cpu"][1][:3].sum()) != float(results["cpu"][0][:3].sum())
    pc = dict(m_cpu.named_parameters())
    worst, moved = {}, {}
    for n, p in m_gpu.named_parameters():
        worst[n] = rel(p.detach().cpu(), pc[n].detach(), f"{kind} parameter {n}")
        moved[n] = (pc[n].detach() - before[n]).abs().max().item()
    assert max(worst.values()) <= BOUND, worst
    assert moved["progress_monitor.weight"] > 0 and moved["linear.weight"] > 0 and moved["stop_linear.bias"] > 0
    assert moved["state_encoder.rnn.weight_hh_l0"] > 0 and moved["instruction_encoder.encoder_rnn.weight_ih_l0"] > 0
