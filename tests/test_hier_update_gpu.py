"""The hierarchical trainer's fused sub-task head and cross-entropy on the GPU: robo_vln_amd.train.subtask_ce (hcm_op_subtask_ce_train +
hcm_op_subtask_ce_bwd) against float64 on the CPU on every case of tests/subtask_ce_cases.py, the bit identities the header promises, the raw C ABI
with guarded outputs, the label edges, train.HighLevel / train.LowLevel against their own float64 CPU path, and two hier_update steps with Adam.

The bound is the project's rule for the training ops (tests/vla_train_cases.rel): per tensor max|g - g64| / max|g64| <= 1e-5, a reference that is
identically zero matched exactly.  The loss, the logits and each gradient are held to it on their own; the counts are exact."""
import math

import pytest
import torch

from robo_vln_amd import _lib, train
from tests import subtask_ce_cases as sc
from tests import val_ref
from tests.vla_train_cases import rel

pytestmark = pytest.mark.gpu
BOUND = 1e-5


def _cuda(t):
    return t.cuda()


def _to64(t):
    return t.double()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _val_loss(logits, oracle, nst):
    """hcm_op_val_loss on this call's logits and labels with dummy low-level tensors -> result (8,)"""
    rows, A = logits.shape
    res = torch.full((8,), float("nan"), device="cuda")
    vel, stop, corrected, ostop = (torch.zeros(rows, n, device="cuda") for n in (2, 1, 2, 1))
    o = oracle.cuda().reshape(-1).to(torch.int64)
    _lib.check(_lib.lib().hcm_op_val_loss(logits.data_ptr(), vel.data_ptr(), stop.data_ptr(), o.data_ptr(), corrected.data_ptr(), ostop.data_ptr(),
                                          res.data_ptr(), rows, A, nst, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("rows,A,nst,dx,bad", sc.CASES)
def test_matches_float64_and_the_validation_criterion_bit_for_bit(rows, A, nst, dx, bad):
    c = sc.case(rows, A, nst, dx, bad)
    result, logits, grads = sc.run(train.subtask_ce, c["args"], nst, dx, _cuda)
    torch.cuda.synchronize()
    what = f"{(rows, A, nst, dx, bad)}"
    worst = {"logits": rel(logits.cpu(), c["logits64"], what + " logits")}
    if c["result64"][4] > 0:
        worst["loss"] = rel(result[:1].cpu(), c["result64"][:1], what + " result[0]")
    else:
        assert math.isnan(float(result[0])) and math.isnan(float(c["result64"][0]))
    assert set(grads) == set(c["ref"])
    for name, g in grads.items():
        worst[name] = rel(g.cpu(), c["ref"][name], f"{what} {name}")
    assert result[1:].tolist() == c["result64"][1:].tolist()
    assert max(worst.values()) <= BOUND, worst
    # the criterion is the validation step's: words [0], [3], [4], [6] have the bits of hcm_op_val_loss on this call's own logits
    want = _val_loss(logits, c["args"][3], nst)
    for k in (0, 3, 4, 6):
        assert _same_bits(result[k:k + 1], want[k:k + 1]), k
    assert result[[1, 2, 5, 7]].tolist() == [0, 0, 0, 0]


def test_a_row_has_the_bits_of_the_same_row_run_alone():
    x, w, b, oracle = (t.cuda() for t in sc.case(300, 4, 4, True, True)["args"])
    with torch.no_grad():
        logits = train.subtask_ce(x, w, b, oracle)[1]
        for r in (0, 3, 37, 255, 299):
            assert _same_bits(train.subtask_ce(x[r:r + 1], w, b, oracle[r:r + 1])[1], logits[r:r + 1]), r
        # ... and of a 65-row call that holds it at another position
        assert _same_bits(train.subtask_ce(x[235:300], w, b, oracle[235:300])[1], logits[235:300])


@pytest.mark.parametrize("rows,A,nst,dx,bad", [(300, 4, 4, True, True), (600, 6, 6, True, False), (257, 6, 5, False, False), (33, 4, 4, False, False)])
def test_two_calls_give_the_same_bits(rows, A, nst, dx, bad):
    args = sc.case(rows, A, nst, dx, bad)["args"]
    a = sc.run(train.subtask_ce, args, nst, dx, _cuda)
    b = sc.run(train.subtask_ce, args, nst, dx, _cuda)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    for name in a[2]:
        assert _same_bits(a[2][name], b[2][name]), name


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


def _raw(args, rows, A, nst, dx, stream=None, hidden=512, null=(), A_arg=None, rows_arg=None, nst_arg=None):
    """both ops through the C ABI on guarded outputs -> (rc forward, rc backward, forward outputs, backward outputs)"""
    x, w, b, oracle = (t.cuda() for t in args)
    o = oracle.reshape(-1).to(torch.int64)
    n = max(rows, 1)
    fo = dict(logits=_Guarded(n * A), result=_Guarded(8))
    bo = dict(d_w=_Guarded(A * 512), d_b=_Guarded(A))
    if dx:
        bo["d_x"] = _Guarded(n * 512)
    work = _Guarded(max(1, _lib.lib().hcm_op_subtask_ce_work_floats(rows, 512, A)))
    d_result = sc.cotangent(device="cuda")
    torch.cuda.synchronize()

    def p(t, name=None):
        if name in null or t is None:
            return None
        return (t.t if isinstance(t, _Guarded) else t).data_ptr()

    st = stream.cuda_stream if stream is not None else None
    A_, rows_, nst_ = A if A_arg is None else A_arg, rows if rows_arg is None else rows_arg, nst if nst_arg is None else nst_arg
    l = _lib.lib()
    rc_f = l.hcm_op_subtask_ce_train(p(x, "x"), p(w), p(b), p(o), p(fo["logits"], "logits"), p(fo["result"]), rows_, hidden, A_, nst_, st)
    rc_b = l.hcm_op_subtask_ce_bwd(p(d_result), p(x, "x"), p(w), p(fo["logits"]), p(o), p(fo["result"]), p(bo.get("d_x")), p(bo["d_w"], "d_w"),
                                   p(bo["d_b"]), p(work), rows_, hidden, A_, nst_, st)
    torch.cuda.synchronize()
    assert work.guards_intact()
    return rc_f, rc_b, fo, bo


@pytest.mark.parametrize("rows,A,nst,dx,bad,own_stream", [(33, 4, 4, False, False, False), (65, 4, 4, True, False, True), (5, 4, 4, True, True, True),
                                                           (300, 4, 4, True, True, False), (17, 6, 4, True, True, True)])
def test_raw_abi_writes_every_output_and_nothing_else(rows, A, nst, dx, bad, own_stream):
    """NaN-filled outputs between guards: every output element is written and no guard is touched; NULL d_x and a stream of the caller's own; the
    results are the autograd wrapper's, bit for bit"""
    args = sc.case(rows, A, nst, dx, bad)["args"]
    stream = torch.cuda.Stream() if own_stream else None
    rc_f, rc_b, fo, bo = _raw(args, rows, A, nst, dx, stream)
    assert rc_f == 0 and rc_b == 0, _lib.last_error()
    for name, g in {**fo, **bo}.items():
        assert g.guards_intact(), name
        assert g.written(), name
    result, logits, grads = sc.run(train.subtask_ce, args, nst, dx, _cuda)
    assert _same_bits(fo["result"].t, result) and _same_bits(fo["logits"].t.view(rows, A), logits)
    for name, g in grads.items():
        assert _same_bits(bo[name].t.view(g.shape), g), name


def test_raw_abi_zero_rows_and_refusals_write_nothing():
    args = sc.case(5, 4, 4, True, True)["args"]
    empty = (args[0][:0], args[1], args[2], args[3][:0])
    rc_f, rc_b, fo, bo = _raw(empty, 0, 4, 4, True)
    assert rc_f == 0 and rc_b == 0, _lib.last_error()
    for name, g in {**fo, **bo}.items():
        assert g.guards_intact() and g.untouched(), name
    for what, kw in (("hidden", dict(hidden=256)), ("no classes", dict(A_arg=0)), ("seven classes", dict(A_arg=7)), ("rows", dict(rows_arg=-1)),
                     ("no sub-tasks", dict(nst_arg=0)), ("more sub-tasks than classes", dict(nst_arg=5)), ("x NULL", dict(null=("x",)))):
        rc_f, rc_b, fo, bo = _raw(args, 5, 4, 4, True, **kw)
        assert rc_f == -1 and rc_b == -1 and _lib.last_error().startswith("subtask_ce:"), what
        for name, g in {**fo, **bo}.items():
            assert g.guards_intact() and g.untouched(), (what, name)
    rc_f, rc_b, fo, bo = _raw(args, 5, 4, 4, True, null=("logits", "d_w"))
    assert rc_f == -1 and rc_b == -1
    assert all(g.guards_intact() and g.untouched() for g in {**fo, **bo}.values())


def test_wrapper_refusals_and_restatement_routes():
    c = sc.case(5, 4, 4, True, True)
    x, w, b, oracle = (t.cuda() for t in c["args"])
    with pytest.raises(ValueError, match="w is on cpu"):
        train.subtask_ce(x, w.cpu(), b, oracle)
    with pytest.raises(ValueError, match="one sub-task label per row"):
        train.subtask_ce(x, w, b, oracle[:4])
    with pytest.raises(ValueError, match="b has shape"):
        train.subtask_ce(x, w, b[:3], oracle)
    # labels on the host, and integer labels, are brought to the device and mean the same
    want = train.subtask_ce(x, w, b, oracle)
    for o in (oracle.cpu(), oracle.reshape(-1).to(torch.int32), oracle.reshape(-1).to(torch.int64)):
        got = train.subtask_ce(x, w, b, o)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    # float64 on the device, a hidden size and a class count the kernels do not serve go through the restatement
    r64 = train.subtask_ce(x.double(), w.double(), b.double(), oracle, 4)[0]
    assert r64.dtype == torch.float64 and rel(r64[:1].cpu(), c["result64"][:1], "float64 on the device") <= 1e-12
    xs, ws = x[:, :256].contiguous(), w[:, :256].contiguous()
    assert rel(train.subtask_ce(xs, ws, b, oracle)[0][:1].cpu(), train.subtask_ce_ref(xs.cpu().double(), ws.cpu().double(), b.cpu().double(),
                                                                                  oracle.cpu())[0][:1], "hidden 256 on the device") <= BOUND
    w8, b8 = torch.cat([w, w]), torch.cat([b, b])
    assert rel(train.subtask_ce(x, w8, b8, oracle, 4)[0][:1].cpu(), train.subtask_ce_ref(x.cpu().double(), w8.cpu().double(), b8.cpu().double(),
                                                                                       oracle.cpu(), 4)[0][:1], "eight classes on the device") <= BOUND


# ---------------------------------------------------------------- labels
@pytest.mark.parametrize("fill", [0.0, 9.0])
def test_no_valid_row_gives_a_nan_loss_and_exact_zero_gradients(fill):
    rows, A = 70, 4
    x, w, b, _ = sc.make_inputs(rows, A, A, False)
    result, logits, grads = sc.run(train.subtask_ce, (x, w, b, torch.full((rows, 1), fill)), A, True, _cuda)
    torch.cuda.synchronize()
    assert math.isnan(float(result[0])) and result[1:].tolist() == [0, 0, 0, 0, 0, rows if fill else 0, 0]
    assert torch.isfinite(logits).all()
    for name, g in grads.items():
        assert (g == 0).all(), name


def test_padded_and_out_of_range_rows_of_a_mixed_batch_get_exact_zero_d_x_rows():
    c = sc.case(300, 4, 4, True, True)
    o = c["args"][3][:, 0]
    off = (o == 0) | (o > 4)
    assert 40 < int(off.sum()) < 60 and int((o > 4).sum()) == 1
    _, _, grads = sc.run(train.subtask_ce, c["args"], 4, True, _cuda)
    d_x = grads["d_x"].cpu()
    assert (d_x[off] == 0).all() and (d_x[~off] != 0).any(1).all()
    assert (c["ref"]["d_x"][off] == 0).all()


def test_a_nan_in_a_valid_row_s_logits_reaches_the_loss_and_one_in_a_padded_row_does_not():
    x, w, b, oracle = (t.cuda() for t in sc.case(33, 4, 4, False, False)["args"])
    o = oracle[:, 0]
    valid, padded = int((o != 0).nonzero()[5]), int((o == 0).nonzero()[0])
    for row, want_nan in ((valid, True), (padded, False)):
        xn = x.clone()
        xn[row, 7] = float("nan")
        result, logits = train.subtask_ce(xn, w, b, oracle)
        assert torch.isnan(logits[row]).all() and math.isnan(float(result[0])) == want_nan, row
        assert _same_bits(result[[0, 3, 4, 6]], _val_loss(logits, oracle, 4)[[0, 3, 4, 6]]), row


# ---------------------------------------------------------------- modules on the device
def _module_pair(T, N, **kw):
    cfg, hi_c, lo_c, obs, h_hi, h_lo, prev, masks, corrected, stop = sc.module_case(T, N, **kw)
    _, hi_g, lo_g, *_ = sc.module_case(T, N, **kw)
    return cfg, (hi_c.double(), lo_c.double()), (hi_g.cuda(), lo_g.cuda()), obs, h_hi, h_lo, prev, masks, corrected, stop


def _assert_grads_close(m_gpu, m_cpu, what):
    """every parameter gradient against float64 by the project's rule.  fc_k.bias as in tests/test_vla_layer_train_gpu.py and
    tests/test_embed_train_gpu.py: its exact gradient is zero (a bias on the keys shifts every score of a row alike, which softmax ignores),
    float64 autograd leaves rounding noise rather than an identical zero, so it is held to the bound on fc_k.weight's scale."""
    worst = {}
    gc = {n: p.grad for n, p in m_cpu.named_parameters()}
    for n, pg in m_gpu.named_parameters():
        if n.startswith(("progress_monitor.", "ins_fc.")):
            assert pg.grad is None and gc[n] is None, n
            continue
        if n.endswith("enc_att.attention.fc_k.bias"):
            scale = gc[n[:-4] + "weight"].abs().max().item()
            assert gc[n].abs().max().item() <= 1e-12 * scale                  # the reference itself: zero up to float64 noise
            worst[n] = (pg.grad.cpu().double() - gc[n]).abs().max().item() / scale
            print(f"{what} {n} (on fc_k.weight's scale): {worst[n]:.3e}")
            continue
        worst[n] = rel(pg.grad.cpu(), gc[n], f"{what} {n}")
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("T,N,kw", [(3, 2, {}), (1, 2, dict(rnn_type="LSTM"))])
def test_update_loss_of_both_models_matches_their_cpu_path(T, N, kw):
    """update_loss on the device against the same module's float64 CPU path: the losses, the counts, the states and every parameter gradient"""
    cfg, cpu, gpu, obs, h_hi, h_lo, prev, masks, corrected, stop = _module_pair(T, N, **kw)
    out = {}
    for name, (high, low), conv in (("cpu", cpu, _to64), ("gpu", gpu, _cuda)):
        o = sc.convert_obs(obs, conv)
        res_hi, hid_hi = high.update_loss((o, conv(h_hi), conv(prev), conv(masks)), o["vln_oracle_action_sensor"])
        res_hi[0].backward()
        sub = val_ref.remap(obs["vln_oracle_action_sensor"], cfg.num_sub_tasks).to(hid_hi.device)
        res_lo, hid_lo = low.update_loss((o, conv(h_lo), conv(prev), conv(masks), sub), corrected, stop)
        (res_lo[0] + res_lo[1]).backward()
        out[name] = (res_hi.detach().cpu(), hid_hi.cpu(), res_lo.detach().cpu(), hid_lo.cpu())
    torch.cuda.synchronize()
    what = f"({T}, {N}) {kw}"
    c, g = out["cpu"], out["gpu"]
    worst = {"high loss": rel(g[0][:1], c[0][:1], what + " high result[0]"), "high hidden": rel(g[1], c[1], what + " high hidden"),
             "action loss": rel(g[2][:1], c[2][:1], what + " low result[0]"), "stop loss": rel(g[2][1:2], c[2][1:2], what + " low result[1]"),
             "low hidden": rel(g[3], c[3], what + " low hidden")}
    assert g[0][1:].tolist() == c[0][1:].tolist() and g[2][2:].tolist() == c[2][2:].tolist()
    assert max(worst.values()) <= BOUND, worst
    _assert_grads_close(gpu[0], cpu[0], what + " high")
    _assert_grads_close(gpu[1], cpu[1], what + " low")


def test_two_hier_update_steps_match_the_cpu_path():
    """Two hier_update steps with Adam (lr 1e-3, eps 1e-3: the construction of tests/test_embed_train_gpu.py -- with the default eps a parameter
    whose gradient is round-off takes a full step of either sign) on the device and on the float64 CPU path: every parameter within 1e-5 of its
    largest element, the results of both steps within the bound, and the second step saw the first one's weights"""
    cfg, cpu, gpu, obs, h_hi, h_lo, prev, masks, corrected, stop = _module_pair(3, 2)
    before = {n: p.detach().clone() for n, p in cpu[0].named_parameters()}
    results = {}
    for name, (high, low), conv in (("cpu", cpu, _to64), ("gpu", gpu, _cuda)):
        opt_hi = torch.optim.Adam(high.parameters(), lr=1e-3, eps=1e-3)
        opt_lo = torch.optim.Adam(low.parameters(), lr=1e-3, eps=1e-3)
        o, hh, lh = sc.convert_obs(obs, conv), conv(h_hi), conv(h_lo)
        results[name] = []
        for _ in range(2):
            res_hi, res_lo, hh, lh = train.hier_update(high, low, opt_hi, opt_lo, o, conv(prev), conv(masks), corrected, stop, hh, lh)
            for t in (res_hi, res_lo, hh, lh):
                assert not t.requires_grad and t.device == hh.device
            results[name].append((res_hi.cpu().double(), res_lo.cpu().double()))
    torch.cuda.synchronize()
    for i in range(2):
        (gh, gl), (ch, cl) = results["gpu"][i], results["cpu"][i]
        assert rel(gh[:1], ch[:1], f"step {i} high result[0]") <= BOUND
        for k in range(2):
            assert rel(gl[k:k + 1], cl[k:k + 1], f"step {i} low result[{k}]") <= BOUND
        assert gh[1:].tolist() == ch[1:].tolist() and gl[2:].tolist() == cl[2:].tolist()
    assert float(results["cpu"][1][0][0]) != float(results["cpu"][0][0][0]) and float(results["cpu"][1][1][0]) != float(results["cpu"][0][1][0])
    for m_gpu, m_cpu, which in ((gpu[0], cpu[0], "high"), (gpu[1], cpu[1], "low")):
        pc = dict(m_cpu.named_parameters())
        worst = {n: rel(p.detach().cpu(), pc[n].detach(), f"{which} parameter {n}") for n, p in m_gpu.named_parameters()}
        assert max(worst.values()) <= BOUND, worst
    moved = {n: (p.detach() - before[n]).abs().max().item() for n, p in cpu[0].named_parameters()}
    assert moved["linear.weight"] > 0 and moved["state_encoder.rnn.weight_hh_l0"] > 0 and moved["rgb_kv.weight"] > 0
    assert moved["image_cm_encoder.layers.0.pwff.fc1.weight"] > 0 and moved["progress_monitor.weight"] == 0
