"""The flat trainer's validation step on the GPU (hcm_flat_val_step, CMAEngine.val_step, S2SEngine.val_step, FlatValidator): the criterion
kernel against torch's criteria, bit-identity with the kind's sequence forward, parity with the goldens and the CPU restatement, the NaN
contract, capture-legality, T = 1 and the validation epoch.

One engine per (case, precision) and one CPU restatement per case for the whole module.

Measured on one MI355X: the file's 39 tests take 8.2 s (`pytest --durations=0`; no item above 0.45 s, the eleven engines are created inside
the first test that needs one).  Largest measured errors against the restatement / golden, bounds in brackets: outputs fp32 2.0e-6 [1e-3],
fp16 1.6e-3 [1e-2]; fp32 action 1.1e-6 [1.3e-3], stop 4.8e-7 [1e-3], aux 1.4e-6 [3.2e-3]; fp16 action 8.8e-4 [1.2e-2], stop 5.1e-4 [1e-2],
aux 3.0e-3 [2.3e-2] (the last three in the validator's two-row chunks); counts equal in every case."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import flat_val_ref as fv

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 1e-2}       # the output tolerance of tests/test_parity_gpu.py
PM = "flatval_s2s_pm_T3_N2_gru"
CMA = "flatval_cma_T4_N2"


@pytest.fixture(scope="module")
def engines():
    from robo_vln_amd.cma import CMAEngine
    from robo_vln_amd.seq2seq import S2SEngine
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            kind, cfg, T, N = fv.case(name)
            made[(name, precision)] = (CMAEngine if kind == "cma" else S2SEngine)(cfg, fv.weights(kind, cfg), max_batch=T * N, precision=precision)
        return made[(name, precision)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def restated():
    made = {}

    def get(name):
        if name not in made:
            kind, cfg, T, N, obs, corrected, stop, m, h0 = fv.inputs(name)
            made[name] = fv.oracle(name).val_step(obs, corrected, stop, h0.clone(), m, return_outputs=True)
        return made[name]
    return get


def _inputs(name, label_kind="mixed"):
    kind, cfg, T, N, obs, corrected, stop, m, h0 = fv.inputs(name, label_kind)
    obs = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in obs.items()}
    masks = torch.from_numpy(m).view(-1, 1).expand(-1, 2).contiguous().cuda()          # reference-shaped (T*N, 2)
    return kind, cfg, T, N, obs, torch.from_numpy(corrected).cuda(), torch.from_numpy(stop).cuda(), masks, h0.cuda()


def _forward_seq(eng, kind, obs, h0, masks, T, N):
    """-> (out, stop, progress_hat or None, hidden) of the kind's sequence forward"""
    o = {k: v for k, v in obs.items() if k != "progress"}
    if kind == "cma":
        out, stop, hid = eng.forward_seq(o, h0, masks, T, N)
        return out, stop, None, hid
    return eng.forward_seq(o, h0, masks, T, N)


def _bounds(tol, out_ref, corrected, prog_ref, progress):
    """Bounds of the three losses from the output tolerance `tol`, as tests/test_val_gpu._check_losses derives them: stop tol (BCE-with-logits is
    1-Lipschitz in the logit); action 2*tol*mean|out_ref_masked - target| + tol^2 (|a^2 - b^2| <= 2|b||a-b| + |a-b|^2, element by element);
    aux the same with mean|p_ref - y| over the selected rows (tanh is 1-Lipschitz, so progress_hat obeys the output tolerance)."""
    c = torch.as_tensor(corrected).float().cpu()
    resid = (torch.as_tensor(out_ref).float().cpu().masked_fill(c == 0, 0) - c).abs().mean().item()
    aux = 0.0
    if prog_ref is not None:
        sel = c[:, 0] != 0
        p, y = torch.as_tensor(prog_ref).float().cpu().reshape(-1), torch.as_tensor(progress).float().cpu().reshape(-1)
        aux = 2 * tol * (p[sel] - y[sel]).abs().mean().item() + tol * tol
    return (2 * tol * resid + tol * tol, tol, aux)


def _check_losses(got, ref, bounds, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    errs = [abs(got[i] - ref[i]) for i in range(3)]
    print(f"{what}: |action| err {errs[0]:.3e} (<= {bounds[0]:.2e})  |stop| err {errs[1]:.3e} (<= {bounds[1]:.1e})  "
          f"|aux| err {errs[2]:.3e} (<= {bounds[2]:.2e})  stop rows {got[3]:.0f}/{ref[3]:.0f} aux rows {got[4]:.0f}/{ref[4]:.0f}")
    for e, b in zip(errs, bounds):
        assert e <= b
    assert got[3:].tolist() == ref[3:].tolist()


# ---------------------------------------------------------------- the criterion kernel alone
def _kernel_alone(out, stop, prog_hat, corrected, ostop, prog):
    from robo_vln_amd import _lib
    dev = [None if t is None else t.float().cuda().contiguous() for t in (out, stop, prog_hat, corrected, ostop, prog)]
    res = torch.full((8,), -7.0, device="cuda")
    rc = _lib.lib().hcm_op_flat_val_loss(*[None if t is None else t.data_ptr() for t in dev], res.data_ptr(), out.shape[0], out.shape[1],
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return res.cpu().numpy()


@pytest.mark.parametrize("rows", [70, 300, 1000])
def test_criterion_kernel_alone_over_many_rows(rows):
    """More rows than one wave (70), than the workgroup (300: the stride) and several strides (1000): every lane, all four waves' LDS sums and
    the integer counts carry data.  Against torch's criteria in fp32 on the CPU.  Bound, from the number format (the derivation of
    tests/test_val_gpu.py's criterion test): each side sums `rows` f32 terms of one sign in its own order, at most rows * 2^-24 relative per
    side, plus 1e-5 for the exp / log evaluations: rtol = 2 * rows * 2^-24 + 1e-5."""
    rtol = 2 * rows * 2.0 ** -24 + 1e-5
    g = torch.Generator().manual_seed(rows)
    out = torch.randn(rows, 2, generator=g)
    stop = torch.randn(rows, 1, generator=g) * 3
    p_hat = torch.tanh(torch.randn(rows, 1, generator=g))
    corrected = torch.randn(rows, 2, generator=g)
    corrected[torch.rand(rows, 2, generator=g) < 0.2] = 0
    ostop = torch.randint(-1, 2, (rows, 1), generator=g).float()
    prog = torch.rand(rows, generator=g)
    got = _kernel_alone(out, stop, p_hat, corrected, ostop, prog)
    ref = fv.criteria(out, stop, p_hat, corrected, ostop, prog).numpy()
    print(f"rows {rows}: kernel {got} torch {ref} rel {np.abs(got[:3] - ref[:3]) / np.abs(ref[:3])}")
    np.testing.assert_allclose(got[:3], ref[:3], rtol=rtol, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[3] > rows // 2 and got[4] > rows // 2 and got[4] < rows
    again = _kernel_alone(out, stop, p_hat, corrected, ostop, prog)
    assert got.tobytes() == again.tobytes()
    # the monitor pointers NULL: aux exactly +0 and its count 0, the other words unchanged
    off = _kernel_alone(out, stop, None, corrected, ostop, None)
    assert off[2].tobytes() == np.float32(0).tobytes() and off[4] == 0 and off[[0, 1, 3]].tobytes() == got[[0, 1, 3]].tobytes()
    # labels present in the last two rows only: what the last stride's lanes hold must arrive
    c2 = torch.zeros(rows, 2); c2[-1] = torch.tensor([0.5, -0.25])
    s2 = torch.full((rows, 1), -1.0); s2[-2] = 1.0
    got = _kernel_alone(out, stop, p_hat, c2, s2, prog)
    ref = fv.criteria(out, stop, p_hat, c2, s2, prog).numpy()
    np.testing.assert_allclose(got[:3], ref[:3], rtol=rtol, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[3] == 1 and got[4] == 1


# ---------------------------------------------------------------- the call
@pytest.mark.parametrize("name,precision", [(PM, "fp32"), (PM, "fp16"), (PM, "bf16"), (CMA, "fp32"), (CMA, "fp16"), (CMA, "bf16")])
def test_criterion_kernel_is_exact_on_the_calls_own_outputs(name, precision, engines):
    """Only the order of an f32 sum differs between the kernel and torch's criteria applied on the CPU to the outputs the same call returned:
    relative 1e-5 on the three losses (T*N <= 64 terms of magnitude O(1)), counts equal."""
    eng = engines(name, precision)
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hid, (out, st, prog) = eng.val_step(obs, corrected, stop, h0, masks, return_outputs=True)
    assert res.shape == (8,) and res.dtype == torch.float32 and res.is_cuda and (prog is not None) == (name == PM)
    ref = fv.criteria(out, st, prog, corrected, stop, obs.get("progress")).numpy()
    got = res.cpu().numpy()
    print(f"{name} {precision}: kernel {got} torch {ref}")
    np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-5, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[3] == T * N - 1 and got[4] == (T * N - 2 if name == PM else 0)
    if name != PM:
        assert got[2].tobytes() == np.float32(0).tobytes()


@pytest.mark.parametrize("name", list(fv.FLAT_VAL_CASES))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_outputs_are_bit_identical_to_the_sequence_forward(name, precision, engines):
    eng = engines(name, precision)
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hid, (out, st, prog) = eng.val_step(obs, corrected, stop, h0, masks, return_outputs=True)
    o2, s2, p2, h2 = _forward_seq(eng, kind, obs, h0, masks, T, N)
    for a, b, what in ((out, o2, "out"), (st, s2, "stop"), (hid, h2, "hidden")):
        assert torch.equal(a, b), what
    assert (prog is None and p2 is None) or torch.equal(prog, p2)
    # the same call again, this time without the optional outputs: the same eight words
    res2, hid2 = eng.val_step(obs, corrected, stop, h0, masks)
    assert torch.equal(res.view(torch.int32), res2.view(torch.int32)) and torch.equal(hid, hid2)


@pytest.mark.parametrize("name", list(fv.FLAT_VAL_CASES))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_parity_with_golden_and_restatement(name, precision, engines, restated):
    eng = engines(name, precision)
    tol = TOL[precision]
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hid, (out, st, prog) = eng.val_step(obs, corrected, stop, h0, masks, return_outputs=True)
    r_res, r_hid, (r_out, r_stop, r_prog) = restated(name)
    progress = obs.get("progress")
    pairs = [(out, r_out, "out"), (st, r_stop, "stop")] + ([(prog, r_prog, "progress_hat")] if r_prog is not None else [])
    for got, ref, what in pairs:
        err = (got.cpu() - ref).abs().max().item()
        print(f"{name} {precision}: {what} vs restatement {err:.3e} (<= {tol:.0e})")
        assert err <= tol, what
    _check_losses(res.cpu().numpy(), r_res.numpy(), _bounds(tol, r_out, corrected, r_prog, progress), f"{name} {precision} vs restatement")
    if name in fv.FLAT_VAL_GOLDEN:
        gold = np.load(os.path.join(GOLD, name + ".npz"))
        for got, ref, what in pairs:
            key = what
            err = np.abs(got.cpu().numpy() - gold[key]).max()
            print(f"{name} {precision}: {what} vs golden {err:.3e} (<= {tol:.0e})")
            assert err <= tol, what
        g_prog = gold["progress_hat"] if r_prog is not None else None
        _check_losses(res.cpu().numpy(), gold["result"], _bounds(tol, gold["out"], corrected, g_prog, progress), f"{name} {precision} vs golden")


@pytest.mark.parametrize("name", [PM, CMA])
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_all_padded_labels_give_nan_and_leave_the_guard_alone(name, precision, engines):
    from robo_vln_amd import _lib
    eng = engines(name, precision)
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name, "padded")
    before = (eng.query(_lib.HCM_STEP_NONFINITE), eng.query(_lib.HCM_CALIB_NONFINITE))
    res, hid = eng.val_step(obs, corrected, stop, h0, masks)
    r = res.cpu().numpy()
    assert r[0] == 0.0 and math.isnan(r[1]) and r[3:].tolist() == [0, 0, 0, 0, 0]
    assert math.isnan(r[2]) if name == PM else r[2] == 0.0
    assert (eng.query(_lib.HCM_STEP_NONFINITE), eng.query(_lib.HCM_CALIB_NONFINITE)) == before == (0, 0)
    assert torch.isfinite(hid).all()
    gold = np.load(os.path.join(GOLD, name + ".npz"))["result_padded"]
    assert np.array_equal(np.isnan(gold), np.isnan(r)) and np.array_equal(np.nan_to_num(gold), np.nan_to_num(r))


def test_val_step_is_legal_inside_a_stream_capture(engines):
    """After one eager call at the same shape, one val_step captured on a side stream and replayed once gives the eager result bit for bit."""
    eng = engines(PM, "fp16")
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(PM)
    e_res, e_hid, e_out = eng.val_step(obs, corrected, stop, h0, masks, return_outputs=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_res, g_hid, g_out = eng.val_step(obs, corrected, stop, h0, masks, return_outputs=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(e_res.view(torch.int32), g_res.view(torch.int32)) and torch.equal(e_hid, g_hid)
    for a, b in zip(e_out, g_out):
        assert torch.equal(a, b)
    del graph


@pytest.mark.parametrize("name,precision", [(CMA, "fp32"), (PM, "fp16")])
def test_one_time_step_equals_the_single_step_forward_plus_criteria(name, precision, engines):
    eng = engines(name, precision)
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    o1 = {k: v[:N] for k, v in obs.items()}
    res, hid, (out, st, prog) = eng.val_step(o1, corrected[:N], stop[:N], h0, masks[:N], return_outputs=True)
    fwd = eng.forward({k: v for k, v in o1.items() if k != "progress"}, h0, masks[:N])
    f_out, f_stop, f_prog, f_hid = (fwd[0], fwd[1], None, fwd[2]) if kind == "cma" else fwd
    assert torch.equal(out, f_out) and torch.equal(st, f_stop) and torch.equal(hid, f_hid)
    assert (prog is None and f_prog is None) or torch.equal(prog, f_prog)
    ref = fv.criteria(f_out, f_stop, f_prog, corrected[:N], stop[:N], o1.get("progress")).numpy()
    got = res.cpu().numpy()
    np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-5, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[3] == N


def test_argument_errors_on_a_live_engine(engines):
    eng = engines(PM, "fp32")
    kind, cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(PM)
    with pytest.raises(ValueError, match="progress"):
        eng.val_step({k: v for k, v in obs.items() if k != "progress"}, corrected, stop, h0, masks)
    with pytest.raises(ValueError, match="progress"):
        eng.val_step(dict(obs, progress=obs["progress"][:3]), corrected, stop, h0, masks)
    with pytest.raises(ValueError, match="corrected_actions"):
        eng.val_step(obs, corrected[:3], stop, h0, masks)
    with pytest.raises(ValueError, match="oracle_stop"):
        eng.val_step(obs, corrected, stop[:3], h0, masks)
    with pytest.raises(ValueError, match="masks"):
        eng.val_step(obs, corrected, stop, h0, masks[:3])
    with pytest.raises(ValueError, match="result"):
        eng.val_step(obs, corrected, stop, h0, masks, result=torch.empty(8))
    with pytest.raises(ValueError, match="multiple"):
        eng.val_step(obs, corrected, stop, torch.zeros(1, 4, cfg.hidden), masks)
    with pytest.raises(ValueError, match="hidden"):
        eng.val_step(obs, corrected, stop, torch.zeros(2, N, cfg.hidden), masks)
    # labels and masks in the other shapes the trainer may carry them in, and a caller's result row, give the same words
    a = eng.val_step(obs, corrected, stop, h0, masks)[0]
    table = torch.zeros(2, 8, device="cuda")
    b = eng.val_step(dict(obs, progress=obs["progress"].reshape(-1, 1)), corrected, stop.reshape(-1), h0, masks[:, 0], result=table[1])[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and b.data_ptr() == table[1].data_ptr() and not table[0].any()
    # one instruction for every frame (seq2seq.py:163): the library's B_instr = 1
    one = dict(obs, instruction=obs["instruction"][:1])
    r1, h1, (o1, s1, p1) = eng.val_step(one, corrected, stop, h0, masks, return_outputs=True)
    o2, s2, p2, h2 = eng.forward_seq({k: v for k, v in one.items() if k != "progress"}, h0, masks, T, N)
    assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(p1, p2) and torch.equal(h1, h2)


# ---------------------------------------------------------------- the epoch
_VALIDATOR_REF = {}


def _restated_validator(name, N, steps, batches):
    """The same epoch through the CPU stand-in (once for the module), keeping every chunk's unmasked outputs for the loss bounds."""
    from robo_vln_amd.validate import FlatValidator
    if not _VALIDATOR_REF:
        orc = fv.oracle(name)
        outs = []
        inner = orc.val_step

        def spy(*a, **k):
            k["return_outputs"] = True
            res, h, o = inner(*a, **k)
            outs.append(o)
            return res, h
        orc.val_step = spy
        _VALIDATOR_REF.update(out=FlatValidator(orc, tbptt_steps=steps, batch_size=N).run(batches), outs=outs)
    return _VALIDATOR_REF


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_validator_over_two_batches_of_three_chunks(precision, engines):
    from robo_vln_amd.validate import FlatValidator
    eng = engines(PM, precision)
    tol = TOL[precision]
    kind, cfg, _, N = fv.case(PM)
    steps = N                                                   # one time step per chunk: 3 steps -> 3 chunks of N rows
    batches = fv.epoch_batches(PM, 2, 3)
    got = FlatValidator(eng, tbptt_steps=steps, batch_size=N).run(batches)
    orc = _restated_validator(PM, N, steps, batches)
    ref = orc["out"]
    assert got["chunks"] == ref["chunks"] == 6
    mean_b = np.zeros(3)
    for i in range(6):
        corrected = batches[i // 3][3].split(steps, 0)[i % 3]
        progress = batches[i // 3][0]["progress"].split(steps, 0)[i % 3]
        r_out, r_stop, r_prog = orc["outs"][i]
        b = _bounds(tol, r_out, corrected, r_prog, progress)
        _check_losses(got["table"][i].numpy(), ref["table"][i].numpy(), b, f"{precision} chunk {i}")
        mean_b += np.asarray(b) / 6
    # the epoch figures are means of the per-chunk figures, so they obey the means of the per-chunk bounds
    for k, key in enumerate(("action_loss", "stop_loss", "aux_loss")):
        assert abs(got[key] - ref[key]) <= mean_b[k], key
    assert abs(got["val_loss"] - ref["val_loss"]) <= mean_b.sum()
