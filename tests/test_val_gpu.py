"""Teacher-forced validation step on the GPU (hcm_val_step, HCMEngine.val_step, HCMValidator): the criterion kernel against torch's
criteria on the call's own outputs, bit-identity with the two sequence calls, parity with the golden and the CPU restatement, the NaN
contract, out-of-range labels, capture-legality and the validation epoch.

One engine per (case, precision) and one CPU restatement per case for the whole module.

Measured on one MI355X: the file's 23 tests take 12.4 s (`pytest --durations=0`; the largest items are the engines, 1.3-1.6 s each, created
inside the first test that needs one).  Largest measured errors against the restatement / golden, bounds in brackets: fp32 cross-entropy
2.0e-6 [2e-3], action 7.7e-7 [5.5e-4], stop 7.2e-7 [1e-3]; fp16 cross-entropy 1.3e-3 [2e-2], action 7.7e-4 [5.6e-3], stop 7.7e-4 [1e-2];
correct / total equal in every case."""
import math
import os

import numpy as np
import pytest
import torch

from tests import val_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 1e-2}       # the output tolerance of tests/test_parity_gpu.py


@pytest.fixture(scope="module")
def engines():
    from robo_vln_amd.policy import HCMEngine
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            cfg, T, N = val_ref.case(name)
            made[(name, precision)] = HCMEngine(cfg, *val_ref.weights(cfg), max_batch=T * N, precision=precision)
        return made[(name, precision)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def restated():
    made = {}

    def get(name):
        if name not in made:
            cfg, T, N = val_ref.case(name)
            orc = val_ref.ValOracle(cfg, *val_ref.weights(cfg))
            obs, corrected, stop, m = val_ref.observations(cfg, T, N)
            h0 = val_ref.h0(cfg, N)
            made[name] = orc.val_step(obs, corrected, stop, h0.clone(), h0.clone(), m, return_outputs=True)
        return made[name]
    return get


def _inputs(name, kind="mixed"):
    cfg, T, N = val_ref.case(name)
    obs, corrected, stop, m = val_ref.observations(cfg, T, N, kind)
    obs = {k: torch.from_numpy(v).cuda() for k, v in obs.items()}
    masks = torch.from_numpy(m).view(-1, 1).expand(-1, 2).contiguous().cuda()          # reference-shaped (T*N, 2)
    h0 = val_ref.h0(cfg, N).cuda()
    return cfg, T, N, obs, torch.from_numpy(corrected).cuda(), torch.from_numpy(stop).cuda(), masks, h0


def _check_losses(got, ref, vel_ref, corrected, tol, what):
    """The bounds of the three losses from the output tolerance `tol`: cross-entropy 2*tol (log-sum-exp and the picked logit are each
    1-Lipschitz in the largest logit error), stop tol (BCE-with-logits is 1-Lipschitz in the logit), action 2*tol*mean|vel_ref - target| +
    tol^2 (|a^2 - b^2| <= 2|b||a-b| + |a-b|^2, element by element)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    c = torch.as_tensor(corrected).float().cpu()
    resid = (torch.as_tensor(vel_ref).float().cpu().masked_fill(c == 0, 0) - c).abs().mean().item()
    bounds = (2 * tol, 2 * tol * resid + tol * tol, tol)
    errs = [abs(got[i] - ref[i]) for i in range(3)]
    print(f"{what}: |cross-entropy| err {errs[0]:.3e} (<= {bounds[0]:.1e})  |action| err {errs[1]:.3e} (<= {bounds[1]:.2e})  "
          f"|stop| err {errs[2]:.3e} (<= {bounds[2]:.1e})  correct/total {got[3]:.0f}/{got[4]:.0f} vs {ref[3]:.0f}/{ref[4]:.0f}")
    for e, b in zip(errs, bounds):
        assert e <= b
    assert got[3] == ref[3] and got[4] == ref[4]
    return bounds


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_criterion_kernel_is_exact_on_the_calls_own_outputs(precision, engines):
    """Only the order of an f32 sum differs between the kernel and torch's criteria applied on the CPU to the outputs the same call
    returned: relative 1e-5 on the three losses (T*N <= 64 terms of magnitude O(1)), counts equal."""
    name = "val_T4_N2_gru"
    eng = engines(name, precision)
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hh, lh, (logits, vel, st) = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    assert res.shape == (8,) and res.dtype == torch.float32 and res.is_cuda
    ref = val_ref.criteria(logits, vel, st, obs["vln_oracle_action_sensor"], corrected, stop, cfg.num_sub_tasks).numpy()
    got = res.cpu().numpy()
    print(f"{precision}: kernel {got} torch {ref}")
    np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-5, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[4] == 7 and got[5] == 7 and got[6] == 0 and got[7] == 0


def _kernel_alone(logits, vel, stop, oracle, corrected, ostop, num_sub_tasks=4):
    import ctypes as C
    from robo_vln_amd import _lib
    dev = [t.cuda().contiguous() for t in (logits.float(), vel.float(), stop.float(), oracle.reshape(-1).to(torch.int64), corrected.float(), ostop.float())]
    res = torch.full((8,), -7.0, device="cuda")
    rc = _lib.lib().hcm_op_val_loss(*[t.data_ptr() for t in dev], res.data_ptr(), logits.shape[0], logits.shape[1], num_sub_tasks,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return res.cpu().numpy()


@pytest.mark.parametrize("rows,A", [(70, 4), (300, 4), (1000, 8)])
def test_criterion_kernel_alone_over_many_rows(rows, A):
    """More rows than one wave (70), than the workgroup (300: the stride) and several strides (1000), with A = 8 logits: every lane, all four
    waves' LDS sums and the integer counts carry data.  Against torch's criteria in fp32 on the CPU.  Bound, from the number format: each side
    sums `rows` f32 terms of one sign in its own order, which costs at most rows * 2^-24 relative per side; the issue's 1e-5 (set for up to 64
    terms) is kept on top for the exp / log evaluations: rtol = 2 * rows * 2^-24 + 1e-5."""
    g = torch.Generator().manual_seed(rows)
    logits = torch.randn(rows, A, generator=g) * 2
    vel = torch.randn(rows, 2, generator=g)
    stop = torch.randn(rows, 1, generator=g) * 3
    oracle = torch.randint(0, 5, (rows,), generator=g)
    corrected = torch.randn(rows, 2, generator=g)
    corrected[torch.rand(rows, 2, generator=g) < 0.2] = 0
    ostop = torch.randint(-1, 2, (rows, 1), generator=g).float()
    got = _kernel_alone(logits, vel, stop, oracle, corrected, ostop)
    ref = val_ref.criteria(logits, vel, stop, oracle, corrected, ostop).numpy()
    print(f"rows {rows}: kernel {got} torch {ref} rel {np.abs(got[:3] - ref[:3]) / np.abs(ref[:3])}")
    np.testing.assert_allclose(got[:3], ref[:3], rtol=2 * rows * 2.0 ** -24 + 1e-5, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[4] > rows // 2 and got[5] > rows // 2        # (uniform labels: 4 of 5 and 2 of 3 rows are valid)
    again = _kernel_alone(logits, vel, stop, oracle, corrected, ostop)
    assert got.tobytes() == again.tobytes()
    # labels in the last rows only: what the last stride's lanes hold must arrive
    o2 = torch.zeros(rows, dtype=torch.int64); o2[-1] = 2
    s2 = torch.full((rows, 1), -1.0); s2[-2] = 1.0
    got = _kernel_alone(logits, vel, stop, o2, corrected, s2)
    ref = val_ref.criteria(logits, vel, stop, o2, corrected, s2).numpy()
    np.testing.assert_allclose(got[:3], ref[:3], rtol=2 * rows * 2.0 ** -24 + 1e-5, atol=0)
    assert got[3:].tolist() == ref[3:].tolist() and got[4] == 1 and got[5] == 1


def test_criterion_kernel_counts_a_nan_logit_as_torch_argmax_does():
    logits = torch.tensor([[0.1, float("nan"), 0.3, 0.2], [float("nan"), 0.5, 0.1, float("nan")], [0.3, 0.1, 0.9, 0.2]])
    oracle = torch.tensor([2, 1, 3])
    z2, z1 = torch.zeros(3, 2), torch.zeros(3, 1)
    got = _kernel_alone(logits, z2, z1, oracle, z2, z1)
    ref = val_ref.criteria(logits, z2, z1, oracle, z2, z1).numpy()
    assert math.isnan(got[0]) and math.isnan(ref[0])
    assert got[3:].tolist() == ref[3:].tolist() == [3, 3, 3, 0, 0]


@pytest.mark.parametrize("name,precision", [("val_T4_N2_gru", "fp32"), ("val_T4_N2_gru", "fp16"), ("val_T4_N2_gru", "bf16"),
                                            ("val_T4_N2_lstm", "fp16"), ("val_T4_N2_lstm", "fp32")])
def test_outputs_are_bit_identical_to_the_two_sequence_calls(name, precision, engines):
    eng = engines(name, precision)
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hh, lh, (logits, vel, st) = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    l2, hh2 = eng.high_forward_seq(obs, h0, masks)
    v2, s2, lh2 = eng.low_forward_seq(obs, h0, masks, val_ref.remap(obs["vln_oracle_action_sensor"].cpu(), cfg.num_sub_tasks).cuda())
    for a, b, what in ((logits, l2, "logits"), (vel, v2, "vel"), (st, s2, "stop"), (hh, hh2, "hi_hidden"), (lh, lh2, "lo_hidden")):
        assert torch.equal(a, b), what
    # the same call again, this time without the optional outputs: the same eight words
    res2, hh3, lh3 = eng.val_step(obs, corrected, stop, h0, h0, masks)
    assert torch.equal(res.view(torch.int32), res2.view(torch.int32)) and torch.equal(hh, hh3) and torch.equal(lh, lh3)


@pytest.mark.parametrize("name", list(val_ref.VAL_CASES))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_parity_with_golden_and_restatement(name, precision, engines, restated):
    eng = engines(name, precision)
    tol = TOL[precision]
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    res, hh, lh, (logits, vel, st) = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    r_res, r_hh, r_lh, (r_logits, r_vel, r_stop) = restated(name)
    for got, ref in ((logits, r_logits), (vel, r_vel), (st, r_stop)):
        assert (got.cpu() - ref).abs().max().item() <= tol
    _check_losses(res.cpu().numpy(), r_res.numpy(), r_vel, corrected, tol, f"{name} {precision} vs restatement")
    if name in val_ref.VAL_GOLDEN:
        gold = np.load(os.path.join(GOLD, name + ".npz"))
        for got, key in ((logits, "logits"), (vel, "vel"), (st, "stop")):
            assert np.abs(got.cpu().numpy() - gold[key]).max() <= tol
        _check_losses(res.cpu().numpy(), gold["result"], r_vel, corrected, tol, f"{name} {precision} vs golden")


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_all_padded_labels_give_nan_and_leave_the_guard_alone(precision, engines):
    from robo_vln_amd import _lib
    name = "val_T4_N2_gru"
    eng = engines(name, precision)
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name, "padded")
    before = (eng.query(_lib.HCM_STEP_NONFINITE), eng.query(_lib.HCM_CALIB_NONFINITE))
    res, hh, lh = eng.val_step(obs, corrected, stop, h0, h0, masks)
    r = res.cpu().numpy()
    assert math.isnan(r[0]) and math.isnan(r[2]) and r[1] == 0.0 and r[3:].tolist() == [0, 0, 0, 0, 0]
    assert (eng.query(_lib.HCM_STEP_NONFINITE), eng.query(_lib.HCM_CALIB_NONFINITE)) == before == (0, 0)
    assert torch.isfinite(hh).all() and torch.isfinite(lh).all()
    gold = np.load(os.path.join(GOLD, name + ".npz"))["result_padded"]
    assert np.array_equal(np.isnan(gold), np.isnan(r)) and np.array_equal(np.nan_to_num(gold), np.nan_to_num(r))


def test_out_of_range_label_is_counted_and_raised(engines, restated):
    """The kernels clamp before use: the row is counted, treated as padded, and the low-level model gets the padded sub-task."""
    name = "val_T4_N2_gru"
    eng = engines(name, "fp32")
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name, "bad")
    res, hh, lh, (logits, vel, st) = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    r = res.cpu().numpy()
    assert r[6] == 1 and r[4] == 6 and r[5] == 7 and np.isfinite(r).all()
    ref = val_ref.criteria(logits, vel, st, obs["vln_oracle_action_sensor"], corrected, stop, cfg.num_sub_tasks).numpy()
    np.testing.assert_allclose(r[:3], ref[:3], rtol=1e-5, atol=0)
    assert r[3:].tolist() == ref[3:].tolist()
    v2, s2, _ = eng.low_forward_seq(obs, h0, masks, val_ref.remap(obs["vln_oracle_action_sensor"].cpu(), cfg.num_sub_tasks).cuda())
    assert torch.equal(vel, v2) and torch.equal(st, s2)
    with pytest.raises(ValueError, match="outside"):
        eng.check_val_result(res)


def test_val_step_is_legal_inside_a_stream_capture(engines):
    """After one eager call at the same shape, one val_step captured on a side stream and replayed once gives the eager result bit for bit."""
    name = "val_T4_N2_gru"
    eng = engines(name, "fp16")
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    e_res, e_hh, e_lh, e_out = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_res, g_hh, g_lh, g_out = eng.val_step(obs, corrected, stop, h0, h0, masks, return_outputs=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(e_res.view(torch.int32), g_res.view(torch.int32))
    assert torch.equal(e_hh, g_hh) and torch.equal(e_lh, g_lh)
    for a, b in zip(e_out, g_out):
        assert torch.equal(a, b)
    del graph


def test_argument_errors_on_a_live_engine(engines):
    name = "val_T4_N2_gru"
    eng = engines(name, "fp32")
    cfg, T, N, obs, corrected, stop, masks, h0 = _inputs(name)
    with pytest.raises(ValueError, match="vln_oracle_action_sensor"):
        eng.val_step(dict(obs, vln_oracle_action_sensor=obs["vln_oracle_action_sensor"][:3]), corrected, stop, h0, h0, masks)
    with pytest.raises(ValueError, match="result"):
        eng.val_step(obs, corrected, stop, h0, h0, masks, result=torch.empty(8))
    with pytest.raises(ValueError, match="multiple"):
        eng.val_step(obs, corrected, stop, torch.zeros(1, 3, cfg.hidden), torch.zeros(1, 3, cfg.hidden), masks)
    # labels in the other dtypes and shapes the trainer may carry them in give the same words
    a = eng.val_step(obs, corrected, stop, h0, h0, masks)[0]
    b = eng.val_step(dict(obs, vln_oracle_action_sensor=obs["vln_oracle_action_sensor"].reshape(-1).long()), corrected, stop.reshape(-1), h0, h0, masks[:, 0])[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_validator_over_two_batches_of_three_chunks(precision, engines):
    from robo_vln_amd.validate import HCMValidator
    from tests.test_val_cpu import _batches
    name = "val_T4_N2_gru"
    eng = engines(name, precision)
    tol = TOL[precision]
    cfg, _, N = val_ref.case(name)
    steps = N                                                   # one time step per chunk: 3 steps -> 3 chunks of N rows
    batches = _batches(cfg, 2, 3, N)
    got = HCMValidator(eng, tbptt_steps=steps, batch_size=N).run(batches)
    orc = _restated_validator(cfg, N, steps, batches)
    ref = orc["out"]
    assert got["chunks"] == ref["chunks"] == 6
    low_bound = 0.0
    for i in range(6):
        corrected = batches[i // 3][3].split(steps, 0)[i % 3]
        b = _check_losses(got["table"][i].numpy(), ref["table"][i].numpy(), orc["vel"][i], corrected, tol, f"{precision} chunk {i}")
        low_bound += (b[1] + b[2]) / 6
        assert got["table"][i, 5] == ref["table"][i, 5] and got["table"][i, 6] == 0
    # the epoch figures are means of the per-chunk figures, so they obey the means of the per-chunk bounds
    assert got["accuracy"] == ref["accuracy"]
    assert abs(got["high_loss"] - ref["high_loss"]) <= 2 * tol and abs(got["low_loss"] - ref["low_loss"]) <= low_bound


_VALIDATOR_REF = {}


def _restated_validator(cfg, N, steps, batches):
    """The same epoch through the CPU restatement (once for the module), keeping every chunk's unmasked vel for the action-loss bound."""
    from robo_vln_amd.validate import HCMValidator
    if not _VALIDATOR_REF:
        orc = val_ref.ValOracle(cfg, *val_ref.weights(cfg))
        vels = []
        inner = orc.val_step

        def spy(*a, **k):
            k["return_outputs"] = True
            res, hh, lh, (logits, vel, stop) = inner(*a, **k)
            vels.append(vel)
            return res, hh, lh
        orc.val_step = spy
        _VALIDATOR_REF.update(out=HCMValidator(orc, tbptt_steps=steps, batch_size=N).run(batches), vel=vels)
    return _VALIDATOR_REF
