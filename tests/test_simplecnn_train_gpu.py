"""train.simple_cnn on the device (csrc/simplecnn_train.hip) against the float64 autograd of its restatement on the CPU, its exact-bit
properties, and the SimpleCNN models around it: both model cases of tests/simplecnn_train_cases.py through update_loss + backward and the two-step
train.hier_update / train.flat_update trajectory against the reference's fixtures and the oracle's functions in float64 under torch autograd, and the round trip of a trained
state dict into HCMEngine.

Every case of tests/simplecnn_train_cases.OP_CASES crosses a boundary of the kernels' tiling (see the comment there).  The issue's eight cases
stay below the 16384 output pixels from which a weight-gradient chunk grows past 64 pixels, so one case is added: 5 rows of 256 x 256 depth
(19845 map-1 pixels, chunks of 96), the smallest that crosses it; the largest chunk, 1024 pixels, needs 64 rows of 256 x 256 and is measured
off the suite (profiles/simplecnn_train.md).  The models run against the fixtures of tools/gen_simplecnn_update_golden.py (the reference's own
float64 autograd) and against the oracle's functions under float64 autograd (tests/simplecnn_train_cases.run_oracle).  The bound is the
project's per-tensor rule, max|g - g_ref| / max|g_ref| <= 1e-5, forward values on their tensor's largest element.

Worst figure per case (the op: forward / worst of the six gradients; the models: worst figure against the oracle's float64 autograd and,
`fixture`, against the reference's own), MI355X:
    simple_cnn B1_36x36_c1: forward 3.752e-07, gradients 5.168e-07
    simple_cnn B3_36x36_c3: forward 5.100e-07, gradients 4.800e-07
    simple_cnn B2_40x52_c1: forward 4.839e-07, gradients 4.106e-07
    simple_cnn B5_50x50_c3: forward 5.678e-07, gradients 5.406e-07
    simple_cnn B3_52x66_c1: forward 8.801e-07, gradients 3.281e-07
    simple_cnn B2_64x64_c3: forward 6.158e-07, gradients 4.410e-07
    simple_cnn B6_64x64_c1: forward 4.503e-07, gradients 4.609e-07
    simple_cnn B2_128x128_c1: forward 6.017e-07, gradients 3.429e-07
    simple_cnn B5_256x256_c1: forward 1.122e-06, gradients 8.016e-07
    simple_cnn B2_64x64_c3 uint8: forward 6.158e-07, gradients 4.410e-07
    update_lo_simplecnn_T2_N2 [hip]: worst 1.010e-06 (grad/state_encoder.rnn.weight_ih_l0); gradients 1.010e-06, final parameters 8.730e-07
    update_lo_simplecnn_T2_N2 [auto]: worst 1.282e-06 (grad/linear.weight); gradients 1.282e-06, final parameters 5.371e-07
    update_s2s_simplecnn_T3_N2_gru [hip]: worst 1.168e-06 (grad/depth_encoder.cnn.7.weight); gradients 1.168e-06, final parameters 7.187e-07
    update_s2s_simplecnn_T3_N2_gru [auto]: worst 9.086e-07 (grad/linear.bias); gradients 9.086e-07, final parameters 6.589e-07
    update_lo_simplecnn_T2_N2 fixture [hip]: worst 9.654e-07 (grad/state_encoder.rnn.bias_ih_l0); gradients 9.654e-07, final parameters 7.447e-07
    update_lo_simplecnn_T2_N2 fixture [auto]: worst 8.595e-07 (grad/linear.weight); gradients 8.595e-07, final parameters 5.490e-07
    update_s2s_simplecnn_T3_N2_gru fixture [hip]: worst 7.199e-07 (grad/linear.bias); gradients 7.199e-07, final parameters 2.322e-07
    update_s2s_simplecnn_T3_N2_gru fixture [auto]: worst 9.086e-07 (grad/linear.bias); gradients 9.086e-07, final parameters 1.610e-07
    round trip: engine against train model 2.384e-07 / 5.960e-08
"""
import pytest
import torch

from robo_vln_amd import train
from tests import simplecnn_train_cases as sc

pytestmark = pytest.mark.gpu

NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


def _device_run(x, params, d_y, scale):
    ps = [p.cuda().requires_grad_(True) for p in params]
    y = train.simple_cnn(x.cuda(), *ps, scale=scale)
    grads = torch.autograd.grad(y, ps, d_y.cuda())
    return y.detach(), list(grads)


def _check(case, uint8):
    seed = sc.OP_SEEDS[case]
    assert sc.op_kink_margin(case, seed) >= sc.KINK_RATIO
    x, params, d_y = sc.op_inputs(case, seed, uint8)
    y_ref, g_ref, _ = sc.op_reference(case, seed)
    y, g = _device_run(x, params, d_y, sc.op_scale(case[3]))
    fig = {"y": sc.rel(y, y_ref), **{n: sc.rel(a, b) for n, a, b in zip(NAMES, g, g_ref)}}
    print(f"simple_cnn {sc.op_id(case)}{' uint8' if uint8 else ''}: forward {fig['y']:.3e}, gradients {max(fig[n] for n in NAMES):.3e}  "
          + " ".join(f"{n} {fig[n]:.2e}" for n in NAMES))
    assert not {k: v for k, v in fig.items() if not v <= sc.BOUND}


@pytest.mark.parametrize("case", sc.OP_CASES, ids=sc.op_id)
def test_op_against_float64_autograd(case):
    _check(case, False)


def test_op_uint8_rgb_frames_against_float64_autograd():
    _check(sc.UINT8_CASE, True)


def test_two_runs_give_equal_bits():
    case = (5, 50, 50, 3)
    x, params, d_y = sc.op_inputs(case, 0)
    a, b = _device_run(x, params, d_y, 1 / 255.0), _device_run(x, params, d_y, 1 / 255.0)
    assert torch.equal(a[0], b[0])
    for n, p, q in zip(NAMES, a[1], b[1]):
        assert torch.equal(p, q), n


def test_a_rows_forward_bits_do_not_depend_on_the_batch():
    case = (5, 50, 50, 3)
    x, params, _ = sc.op_inputs(case, 0)
    ps = [p.cuda() for p in params]
    with torch.no_grad():
        y = train.simple_cnn(x.cuda(), *ps, scale=1 / 255.0)
        for r in range(case[0]):
            assert torch.equal(train.simple_cnn(x[r:r + 1].cuda(), *ps, scale=1 / 255.0)[0], y[r]), r


def test_uncovered_frame_columns_do_not_reach_dw1():
    """W = 50: the windows of conv1 end at column 47, so columns 48 and 49 are read by nobody -- garbage there leaves dW1's bits alone"""
    case = (5, 50, 50, 3)
    x, params, d_y = sc.op_inputs(case, 0)
    zero, junk = x.clone(), x.clone()
    zero[:, :, 48:], junk[:, :, 48:] = 0, 1e30
    zero[:, 48:], junk[:, 48:] = 0, 1e30
    a, b = _device_run(zero, params, d_y, 1 / 255.0), _device_run(junk, params, d_y, 1 / 255.0)
    assert torch.equal(a[1][0], b[1][0]) and torch.isfinite(b[1][0]).all()


def test_uncovered_map_pixels_receive_exact_zeros():
    """W = 50: map 1 is 11 wide and conv2 reads columns 0-9, so column 10 has a zero gradient and dW1 is what the frame columns 0-43 give: a
    cotangent reaching conv1 through column 10 would show in dW1[..., 4:] against the float64 reference (covered by the parity test); here the
    sharper form -- with b1 = -1e3 map 1 is all non-positive, the gate closes everywhere and dW1, db1, dW2 are exact zeros"""
    case = (5, 50, 50, 3)
    x, params, d_y = sc.op_inputs(case, 0)
    params = list(params)
    params[1] = torch.full((32,), -1e3)
    _, g = _device_run(x, params, d_y, 1 / 255.0)
    for n in ("dW1", "db1", "dW2"):
        assert (g[NAMES.index(n)] == 0).all(), n
    assert (g[NAMES.index("dW3")] != 0).any()


# ---------------------------------------------------------------- the models
@pytest.mark.parametrize("route", ["hip", "auto"])
@pytest.mark.parametrize("name", list(sc.MODEL_CASES))
def test_update_step_and_trajectory_against_the_oracles_autograd(name, route):
    """Both model cases on the device -- the encoders' convolutions on the op ("hip") and on the modules' own measured routing ("auto") -- through
    update_loss + backward and the two-step train.hier_update / train.flat_update trajectory, against the oracle's functions in float64 under
    torch autograd and Adam (tests/simplecnn_train_cases.run_oracle): every loss, state, gradient and final parameter within the bound per
    tensor on its largest element, the counts and the sets of gradients exact"""
    seed = sc.MODEL_SEEDS[name]
    worst = sc.compare(f"{name} [{route}]", sc.run_train(name, seed, lambda t: t.cuda(), route), sc.oracle_run(name, seed))
    assert not {k: v for k, v in worst.items() if not v <= sc.BOUND}


@pytest.mark.parametrize("route", ["hip", "auto"])
@pytest.mark.parametrize("name", list(sc.MODEL_CASES))
def test_update_step_and_trajectory_against_the_reference_fixture(name, route):
    """The same runs against the fixtures recorded from the imported reference's own float64 autograd and Adam
    (tools/gen_simplecnn_update_golden.py), by update_ref.errors' figures: within the bound, counts and the sets of gradients exact"""
    worst = sc.compare_gold(f"{name} fixture [{route}]", sc.run_train(name, sc.MODEL_SEEDS[name], lambda t: t.cuda(), route), sc.load_gold(name))
    assert not {k: v for k, v in worst.items() if not v <= sc.BOUND}


def test_trained_state_dict_runs_in_the_engine():
    """Two train.hier_update steps with the SimpleCNN low-level model on the kernels, then LowLevel.state_dict() into HCMEngine(precision fp32):
    the engine's low_forward on the same frames agrees with the train model's forward at the project's fp32 tolerance"""
    from robo_vln_amd.policy import HCMEngine
    from tests import update_ref as ur
    name = "update_lo_simplecnn_T2_N2"
    c = sc.model_inputs(name, 0)
    cfg, N = c["cfg"], c["N"]
    conv = lambda t: t.cuda()
    net, high = sc.build_model(name, 0, conv, "hip"), sc._high(conv)
    before = net.depth_encoder.cnn[0].weight.detach().clone()
    obs = {k: v.cuda() for k, v in c["obs"].items()}
    opt, opt_hi = torch.optim.Adam(net.parameters(), **ur.ADAM), torch.optim.Adam(high.parameters(), **ur.ADAM)
    state, hi_state = c["h0"].cuda(), torch.zeros(1, N, cfg.hidden, device="cuda")
    for _ in range(2):
        _, _, hi_state, state = train.hier_update(high, net, opt_hi, opt, obs, c["prev"].cuda(), c["masks"].cuda(), c["corrected"], c["stop"], hi_state, state)
    assert not torch.equal(net.depth_encoder.cnn[0].weight, before)
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    step_obs = {k: obs[k][:N].contiguous() for k in ("rgb", "depth")}
    st, m, h0 = c["sub"][:N].clamp(max=cfg.num_sub_tasks - 1).cuda(), torch.ones(N, device="cuda"), c["h0"].cuda()
    with torch.no_grad():
        vel, stop_out, h2 = net((step_obs, h0, None, m.view(N, 1), st))
    eng = HCMEngine(cfg, None, sd, max_batch=N, precision="fp32", graph=False)
    e_vel, e_stop, e_h = eng.low_forward(step_obs, h0.contiguous(), m, st)
    torch.cuda.synchronize()
    e1, e2 = (e_vel - vel).abs().max().item(), (e_stop - stop_out).abs().max().item()
    print(f"round trip: engine against train model {e1:.3e} / {e2:.3e}")
    assert e1 <= 1e-3 and e2 <= 1e-3
    assert ((e_h - h2).norm() / h2.norm()).item() <= 1e-3
    eng.close()
