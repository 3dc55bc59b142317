"""The trainable models' gradients against the reference's own autograd, on the CPU path of the train modules: the fixtures
tests/golden/update_*.npz (tools/gen_update_golden.py: the imported reference models in float64, the criterion as the trainer writes it,
loss.backward(), and two Adam steps) against train.HighLevel / train.LowLevel, train.CMANet and train.Seq2SeqNet on the same seeded inputs.

  partition  the state-dict keys outside the frozen parts, the parameters with a gradient and the parameters with None are the fixture's sets
  float64    every figure -- losses, outputs, state, every stored gradient value, max|g|, sum|g|, every projection, the trajectory's losses, final
             state and final parameters -- within 1e-9 of the tensor's largest element (a projection: 1e-9 sqrt(n) max|g|; sum|g|: 1e-9 n max|g|).  Float64 round-off
             over these reductions is ~1e-14 and the float32 bound 5e-6: 1e-9 separates "the same function" from "the same to float32".
  zeros      a key bias cancels in the softmax: the fixture's own values are below 1e-12 of the partner weight's gradient, ours are compared on
             that scale, and where train/models.py promises exact zeros (_ZeroGrad, the unused key halves, an ablated modality) they are exact
  float32    a condition on the cases, not a tolerance on the code (tests/test_train_coverage_cpu.py): the same modules in float32 on the CPU
             stay within half the GPU bound, 5e-6, of the fixture in every figure, so that the GPU tests' 1e-5 has room for the kernels.

Measured worst figures (bound): float64 6.7e-15 (1e-9); float32 single step 2.2e-6 (update_hier_ablate_depth_T2_N2, fc_q.bias's gradient),
trajectory 2.9e-6 (update_hier_T4_N2_gru's final low-level state) (5e-6).  The inputs and the seeds that make these figures the same on every
machine: tests/update_ref.frozen_outputs, tests/update_ref.SEEDS, whose rule the last two tests check.  A NaN in any figure fails
(tests/update_ref.over, test_a_nan_anywhere_fails_the_comparison)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import update_ref as ur

NAMES = list(ur.UPDATE_CASES)
F64_BOUND = 1e-9
F32_BOUND = 5e-6          # half of the training tests' BOUND
LIMIT = 300 * 1024


def _d(t):
    return t.double()


def _f(t):
    return t


@functools.lru_cache(maxsize=None)
def _gold(name):
    return ur.load(name)


def _single(name, conv, what):
    nets = ur.modules(name, conv)
    return ur.compare(name, _gold(name), nets, ur.forward_backward(name, nets, conv), None, what)


def _trajectory(name, conv, what):
    nets = ur.modules(name, conv)
    return ur.compare(name, _gold(name), nets, None, ur.trajectory(name, nets, conv), what)


# ---------------------------------------------------------------- the fixtures themselves
@pytest.mark.parametrize("name", NAMES)
def test_fixture_places_every_reference_parameter_once_and_names_its_layers(name):
    gold = _gold(name)
    kind, cfg, T, N, trajectory = ur.case(name)
    assert os.path.getsize(os.path.join(ur.GOLD, name + ".npz")) <= LIMIT
    meta = str(gold["meta"])
    assert all(f"'layer{i}':" in meta for i in (1, 2, 3, 4)) and name in meta
    grad, nograd, frozen, buffers = ur.partition(gold)
    assert grad and frozen and not (grad & nograd or grad & frozen or nograd & frozen or buffers & (grad | nograd | frozen))
    assert {k.split("/")[0] for k in grad} == set(ur.MODELS[kind])
    for k in grad:
        assert gold["gstat/" + k].shape == (3,) and gold["gproj/" + k].shape == (ur.PROJECTIONS,)
        n, sub = int(gold["gstat/" + k][2]), int(gold["subsample"])
        assert gold["grad/" + k].size == (n if n <= sub else math.ceil(n / ur.stride_of(n, sub))) and gold["grad/" + k].dtype == np.float64
    # nothing inside a frozen part has a gradient; the trainer adds no aux loss without the monitor, so the monitor's parameters have None
    assert not any(k.split("/", 1)[1].startswith(ur.FROZEN[k.split("/")[0]]) for k in grad)
    monitor = bool(getattr(cfg, "progress_monitor", False))
    for tag in ur.MODELS[kind]:
        assert (f"{tag}/progress_monitor.weight" in grad) == monitor and (f"{tag}/progress_monitor.weight" in nograd) != monitor
    assert (float(gold["losses"][2]) > 0) == (monitor or kind == "hier")
    assert ("traj_losses" in gold) == trajectory == (name in ur.TRAJECTORY)
    if trajectory:
        assert gold["traj_losses"].shape == (ur.STEPS, ur.TERMS) and all("final/" + k in gold for k in grad)
        if name not in ur.TRAJECTORY_T:                                                     # (a trajectory on the chunk's first steps has other rows)
            assert np.array_equal(gold["traj_losses"][0], gold["losses"])                   # the first step starts from the fixture's weights
        assert all(gold["traj_losses"][1, k] != gold["traj_losses"][0, k] for k in range(ur.TERMS) if gold["losses"][k] != 0)


def test_labels_and_masks_have_the_edges():
    """mixed labels: from five rows up a padded row, a valid row with an exact 0 in corrected[:, 0], stop -1; a mask that is zero inside the chunk"""
    for name in NAMES:
        c = ur.inputs(name)
        rows = c["T"] * c["N"]
        assert rows <= 8 and float(c["corrected"][1, 0]) == 0.0 and float(c["corrected"][1, 1]) != 0.0
        if rows > 4:
            assert (c["corrected"][4] == 0).all() and float(c["stop"][4]) == -1.0
        assert (c["masks"][:, 0] == c["masks"][:, 1]).all() and (c["masks"][:c["N"], 0] == 0).any()
        if c["T"] > 2 or c["kind"] == "cma":
            assert (c["masks"][c["N"]:, 0] == 0).any()                        # a reset inside the chunk: a segment boundary of seq_forward


def test_ablated_fixture_has_exact_zero_weight_gradients_and_live_biases():
    gold = _gold("update_hier_ablate_depth_T2_N2")
    for k in ("hi/depth_kv.weight", "hi/depth_linear.1.weight", "hi/depth_encoder.spatial_embeddings.weight", "lo/depth_encoder.visual_fc.1.weight"):
        assert gold["gstat/" + k][0] == 0.0 and not gold["grad/" + k].any() and not gold["gproj/" + k].any(), k
    for k in ("hi/depth_kv.bias", "hi/depth_linear.1.bias", "hi/rgb_kv.weight", "hi/rgb_linear.2.weight"):
        assert gold["gstat/" + k][0] > 0.0, k
    gold = _gold("update_cma_ablate_instr_T2_N2")
    for k in ("net/instruction_encoder.embedding_layer.weight", "net/instruction_encoder.encoder_rnn.weight_hh_l0", "net/text_k.weight"):
        assert gold["gstat/" + k][0] == 0.0, k
    assert gold["gstat/net/text_q.bias"][0] > 0.0 and gold["gstat/net/rgb_kv.weight"][0] > 0.0


# ---------------------------------------------------------------- the encoding catches what it is there for
def test_the_subsample_catches_a_scaled_tensor_and_the_projections_a_zeroed_row():
    g = np.random.RandomState(5).standard_normal((700, 300))
    key, sub = "some/weight", 256
    values, stat, proj = ur.encode(key, g, sub)
    assert values.size == math.ceil(g.size / ur.stride_of(g.size, sub)) <= sub
    assert max(ur.errors(key, g, values, stat, proj, sub)) == 0.0
    assert max(ur.errors(key, g.astype(np.float32), values, stat, proj, sub)) <= 1e-7
    scaled = ur.errors(key, g * (1 + 1e-4), values, stat, proj, sub)
    assert scaled[0] > 1e-5                                                   # a dense error: every stored value moves
    row = g.copy()
    row[17] = 0                                                               # a sparse one: 300 of 210000 elements
    e = ur.errors(key, row, values, stat, proj, sub)
    assert e[3] > 1e-5 and e[2] > 1e-4
    one = g.copy()
    one[123, 46] += 1e-3                                                      # a single element off the stride
    assert (123 * 300 + 46) % ur.stride_of(g.size, sub) != 0
    e = ur.errors(key, one, values, stat, proj, sub)
    assert e[0] == 0.0 and e[3] * math.sqrt(g.size) * stat[0] == pytest.approx(1e-3, rel=1e-6)
    # another key draws other signs
    assert not np.array_equal(ur.signs(key, 64), ur.signs("other/weight", 64))
    zeros = ur.encode(key, np.zeros(2000), sub)
    assert max(ur.errors(key, np.zeros(2000), *zeros, sub)) == 0.0 and min(ur.errors(key, np.full(2000, 1e-30), *zeros, sub)) == math.inf


# ---------------------------------------------------------------- float64: the same function
@pytest.mark.parametrize("name", NAMES)
def test_float64_cpu_path_matches_the_reference_autograd(name):
    worst = _single(name, _d, "float64 CPU path")
    assert not ur.over(worst, F64_BOUND), ur.over(worst, F64_BOUND)


@pytest.mark.parametrize("name", ur.TRAJECTORY)
def test_float64_adam_trajectory_matches_the_reference_s(name):
    worst = _trajectory(name, _d, "float64 CPU path, trajectory")
    assert not ur.over(worst, F64_BOUND), ur.over(worst, F64_BOUND)


def test_ablated_modality_gets_exact_zero_gradients_not_none():
    name = "update_hier_ablate_depth_T2_N2"
    nets = ur.modules(name, _d)
    ur.forward_backward(name, nets, _d)
    hi = dict(nets["hi"].named_parameters())
    for k in ("depth_kv.weight", "depth_linear.1.weight", "depth_encoder.spatial_embeddings.weight"):
        assert hi[k].grad is not None and not hi[k].grad.any(), k
    assert hi["depth_kv.bias"].grad.any() and hi["depth_linear.1.bias"].grad.any()


# ---------------------------------------------------------------- float32: the cases leave the GPU bound its room
@pytest.mark.parametrize("name", NAMES)
def test_float32_cpu_path_stays_within_half_the_gpu_bound(name):
    worst = _single(name, _f, "float32 CPU path")
    assert not ur.over(worst, F32_BOUND), ur.over(worst, F32_BOUND)


@pytest.mark.parametrize("name", ur.TRAJECTORY)
def test_float32_trajectory_stays_within_half_the_gpu_bound(name):
    worst = _trajectory(name, _f, "float32 CPU path, trajectory")
    assert not ur.over(worst, F32_BOUND), ur.over(worst, F32_BOUND)


# ---------------------------------------------------------------- a NaN is an error, wherever it sits
def test_a_nan_anywhere_fails_the_comparison():
    name = "update_s2s_pm_T3_N2_gru"
    nets = ur.modules(name, _d)
    run = ur.forward_backward(name, nets, _d)
    nets["net"].linear.weight.grad.fill_(float("nan"))                       # not the first figure of the comparison
    worst = ur.compare(name, _gold(name), nets, run, None, "NaN gradient")
    assert set(ur.over(worst, F64_BOUND)) == {"grad/net/linear.weight", "gsum/net/linear.weight", "gproj/net/linear.weight"}
    assert math.isnan(ur.worse(0.0, float("nan"), 1.0)) and ur.worse() == 0.0 and ur.worse(1.0, 3.0, 2.0) == 3.0
    nets = ur.modules(name, _d)
    losses, counts, state = ur.trajectory(name, nets, _d)
    with torch.no_grad():
        nets["net"].stop_linear.bias.fill_(float("nan"))
        losses[1, 1] = float("nan")
    worst = ur.compare(name, _gold(name), nets, None, (losses, counts, state), "NaN parameter")
    assert {"step 1 loss[1]", "final/net/stop_linear.bias", "fproj/net/stop_linear.bias"} <= set(ur.over(worst, F64_BOUND))
    assert not ur.over({"a": 1e-10, "b": 0.0}, F64_BOUND) and set(ur.over({"a": 1e-10, "b": math.inf, "c": float("nan")}, F64_BOUND)) == {"b", "c"}


# ---------------------------------------------------------------- the seeds are the rule's
@pytest.mark.parametrize("name", NAMES)
def test_the_case_s_seed_meets_both_conditions(name):
    """tests/update_ref.SEEDS: the chosen weight seed keeps every ReLU off its kink and the float32 run within the half bound (first_seed finds
    it; a whole search is too slow for a test)"""
    seed = ur.SEEDS.get(name, ur.cases.SEED)
    margin, cond = ur.kink_margin(name, seed), ur.conditioning(name, seed)
    print(f"{name} seed {seed}: kink margin {margin:.2f} (at least {ur.KINK_RATIO}), conditioning {cond:.2e} (at most {ur.SEED_BOUND})")
    assert margin >= ur.KINK_RATIO and cond <= ur.SEED_BOUND
    assert set(ur.SEEDS) <= set(NAMES) and all(s > ur.cases.SEED for s in ur.SEEDS.values())


def test_the_seed_before_a_chosen_one_fails_the_rule():
    for name, seed in list(ur.SEEDS.items()):
        assert ur.kink_margin(name, seed - 1) < ur.KINK_RATIO or ur.conditioning(name, seed - 1) > ur.SEED_BOUND, name
