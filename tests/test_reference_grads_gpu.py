"""The trainable models' gradients against the reference's own autograd, on the device: the fixtures tests/golden/update_*.npz
(tools/gen_update_golden.py: the imported reference models in float64, the criterion as the trainer writes it, loss.backward(), and two Adam
steps -- the pair's on the first two steps of its chunk) against train.HighLevel / train.LowLevel, train.CMANet and train.Seq2SeqNet with every op on its HIP kernel, on the same seeded inputs.
The trunk features and the BERT stream (tests/update_ref.frozen_outputs: the computation of tests/features_ref.trunk_features and
oracle/hcm_oracle.bert_encoder in float64, rounded to 1/4096 so that every machine gets the same bits) are computed on the CPU, once, and moved
to the device; nothing outside the repository is read.

The bound is the project's rule for the training ops, BOUND = 1e-5: per tensor max|g - g_ref| / max|g_ref| on the stored values, forward values
on their tensor's largest element, a projection on sqrt(n) max|g_ref|, sum|g| on n max|g_ref| (tests/update_ref.errors).  The counts, the
partition of the parameters into gradient / None, and the zeros train/models.py promises are exact; a cancelling key bias is held to the bound on its
weight's scale.  The float32 CPU run of the same modules stays within half of it (tests/test_reference_grads_cpu.py), which leaves the kernels
the other half.

Measured on an MI355X, worst figure per case (bound 1e-5), single step / two-step trajectory:
  update_hier_T4_N2_gru            3.2e-6 (the low-level stop_linear.weight's gradient) / 3.8e-6 (final high-level state)
  update_hier_ablate_depth_T2_N2   2.0e-6 (fc_q.bias's gradient)
  update_cma_T4_N2                 1.6e-6 (out) / 3.0e-6 (final state)
  update_cma_ablate_instr_T2_N2    2.8e-6 (out)
  update_s2s_T4_N2_gru             2.1e-6 (stop)
  update_s2s_pm_T3_N2_gru          3.3e-6 (stop) / 3.3e-6 (final state)
Losses within 8.7e-7, gradients within 3.2e-6, final parameters within 3.8e-6.  A NaN in any figure fails (tests/update_ref.over).  The file
takes 10 s, 3.5 s of it the inputs on the CPU."""
import functools

import pytest
import torch

from tests import update_ref as ur

pytestmark = pytest.mark.gpu
BOUND = 1e-5
NAMES = list(ur.UPDATE_CASES)


def _cuda(t):
    return t.cuda()


@functools.lru_cache(maxsize=None)
def _gold(name):
    return ur.load(name)


@pytest.fixture(scope="module")
def cpu_inputs():
    """every case's inputs -- trunk features and BERT stream included -- computed on the CPU once for the module (tests/update_ref.inputs keeps
    them); the tests move them to the device"""
    return {name: ur.inputs(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_update_loss_and_backward_match_the_reference_autograd(cpu_inputs, name):
    """update_loss and backward of every model on the device: the losses, the raw outputs, the new state, every stored gradient value, max|g|,
    sum|g| and every projection within the bound; the counts, the partition and the promised zeros exact"""
    nets = ur.modules(name, _cuda)
    assert all(p.is_cuda for net in nets.values() for p in net.parameters())
    run = ur.forward_backward(name, nets, _cuda)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in run["state"].values())
    worst = ur.compare(name, _gold(name), nets, run, None, "device")
    assert not ur.over(worst, BOUND), ur.over(worst, BOUND)


@pytest.mark.parametrize("name", ur.TRAJECTORY)
def test_adam_trajectory_matches_the_reference_s(cpu_inputs, name):
    """hier_update / flat_update run ur.STEPS times with the fixture's Adam: the losses of every step, the final state and every final parameter
    within the bound, and the second step saw the first one's weights"""
    nets = ur.modules(name, _cuda)
    traj = ur.trajectory(name, nets, _cuda)
    torch.cuda.synchronize()
    losses = traj[0].cpu()
    gold = _gold(name)
    for k in range(ur.TERMS):
        if gold["losses"][k] != 0:
            assert float(losses[1, k]) != float(losses[0, k]) and gold["traj_losses"][1, k] != gold["traj_losses"][0, k], k
    worst = ur.compare(name, gold, nets, None, traj, "device, trajectory")
    assert not ur.over(worst, BOUND), ur.over(worst, BOUND)
