"""The SimpleCNN training side without a GPU: train.simple_cnn_ref against the oracle's convolutions, the drop-in modules' keys, shapes and
initialisation, every refusal of train.simple_cnn, the constructors' keyword, the kink condition of the committed seeds, both model cases'
float32 CPU run (update_loss + backward and the two-step hier_update / flat_update trajectory) against the fixtures recorded from the
reference's own float64 autograd and against the oracle's float64 autograd, and the
forward of train.LowLevel(cfg, trainable_trunks=True) on the CPU against the goldens captured from the imported reference."""
import os

import numpy as np
import pytest
import torch

from oracle import cases, hcm_oracle
from robo_vln_amd import synth, train
from robo_vln_amd.config import HCMConfig, S2SConfig
from tests import simplecnn_train_cases as sc

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 5e-5          # tests/test_oracle_golden.py: fp32 CPU restatement against the fp32 CPU reference
SIMPLE = dict(rgb_encoder="SimpleRGBCNN", depth_encoder="SimpleDepthCNN")


@pytest.mark.parametrize("case", [(2, 52, 66, 1), (2, 48, 60, 3)], ids=sc.op_id)
def test_restatement_is_the_oracles_convolutions(case):
    x, params, _ = sc.op_inputs(case, 0)
    names = ("cnn.0.weight", "cnn.0.bias", "cnn.2.weight", "cnn.2.bias", "cnn.4.weight", "cnn.4.bias")
    h3, w3 = train.simple_cnn_out_hw(case[1], case[2])
    fc_w = torch.eye(32 * h3 * w3)
    w = dict(zip(names, params), **{"cnn.7.weight": fc_w, "cnn.7.bias": torch.zeros(32 * h3 * w3)})
    oracle = (hcm_oracle.simple_rgb_cnn if case[3] == 3 else hcm_oracle.simple_depth_cnn)(x, w.__getitem__)
    y = train.simple_cnn_ref(x, *params, scale=sc.op_scale(case[3]))
    assert tuple(y.shape) == (case[0], 32, h3, w3)
    # behind the identity cnn.7 the oracle returns relu(Flatten(conv3)): the Flatten order is y.flatten(1)
    assert torch.allclose(torch.relu(y.flatten(1)), oracle, atol=1e-6, rtol=0)


@pytest.mark.parametrize("cls,ch,hw", [(train.SimpleDepthCNN, 1, (52, 66)), (train.SimpleRGBCNN, 3, (48, 60)), (train.SimpleDepthCNN, 1, 64)])
def test_module_keys_shapes_and_initialisation(cls, ch, hw):
    torch.manual_seed(0)
    m = cls(hw, 48)
    spec = {k: shape for k, shape, _, _ in synth.simple_cnn_spec("", ch, hw, 48)}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == spec
    assert all((p == 0).all() for k, p in m.named_parameters() if k.endswith("bias"))
    w = m.cnn[2].weight
    # habitat's layer_init hands the ReLU gain to kaiming_normal_ as its second positional argument, the slope `a`: std = sqrt(2 / (1 + 2) / fan_in)
    assert abs(w.std().item() / (2.0 / 3.0 / 512) ** 0.5 - 1) < 0.05
    key = "depth" if ch == 1 else "rgb"
    H, W = (hw, hw) if isinstance(hw, int) else hw
    y = m({key: torch.rand(3, H, W, ch)})
    assert tuple(y.shape) == (3, 48) and (y >= 0).all()
    with pytest.raises(ValueError, match="is missing"):
        m({})
    with pytest.raises(ValueError, match="takes observations"):
        m({key: torch.rand(3, H + 1, W, ch)})


def test_load_reference_state_dict_is_strict_about_the_encoders():
    cfg = sc.lo_config()
    sd = sc.lo_state_dict(cfg)
    net = train.LowLevel(cfg, trainable_trunks=True)
    assert set(net.state_dict()) == set(sd)
    net.load_reference_state_dict(sd)
    assert torch.equal(net.depth_encoder.cnn[0].weight, torch.as_tensor(sd["depth_encoder.cnn.0.weight"]))
    assert torch.equal(net.rgb_encoder.cnn[7].weight, torch.as_tensor(sd["rgb_encoder.cnn.7.weight"]))
    with pytest.raises(RuntimeError, match="rgb_encoder.cnn.4.bias"):
        net.load_reference_state_dict({k: v for k, v in sd.items() if k != "rgb_encoder.cnn.4.bias"})
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_reference_state_dict(dict(sd, **{"depth_encoder.cnn.0.weight": np.zeros((32, 3, 8, 8), np.float32)}))


def test_every_refusal_of_the_op():
    x, params, _ = sc.op_inputs((1, 36, 36, 1), 0)
    with pytest.raises(ValueError, match="runs on the device"):
        train.simple_cnn(x, *params)
    with pytest.raises(ValueError, match="must not require a gradient"):
        train.simple_cnn(x.clone().requires_grad_(), *params)
    with pytest.raises(ValueError, match="Cin in"):
        train.simple_cnn(torch.zeros(1, 36, 36, 2), *params)
    with pytest.raises(ValueError, match="at least 36 x 36"):
        train.simple_cnn(torch.zeros(1, 35, 40, 1), *params)
    with pytest.raises(ValueError, match="at least 36 x 36"):
        train.simple_cnn(torch.zeros(1, 40, 35, 1), *params)
    with pytest.raises(ValueError, match="float32 frames, or uint8 RGB"):
        train.simple_cnn(torch.zeros(1, 36, 36, 1, dtype=torch.uint8), *params)
    with pytest.raises(ValueError, match="float32 frames, or uint8 RGB"):
        train.simple_cnn(torch.zeros(1, 36, 36, 1, dtype=torch.float64), *params)
    with pytest.raises(ValueError, match="w1 has shape"):
        train.simple_cnn(torch.zeros(1, 36, 36, 3), *params)
    assert (train.SIMPLE_CNN_MIN_HW, train.SIMPLE_CNN_CHANNELS) == (36, (1, 3))


def test_library_refuses_instead_of_launching():
    from robo_vln_amd import _lib
    lib = _lib.lib()
    assert lib.hcm_op_simplecnn_work_floats(2, 36, 36, 1) > 0
    for bad in ((2, 35, 36, 1), (2, 36, 35, 3), (2, 64, 64, 2), (-1, 64, 64, 1)):
        assert lib.hcm_op_simplecnn_work_floats(*bad) == 0
    one = (np.zeros(4, np.float32).ctypes.data,)
    assert lib.hcm_op_simplecnn_train(*one, _lib.HCM_F32, 1.0, *one * 8, 1, 35, 36, 1, None) == -1
    assert lib.hcm_op_simplecnn_train(*one, _lib.HCM_U8, 1.0, *one * 8, 1, 36, 36, 1, None) == -1
    assert lib.hcm_op_simplecnn_train(None, _lib.HCM_F32, 1.0, *one * 8, 1, 36, 36, 1, None) == -1
    assert "NULL" in _lib.last_error()
    assert lib.hcm_op_simplecnn_bwd(*one * 2, _lib.HCM_F32, 1.0, *one * 2, None, *one * 6, 1, 36, 36, 1, None) == -1


@pytest.mark.parametrize("cls,cfg", [(train.LowLevel, lambda: HCMConfig(**SIMPLE)), (train.Seq2SeqNet, lambda: S2SConfig(**SIMPLE))])
def test_default_refusal_stays_and_the_keyword_is_accepted(cls, cfg):
    with pytest.raises(ValueError, match="trainable trunks with nothing to cache"):
        cls(cfg().validate())
    net = cls(cfg().validate(), trainable_trunks=True)
    assert isinstance(net.rgb_encoder, train.SimpleRGBCNN) and isinstance(net.depth_encoder, train.SimpleDepthCNN)
    assert net.FROZEN_PREFIXES == ()


def test_high_level_and_cmanet_keep_refusing():
    with pytest.raises(ValueError, match="nothing to cache"):
        train.HighLevel(HCMConfig(**SIMPLE).validate())
    with pytest.raises(TypeError):
        train.HighLevel(HCMConfig(**SIMPLE).validate(), trainable_trunks=True)


def test_mixed_model_trains_the_resnet_modality_from_its_feature():
    cfg = S2SConfig(rgb_encoder="SimpleRGBCNN", rgb_hw=48, rgb_w=60, depth_hw=64, instr_len=6).validate()
    net = train.Seq2SeqNet(cfg, trainable_trunks=True)
    assert net.FROZEN_PREFIXES == ("depth_encoder.visual_encoder.",)
    assert any(k.startswith("rgb_encoder.cnn.0.") for k in net.state_dict()) and "depth_encoder.visual_fc.1.weight" in net.state_dict()
    rows = 2
    fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
    obs = {"rgb": torch.randint(0, 256, (rows, 48, 60, 3)).float(), "depth_features": torch.rand(rows, cc, fs, fs),
           "instruction": torch.randint(1, 20, (rows, 6))}
    out, stop, h = net((obs, torch.zeros(net.num_recurrent_layers, rows, cfg.hidden), None, torch.ones(rows, 1)))
    (out.sum() + stop.sum()).backward()
    assert net.rgb_encoder.cnn[0].weight.grad.abs().max() > 0 and net.depth_encoder.visual_fc[1].weight.grad.abs().max() > 0


def test_ablation_runs_the_encoder_and_gives_zero_gradients():
    cfg = HCMConfig(**SIMPLE, rgb_hw=48, rgb_w=60, depth_hw=52, depth_w=66, ablate_depth=True).validate()
    net = train.LowLevel(cfg, trainable_trunks=True)
    rows = 2
    frames = sc.lo_frames(cfg, rows)
    for obs in (frames, {"rgb": frames["rgb"]}):                              # with the frames key, and without it
        net.zero_grad()
        out, stop, _ = net((obs, torch.zeros(net.num_recurrent_layers, rows, cfg.hidden), None, torch.ones(rows, 1), torch.tensor([0, 2])))
        (out.sum() + stop.sum()).backward()
        for k, p in net.depth_encoder.named_parameters():
            assert p.grad is not None and (p.grad == 0).all(), k
        assert net.rgb_encoder.cnn[0].weight.grad.abs().max() > 0


@pytest.mark.parametrize("case", sc.OP_CASES, ids=sc.op_id)
def test_kink_condition_of_the_committed_seeds(case):
    assert sc.op_kink_margin(case, sc.OP_SEEDS[case]) >= sc.KINK_RATIO
    assert sc.first_op_seed(case) == sc.OP_SEEDS[case]


@pytest.mark.parametrize("name", list(sc.MODEL_CASES))
def test_model_case_float32_cpu_run_against_the_oracles_autograd(name):
    """update_ref's two conditions on the draw, asserted for the committed seed: every ReLU input off its kink, and the train modules' float32 CPU
    run -- single step and trajectory through the real update function -- within SEED_BOUND of the oracle's float64 run in every tensor"""
    seed = sc.MODEL_SEEDS[name]
    assert sc.model_kink_margin(name, seed) >= sc.KINK_RATIO
    assert sc.model_conditioning(name, seed) <= sc.SEED_BOUND


@pytest.mark.parametrize("name", list(sc.MODEL_CASES))
def test_model_case_against_the_reference_fixture(name):
    """Both fixture cases (tools/gen_simplecnn_update_golden.py: the imported reference's own float64 autograd and Adam) on the CPU: the train
    modules' float64 run meets the fixture to the generator's own check, 1e-9, and their float32 run -- single step and the two-step
    hier_update / flat_update trajectory -- stays within SEED_BOUND in every tensor; counts and the sets of gradients are exact"""
    gold = sc.load_gold(name)
    seed = sc.MODEL_SEEDS[name]
    assert int(gold["seed"]) == seed and int(gold["subsample"]) == sc.GOLD_SUBSAMPLE
    worst = sc.compare_gold(name + " float64 CPU", sc.run_train(name, seed, lambda t: t.double()), gold)
    assert not {k: v for k, v in worst.items() if not v <= 1e-9}
    worst = sc.compare_gold(name + " float32 CPU", sc.run_train(name, seed, lambda t: t), gold)
    assert not {k: v for k, v in worst.items() if not v <= sc.SEED_BOUND}


@pytest.mark.parametrize("name", list(sc.MODEL_CASES))
def test_model_case_float64_run_is_the_oracles(name):
    """in float64 the train modules and the oracle's functions, which share no model code, agree to rounding: 1e-12"""
    worst = sc.compare(name + " float64", sc.run_train(name, sc.MODEL_SEEDS[name], lambda t: t.double()), sc.oracle_run(name, sc.MODEL_SEEDS[name]))
    assert max(worst.values()) <= 1e-12


@pytest.mark.parametrize("name", ["lo_simplecnn_rgb_120x176", "lo_simplecnn_depth_152x218"])
def test_low_level_forward_against_the_reference_golden(name):
    """train.LowLevel(cfg, trainable_trunks=True) on the CPU stepped as tests/test_oracle_golden.py steps the oracle, against the records the
    imported reference wrote, at that test's tolerance"""
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, B, T, which = cases.case_config(name)
    assert which == "lo"
    net = train.LowLevel(cfg, trainable_trunks=True).eval()
    net.load_reference_state_dict(synth.materialize(synth.low_level_spec(cfg), "lo", cases.SEED))
    h = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden)
    with torch.no_grad():
        for t in range(T):
            obs = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_observations(cfg, B, step=t, seed=cases.SEED).items()}
            m = torch.from_numpy(cases.step_masks(B, t)).float().view(B, 1)
            vel, stop, h = net((obs, h, None, m, torch.from_numpy(cases.fixed_subtask(B, t))))
            np.testing.assert_allclose(torch.cat([vel, stop], 1).numpy(), gold["records"][t][:, 4:], atol=TOL, rtol=0)
    np.testing.assert_allclose(h.numpy(), gold["lo_hidden"], atol=TOL, rtol=0)
