"""The structured cases of tests/structured_cases.py are what the GPU tests assume -- checked on the reference alone (no GPU):

  * which frames drive a GroupNorm group's variance to 0 (`zeros`), to a few eps (`impulse`), and which stay far above eps;
  * the oracle is well conditioned on every frame: rounding every GroupNorm input to fp16 moves the action record by at most 2.5e-3, a quarter
    of the 16-bit bound -- so a 16-bit engine that misses 1e-2 on one of these frames is wrong, not unlucky.  A condition on the inputs;
  * offset_rows has the |mean| / std it was asked for;
  * torch's float32 CPU group_norm / layer_norm -- the e32 yardstick of tests/test_norm_conditioning_gpu.py -- stays within 1e-4 of float64 at
    every ratio used there."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from robo_vln_amd import synth
from robo_vln_amd.config import HCMConfig
from tests import structured_cases as sc

B = 2
RATIOS = (0, 4, 16, 32, 64, 256)
# the frames of tests/test_structured_frames_gpu.py: every depth frame with noise RGB; depth zeros / ones with RGB zeros / all_255
COMBOS = [(d, None) for d in sc.DEPTH_NAMES] + [(d, r) for d in ("zeros", "ones") for r in ("zeros", "all_255")]


@functools.lru_cache(maxsize=None)
def _setup():
    cfg = HCMConfig(rgb_hw=64, depth_hw=128, instr_len=12, bert_layers=1).validate()
    hi_sd, lo_sd = synth.make_weights(cfg, seed=3)
    return cfg, hi_sd, lo_sd, sc.depth_frames(B, 128, 128), sc.rgb_frames(B, 64, 64)


@functools.lru_cache(maxsize=None)
def _stats(depth, rgb):
    cfg, hi_sd, lo_sd, df, rf = _setup()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    obs = sc.observations(cfg, B, df[depth], rf[rgb] if rgb else None)
    with sc.group_norm_spy() as seen:
        rec = sc.oracle_record(cfg, hi_sd, lo_sd, obs)[0]
    with sc.group_norm_spy(round_fp16=True):
        rec16 = sc.oracle_record(cfg, hi_sd, lo_sd, obs)[0]
    return min(seen["min_var"]), len(seen["min_var"]), (rec - rec16).abs().max().item()


def test_frames_obey_the_batch_obs_contract():
    cfg, _, _, df, rf = _setup()
    assert tuple(df) == sc.DEPTH_NAMES and tuple(rf) == sc.RGB_NAMES
    for v in df.values():
        assert v.shape == (B, 128, 128, 1) and v.dtype == np.float32 and v.min() >= 0 and v.max() <= 1
    for v in rf.values():
        assert v.shape == (B, 64, 64, 3) and v.dtype == np.float32 and (v == np.floor(v)).all() and v.min() >= 0 and v.max() <= 255
    assert df["impulse"].sum() == B and (df["ramp"][0] != df["ramp"][1]).any() and (df["rows_identical"][0] == df["rows_identical"][1]).all()
    again = sc.depth_frames(B, 128, 128)
    assert all((df[k] == again[k]).all() for k in df)


@pytest.mark.parametrize("depth", sc.DEPTH_NAMES)
def test_smallest_group_variance_per_depth_frame(depth):
    min_var, calls, _ = _stats(depth, None)
    print(f"depth {depth}: smallest group variance {min_var:.3e} over {calls} GroupNorms")
    assert calls == 108                    # 54 per depth trunk, hi and lo
    if depth == "zeros":
        assert min_var == 0.0
    elif depth == "impulse":
        assert 0 < min_var < 1e-3
    else:
        assert min_var >= 1e-2


def test_oracle_min_group_var_restores_the_oracle():
    from oracle import hcm_oracle
    cfg, hi_sd, lo_sd, df, _ = _setup()
    before = hcm_oracle.F.group_norm
    mv, ratio = sc.oracle_min_group_var(cfg, hi_sd, lo_sd, sc.observations(cfg, B, df["zeros"]))
    assert hcm_oracle.F.group_norm is before is F.group_norm
    assert mv == _stats("zeros", None)[0] == 0.0 and ratio > 0


@pytest.mark.parametrize("depth,rgb", COMBOS)
def test_oracle_is_well_conditioned_on_every_frame(depth, rgb):
    _, _, moved = _stats(depth, rgb)
    print(f"depth {depth} rgb {rgb or 'noise'}: fp16-rounded GroupNorm inputs move the record by {moved:.2e}")
    assert moved <= 2.5e-3


@pytest.mark.parametrize("ratio", RATIOS)
def test_offset_rows_ratio(ratio):
    x = sc.offset_rows((2048,), ratio, seed=1)
    got = (x.mean().abs() / x.std(unbiased=False)).item()
    assert abs(x.std(unbiased=False).item() - 1) <= 0.02
    assert abs(got - ratio) <= (0.02 * ratio if ratio else 0.05), got      # (ratio 0: the sample mean of 2 048 unit-variance draws, 2.3 sigma)


@pytest.mark.parametrize("ratio", RATIOS)
def test_torch_float32_norms_are_a_usable_yardstick(ratio):
    worst = 0.0
    for n, seed in ((2048, 0), (32768, 1), (131072, 2)):
        x = sc.offset_rows((2, 4, n), ratio, seed).float()
        e = (F.group_norm(x, 4).double() - F.group_norm(x.double(), 4)).abs().max().item()
        worst = max(worst, e)
    for D in (256, 768):
        x = sc.offset_rows((37, D), ratio, D).float()
        e = (F.layer_norm(x, (D,)).double() - F.layer_norm(x.double(), (D,))).abs().max().item()
        worst = max(worst, e)
    print(f"ratio {ratio}: torch float32 group_norm / layer_norm against float64, max-abs {worst:.2e}")
    assert worst <= 1e-4
