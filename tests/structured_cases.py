"""Shared structured inputs of the normalisation tests (CPU only): the frames a simulator hands a policy at resets, in front of walls or from an
invalid sensor -- all-zero, saturated, constant, piecewise constant -- and rows whose mean is far from zero against their spread.

Every other input of the suite is zero-centred white noise, for which no group's variance comes near GroupNorm's eps and |mean| / std stays
below 1.  Everything here is deterministic (closed forms, or a seeded generator).

  depth_frames(B, H, W)   name -> (B, H, W, 1) float32 in [0, 1]                          (the `batch_obs` contract of synth.make_observations)
  rgb_frames(B, H, W)     name -> (B, H, W, 3) float32 holding integers 0 .. 255
  offset_rows(shape, ratio, seed)   ratio + U(-sqrt 3, sqrt 3): unit standard deviation, |mean| / std = ratio
  oracle_min_group_var(cfg, hi_sd, lo_sd, obs)   the oracle's act() with a spy on its F.group_norm: the smallest group variance and the largest
                          |mean| / std over every GroupNorm of the step, in float64 (and the record)"""
import contextlib

import numpy as np
import torch

from oracle import hcm_oracle
from robo_vln_amd import synth

DEPTH_NAMES = ("zeros", "ones", "const_0.37", "ramp", "step_edge", "checker4", "impulse", "const_plus_1e-3_noise", "rows_identical")
RGB_NAMES = ("zeros", "all_255", "ramp", "checker4")


def _grid(H, W):
    return np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")


def _checker(H, W):
    yy, xx = np.meshgrid(np.arange(H) // 4, np.arange(W) // 4, indexing="ij")
    return ((yy + xx) % 2).astype(np.float64)


def depth_frames(B, H, W):
    """Named depth frames, (B, H, W, 1) float32 in [0, 1].  `ramp`: an x ramp in row 0, a y ramp in row 1 (alternating beyond); `impulse`: one
    pixel at 1 in a zero frame; `rows_identical`: every batch row the same x ramp."""
    yy, xx = _grid(H, W)
    xr, yr = 0.2 + 0.6 * xx, 0.9 - 0.5 * yy
    rep = lambda a: np.repeat(a[None], B, 0)
    imp = np.zeros((H, W))
    imp[H // 2, W // 2] = 1.0
    g = np.random.default_rng(1234)
    f = {
        "zeros": np.zeros((B, H, W)),
        "ones": np.ones((B, H, W)),
        "const_0.37": np.full((B, H, W), 0.37),
        "ramp": np.stack([xr if b % 2 == 0 else yr for b in range(B)]),
        "step_edge": rep(np.where(xx < 0.5, 0.25, 0.8)),
        "checker4": rep(_checker(H, W) * 0.7 + 0.1),
        "impulse": rep(imp),
        "const_plus_1e-3_noise": 0.6 + 1e-3 * (g.random((B, H, W)) - 0.5),
        "rows_identical": rep(xr),
    }
    assert tuple(f) == DEPTH_NAMES
    return {k: np.ascontiguousarray(v[..., None], dtype=np.float32) for k, v in f.items()}


def rgb_frames(B, H, W):
    """Named RGB frames, (B, H, W, 3) float32 holding integers 0 .. 255 (cast to uint8 exactly)."""
    yy, xx = _grid(H, W)
    ramp = np.stack([np.floor(255 * xx), np.floor(255 * yy), np.floor(255 * (1 - xx))], -1)
    chk = _checker(H, W)[..., None] * np.array([200.0, 120.0, 255.0]) + np.array([20.0, 60.0, 0.0])
    rep = lambda a: np.repeat(a[None], B, 0)
    f = {"zeros": np.zeros((B, H, W, 3)), "all_255": np.full((B, H, W, 3), 255.0), "ramp": rep(ramp), "checker4": rep(chk)}
    assert tuple(f) == RGB_NAMES
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in f.items()}


def offset_rows(shape, ratio, seed):
    """ratio + U(-sqrt 3, sqrt 3), a float64 tensor (the caller rounds it to its storage type): unit standard deviation about a mean of `ratio`"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * 3.0 ** 0.5 + float(ratio)


def observations(cfg, B, depth=None, rgb=None, seed=3, rgb_uint8=False, same_instruction=False, make=synth.make_observations):
    """make(cfg, B, step=0, seed=seed) with the depth and / or RGB frames replaced (None: the noise frames stay)"""
    obs = dict(make(cfg, B, step=0, seed=seed))
    if depth is not None:
        assert depth.shape == obs["depth"].shape and depth.min() >= 0 and depth.max() <= 1
        obs["depth"] = depth
    if rgb is not None:
        assert rgb.shape == obs["rgb"].shape and (rgb == np.floor(rgb)).all() and rgb.min() >= 0 and rgb.max() <= 255
        obs["rgb"] = rgb
    if rgb_uint8:
        obs["rgb"] = obs["rgb"].astype(np.uint8)
    if same_instruction:
        obs["instruction"] = np.repeat(obs["instruction"][:1], B, 0)
    return obs


@contextlib.contextmanager
def group_norm_spy(round_fp16=False):
    """Replaces oracle.hcm_oracle.F.group_norm for the duration: records, per call, the smallest group variance and the largest |mean| / std of
    its input in float64 (a constant group counts as ratio 0 when it is zero, inf otherwise); round_fp16 rounds every GroupNorm input to fp16
    and back first.  The original is restored on exit."""
    F = hcm_oracle.F
    orig = F.group_norm
    seen = {"min_var": [], "max_ratio": []}

    def spy(x, num_groups, weight=None, bias=None, eps=1e-5):
        if round_fp16:
            x = x.half().to(x.dtype)
        xx = x.detach().double().reshape(x.shape[0], num_groups, -1)
        var, mean = xx.var(-1, unbiased=False), xx.mean(-1)
        ratio = torch.where(var > 0, mean.abs() / var.sqrt().clamp_min(1e-300), torch.where(mean == 0, 0.0, float("inf")).double())
        seen["min_var"].append(var.min().item())
        seen["max_ratio"].append(ratio.max().item())
        return orig(x, num_groups, weight, bias, eps)

    F.group_norm = spy
    try:
        yield seen
    finally:
        F.group_norm = orig


def oracle_record(cfg, hi_sd, lo_sd, obs):
    """PolicyOracle.act from a zero state with a zero mask: (record, hi state, lo state)"""
    B = obs["depth"].shape[0]
    R = cfg.num_recurrent_layers
    ora = hcm_oracle.PolicyOracle(cfg, hi_sd, lo_sd)
    o = {k: torch.from_numpy(np.asarray(v).astype(np.float32) if k == "rgb" else np.asarray(v)) for k, v in obs.items()}
    return ora.act(o, torch.zeros(R, B, cfg.hidden), torch.zeros(R, B, cfg.hidden), torch.zeros(B))


def oracle_min_group_var(cfg, hi_sd, lo_sd, obs):
    """(smallest group variance, largest |mean| / std) over every GroupNorm of one oracle step on `obs`, in float64"""
    with group_norm_spy() as seen:
        oracle_record(cfg, hi_sd, lo_sd, obs)
    return min(seen["min_var"]), max(seen["max_ratio"])
