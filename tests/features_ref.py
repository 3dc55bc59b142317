"""A features path for the CPU oracle without changing it: inside `given(rgb_features=..., depth_features=...)` the oracle's trunk functions
(`hcm_oracle.tv_resnet50_trunk`, `hcm_oracle.habitat_resnet_encoder`) return the given tensors instead of running, which is what the reference's
encoders do when the observation dict carries the keys (resnet_encoders.py:83-86, :207-214).  The pools that follow the trunk in the oracle --
adaptive_avg_pool2d((4,4)) on a (B,2048,4,4) tensor, adaptive_avg_pool2d(1) on (B,2048,1,1) -- are identities on these shapes.

Also: the oracle's own features from frames (`trunk_features`), the observation sets of the feature tests and `blank_frames`, the frames an oracle
forward still wants to find in the dict (shape only) when the features replace them."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import hcm_oracle


@contextlib.contextmanager
def given(rgb_features=None, depth_features=None):
    """Swap the oracle's two trunk functions for ones that return the given tensors (None = that trunk runs as usual)."""
    tv, hab = hcm_oracle.tv_resnet50_trunk, hcm_oracle.habitat_resnet_encoder
    try:
        if rgb_features is not None:
            hcm_oracle.tv_resnet50_trunk = lambda x, w: torch.as_tensor(np.asarray(rgb_features)).float()
        if depth_features is not None:
            hcm_oracle.habitat_resnet_encoder = lambda depth, w, ngroups: torch.as_tensor(np.asarray(depth_features)).float()
        yield
    finally:
        hcm_oracle.tv_resnet50_trunk, hcm_oracle.habitat_resnet_encoder = tv, hab


@torch.no_grad()
def trunk_features(cfg, sd, obs, spatial):
    """(rgb_features, depth_features) of one model's state_dict `sd` on the frames of `obs`, as the reference's encoders would cache them:
    the hooked avgpool output -- adaptive_avg_pool2d((4,4)) for a spatial encoder, the global pool for a flat one -- and the ResNetEncoder output."""
    w = hcm_oracle.Weights(sd)
    rgb = torch.as_tensor(np.asarray(obs["rgb"])).float().permute(0, 3, 1, 2) / 255.0
    x = hcm_oracle.tv_resnet50_trunk(rgb.contiguous(), w.sub("rgb_encoder.cnn."))
    x = F.adaptive_avg_pool2d(x, (4, 4) if spatial else 1)
    d = hcm_oracle.habitat_resnet_encoder(torch.as_tensor(np.asarray(obs["depth"])).float(), w.sub("depth_encoder.visual_encoder."),
                                          cfg.depth_baseplanes // 2)
    return x.contiguous(), d.contiguous()


def blank_frames(obs):
    """`obs` with NaN-filled frames of the same shapes: the oracle reads their shape, and an engine given features must not read them at all."""
    out = dict(obs)
    out["rgb"] = np.full(np.asarray(obs["rgb"]).shape, np.nan, dtype=np.float32)
    out["depth"] = np.full(np.asarray(obs["depth"]).shape, np.nan, dtype=np.float32)
    return out
