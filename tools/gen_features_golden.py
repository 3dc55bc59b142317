"""Golden vectors for the feature keys: builds the reference's own Seq2Seq_HighLevel_CMA, Seq2Seq_LowLevel and CMANet through oracle/ref_shims.py,
loads the synthetic weights with strict=True and calls each on observations that hold ONLY `rgb_features` / `depth_features` -- no `rgb`, no
`depth` -- so that TorchVisionResNet50.forward and VlnResnetDepthEncoder.forward take the keys instead of running their trunks
(models/encoders/resnet_encoders.py:207-214, :83-86).  Writes tests/golden/features_128_L12.npz: the features and the outputs.

128-pixel frames, L = 12, seed-0 `synth` weights.  The features are inputs, so any tensor of the right shape serves: seeded half-normal draws
(post-ReLU-like), stored as f32 values that fp16 holds exactly so that every precision mode ingests them without rounding and the file stays
small.  B = 2, except B = 1 for the (B,2048,4,4) tensor, which the high-level model and CMANet share.
Needs the reference checkout; runs on the build machine, never on the GPU box.

    python tools/gen_features_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from oracle import ref_shims                     # noqa: E402
from robo_vln_amd import synth                   # noqa: E402
from tests import features_cases as fc           # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "features_128_L12.npz")


def main():
    cfg, ccfg = fc.hcm_cfg(), fc.cma_cfg()
    feats = fc.draw_features(cfg)
    hi_sd, lo_sd = synth.make_weights(cfg, fc.SEED)
    cma_sd = synth.make_cma_weights(ccfg, fc.SEED)
    hi, lo = ref_shims.build_models(cfg, hi_sd, lo_sd)
    cma = ref_shims.build_cma(ccfg, cma_sd)
    gold = dict(feats)
    t = {k: torch.from_numpy(v) for k, v in feats.items()}
    with torch.no_grad():
        # high-level model and CMANet: one row (the spatial RGB feature has B = 1)
        ids, h0, m = fc.hi_inputs(cfg)
        logits, hid = hi(({"rgb_features": t["rgb_spatial"], "depth_features": t["depth"][:1], "instruction": torch.from_numpy(ids).float()},
                          h0.clone(), torch.zeros(1, 1), ref_shims.ref_masks(m)))
        gold.update(hi_logits=logits.numpy(), hi_hidden=hid.numpy())
        ids, h0, m = fc.cma_inputs(ccfg)
        out, stop, hid = cma(({"rgb_features": t["rgb_spatial"], "depth_features": t["depth"][:1], "instruction": torch.from_numpy(ids).float()},
                              h0.clone(), torch.zeros(1, 2), ref_shims.ref_masks(m)))
        gold.update(cma_out=out.numpy(), cma_stop=stop.numpy(), cma_hidden=hid.numpy())
        # low-level model: two rows
        h0, m, sub = fc.lo_inputs(cfg)
        vel, stop, hid = lo(({"rgb_features": t["rgb_flat"], "depth_features": t["depth"]}, h0.clone(), torch.zeros(2, 1), ref_shims.ref_masks(m),
                             torch.from_numpy(sub)))
        gold.update(lo_vel=vel.numpy(), lo_stop=stop.numpy(), lo_hidden=hid.numpy())
    gold["meta"] = np.array(repr(dict(config=repr(cfg.to_dict()), cma_config=repr(ccfg.to_dict()), seed=fc.SEED,
                                      note="reference forwards on observations holding only rgb_features / depth_features")))
    np.savez_compressed(OUT, **gold)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
