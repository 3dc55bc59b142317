"""Write tests/golden/ref_checkpoint_roundtrip.pth.xz: the REAL reference models imported from
the reference checkout (configuration tests/test_checkpoint_cpu.py ROUNDTRIP_CFG), loaded with strict=True from the per-tensor patterned
weights of tests/test_checkpoint_cpu.pattern_weights, saved exactly as the reference trainer's `save_checkpoint` does
(hierarchical_trainer.py:349-363: {"high_level_state_dict", "low_level_state_dict", "config"}, `torch.save`) and xz-compressed (the
patterns make the ~440 MB of tensors about 140 KB).

Run where the reference checkout can be imported:   python oracle/gen_checkpoint_roundtrip_fixture.py
Test infrastructure.  tests/test_checkpoint_cpu.py reads the fixture through robo-vln_amd/checkpoint.py and the strict loader of libhcm.
"""
import io
import lzma
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hcm_pkg  # noqa: E402

hcm_pkg.load()
from robo_vln_amd.config import HCMConfig  # noqa: E402
from oracle import ref_shims  # noqa: E402
from tests.test_checkpoint_cpu import ROUNDTRIP_CFG, pattern_weights  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    cfg = HCMConfig(**ROUNDTRIP_CFG).validate()
    hi_sd, lo_sd = pattern_weights(cfg)
    hi, lo = ref_shims.build_models(cfg, hi_sd, lo_sd)
    ckpt = {"high_level_state_dict": hi.state_dict(), "low_level_state_dict": lo.state_dict(), "config": ref_shims.model_config(cfg)}
    buf = io.BytesIO()
    torch.save(ckpt, buf)
    with open(os.path.join(GOLD, "ref_checkpoint_roundtrip.pth.xz"), "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print(f"wrote {GOLD}/ref_checkpoint_roundtrip.pth.xz ({len(buf.getvalue()) / 1e6:.0f} MB uncompressed)")


if __name__ == "__main__":
    main()
