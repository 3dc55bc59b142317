"""tests/depth_run_cases.py on its own: the float64 block reference against the oracle's block statements, and the case list against the
kernels' template instantiations.  (The GPU side is tests/test_depth_runs_gpu.py.)"""
import re
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import hcm_oracle
from tests import depth_run_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("side", [32, 16, 8])
def test_block_ref_equals_the_oracles_block_statements(side):
    """block_ref without the storage rounding, every eps 1e-5, two trunks: the statements of habitat_resnet_encoder's inner loop
    (oracle/hcm_oracle.py, an identity block: bi > 0, stride 1) on a state dict in torch's own layouts -- OIHW weights, NCHW activations --
    through the oracle's Weights and _gn.  Ties the kernels' layouts (NHWC, k = tap*CM + ci, trunks side by side) to the oracle's."""
    run = dc.make_run(side, "fp16", 2, 2, 1, seed=3)
    C, CM = run.C, run.CM
    w64 = tuple(t.double() for t in run.w[0])
    got = dc.block_ref(run.x.double(), w64, run.gn[0], (1e-5, 1e-5, 1e-5), None)
    for g in range(2):
        gn = [t.double()[g * ch:(g + 1) * ch] for t, ch in zip(run.gn[0], (CM, CM, CM, CM, C, C))]
        p = "layer1.1."
        sd = {p + "convs.0.weight": w64[0][g].view(CM, C, 1, 1), p + "convs.3.weight": w64[1][g].view(CM, 3, 3, CM).permute(0, 3, 1, 2).contiguous(),
              p + "convs.6.weight": w64[2][g].view(C, CM, 1, 1)}
        for i, name in enumerate(("convs.1", "convs.4", "convs.7")):
            sd[p + name + ".weight"], sd[p + name + ".bias"] = gn[2 * i], gn[2 * i + 1]
        b = hcm_oracle.Weights({k: v.numpy() for k, v in sd.items()})          # (a numpy state dict, float64 here)
        x = run.x.double()[:, :, g * C:(g + 1) * C].reshape(2, side, side, C).permute(0, 3, 1, 2)
        # oracle/hcm_oracle.py habitat_resnet_encoder, the loop body for bi > 0 (no down-sample), stride 1, ngroups 16
        idt = x
        o = F.relu(hcm_oracle._gn(F.conv2d(x, b(p + "convs.0.weight")), b, p + "convs.1", 16))
        o = F.relu(hcm_oracle._gn(F.conv2d(o, b(p + "convs.3.weight"), stride=1, padding=1), b, p + "convs.4", 16))
        o = hcm_oracle._gn(F.conv2d(o, b(p + "convs.6.weight")), b, p + "convs.7", 16)
        ref = F.relu(o + idt).permute(0, 2, 3, 1).reshape(2, side * side, C)
        err = (got[:, :, g * C:(g + 1) * C] - ref).abs().max().item()
        assert err <= 1e-12, (g, err)


def test_cases_cover_every_template_instantiation():
    """2 storage types x 3 shapes: the four depth_blk_kernel<T, LOGW, C, CM> instantiations named in launch_depth_blk, the two
    depth_l3_kernel<T> in launch_depth_l3 (its <f16, true> is the development build's profiled copy)"""
    assert sorted(dc.CASES) == sorted((p, s) for p in ("fp16", "bf16") for s in (32, 16, 8))
    blk = open(os.path.join(ROOT, "robo-vln_amd", "csrc", "depth_blk.hip")).read()
    inst = set(re.findall(r"depth_blk_kernel<(bf16|f16), (\d), (\d+), (\d+)>", blk))
    want = {({"fp16": "f16", "bf16": "bf16"}[p], str({32: 5, 16: 4}[s]), str(dc.SHAPES[s][0]), str(dc.SHAPES[s][1])) for p, s in dc.CASES if s != 8}
    assert inst == want, inst
    l3 = open(os.path.join(ROOT, "robo-vln_amd", "csrc", "igemm.hip")).read()
    assert set(re.findall(r"depth_l3_kernel<(bf16|f16)>", l3)) == {"bf16", "f16"}
    assert dc.SHAPES[8] == (512, 128) and dc.MAX_BLOCKS == {32: 4, 16: 4, 8: 6}


def test_every_conv_of_neighbouring_blocks_has_its_own_eps():
    for blk in range(6):
        e = [dc.eps_of(blk, i) for i in range(3)]
        assert len(set(e)) == 3
        assert all(dc.eps_of(blk, i) != dc.eps_of(blk + 1, i) for i in range(3))
    assert dc.eps_of(0, 0) == pytest.approx(1e-5, rel=1e-6)


@pytest.mark.parametrize("side", [32, 16, 8])
def test_low_variance_case_is_decided_by_eps(side):
    """conv1's weights times 2^-8: its group variances lie below eps1, and another eps1 (4e-5 for 1e-5) moves the float64 block output by far
    more than the parity bound of that case (fp16: 3e-3 x max |ref|) -- a kernel that ignores eps1 cannot pass there"""
    run = dc.make_run(side, "fp16", 1, 1, 1, low_variance=(0,))
    var = dc.group_variance(dc.conv1_out(run.x, run.w[0][0][0], side)).max().item()
    assert var < run.eps[0][0], var
    ref = dc.block_ref(run.x, run.w[0], run.gn[0], run.eps[0], dc.TDT["fp16"])
    other = dc.block_ref(run.x, run.w[0], run.gn[0], (4e-5,) + run.eps[0][1:], dc.TDT["fp16"])
    moved, bound = (ref - other).abs().max().item(), 3e-3 * max(1.0, ref.abs().max().item())
    print(f"side {side}: conv1 group variance <= {var:.2e}; eps1 1e-5 -> 4e-5 moves the output by {moved:.3f}, bound {bound:.3f}")
    assert moved > 4 * bound
