"""The stage transition layer2 -> layer3 of the RGB trunk: layer2's LAST bottleneck (128 mid channels) computes layer3 block 0's 1x1 reduction
(512 -> 256 channels) from its output tile in the same launch (bneck231r_kernel<.., 128, 256, ..>, one buffer for the 32 KB weight slice).  Same MFMA
instruction, operand roles, k order and epilogue operations as the stand-alone reduction launch, so BOTH outputs must equal the three separate conv
launches to the bit -- at operator level (every tile form: 64-pixel halo tiles, the classic ring on a ragged map, 128-pixel tiles from 192 tiles
up; one bottleneck and the hi|lo pair layout; fp16 and bf16) and for a whole step (HCM_NO_BNECK_NEXT256 of the development build).

The stage transition layer1 -> layer2: layer2 block 0's stride-2 1x1 down-sample conv (256 -> 512) rides in the expansion GEMM as four more K blocks
([W3 | Wds], K = 384, bias b3 + bds; bneck231r_kernel<.., 64, 128, 128, 4>).  The identity is no longer rounded to the storage type before the add, so
against the separate launches the block output agrees to one rounding, and it must be at least as close to a float32 computation as they are."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import hcm_pkg
    hcm_pkg.load()
    from robo_vln_amd import _lib as L
    return L.lib(), L


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _p(t):
    return t.data_ptr()


_CASES = {}


def _case(prec, cfg):
    """Inputs of one case and the outputs of the separate launches (three hcm_op_conv2d per group on that group's channels), computed once."""
    key = (prec, cfg)
    if key in _CASES:
        return _CASES[key]
    lib, L = _lib()
    code, tdt = (L.HCM_F16, torch.float16) if prec == "fp16" else (L.HCM_BF16, torch.bfloat16)
    B, H, W, G = cfg
    C1, C3, CN = 128, 512, 256
    x = _rnd(B, H, W, G * C1).cuda().to(tdt)
    w2 = _rnd(G, C1, 3, 3, C1, scale=(9 * C1) ** -0.5 * 1.7, seed=1).cuda().to(tdt)
    b2 = _rnd(G, C1, scale=0.2, seed=2).cuda()
    w3 = _rnd(G, C3, C1, scale=C1 ** -0.5 * 1.7, seed=3).cuda().to(tdt)
    b3 = _rnd(G, C3, scale=0.2, seed=4).cuda()
    w1 = _rnd(G, CN, C3, scale=C3 ** -0.5 * 1.7, seed=6).cuda().to(tdt)
    b1 = _rnd(G, CN, scale=0.2, seed=7).cuda()
    idt = _rnd(B, H, W, G * C3, seed=5).cuda().to(tdt)
    y_ref = torch.empty(B, H, W, G * C3, device="cuda", dtype=tdt)
    o_ref = torch.empty(B, H, W, G * CN, device="cuda", dtype=tdt)
    for g in range(G):
        xg = x[..., g * C1:(g + 1) * C1].contiguous()
        ig = idt[..., g * C3:(g + 1) * C3].contiguous()
        mid = torch.empty(B, H, W, C1, device="cuda", dtype=tdt)
        yg = torch.empty(B, H, W, C3, device="cuda", dtype=tdt)
        og = torch.empty(B, H, W, CN, device="cuda", dtype=tdt)
        assert lib.hcm_op_conv2d(_p(xg), _p(w2[g]), _p(b2[g]), None, _p(mid), code, B, H, W, C1, C1, 3, 3, 1, 1, L.ACT_RELU, None) == 0
        assert lib.hcm_op_conv2d(_p(mid), _p(w3[g]), _p(b3[g]), _p(ig), _p(yg), code, B, H, W, C1, C3, 1, 1, 1, 0, L.ACT_RELU, None) == 0
        assert lib.hcm_op_conv2d(_p(yg), _p(w1[g]), _p(b1[g]), None, _p(og), code, B, H, W, C3, CN, 1, 1, 1, 0, L.ACT_RELU, None) == 0
        y_ref[..., g * C3:(g + 1) * C3] = yg
        o_ref[..., g * CN:(g + 1) * CN] = og
    torch.cuda.synchronize()
    _CASES[key] = dict(code=code, tdt=tdt, x=x, w2=w2, b2=b2, w3=w3, b3=b3, w1=w1, b1=b1, idt=idt, y_ref=y_ref, o_ref=o_ref)
    return _CASES[key]


def _fused(c, cfg):
    lib, L = _lib()
    B, H, W, G = cfg
    y = torch.full_like(c["y_ref"], float("nan"))
    o1 = torch.full_like(c["o_ref"], float("nan"))
    rc = lib.hcm_op_bottleneck_stage(_p(c["x"]), _p(c["w2"]), _p(c["b2"]), _p(c["w3"]), _p(c["b3"]), _p(c["idt"]), None, _p(y), _p(c["w1"]),
                                     _p(c["b1"]), _p(o1), c["code"], B, H, W, 128, 1, 256, 0, G, None)
    assert rc == 0
    torch.cuda.synchronize()
    return y, o1


# (B, H, W, groups): 16 x 16 and 32 x 32 block inputs (64-pixel halo tiles, four / two image rows per tile), one bottleneck and the pair layout;
# a 17 x 15 map (M = 765: the classic ring and its ragged last tile, whose waves issue fewer stores than the counted waits assume by default);
# 192 tiles of 128 pixels (the one-workgroup-per-CU form the bench shape takes)
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("cfg", [(3, 16, 16, 1), (3, 16, 16, 2), (2, 32, 32, 1), (2, 32, 32, 2), (3, 17, 15, 1), (3, 17, 15, 2), (24, 32, 32, 1), (12, 32, 32, 2)])
def test_last_block_with_next_stage_reduction_equals_the_separate_launches(prec, cfg):
    c = _case(prec, cfg)
    y, o1 = _fused(c, cfg)
    assert torch.equal(y.view(torch.int16), c["y_ref"].view(torch.int16))
    assert torch.equal(o1.view(torch.int16), c["o_ref"].view(torch.int16))
    y2, o2 = _fused(c, cfg)           # two calls give the same bits
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(o1.view(torch.int16), o2.view(torch.int16))


def test_grouped_operator_equals_the_single_bottleneck_entry_points():
    """hcm_op_bottleneck_stage with groups = 1 is hcm_op_bottleneck_tail_next (and takes its shapes)."""
    lib, L = _lib()
    cfg = (3, 16, 16, 1)
    c = _case("fp16", cfg)
    y, o1 = _fused(c, cfg)
    y2, o2 = torch.empty_like(y), torch.empty_like(o1)
    assert lib.hcm_op_bottleneck_tail_next(_p(c["x"]), _p(c["w2"]), _p(c["b2"]), _p(c["w3"]), _p(c["b3"]), _p(c["idt"]), _p(y2), _p(c["w1"]), _p(c["b1"]),
                                           _p(o2), c["code"], 3, 16, 16, 128, 1, 256, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(o1.view(torch.int16), o2.view(torch.int16))


_DS = {}


def _ds_case(prec, cfg):
    """Inputs of one stage-first case; per group the four separate launches (3x3/2, down-sample 1x1/2, expansion + identity, next reduction) and a
    float32 torch computation of the block output from the launches' own (bit-identical) mid tensor.  Computed once."""
    key = (prec, cfg)
    if key in _DS:
        return _DS[key]
    lib, L = _lib()
    code, tdt = (L.HCM_F16, torch.float16) if prec == "fp16" else (L.HCM_BF16, torch.bfloat16)
    B, H, W, G = cfg
    C1, Cd, C3, CN = 128, 256, 512, 128
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = _rnd(B, H, W, G * C1).cuda().to(tdt)
    xd = _rnd(B, H, W, G * Cd, seed=8).cuda().to(tdt)
    w2 = _rnd(G, C1, 3, 3, C1, scale=(9 * C1) ** -0.5 * 1.7, seed=1).cuda().to(tdt)
    b2 = _rnd(G, C1, scale=0.2, seed=2).cuda()
    w3 = _rnd(G, C3, C1, scale=C1 ** -0.5 * 1.2, seed=3).cuda().to(tdt)
    b3 = _rnd(G, C3, scale=0.2, seed=4).cuda()
    wd = _rnd(G, C3, Cd, scale=Cd ** -0.5 * 1.2, seed=9).cuda().to(tdt)
    bd = _rnd(G, C3, scale=0.2, seed=10).cuda()
    w1 = _rnd(G, CN, C3, scale=C3 ** -0.5 * 1.7, seed=6).cuda().to(tdt)
    b1 = _rnd(G, CN, scale=0.2, seed=7).cuda()
    w3ds = torch.cat([w3, wd], dim=2).contiguous()
    b3ds = (b3 + bd).contiguous()
    y_sep = torch.empty(B, Ho, Wo, G * C3, device="cuda", dtype=tdt)
    idt = torch.empty(B, Ho, Wo, G * C3, device="cuda", dtype=tdt)
    ref = torch.empty(B, Ho, Wo, G * C3, device="cuda", dtype=torch.float32)
    for g in range(G):
        xg = x[..., g * C1:(g + 1) * C1].contiguous()
        xdg = xd[..., g * Cd:(g + 1) * Cd].contiguous()
        mid = torch.empty(B, Ho, Wo, C1, device="cuda", dtype=tdt)
        ig = torch.empty(B, Ho, Wo, C3, device="cuda", dtype=tdt)
        yg = torch.empty(B, Ho, Wo, C3, device="cuda", dtype=tdt)
        assert lib.hcm_op_conv2d(_p(xg), _p(w2[g]), _p(b2[g]), None, _p(mid), code, B, H, W, C1, C1, 3, 3, 2, 1, L.ACT_RELU, None) == 0
        assert lib.hcm_op_conv2d(_p(xdg), _p(wd[g]), _p(bd[g]), None, _p(ig), code, B, H, W, Cd, C3, 1, 1, 2, 0, L.ACT_NONE, None) == 0
        assert lib.hcm_op_conv2d(_p(mid), _p(w3[g]), _p(b3[g]), _p(ig), _p(yg), code, B, Ho, Wo, C1, C3, 1, 1, 1, 0, L.ACT_RELU, None) == 0
        torch.cuda.synchronize()
        y_sep[..., g * C3:(g + 1) * C3] = yg
        idt[..., g * C3:(g + 1) * C3] = ig
        xs = xdg[:, ::2, ::2, :].double()
        r = mid.double() @ w3[g].double().t() + b3[g].double() + xs @ wd[g].double().t() + bd[g].double()
        ref[..., g * C3:(g + 1) * C3] = torch.relu(r).float()
    torch.cuda.synchronize()
    _DS[key] = dict(code=code, tdt=tdt, x=x, xd=xd, w2=w2, b2=b2, w3ds=w3ds, b3ds=b3ds, w1=w1, b1=b1, y_sep=y_sep, idt=idt, ref=ref)
    return _DS[key]


def _ds_fused(c, cfg):
    lib, L = _lib()
    B, H, W, G = cfg
    y = torch.full_like(c["y_sep"], float("nan"))
    o1 = torch.full((B, y.shape[1], y.shape[2], G * 128), float("nan"), device="cuda", dtype=c["tdt"])
    rc = lib.hcm_op_bottleneck_stage(_p(c["x"]), _p(c["w2"]), _p(c["b2"]), _p(c["w3ds"]), _p(c["b3ds"]), None, _p(c["xd"]), _p(y), _p(c["w1"]),
                                     _p(c["b1"]), _p(o1), c["code"], B, H, W, 128, 2, 128, 4, G, None)
    assert rc == 0
    torch.cuda.synchronize()
    return y, o1


# (B, H, W, groups) of the block input: 3 x 16 x 16 -> M = 192 output pixels, 2 x 32 x 32 -> 512 (whole 64-pixel tiles both; 3 x 18 x 14 -> 189: a
# ragged last tile, whose rows past M request the out-of-range sentinel)
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("cfg", [(3, 16, 16, 1), (3, 16, 16, 2), (2, 32, 32, 1), (2, 32, 32, 2), (3, 18, 14, 1), (3, 18, 14, 2)])
def test_stage_first_block_with_folded_downsample(prec, cfg):
    lib, L = _lib()
    c = _ds_case(prec, cfg)
    B, H, W, G = cfg
    y, o1 = _ds_fused(c, cfg)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(o1).all())
    # against the separate launches: they round the identity to the storage type (error <= eps/2 * |identity|) before the add; both sides then round
    # the sum once (<= eps/2 * |y| each).  eps = spacing of the storage type relative to the value: 2^-10 (fp16), 2^-7 (bf16).  The f32 accumulation
    # order differs too (K = 384 in one accumulator against 128 and 256): 1e-5 relative to the largest output covers it.
    eps = 2.0 ** -10 if prec == "fp16" else 2.0 ** -7
    yf, ys = y.float(), c["y_sep"].float()
    bound = 0.5 * eps * c["idt"].float().abs() + eps * torch.maximum(yf.abs(), ys.abs()) + 1e-5 * ys.abs().max()
    excess = ((yf - ys).abs() - bound).max().item()
    print("max |fused - separate| =", (yf - ys).abs().max().item(), "excess over the one-rounding bound =", excess)
    assert excess <= 0.0, excess
    # against float32: at least as close as the separate launches
    ef, es = (yf - c["ref"]).abs().max().item(), (ys - c["ref"]).abs().max().item()
    print("max error against float32: fused", ef, "separate", es)
    assert ef <= es, (ef, es)
    # the next block's reduction is the stand-alone launch's, from the kernel's own block output
    for g in range(G):
        yg = y[..., g * 512:(g + 1) * 512].contiguous()
        og = torch.empty(B, y.shape[1], y.shape[2], 128, device="cuda", dtype=c["tdt"])
        assert lib.hcm_op_conv2d(_p(yg), _p(c["w1"][g]), _p(c["b1"][g]), None, _p(og), c["code"], B, y.shape[1], y.shape[2], 512, 128, 1, 1, 1, 0,
                                 L.ACT_RELU, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o1[..., g * 128:(g + 1) * 128].contiguous().view(torch.int16), og.view(torch.int16))
    y2, o2 = _ds_fused(c, cfg)        # two calls give the same bits
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(o1.view(torch.int16), o2.view(torch.int16))


SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
import hcm_pkg; hcm_pkg.load()
from robo_vln_amd import synth
from robo_vln_amd.config import baseline_config
from robo_vln_amd.policy import HCMEngine
cfg = baseline_config(0)
B = 3
hi_sd, lo_sd = synth.make_weights(cfg, seed=5)
eng = HCMEngine(cfg, hi_sd, lo_sd, max_batch=B, precision="fp16", graph=False)
obs = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in synth.make_observations(cfg, B, step=0, seed=5).items()}
R = cfg.num_recurrent_layers
hh = torch.zeros(R, B, cfg.hidden, device="cuda"); lh = torch.zeros(R, B, cfg.hidden, device="cuda")
rec, hh2, lh2 = eng.act(obs, hh, lh, torch.zeros(B, device="cuda"))
torch.cuda.synchronize()
np.savez(sys.argv[1], rec=rec.cpu().numpy(), hh=hh2.cpu().numpy(), lh=lh2.cpu().numpy())
eng.close()
""" % ROOT


def _run(env_extra, path):
    """-> (outputs, the implicit-GEMM shapes the step launched: HCM_IGEMM_LOG of the development build prints each new one once)"""
    env = dict(os.environ, HCM_DEV_LIB="1", HCM_IGEMM_LOG="1")
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", SCRIPT, path], check=True, env=env, cwd=ROOT, timeout=600, stderr=subprocess.PIPE, text=True)
    return dict(np.load(path)), r.stderr


RED = "N=256 K=512 "        # layer3 block 0's reduction as a launch of its own (no other conv of the step has this shape)
DS2 = "N=512 K=256 "        # layer2 block 0's down-sample conv


def _close(a, b):
    """the fp16 parity tolerance of tests/test_parity_gpu.py: records within 1e-2, hidden states within 1e-2 relative (l2)"""
    assert float(np.abs(a["rec"] - b["rec"]).max()) <= 1e-2
    for k in ("hh", "lh"):
        rel = float(np.linalg.norm(a[k] - b[k]) / max(np.linalg.norm(b[k]), 1e-30))
        print(k, rel)
        assert rel <= 1e-2, (k, rel)


def test_step_with_the_stage_transitions_fused_equals_the_step_without():
    """The small configuration (128-pixel frames), development library.  Toggling only the layer2 -> layer3 reduction: bit-equal.  The default step
    against the step with both stage-first down-sample convs and that reduction as launches of their own (HCM_NO_BNECK_DSFOLD: one rounding more on the
    identity paths): within the fp16 parity tolerance.  The shape log says which launches each run made, so a switch without effect fails."""
    with tempfile.TemporaryDirectory() as d:
        default, log_d = _run({}, os.path.join(d, "a.npz"))
        nonext, log_n = _run({"HCM_NO_BNECK_NEXT256": "1"}, os.path.join(d, "b.npz"))
        plain, log_p = _run({"HCM_NO_BNECK_NEXT256": "1", "HCM_NO_BNECK_DSFOLD": "1"}, os.path.join(d, "c.npz"))
        nods2, log_2 = _run({"HCM_NO_BNECK_DSFOLD128": "1"}, os.path.join(d, "e.npz"))
    assert "[igemm]" in log_d
    assert RED not in log_d and DS2 not in log_d
    assert RED in log_n and DS2 not in log_n
    assert RED in log_p and DS2 in log_p
    assert RED not in log_2 and DS2 in log_2
    assert np.isfinite(default["rec"]).all()
    for k in ("rec", "hh", "lh"):
        assert np.array_equal(default[k], nonext[k]), (k, float(np.abs(default[k] - nonext[k]).max()))
    _close(default, plain)
    _close(default, nods2)
