"""Normalisation operators on OFFSET data: every GroupNorm / LayerNorm kernel reachable through the C ABI and the training wrappers against
float64 torch on the same (storage-rounded) inputs, with |mean| / std = 0 ... 256.  Every other operator test feeds zero-centred noise, where a
one-pass variance E[x^2] - mean^2 and a centred one cannot be told apart; here they can.

Bounds (none taken from what the kernels give):
  ratios 0, 4, 16       the operator tests' own bound of tests/test_ops_gpu.py for the hook (3 x tol; 4 x tol x max(1, |ref|) for the epilogue-fed
                        routes, which go to ratio 32 in fp16), all storage types;
  ratios 64, 256        float32 only: max(3 x 2e-4, 8 x e32), e32 = torch's float32 CPU op against float64 on the same inputs (computed here);
                        8 covers another summation order over at most 131 072 elements;
  training LayerNorms   the project's rel rule, max(1e-5, 4 x e32) with e32 the same quantity from the float32 CPU *_ref.
The epilogue-fed statistics (conv2d_gn, _gn_large, _gn_pool, _gn_res2) are one-pass by design and are not asserted beyond ratio 16 (bf16) / 32
(fp16): DESIGN.md states the envelope.  One line per case is printed with the measured error (profiles/norm_conditioning.md holds them)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from robo_vln_amd import train
from tests import embed_train_cases as ec
from tests import structured_cases as sc
from tests import vla_train_cases as vc
from tests.test_embed_train_gpu import _raw_forward
from tests.test_ops_gpu import DT, _lib, _p, _rnd, _vla_layer_ref

pytestmark = pytest.mark.gpu

LOW, HIGH = (0, 4, 16), (64, 256)
CASES = [(r, p) for r in LOW for p in ("fp32", "fp16", "bf16")] + [(r, "fp32") for r in HIGH]
CASES16 = [(r, p) for r in LOW for p in ("fp16", "bf16")] + [(32, "fp16")]
_ids = lambda c: f"ratio{c[0]}-{c[1]}"


def _bound(ratio, prec, e32, low):
    """the hook's own bound up to ratio 16; float32 beyond: max(3 x 2e-4, 8 x e32)"""
    if ratio in LOW:
        return low
    assert prec == "fp32"
    return max(3 * 2e-4, 8 * e32)


# ------------------------------------------------------------------------------------------------ GroupNorm, statistics computed by the kernel
# (B, H, W, C, G) per route of launch_groupnorm (csrc/elementwise.hip), as hcm_op_groupnorm calls it (a statistics buffer, no padded channels):
#   HW >= 1024 (or C <= 256 from 256 pixels), C <= 512                        -> gn_stats_kernel + gn_apply_kernel
#   fewer pixels / more channels, a group no wider than 1024 channels          -> gn_fused_kernel (the slab kernel), CS = 256 / 128 (f32) channels
#   one group of 2048 channels (CS > 1024)                                     -> gn_generic_kernel
# (cg_true, the padded-channel count, is not reachable through the hook: launch_groupnorm's last argument stays 0.)
GN_SHAPES = {"stats_apply": (2, 32, 32, 32, 16), "slab_512": (2, 8, 8, 512, 16), "slab_1024": (2, 4, 4, 1024, 16), "generic_2048": (3, 1, 1, 2048, 1),
             "stats_apply_16part": (1, 64, 64, 64, 2)}      # 131 072 elements per group in 16 partials: the longest sum the factor 8 was set for


@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("route", list(GN_SHAPES))
def test_groupnorm_offset(route, case):
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, H, W, Cc, G = GN_SHAPES[route]
    x = sc.offset_rows((B, Cc, H, W), ratio, seed=Cc + ratio).to(tdt).double()
    r = _rnd(B, Cc, H, W, seed=1).to(tdt).double()
    g, b = (_rnd(Cc, seed=2) + 1.5).double(), _rnd(Cc, seed=3).double()
    ref = F.relu(F.group_norm(x, G, g, b, 1e-5) + r)
    e32 = (F.relu(F.group_norm(x.float(), G, g.float(), b.float(), 1e-5) + r.float()).double() - ref).abs().max().item()
    xd = x.permute(0, 2, 3, 1).contiguous().to("cuda", tdt)
    rd = r.permute(0, 2, 3, 1).contiguous().to("cuda", tdt)
    gd, bd = g.float().cuda(), b.float().cuda()
    assert lib.hcm_op_groupnorm(_p(xd), _p(rd), _p(gd), _p(bd), code, B, H * W, Cc, G, 1e-5, 1, None) == 0
    torch.cuda.synchronize()
    err = (xd.double().cpu().permute(0, 3, 1, 2) - ref).abs().max().item()
    bound = _bound(ratio, prec, e32, 3 * tol)
    print(f"groupnorm {route} ratio {ratio} [{prec}]: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert err <= bound, (err, e32)


def test_groupnorm_float32_outlier_in_the_pivot_element():
    """The float32 kernels sum about K = the group's first element.  When that element is itself an outlier (a spike of 100 in unit noise at
    pixel 0, first channel of every group) |mean - K| / std is not <~ 2 but r = 41 here -- its ceiling is sqrt(n), 45 -- and the shifted sums cancel WORSE
    than the plain ones would (those see |mean| / std of 0.02).  This case documents that behaviour against the rounding analysis, not against the
    6e-4 of the well-conditioned cases: every element passes through at most d additions (slab kernel, (2, 8, 8, 512, 16) in float32: 8 pixels per
    thread, one butterfly step, two steps over the four waves, 32 channels of the group: d = 43), so each of q / n and (a / n)^2 carries a relative
    error of at most d x 2^-24 (first order), the variance q / n - (a / n)^2 one of 3 d 2^-24 (1 + r^2), rstd half of it, and an output o of magnitude
    |o - beta| moves by that fraction.  Bound: 6e-4 + max|ref - beta| x 1.5 d 2^-24 (1 + r^2), r measured in float64 in the test."""
    lib, L = _lib()
    code, tdt, tol = DT["fp32"]
    B, H, W, Cc, G = GN_SHAPES["slab_512"]
    Cg, d = Cc // G, 8 + 1 + 2 + 32
    x = sc.offset_rows((B, Cc, H, W), 0, seed=5).float().double()
    x[:, ::Cg, 0, 0] = 100.0
    g, b = (_rnd(Cc, seed=2) + 1.5).double(), _rnd(Cc, seed=3).double()
    ref = F.group_norm(x, G, g, b, 1e-5)
    grp = x.reshape(B, G, -1)
    r = ((grp.mean(-1) - 100.0).abs() / grp.std(-1, unbiased=False)).max().item()
    e32 = (F.group_norm(x.float(), G, g.float(), b.float(), 1e-5).double() - ref).abs().max().item()
    bound = 3 * tol + (ref - b.view(1, -1, 1, 1)).abs().max().item() * 1.5 * d * 2.0 ** -24 * (1 + r * r)
    xd = x.permute(0, 2, 3, 1).contiguous().to("cuda", tdt)
    gd, bd = g.float().cuda(), b.float().cuda()
    assert lib.hcm_op_groupnorm(_p(xd), None, _p(gd), _p(bd), code, B, H * W, Cc, G, 1e-5, 0, None) == 0
    torch.cuda.synchronize()
    err = (xd.double().cpu().permute(0, 3, 1, 2) - ref).abs().max().item()
    print(f"groupnorm slab_512 outlier in the pivot element [fp32]: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  |mean - K|/std {r:.1f}  max|ref| {ref.abs().max().item():.1f}")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ GroupNorm fed by the conv epilogue's statistics
def _offset_conv(B, H, Cin, Cout, ratio, tdt, seed, K=1):
    """x (B, H, H, Cin) with the last channel constant 1, w (Cout, K, K, Cin) whose last input channel carries m / K^2 on every tap, m = ratio x the
    standard deviation of the conv without it: a K = 1 conv output is (noise conv) + m exactly.  Returns x, w (storage type) and m."""
    x = _rnd(B, H, H, Cin, seed=seed).to(tdt)
    w = (_rnd(Cout, K, K, Cin, seed=seed + 1) * (2.0 / (Cin * K * K)) ** 0.5).to(tdt)
    x[..., -1] = 1.0
    w[..., -1] = 0.0
    std = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, padding=K // 2).std().item()
    m = torch.tensor(ratio * std / (K * K)).to(tdt)
    w[..., -1] = m
    return x, w, m.item() * K * K


def _conv64(x, w, tdt, stride=1, pad=0):
    """the conv in float64 on the stored operands, rounded to the storage type as the step stores it"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, stride=stride, padding=pad).to(tdt).double()


def _group_ratio(conv, G):
    v = conv.reshape(conv.shape[0], G, -1)
    return (v.mean(-1).abs() / v.std(-1, unbiased=False)).max().item()


def _check16(what, ratio, prec, got, ref, extra=""):
    tol = DT[prec][2]
    err = (got - ref).abs().max().item()
    bound = 4 * tol * max(1.0, ref.abs().max().item())
    print(f"{what} ratio {ratio} [{prec}]: err {err:.3e}  bound {bound:.3e}{extra}")
    assert err <= bound, err


@pytest.mark.parametrize("case", CASES16, ids=_ids)
def test_conv2d_gn_small_map_offset(case):
    """hcm_op_conv2d_gn (conv + GroupNorm + residual + ReLU in one launch, <= 64 pixels per sample): (4, 2, 256, 512, 1, 1, 0, 32, res, relu)"""
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, H, Cin, Cout, G = 4, 2, 256, 512, 32
    x, w, m = _offset_conv(B, H, Cin, Cout, ratio, tdt, seed=1)
    gamma, beta = _rnd(Cout, seed=3) * 0.5 + 1.0, _rnd(Cout, seed=4) * 0.1
    res = _rnd(B, H, H, Cout, seed=5).to(tdt)
    conv = _conv64(x, w, tdt)
    ref = F.relu(F.group_norm(conv, G, gamma.double(), beta.double(), 1e-5) + res.double().permute(0, 3, 1, 2))
    xd, wd, gd, bd, rd = x.cuda(), w.cuda(), gamma.cuda(), beta.cuda(), res.cuda()
    y = torch.full((B, H, H, Cout), float("nan"), device="cuda", dtype=tdt)
    assert lib.hcm_op_conv2d_gn(_p(xd), _p(wd), _p(gd), _p(bd), _p(rd), _p(y), code, B, H, H, Cin, Cout, 1, 1, 1, 0, G, 1e-5, 1, None) == 0
    torch.cuda.synchronize()
    _check16("conv2d_gn", ratio, prec, y.double().cpu().permute(0, 3, 1, 2), ref, f"  m {m:.3f}  group |mean|/std {_group_ratio(conv, G):.1f}")


@pytest.mark.parametrize("case", CASES16, ids=_ids)
def test_conv2d_gn_large_map_offset(case):
    """hcm_op_conv2d_gn_large (epilogue statistics + gn_apply_kernel): (7, 16, 64, 128, 1, 1, 0, 32, no residual, relu)"""
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, H, Cin, Cout, G = 7, 16, 64, 128, 32
    x, w, m = _offset_conv(B, H, Cin, Cout, ratio, tdt, seed=1)
    gamma, beta = _rnd(Cout, seed=3) * 0.5 + 1.0, _rnd(Cout, seed=4) * 0.1
    conv = _conv64(x, w, tdt)
    ref = F.relu(F.group_norm(conv, G, gamma.double(), beta.double(), 1e-5))
    xd, wd, gd, bd = x.cuda(), w.cuda(), gamma.cuda(), beta.cuda()
    y = torch.full((B, H, H, Cout), float("nan"), device="cuda", dtype=tdt)
    assert lib.hcm_op_conv2d_gn_large(_p(xd), _p(wd), _p(gd), _p(bd), None, _p(y), code, B, H, H, Cin, Cout, 1, 1, 1, 0, G, 1e-5, 1, None) == 0
    torch.cuda.synchronize()
    _check16("conv2d_gn_large", ratio, prec, y.double().cpu().permute(0, 3, 1, 2), ref, f"  m {m:.3f}  group |mean|/std {_group_ratio(conv, G):.1f}")


@pytest.mark.parametrize("case", CASES16, ids=_ids)
def test_two_groupnorms_one_pass_offset(case):
    """hcm_op_conv2d_gn_res2 (gn_apply2_kernel), both convs offset: (2, 16, 16, 64, 64, 1, 256, 16, no relu)"""
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, H, Cin, Cout, G = 2, 16, 64, 256, 16
    x, w, m = _offset_conv(B, H, Cin, Cout, ratio, tdt, seed=1)
    x2, w2, m2 = _offset_conv(B, H, Cin, Cout, ratio, tdt, seed=7)
    g, b = _rnd(Cout, seed=2) * 0.5 + 1.0, _rnd(Cout, seed=3) * 0.3
    g2, b2 = _rnd(Cout, seed=6) * 0.5 + 1.0, _rnd(Cout, seed=7) * 0.3
    c1, c2 = _conv64(x, w, tdt), _conv64(x2, w2, tdt)
    # the down-sample branch's normalised map is rounded to the storage type before the add (gn_apply2_kernel: bit-identical to two apply passes)
    ref = F.group_norm(c1, G, g.double(), b.double(), 1e-5) + F.group_norm(c2, G, g2.double(), b2.double(), 1e-5).to(tdt).double()
    xd, wd, x2d, w2d, gd, bd, g2d, b2d = x.cuda(), w.cuda(), x2.cuda(), w2.cuda(), g.cuda(), b.cuda(), g2.cuda(), b2.cuda()
    y = torch.full((B, H, H, Cout), float("nan"), device="cuda", dtype=tdt)
    assert lib.hcm_op_conv2d_gn_res2(_p(xd), _p(wd), _p(gd), _p(bd), _p(x2d), _p(w2d), _p(g2d), _p(b2d), _p(y), code, B, H, H, Cin, Cin, 1, Cout, G,
                                     1e-5, 0, None) == 0
    torch.cuda.synchronize()
    _check16("conv2d_gn_res2", ratio, prec, y.double().cpu().permute(0, 3, 1, 2), ref, f"  m {m:.3f} / {m2:.3f}  group |mean|/std {_group_ratio(c1, G):.1f}")


@pytest.mark.parametrize("case", CASES16, ids=_ids)
@pytest.mark.parametrize("shape", [(3, 16, 32, 64, 1, 0, 16), (2, 32, 8, 64, 3, 1, 32)], ids=["1x1", "3x3_taps_group_ratio_capped_near_8"])
def test_conv_groupnorm_maxpool_on_load_offset(shape, case):
    """hcm_op_conv2d_gn_pool (maxpool_gn_kernel).  1x1: the offset is exact.  3x3 with padding 1: m / 9 rides on every tap of the constant channel,
    so the conv's border pixels see 6 or 4 taps of it; that spread grows with m, and the group's |mean| / std saturates near 8 on this map however
    large m is (3.8, 7.8, 8.4 at nominal 4, 16, 32; printed) -- the `ratio` in this shape's id is the nominal m / std, not the group's.  The pooled map's border and
    interior pixels are compared separately, both asserted.  At ratio 16 the on-load route must again give the bits of apply pass + plain pool."""
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, H, Cin, Cout, K, pad, G = shape
    x, w, m = _offset_conv(B, H, Cin, Cout, ratio, tdt, seed=1, K=K)
    g, b = _rnd(Cout, seed=2) * 0.5 + 1.0, _rnd(Cout, seed=3) * 0.3
    conv = _conv64(x, w, tdt, pad=pad)
    ref = F.max_pool2d(F.relu(F.group_norm(conv, G, g.double(), b.double(), 1e-5)), 3, 2, 1)
    xd, wd, gd, bd = x.cuda(), w.cuda(), g.cuda(), b.cuda()
    Hp = ref.shape[2]
    y = torch.full((B, Hp, Hp, Cout), float("nan"), device="cuda", dtype=tdt)
    assert lib.hcm_op_conv2d_gn_pool(_p(xd), _p(wd), _p(gd), _p(bd), _p(y), code, B, H, H, Cin, Cout, K, K, 1, pad, G, 1e-5, None) == 0
    torch.cuda.synchronize()
    got = y.double().cpu().permute(0, 3, 1, 2)
    note = f"  m {m:.3f}  group |mean|/std {_group_ratio(conv, G):.1f}"
    inner = torch.zeros(Hp, Hp, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    _check16(f"conv2d_gn_pool {K}x{K} interior", ratio, prec, got[..., inner], ref[..., inner], note)
    _check16(f"conv2d_gn_pool {K}x{K} border", ratio, prec, got[..., ~inner], ref[..., ~inner], note)
    if ratio == 16:
        y2 = torch.empty((B, H, H, Cout), device="cuda", dtype=tdt)
        assert lib.hcm_op_conv2d_gn_large(_p(xd), _p(wd), _p(gd), _p(bd), None, _p(y2), code, B, H, H, Cin, Cout, K, K, 1, pad, G, 1e-5, 1, None) == 0
        y3 = torch.empty_like(y)
        assert lib.hcm_op_maxpool3x3s2(_p(y2), _p(y3), code, B, H, H, Cout, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(y, y3)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("hook", ["layernorm", "layernorm_post"])
def test_layernorm_offset(hook, D, case):
    """hcm_op_layernorm / hcm_op_layernorm_post centre before squaring: the controls -- they meet the float32 rule at ratios 64 and 256 as they are"""
    lib, L = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    rows, prow = 37, 5
    x = sc.offset_rows((rows, D), ratio, seed=D + ratio).to(tdt).double()
    r = _rnd(rows, D, seed=1).to(tdt).double()
    g, b = (_rnd(D, seed=2) + 1.5).double(), _rnd(D, seed=3).double()
    post = _rnd(prow, D, seed=4) if hook == "layernorm_post" else None
    add = post.double()[torch.arange(rows) % prow] if post is not None else 0.0
    ref = F.layer_norm(x + r, (D,), g, b, 1e-12) + add
    e32 = ((F.layer_norm(x.float() + r.float(), (D,), g.float(), b.float(), 1e-12) + (add.float() if post is not None else 0.0)).double() - ref).abs().max().item()
    y = torch.full((rows, D), float("nan"), device="cuda", dtype=tdt)
    xd, rd, gd, bd = x.to("cuda", tdt), r.to("cuda", tdt), g.float().cuda(), b.float().cuda()
    if post is None:
        assert lib.hcm_op_layernorm(_p(xd), _p(rd), _p(gd), _p(bd), _p(y), code, rows, D, 1e-12, None) == 0
    else:
        pd = post.cuda()
        assert lib.hcm_op_layernorm_post(_p(xd), _p(rd), _p(gd), _p(bd), _p(pd), prow, _p(y), code, rows, D, 1e-12, None) == 0
    torch.cuda.synchronize()
    err = (y.double().cpu() - ref).abs().max().item()
    bound = _bound(ratio, prec, e32, 3 * tol)
    print(f"{hook} D {D} ratio {ratio} [{prec}]: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert err <= bound, (err, e32)


@pytest.mark.parametrize("case", CASES16[:-1], ids=_ids)
def test_fused_cross_modal_layer_offset(case):
    """hcm_op_vla_layer and _frag (16-bit only; csrc/vla_fused.hip's one-pass LayerNorm) with the residual input I offset by the ratio, on the
    smallest case of tests/test_ops_gpu.py: (B, L, Lk) = (2, 37, (16, 4)), in-kernel attention, ragged pooled mean; that test's bounds."""
    lib, Lm = _lib()
    ratio, prec = case
    code, tdt, tol = DT[prec]
    B, L, Lk, d, dff = 2, 37, (16, 4), 256, 1024
    W = {"wo": _rnd(d, d, seed=1) * (3.0 / d) ** 0.5, "w1": _rnd(dff, d, seed=2) * (3.0 / d) ** 0.5, "w2": _rnd(d, dff, seed=3) * (3.0 / dff) ** 0.5,
         "bo": _rnd(d, seed=4) * 0.1, "b1": _rnd(dff, seed=5) * 0.1, "b2": _rnd(d, seed=6) * 0.1,
         "g1": _rnd(d, seed=7) * 0.5 + 1.0, "be1": _rnd(d, seed=8) * 0.1, "g2": _rnd(d, seed=9) * 0.5 + 1.0, "be2": _rnd(d, seed=10) * 0.1}
    for k in ("wo", "w1", "w2"):
        W[k] = W[k].to(tdt).float()
    I = sc.offset_rows((B, L, d), ratio, seed=11).to(tdt).float()
    q = _rnd(B, L, d, seed=12).to(tdt).float()
    lens = torch.tensor([L, max(1, L // 3)], dtype=torch.int32)
    dev = lambda t, dt=None: t.to("cuda", dt if dt is not None else tdt).contiguous()
    Wd = {k: dev(v, tdt if k in ("wo", "w1", "w2") else torch.float32) for k, v in W.items()}
    Wf = {}
    for k, (N, K) in (("wo", (d, d)), ("w1", (dff, d)), ("w2", (d, dff))):
        Wf[k] = torch.empty_like(Wd[k])
        assert lib.hcm_op_pack_frag(_p(Wd[k]), _p(Wf[k]), code, N, K, None) == 0
    Id, qd, ld = dev(I), dev(q), lens.cuda()
    kvs = [_rnd(B, Lk[s_], 512, seed=20 + s_).to(tdt).float() for s_ in range(2)]
    ins = [dev(kv) for kv in kvs]
    W64 = {k: v.double() for k, v in W.items()}
    refs = [_vla_layer_ref(q.double(), I.double(), kv.double(), None, W64, L, lens) for kv in kvs]
    arr = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])
    res = {}
    for name, fn, Wm in (("vla_layer", lib.hcm_op_vla_layer, Wd), ("vla_layer_frag", lib.hcm_op_vla_layer_frag, Wf)):
        outs = [torch.full((B, L, d), float("nan"), device="cuda", dtype=tdt) for _ in range(2)]
        pooled = [torch.full((B, 300), float("nan"), device="cuda") for _ in range(2)]
        assert fn(_p(qd), _p(Id), arr(ins), (C.c_int * 2)(*Lk), None, arr(outs), arr([p[:, 17:] for p in pooled]), 300, _p(Wm["wo"]), _p(Wd["bo"]),
                  _p(Wm["w1"]), _p(Wd["b1"]), _p(Wm["w2"]), _p(Wd["b2"]), _p(Wd["g1"]), _p(Wd["be1"]), _p(Wd["g2"]), _p(Wd["be2"]), _p(ld), code, B, L,
                  dff, 2, None) == 0
        torch.cuda.synchronize()
        res[name] = (outs, pooled)
        for s_ in range(2):
            y, pm = refs[s_]
            err = (outs[s_].double().cpu() - y).abs().max().item()
            perr = (pooled[s_][:, 17:17 + d].double().cpu() - pm).abs().max().item()
            print(f"{name} stream {s_} ratio {ratio} [{prec}]: err {err:.3e} (bound {3e-2 if prec == 'bf16' else 6e-3:.0e})  pooled {perr:.3e}")
            assert err <= (3e-2 if prec == "bf16" else 6e-3), (s_, err)
            assert perr <= (8e-3 if prec == "bf16" else 2e-3), (s_, perr)
    for s_ in range(2):          # the two weight layouts stay bit-identical on offset rows
        assert torch.equal(res["vla_layer"][0][s_].view(torch.int16), res["vla_layer_frag"][0][s_].view(torch.int16))
        assert torch.equal(res["vla_layer"][1][s_][:, 17:17 + d], res["vla_layer_frag"][1][s_][:, 17:17 + d])


# ------------------------------------------------------------------------------------------------ training LayerNorms (two-pass, vla_train_dev.h)
def _train_bound(e32):
    return max(1e-5, 4 * e32)


@functools.lru_cache(maxsize=None)
def _embed_case(rows, K, period, m, kill_row):
    """embed_train_cases.make_inputs without dropout, the bias offset by m (the LayerNorm input is m + small), first seed from 0 that keeps every
    pre-activation off the ReLU kink; kill_row: that row of x is zero except a 1 in column 0, whose weights are strongly negative (-5 - |u|)
    while every other row has a 0 there -- a bias that only this row sees: all of its pre-activations are negative."""
    seed = 0
    while True:
        (x, w, b, gamma, beta), keep, post, cot = ec.make_inputs(rows, K, period, 0.0, seed)
        b = b + m
        if kill_row is not None:
            x[:, 0] = 0.0
            x[kill_row] = 0.0
            x[kill_row, 0] = 1.0
            w[:, 0] = -5.0 - w[:, 0].abs()
        if ec.min_preactivation(x, w, b) >= ec.KINK:
            break
        seed += 1
    args = (x, w, b, gamma, beta)
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        leaves = [t.to(dt).requires_grad_() for t in args]
        y = train.embed_ln_ref(*leaves, post=post.to(dt) if post is not None else None)
        out[name] = dict(zip(("y",) + ec.NAMES, (y.detach(),) + torch.autograd.grad(y, leaves, cot.to(dt))))
    return args, post, cot, out["64"], out["32"]


def _embed_run(rows, K, period, m, kill_row=None):
    args, post, cot, r64, r32 = _embed_case(rows, K, period, m, kill_row)
    leaves = [t.cuda().requires_grad_() for t in args]
    pd = post.cuda() if post is not None else None
    y = train.embed_ln(*leaves, post=pd)
    grads = torch.autograd.grad(y, leaves, cot.cuda())
    torch.cuda.synchronize()
    got = dict(zip(("y",) + ec.NAMES, (y.detach().cpu(),) + tuple(g.cpu() for g in grads)))
    worst = {}
    for n, g in got.items():
        e32 = ec.rel(r32[n], r64[n], f"embed_ln {(rows, K, period)} offset {m} {n} float32 CPU (e32)")
        e = ec.rel(g, r64[n], f"embed_ln {(rows, K, period)} offset {m} {n}")
        assert torch.isfinite(g).all()
        worst[n] = (e, _train_bound(e32))
    assert all(e <= bnd for e, bnd in worst.values()), worst
    return args, post, got


@pytest.mark.parametrize("m", [8, 64])
@pytest.mark.parametrize("shape", [(5, 256, 5), (65, 768, 13)])
def test_embed_ln_offset_bias(shape, m):
    _embed_run(*shape, m)


def test_embed_ln_row_with_zero_variance():
    """One whole row killed by the ReLU: its LayerNorm input is all 0, its variance 0, rstd = 1 / sqrt(eps).  y = beta + table and the saved xhat row
    is exactly 0; forward and gradients within the bound like every other case."""
    rows, K, period, kill = 5, 256, 5, 3
    args, post, got = _embed_run(rows, K, period, 0.0, kill_row=kill)
    assert torch.equal(got["y"][kill], args[4] + post[kill % period])
    rc, fw = _raw_forward([t.cuda() for t in args], None, 0.0, post.cuda(), rows, K)
    assert rc == 0
    torch.cuda.synchronize()
    xhat, rstd = fw["xhat"].t.cpu().reshape(rows, ec.D), fw["rstd"].t.cpu()
    assert (xhat[kill] == 0).all() and (fw["gate"].t.cpu().reshape(rows, ec.D)[kill] == 0).all()
    assert abs(rstd[kill].item() * 1e-5 ** 0.5 - 1) <= 1e-6
    assert got["d_x"][kill].abs().max().item() == 0


@functools.lru_cache(maxsize=None)
def _vla_case(m):
    B, L, Lk, d_ff, p = 2, 5, 16, 256, 0.25
    seed = 0
    while True:
        args, keep, cot = vc.make_inputs(B, L, Lk, d_ff, p, seed)
        args = (args[0], args[1] + m) + tuple(args[2:])
        if vc.min_preactivation([t.double() for t in args], keep, p) >= vc.KINK:
            break
        seed += 1
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        leaves = [t.to(dt).requires_grad_() for t in args]
        y = train.vla_layer_ref(*leaves, keep=keep, p=p)
        out[name] = dict(zip(("out",) + vc.NAMES, (y.detach(),) + torch.autograd.grad(y, leaves, cot.to(dt))))
    return args, keep, cot, p, out["64"], out["32"]


@pytest.mark.parametrize("m", [8, 64])
def test_vla_layer_train_offset_residual(m):
    """train.vla_layer at (2, 5, 16, 256, 0.25) with the residual input I offset by m: forward and the thirteen gradients"""
    args, keep, cot, p, r64, r32 = _vla_case(m)
    leaves = [t.cuda().requires_grad_() for t in args]
    y = train.vla_layer(*leaves, keep=tuple(k.cuda() for k in keep), p=p)
    grads = torch.autograd.grad(y, leaves, cot.cuda())
    torch.cuda.synchronize()
    got = dict(zip(("out",) + vc.NAMES, (y.detach().cpu(),) + tuple(g.cpu() for g in grads)))
    worst = {}
    for n, g in got.items():
        e32 = vc.rel(r32[n], r64[n], f"vla_layer offset {m} {n} float32 CPU (e32)")
        e = vc.rel(g, r64[n], f"vla_layer offset {m} {n}")
        assert torch.isfinite(g).all()
        worst[n] = (e, _train_bound(e32))
    assert all(e <= bnd for e, bnd in worst.values()), worst
