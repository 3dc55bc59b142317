"""Differentiable Visual_Ling_Attn without a GPU: the drop-in module's CPU path against the reference's own Visual_Ling_Attn (golden vector written by
tools/gen_vla_encoder_train_golden.py), its state-dict keys, initialisation and seeded train mode, embed_ln_ref against a step-by-step
torch.nn.functional composition, the sinusoid table, the kink condition of the shared cases, the C ABI's declarations and its refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robo_vln_amd import _lib, train
from tests import embed_train_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vla_encoder_train_N2_L5_Lk6.npz")
LAYER_KEYS = [f"{m}.{w}" for m in ("enc_att.attention.fc_q", "enc_att.attention.fc_k", "enc_att.attention.fc_v", "enc_att.attention.fc_o", "enc_att.layer_norm",
                                   "pwff.fc1", "pwff.fc2", "pwff.layer_norm") for w in ("weight", "bias")]
F = torch.nn.functional


def _golden():
    z = np.load(GOLDEN)
    t = {k: torch.from_numpy(z[k]) for k in z.files}
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd/")}
    return t, sd, dict(zip(("N", "vis_in_features", "ins_in_features", "d_model", "h", "d_ff"), (int(v) for v in z["dims"])))


def _module(sd, dims, dropout=0.25):
    m = train.Visual_Ling_Attn(dropout=dropout, **dims).double()
    m.load_state_dict(sd, strict=True)
    return m


def test_drop_in_reproduces_the_reference_module():
    """output, both input gradients and every parameter gradient of the reference's Visual_Ling_Attn (eval mode, float64) to 1e-12"""
    t, sd, dims = _golden()
    m = _module(sd, dims).eval()
    x, x2 = t["input"].clone().requires_grad_(), t["input_2"].clone().requires_grad_()
    out = m(x, x2, None, None)
    assert (out - t["out"]).abs().max().item() <= 1e-12
    params = dict(m.named_parameters())
    grads = torch.autograd.grad(out, [x, x2, *params.values()], t["cotangent"])
    for name, g in zip(["input", "input_2", *params], grads):
        ref = t["grad/" + name]
        assert (g - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), name


def test_state_dict_keys_are_the_references():
    _, sd, dims = _golden()
    want = [f"layers.{i}.{k}" for i in range(dims["N"]) for k in LAYER_KEYS] + [f"{m}.{w}" for m in ("vis_fc", "ins_fc", "layer_norm") for w in ("weight", "bias")]
    assert list(sd) == want
    m = train.Visual_Ling_Attn(dropout=0.1, **dims)
    assert list(m.state_dict()) == want and not list(m.buffers())
    m.table(5, "cpu")
    assert list(m.state_dict()) == want                                   # the table is no buffer


def test_config_object_and_keyword_arguments():
    class Cfg:
        N, vis_in_features, ins_in_features, d_model, h, d_ff, dropout = 1, 256, 768, 256, 4, 1024, 0.1
    m = train.Visual_Ling_Attn(Cfg)
    assert len(m.layers) == 1 and m.ins_fc.in_features == 768 and m.vis_fc.in_features == 256 and m.layers[0].d_ff == 1024 and m.p == 0.1
    assert len(train.Visual_Ling_Attn(Cfg, N=3).layers) == 3
    with pytest.raises(TypeError):
        train.Visual_Ling_Attn(N=1, d_model=256)
    with pytest.raises(TypeError):
        train.Visual_Ling_Attn(Cfg, width=3)


def test_initialisation():
    """nn.Linear's default on vis_fc / ins_fc (uniform within 1 / sqrt(fan_in)), nn.LayerNorm's ones and zeros, the layers' own initialisation"""
    torch.manual_seed(0)
    m = train.Visual_Ling_Attn(N=2, vis_in_features=256, ins_in_features=768, d_model=256, h=4, d_ff=1024, dropout=0.1)
    for fc in (m.vis_fc, m.ins_fc):
        bound = 1 / math.sqrt(fc.in_features)
        assert fc.weight.abs().max().item() <= bound and fc.bias.abs().max().item() <= bound
        assert abs(fc.weight.std().item() - bound / math.sqrt(3)) <= 0.05 * bound
    assert torch.equal(m.layer_norm.weight, torch.ones(256)) and torch.equal(m.layer_norm.bias, torch.zeros(256))
    for layer in m.layers:
        att = layer.enc_att.attention
        assert att.fc_q.bias.abs().max().item() == 0 and abs(att.fc_q.weight.std().item() - math.sqrt(2 / 512)) <= 0.05 * math.sqrt(2 / 512)
    assert not torch.equal(m.layers[0].pwff.fc1.weight, m.layers[1].pwff.fc1.weight)


def test_train_mode_is_seeded_and_masks_have_the_expected_mean():
    t, sd, dims = _golden()
    m = _module(sd, dims).train()
    torch.manual_seed(5)
    y1 = m(t["input"], t["input_2"], None, None)
    torch.manual_seed(5)
    y2 = m(t["input"], t["input_2"], None, None)
    y3 = m(t["input"], t["input_2"], None, None)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    assert not torch.equal(y1, m.eval()(t["input"], t["input_2"], None, None))
    big = train.Visual_Ling_Attn(N=2, vis_in_features=64, ins_in_features=64, d_model=256, h=4, d_ff=256, dropout=0.25)
    torch.manual_seed(6)
    keep = big.draw_keep(8, 40, 16, "cpu")
    assert [tuple(k.shape) for k in keep[:2]] == [(8 * 16, 256), (8 * 40, 256)] and len(keep) == 4
    assert [tuple(k.shape) for k in keep[2]] == [(320, 256), (320, 256), (320, 256)]
    for k in (*keep[:2], *keep[2], *keep[3]):
        assert k.dtype == torch.uint8 and abs(k.float().mean().item() - 0.75) <= 0.01
    torch.manual_seed(6)                                                 # the documented order: vis half, ins half, then each layer's three
    vis = (torch.rand(128, 256) >= 0.25).to(torch.uint8)
    ins = (torch.rand(320, 256) >= 0.25).to(torch.uint8)
    l0 = (torch.rand(320, 256) >= 0.25).to(torch.uint8)
    assert torch.equal(keep[0], vis) and torch.equal(keep[1], ins) and torch.equal(keep[2][0], l0)


def test_masks_are_refused():
    t, sd, dims = _golden()
    m = _module(sd, dims)
    with pytest.raises(ValueError, match="seq2seq_highlevel_cma.py:200-201"):
        m(t["input"], t["input_2"], torch.zeros(2, 5, 5, dtype=torch.bool), None)
    with pytest.raises(ValueError, match="seq2seq_highlevel_cma.py:200-201"):
        m(t["input"], t["input_2"], None, torch.zeros(2, 1, 5, 6, dtype=torch.bool))


def test_sinusoid_table_is_the_references_expression():
    tab = train.sinusoid_table(7, 16)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (7, 16) and not tab.is_cuda
    assert torch.equal(tab[0], torch.tensor([0.0, 1.0] * 8))
    pos, dim = torch.arange(7, dtype=torch.float32).view(-1, 1), torch.arange(8, dtype=torch.float32).view(1, -1)
    assert torch.equal(tab[:, ::2], torch.sin(pos / 10000 ** (2 * dim / 16))) and torch.equal(tab[:, 1::2], torch.cos(pos / 10000 ** (2 * dim / 16)))
    m = train.Visual_Ling_Attn(N=1, vis_in_features=8, ins_in_features=8, d_model=16, h=4, d_ff=32, dropout=0.0)
    assert m.table(7, "cpu") is m.table(7, "cpu") and torch.equal(m.table(7, "cpu"), tab) and m.table(6, "cpu").shape[0] == 6


@pytest.mark.parametrize("with_keep,with_post", [(False, False), (True, False), (False, True), (True, True)])
def test_embed_ln_ref_against_functional_composition(with_keep, with_post):
    g = torch.Generator().manual_seed(3)
    B, L, K, Dm, p = 3, 5, 24, 16, 0.3
    x = torch.rand(B, L, K, generator=g, dtype=torch.float64) * 2 - 1
    w, b = torch.rand(Dm, K, generator=g, dtype=torch.float64) - 0.5, torch.rand(Dm, generator=g, dtype=torch.float64) - 0.5
    gamma, beta = torch.rand(Dm, generator=g, dtype=torch.float64) + 0.5, torch.rand(Dm, generator=g, dtype=torch.float64) - 0.5
    keep = (torch.rand(B * L, Dm, generator=g) >= p).to(torch.uint8) if with_keep else None
    post = train.sinusoid_table(L, Dm) if with_post else None
    got = train.embed_ln_ref(x, w, b, gamma, beta, keep=keep, p=p, post=post)
    r = F.relu(F.linear(x, w, b))
    if with_keep:
        r = r * keep.reshape(B, L, Dm).double() / (1 - p)
    want = F.layer_norm(r, (Dm,), gamma, beta, 1e-5)
    if with_post:
        want = want + post.expand(B, L, Dm)                               # the reference's pe.expand(batch, L, d)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    flat = train.embed_ln_ref(x.reshape(B * L, K), w, b, gamma, beta, keep=keep, p=p, post=post)     # rows counted over all leading dimensions
    assert torch.equal(flat.reshape(B, L, Dm), want)


@pytest.mark.parametrize("case", ec.CASES)
def test_kink_condition_holds(case):
    """every pre-activation of the case is at least 2e-5 from zero in float64, the seed is the first such, and float32 agrees on every sign"""
    c = ec.case(*case)
    print(f"{case}: min |pre-activation| = {c['kink']:.3e}")
    assert c["kink"] >= ec.KINK
    assert ec.SEEDS[case] == ec.first_seed(*case[:4])
    x, w, b = c["args"][:3]
    pre32 = F.linear(x, w, b)
    assert torch.equal(pre32 > 0, F.linear(x.double(), w.double(), b.double()) > 0)
    assert c["gate"].dtype == torch.uint8 and tuple(c["gate"].shape) == (case[0], ec.D)


def test_cases_straddle_the_row_block_and_the_k_slices():
    rows = [c[0] for c in ec.CASES]
    assert {1, 63, 65, 130, 128} <= set(rows) and {64, 128, 192, 256, 320, 384, 448, 576, 768, 832, 960, 1024} == {c[1] for c in ec.CASES}
    assert any(not c[4] for c in ec.CASES) and any(c[2] for c in ec.CASES) and any(c[3] == 0 for c in ec.CASES)


def test_header_declares_and_binding_agrees():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for sym, n in (("hcm_op_embed_ln_train", 17), ("hcm_op_embed_ln_bwd", 14)):
        mt = re.search(r"int %s\(([^;]*)\);" % sym, text)
        assert mt, f"include/hcm.h does not declare {sym}"
        n_args = len([a for a in mt.group(1).split(",") if a.strip()])
        res, args = _lib.EXPORTS[sym]
        assert res is C.c_int and len(args) == n_args == n, (sym, len(args), n_args)
        assert hasattr(_lib.lib(), sym)
    assert re.search(r"int64_t hcm_op_embed_ln_work_floats\(int rows, int K\);", text)
    assert _lib.EXPORTS["hcm_op_embed_ln_work_floats"] == (C.c_int64, [C.c_int] * 2)


def test_work_floats_query():
    l = _lib.lib()
    for rows, K in ((0, 64), (1, 64), (64, 256), (65, 768), (5120, 1024)):
        assert l.hcm_op_embed_ln_work_floats(rows, K) == 256 * K + (rows + 63) // 64 * 1024
    for bad in ((1, 0), (1, 32), (1, 96), (1, 1088), (1, 2048), (1, -64), (-1, 64)):
        assert l.hcm_op_embed_ln_work_floats(*bad) == 0, bad


def test_argument_errors_without_a_device():
    """every refusal returns HCM_ERR_ARG in front of the first device call: sizes, p, the period, null and misaligned pointers, an output in the
    work buffer.  The pointers are host memory that nothing dereferences."""
    l = _lib.lib()
    raw = (C.c_float * 4096)()
    base = (C.addressof(raw) + 63) // 64 * 64
    ok = C.c_void_p(base)

    def fwd(ptrs=None, keep=None, post=None, p=0.0, period=0, rows=1, K=64):
        ptrs = ptrs or [ok] * 10                                          # x w b gamma beta | y xhat rstd gate work
        return l.hcm_op_embed_ln_train(*ptrs[:5], keep, p, post, period, *ptrs[5:], rows, K, None)

    def bwd(ptrs=None, p=0.0, rows=1, K=64):
        ptrs = ptrs or [ok] * 10                                          # d_y w gamma xhat rstd gate | work d_pre d_x d_ln
        return l.hcm_op_embed_ln_bwd(*ptrs[:6], p, *ptrs[6:], rows, K, None)

    for K in (0, 32, 96, 1088):
        assert fwd(K=K) == -1 and bwd(K=K) == -1
    assert fwd(rows=-1) == -1 and bwd(rows=-1) == -1
    for p in (1.0, -0.1, float("nan")):
        assert fwd(p=p) == -1 and bwd(p=p) == -1
    assert fwd(post=ok, period=0) == -1 and fwd(post=ok, period=-3) == -1
    for i in range(10):
        ptrs = [C.c_void_p(base + 64 * 1024 * (j + 1)) for j in range(10)]          # far apart: only the null counts
        ptrs[i] = None
        assert fwd(ptrs) == -1, i
        if i != 8:                                                        # a null d_x is the request not to compute it
            assert bwd(ptrs) == -1, i
    for i in (0, 1, 3, 4, 5, 6, 9):                                      # x w gamma beta y xhat work: 16 bytes
        ptrs = [C.c_void_p(base + 64 * 1024 * (j + 1)) for j in range(10)]
        ptrs[i] = C.c_void_p(ptrs[i].value + 4)
        assert fwd(ptrs) == -1, i
    far = [C.c_void_p(base + 64 * 1024 * (j + 1)) for j in range(10)]
    assert fwd(far, keep=C.c_void_p(base + 2)) == -1 and fwd(far, post=C.c_void_p(base + 8), period=1) == -1
    work_floats = l.hcm_op_embed_ln_work_floats(1, 64)
    for i in (5, 6, 7, 8):                                                # an output that starts in the work buffer's last 16 bytes
        ptrs = list(far)
        ptrs[i] = C.c_void_p(far[9].value + 4 * work_floats - 16)
        assert fwd(ptrs) == -1, i
    for i in (7, 8, 9):
        ptrs = list(far)
        ptrs[i] = C.c_void_p(far[6].value + 4 * work_floats - 16)
        assert bwd(ptrs) == -1, i
    assert fwd(rows=0) == 0                                               # nothing to do, nothing launched


def test_python_level_refusals_without_a_device():
    (x, w, b, gamma, beta), keep, post, _ = ec.make_inputs(5, 256, 5, 0.25, 0)
    with pytest.raises(ValueError, match="embed_ln_ref"):
        train.embed_ln(x, w, b, gamma, beta)
    with pytest.raises(ValueError):
        train.embed_ln(x, w, b, gamma, beta, keep=keep, p=0.25, post=post)
    assert train.embed_k_ok(64) and train.embed_k_ok(768) and train.embed_k_ok(1024)
    assert not any(train.embed_k_ok(K) for K in (0, 32, 96, 1088))
