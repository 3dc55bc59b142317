"""The differentiable cross-modal layer on the GPU: robo_vln_amd.train.vla_layer (hcm_op_vla_layer_train + hcm_op_vla_layer_bwd) against float64
CPU autograd through train.vla_layer_ref on the cases of tests/vla_train_cases.py, the raw C ABI (determinism, NaN pre-fill, zero rows, NULL
masks), the training forward against the 16-bit inference kernel, the InterModuleAttnLayer module against its CPU path and with shared
weights, an optimizer step between two calls, a non-default stream, and the refusals.

Gradient bound: per tensor max|g - g64| / max|g64| <= 1e-5 (the bound and the zero rule of tests/test_state_scan_train_gpu.py; the float32 CPU
restatement lands at 3.8e-7 .. 6.0e-7 on these cases); forward within 1e-5 absolute of float64 (CPU float32: 1.6e-6).  The peaked cases
(q times 16, one key carrying most of a row's mass) run under the same bounds; tests/test_train_coverage_cpu.py holds the float32 CPU
restatement to half of them there (it lands at 2.4e-6 forward, 1.0e-6 on the gradients)."""
import ctypes as C
import functools

import pytest
import torch

from robo_vln_amd import _lib, train
from tests import vla_train_cases as vc

pytestmark = pytest.mark.gpu

BOUND = 1e-5
D = 256
RAW_CASES = [(3, 17, 33, 256, 0.25), (1, 7, 64, 1024, 0.25)] + vc.CASES[7:]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _cuda_keep(keep):
    return None if keep is None else tuple(k.cuda() for k in keep)


@functools.lru_cache(maxsize=None)
def _gpu(case, peaked=False):
    c = vc.peaked_case(*case) if peaked else vc.case(*case)
    leaves = [t.cuda().requires_grad_() for t in c["args"]]
    out = train.vla_layer(*leaves, keep=_cuda_keep(c["keep"]), p=c["p"])
    grads = torch.autograd.grad(out, leaves, c["cot"].cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), dict(zip(vc.NAMES, [g.cpu() for g in grads]))


@pytest.mark.parametrize("case", vc.CASES)
def test_gradients_match_float64_autograd(case):
    c = vc.case(*case)
    _, grads = _gpu(case)
    worst = {n: vc.rel(grads[n], c["ref"][n], f"{case} {n}") for n in vc.NAMES}
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert max(worst.values()) <= BOUND, worst


@pytest.mark.parametrize("case", vc.CASES)
def test_forward_matches_float64(case):
    c = vc.case(*case)
    out, _ = _gpu(case)
    err = (out.double() - c["out64"]).abs().max().item()
    print(f"{case} out: {err:.3e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("case", vc.PEAKED_CASES)
def test_peaked_attention_matches_float64(case):
    """q times 16: one key carries most of a row's mass (the mean largest probability is printed), so P (dP - sum P dP) cancels in the backward.
    The bounds are the ones above; tests/test_train_coverage_cpu.py holds the float32 CPU restatement to half of them on the same inputs."""
    c = vc.peaked_case(*case)
    out, grads = _gpu(case, True)
    err = (out.double() - c["out64"]).abs().max().item()
    print(f"{case} peaked (mean largest probability {vc.mean_peak(c):.3f}) out: {err:.3e}")
    assert err <= 1e-5, err
    worst = {n: vc.rel(grads[n], c["ref"][n], f"{case} peaked {n}") for n in vc.NAMES}
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert max(worst.values()) <= BOUND, worst


def test_one_key_has_no_query_or_key_gradient():
    """Lk = 1: the softmax over one key is the constant 1, so d_q and d_k are exactly zero (d_v is not)"""
    _, grads = _gpu(vc.CASES[0])
    assert vc.CASES[0][2] == 1
    assert grads["d_q"].abs().max().item() == 0
    assert grads["d_kv"][..., :D].abs().max().item() == 0
    assert grads["d_kv"][..., D:].abs().max().item() > 0


# ---- raw C ABI ----
def _raw_forward(a, keep, p, dims, fill=float("nan"), work=None):
    B, L, Lk, d_ff = dims
    rows = B * L
    l = _lib.lib()
    f = lambda *s: torch.full(s, fill, device="cuda")
    o = dict(out=f(rows, D), a=f(rows, D), x1=f(rows, D), x1hat=f(rows, D), h=f(rows, d_ff), x2hat=f(rows, D), rstd=f(rows, 2))
    work = torch.empty(l.hcm_op_vla_train_work_floats(B, L, Lk, d_ff), device="cuda") if work is None else work
    k = keep if keep is not None else (None, None, None)
    rc = l.hcm_op_vla_layer_train(*[_p(t) for t in a], _p(k[0]), _p(k[1]), _p(k[2]), p, _p(o["out"]), _p(o["a"]), _p(o["x1"]), _p(o["x1hat"]), _p(o["h"]),
                                  _p(o["x2hat"]), _p(o["rstd"]), _p(work), B, L, Lk, d_ff, None)
    return rc, o


def _raw_backward(a, keep, p, dims, saved, d_out, fill=float("nan")):
    B, L, Lk, d_ff = dims
    rows = B * L
    l = _lib.lib()
    q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = a
    f = lambda *s: torch.full(s, fill, device="cuda")
    o = dict(d_q=f(rows, D), d_I=f(rows, D), d_kv=f(B, Lk, 2 * D), d_u=f(rows, D), d_hpre=f(rows, d_ff), d_z=f(rows, D), d_ln=f(4, D))
    work = torch.empty(l.hcm_op_vla_train_work_floats(B, L, Lk, d_ff), device="cuda")
    k = keep if keep is not None else (None, None, None)
    rc = l.hcm_op_vla_layer_bwd(_p(d_out), _p(q), _p(kv), _p(wo), _p(w1), _p(w2), _p(g1), _p(g2), _p(k[0]), _p(k[1]), _p(k[2]), p, _p(saved["x1hat"]),
                                _p(saved["h"]), _p(saved["x2hat"]), _p(saved["rstd"]), _p(work), _p(o["d_q"]), _p(o["d_I"]), _p(o["d_kv"]), _p(o["d_u"]),
                                _p(o["d_hpre"]), _p(o["d_z"]), _p(o["d_ln"]), B, L, Lk, d_ff, None)
    return rc, o


@pytest.mark.parametrize("case", vc.PEAKED_CASES)
def test_raw_abi_bitwise_and_fully_written_with_peaked_attention(case):
    _raw_abi_bitwise_and_fully_written(case, True)


@pytest.mark.parametrize("case", RAW_CASES)
def test_raw_abi_bitwise_and_fully_written(case):
    """forward `out` equals the autograd function's bit for bit; two backward runs are bitwise equal; NaN-filled outputs come back fully written"""
    _raw_abi_bitwise_and_fully_written(case, False)


def _raw_abi_bitwise_and_fully_written(case, peaked):
    c = vc.peaked_case(*case) if peaked else vc.case(*case)
    a = [t.cuda() for t in c["args"]]
    keep, dims = _cuda_keep(c["keep"]), case[:4]
    rc, fw = _raw_forward(a, keep, c["p"], dims)
    assert rc == 0
    rc, b1 = _raw_backward(a, keep, c["p"], dims, fw, c["cot"].cuda().reshape(-1, D).contiguous())
    assert rc == 0
    rc, b2 = _raw_backward(a, keep, c["p"], dims, fw, c["cot"].cuda().reshape(-1, D).contiguous(), fill=0.0)
    assert rc == 0
    torch.cuda.synchronize()
    out, grads = _gpu(case, True) if peaked else _gpu(case)
    assert torch.equal(fw["out"].cpu().reshape(out.shape), out)
    for n, t in {**fw, **b1}.items():
        assert torch.isfinite(t).all(), f"{n} keeps pre-filled NaN"
    for n in b1:
        assert torch.equal(b1[n], b2[n]), n
    assert torch.equal(b1["d_q"].cpu().reshape(grads["d_q"].shape), grads["d_q"]) and torch.equal(b1["d_kv"].cpu(), grads["d_kv"])
    assert torch.equal(b1["d_ln"][2].cpu(), grads["d_g2"])


def test_raw_abi_zero_rows_and_null_masks():
    """A row whose keep masks are all zero: out = LN2(LN1(I)) whatever the attention gives, d_hpre, d_z, d_u of the row exactly 0 and d_I the plain
    two-LayerNorm chain; keep2 = 0 alone gives d_hpre of that row exactly 0.  NULL masks equal all-ones masks (p = 0) bit for bit."""
    case = RAW_CASES[0]
    c = vc.case(*case)
    B, L, Lk, d_ff = dims = case[:4]
    a = [t.cuda() for t in c["args"]]
    keep = [k.clone() for k in _cuda_keep(c["keep"])]
    r_all, r_k2 = 5, L + 3                           # r_k2 in the second sample
    for k in keep:
        k[r_all] = 0
    keep[1][r_k2] = 0
    cot = c["cot"].cuda().reshape(-1, D).contiguous()
    rc, fw = _raw_forward(a, keep, c["p"], dims)
    assert rc == 0
    rc, bw = _raw_backward(a, keep, c["p"], dims, fw, cot)
    assert rc == 0
    torch.cuda.synchronize()
    for n in ("d_hpre", "d_z", "d_u"):
        assert bw[n][r_all].abs().max().item() == 0, n
    assert bw["d_hpre"][r_k2].abs().max().item() == 0 and bw["d_z"][r_k2].abs().max().item() > 0
    assert fw["h"][r_all].abs().max().item() == 0 and fw["h"][r_k2].abs().max().item() == 0
    I, g1, be1, g2, be2 = (a[i][..., :].double().cpu() for i in (1, 9, 10, 11, 12))
    Ir = I.reshape(-1, D)[r_all].clone().requires_grad_()
    ln = torch.nn.functional.layer_norm
    y = ln(ln(Ir, (D,), g1, be1, 1e-5), (D,), g2, be2, 1e-5)
    (dI,) = torch.autograd.grad(y, Ir, cot[r_all].double().cpu())
    assert (fw["out"][r_all].double().cpu() - y.detach()).abs().max().item() <= 1e-5
    assert (bw["d_I"][r_all].double().cpu() - dI).abs().max().item() <= BOUND * dI.abs().max().item()
    assert bw["d_q"].reshape(B, L, D)[0, r_all].abs().max().item() == 0       # no gradient reaches the attention from that row

    ones = tuple(torch.ones_like(k) for k in keep)
    rc, f_null = _raw_forward(a, None, 0.0, dims)
    rc2, f_ones = _raw_forward(a, ones, 0.0, dims)
    assert rc == 0 and rc2 == 0
    rc, b_null = _raw_backward(a, None, 0.0, dims, f_null, cot)
    rc2, b_ones = _raw_backward(a, ones, 0.0, dims, f_ones, cot)
    assert rc == 0 and rc2 == 0
    torch.cuda.synchronize()
    for n in f_null:
        assert torch.equal(f_null[n], f_ones[n]), n
    for n in b_null:
        assert torch.equal(b_null[n], b_ones[n]), n


# ---- forward parity with the inference kernel ----
PARITY_LN2 = 0.125


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [(2, 80, 16, 256, 0.0), (1, 1, 1, 256, 0.0)])
def test_forward_parity_with_inference_kernel(case, prec):
    """p = 0: the training forward and hcm_op_vla_layer (16-bit storage) on the same inputs rounded to 16 bits agree within the 16-bit modes'
    1e-2, absolute, in fp16 and in bf16.  The inputs are the case's with the last LayerNorm's weight and bias times PARITY_LN2 = 1/8, so that
    |out| stays below 1 (normalised rows of 256 elements reach about 3.5; weight <= 0.19, bias <= 0.07): an absolute 1e-2 can only be asked of a
    kernel that stores bf16 where half a unit in the last place is below it -- 1.95e-3 under 1, against 1.56e-2 between 4 and 8, where the
    unscaled case's outputs (up to 5.2) lie and where 2.2e-2 was measured in bf16.  Everything in front of that LayerNorm is as in the case.
    A sanity tie between the two kernels, not a precision claim."""
    code, tdt = {"bf16": (_lib.HCM_BF16, torch.bfloat16), "fp16": (_lib.HCM_F16, torch.float16)}[prec]
    B, L, Lk, d_ff = dims = case[:4]
    c = vc.case(*case)
    args = list(c["args"])
    args[11], args[12] = args[11] * PARITY_LN2, args[12] * PARITY_LN2
    r = [t.to(tdt) if i in (0, 1, 2, 3, 5, 7) else t for i, t in enumerate(args)]          # q, I, kv and the three weights live in 16 bits there
    rc, fw = _raw_forward([t.float().cuda() for t in r], None, 0.0, dims)
    assert rc == 0
    d16 = [t.cuda().contiguous() for t in r]
    q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = d16
    out = torch.full((B, L, D), float("nan"), device="cuda", dtype=tdt)
    arr = lambda t: (C.c_void_p * 2)(t.data_ptr(), None)
    rc = _lib.lib().hcm_op_vla_layer(_p(q), _p(I), arr(kv), (C.c_int * 2)(Lk, 0), None, arr(out), None, 0, _p(wo), _p(bo), _p(w1), _p(b1), _p(w2), _p(b2),
                                     _p(g1), _p(be1), _p(g2), _p(be2), None, code, B, L, d_ff, 1, None)
    assert rc == 0
    torch.cuda.synchronize()
    err, scale = (out.float().reshape(-1, D) - fw["out"]).abs().max().item(), fw["out"].abs().max().item()
    print(f"{case} {prec}: max |inference - training| = {err:.3e}, max |out| = {scale:.3f}")
    assert scale < 1.0, scale
    assert torch.isfinite(out.float()).all() and err <= 1e-2, err


# ---- module ----
def _module_pair(d_ff, dropout, seed):
    torch.manual_seed(seed)
    m_cpu = train.InterModuleAttnLayer(d_ff=d_ff, dropout=dropout).double()
    with torch.no_grad():
        for n, prm in m_cpu.named_parameters():                     # LayerNorm parameters and biases off their trivial initial values
            if "layer_norm" in n or n.endswith("bias"):
                prm.add_(torch.rand_like(prm) * 0.2 - 0.1)
    m_gpu = train.InterModuleAttnLayer(d_ff=d_ff, dropout=dropout)
    m_gpu.load_state_dict(m_cpu.state_dict(), strict=True)
    return m_cpu, m_gpu.cuda()


def _assert_params_close(m_gpu, m_cpu, what):
    """Every parameter gradient against float64 by vc.rel.  fc_k.bias is the exception in scale only: its exact gradient is zero (a bias on the
    keys shifts every score of a row alike, which softmax ignores), float64 autograd returns rounding noise near 1e-17 for it rather than an
    identical zero, and a ratio to that noise says nothing -- it is the column sum of the same d_k whose product with the keys (magnitude <= 1)
    is fc_k.weight's gradient, so it is held to the bound on that tensor's scale."""
    worst = {}
    gc = {n: p.grad for n, p in m_cpu.named_parameters()}
    for n, pg in m_gpu.named_parameters():
        if n == "enc_att.attention.fc_k.bias":
            scale = gc["enc_att.attention.fc_k.weight"].abs().max().item()
            assert gc[n].abs().max().item() <= 1e-12 * scale                      # the reference itself: zero up to float64 noise
            worst[n] = (pg.grad.cpu().double() - gc[n]).abs().max().item() / scale
            print(f"{what} {n} (on fc_k.weight's scale): {worst[n]:.3e}")
        else:
            worst[n] = vc.rel(pg.grad.cpu(), gc[n], f"{what} {n}")
    assert max(worst.values()) <= BOUND, worst


def test_module_matches_its_cpu_path():
    """InterModuleAttnLayer on the device against its own CPU path (float64) with the same state dict and the same injected keep masks: forward,
    input gradients and all sixteen parameter gradients"""
    B, L, Lk, d_ff, p = 2, 9, 16, 512, 0.25
    m_cpu, m_gpu = _module_pair(d_ff, p, 3)
    g = torch.Generator().manual_seed(4)
    x1, x2, cot = torch.rand(B, L, D, generator=g) * 2 - 1, torch.rand(B, Lk, D, generator=g) * 2 - 1, torch.rand(B, L, D, generator=g) * 2 - 1
    keep = tuple((torch.rand(B * L, n, generator=g) >= p).to(torch.uint8) for n in (D, d_ff, D))
    a_c, b_c = x1.double().requires_grad_(), x2.double().requires_grad_()
    out_c = m_cpu(a_c, b_c, None, None, _keep=keep)
    out_c.backward(cot.double())
    a_g, b_g = x1.cuda().requires_grad_(), x2.cuda().requires_grad_()
    out_g = m_gpu(a_g, b_g, None, None, _keep=tuple(k.cuda() for k in keep))
    out_g.backward(cot.cuda())
    torch.cuda.synchronize()
    assert (out_g.detach().cpu().double() - out_c.detach()).abs().max().item() <= 1e-5
    assert vc.rel(a_g.grad.cpu(), a_c.grad, "d_input_1") <= BOUND and vc.rel(b_g.grad.cpu(), b_c.grad, "d_input_2") <= BOUND
    _assert_params_close(m_gpu, m_cpu, "module")


def test_module_shared_between_rgb_and_depth_calls():
    """One module called twice in one graph (RGB-like 16 keys, depth-like 36 keys), losses summed: parameter gradients accumulate as in float64"""
    B, L, d_ff = 2, 11, 256
    m_cpu, m_gpu = _module_pair(d_ff, 0.0, 5)
    g = torch.Generator().manual_seed(6)
    ins, rgb, dep = (torch.rand(B, n, D, generator=g) * 2 - 1 for n in (L, 16, 36))
    c1, c2 = torch.rand(B, L, D, generator=g) * 2 - 1, torch.rand(B, L, D, generator=g) * 2 - 1
    loss_c = (m_cpu(ins.double(), rgb.double(), None, None) * c1.double()).sum() + (m_cpu(ins.double(), dep.double(), None, None) * c2.double()).sum()
    loss_c.backward()
    loss_g = (m_gpu(ins.cuda(), rgb.cuda(), None, None) * c1.cuda()).sum() + (m_gpu(ins.cuda(), dep.cuda(), None, None) * c2.cuda()).sum()
    loss_g.backward()
    torch.cuda.synchronize()
    _assert_params_close(m_gpu, m_cpu, "shared")


def test_module_train_mode_draws_masks_from_torch_generator_on_device():
    m = train.InterModuleAttnLayer(d_ff=256, dropout=0.25).cuda().train()
    x1, x2 = torch.rand(2, 5, D, device="cuda"), torch.rand(2, 16, D, device="cuda")
    torch.manual_seed(11)
    y1 = m(x1, x2, None, None)
    torch.manual_seed(11)
    y2 = m(x1, x2, None, None)
    y3 = m(x1, x2, None, None)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    assert torch.equal(m.eval()(x1, x2, None, None), m(x1, x2, None, None))


def test_module_refusals_on_device():
    x1, x2 = torch.rand(1, 3, D, device="cuda"), torch.rand(1, 4, D, device="cuda")
    with pytest.raises(ValueError, match="seq2seq_highlevel_cma.py:200-201"):
        train.InterModuleAttnLayer(d_ff=256).cuda()(x1, x2, None, torch.zeros(1, 4, 3, 4, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        train.InterModuleAttnLayer(d_model=128, h=2, d_ff=256).cuda()(x1[..., :128], x2[..., :128], None, None)
    with pytest.raises(ValueError):
        train.InterModuleAttnLayer(d_ff=384).cuda()(x1, x2, None, None)


# ---- optimizer step ----
def test_adam_step_between_two_calls():
    """Adam (eps 1e-3: with the default eps the first update is lr * sign(g), which hides the gradient's magnitude) between two calls: the second
    forward sees the updated weights, nothing is cached; the parameters after the second step match the CPU float64 run to 1e-5 relative.
    lr = 1e-3, the step of tests/test_state_scan_train_gpu.py: an update lr g / (|g| + eps) moves by at most lr / eps = 1 times a gradient's
    error, so float32 gradients good to 1e-6 of max|g| leave the parameters within the bound (a first form with lr = 1e-2 multiplied the
    gradient error by 10 and read 1.03e-5 on fc_k.weight).  What that makes of this check, plainly: with a parameter of magnitude ~0.25 and a
    sensitivity of 1, the 1e-5 bound on the parameters only notices a gradient error of about 2.5e-6 absolute, roughly 1 % of max|g| here --
    it is a check that the optimizer's step reaches the kernels (`moved >= 50 * off`), not a gradient-accuracy check; the per-tensor gradient
    tests above carry that."""
    B, L, Lk, d_ff = 2, 7, 16, 256
    m_cpu, m_gpu = _module_pair(d_ff, 0.0, 7)
    g = torch.Generator().manual_seed(8)
    x1, x2, cot = torch.rand(B, L, D, generator=g) * 2 - 1, torch.rand(B, Lk, D, generator=g) * 2 - 1, torch.rand(B, L, D, generator=g) * 2 - 1
    outs = {}
    for name, m, cv in (("cpu", m_cpu, lambda t: t.double()), ("gpu", m_gpu, lambda t: t.cuda())):
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-3)
        outs[name] = []
        for _ in range(2):
            opt.zero_grad()
            out = m(cv(x1), cv(x2), None, None)
            (out * cv(cot)).sum().backward()
            opt.step()
            outs[name].append(out.detach().cpu().double())
    torch.cuda.synchronize()
    moved = (outs["cpu"][1] - outs["cpu"][0]).abs().max().item()
    off = [(outs["gpu"][i] - outs["cpu"][i]).abs().max().item() for i in range(2)]
    print(f"adam: the step moved the output by {moved:.3e}; device against float64 before / after the step {off[0]:.3e} / {off[1]:.3e}")
    assert off[0] <= 1e-5 and off[1] <= 1e-5                   # the forward bound, before and after the step ...
    assert moved >= 50 * off[1]                                # ... which the step's own effect exceeds many times: the device saw the new weights
    for (n, pg), (_, pc) in zip(m_gpu.named_parameters(), m_cpu.named_parameters()):
        e = (pg.detach().cpu().double() - pc.detach()).abs().max().item() / pc.detach().abs().max().item()
        print(f"adam {n}: {e:.3e}")
        assert e <= 1e-5, (n, e)


# ---- non-default stream ----
def test_non_default_stream_bitwise():
    case = (2, 5, 16, 256, 0.25)
    c = vc.case(*case)
    out0, grads0 = _gpu(case)
    s = torch.cuda.Stream()
    leaves = [t.cuda().requires_grad_() for t in c["args"]]
    keep, cot = _cuda_keep(c["keep"]), c["cot"].cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = train.vla_layer(*leaves, keep=keep, p=c["p"])
        grads = torch.autograd.grad(out, leaves, cot)
    s.synchronize()
    assert torch.equal(out.detach().cpu(), out0)
    for n, gt in zip(vc.NAMES, grads):
        assert torch.equal(gt.cpu(), grads0[n]), n


# ---- refusals ----
@pytest.mark.parametrize("Lk,d_ff", [(0, 256), (65, 256), (16, 1280), (16, 384)])
def test_unsupported_sizes_are_refused(Lk, d_ff):
    B, L = 1, 3
    l = _lib.lib()
    assert l.hcm_op_vla_train_work_floats(B, L, Lk, d_ff) == 0
    a, _, _ = vc.make_inputs(B, L, max(Lk, 1), d_ff, 0.0, 0)
    a = [t.cuda() for t in a]
    work = torch.zeros(l.hcm_op_vla_train_work_floats(B, L, 16, 1024), device="cuda")
    rc, fw = _raw_forward(a, None, 0.0, (B, L, Lk, d_ff), work=work)
    assert rc == -1
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in fw.values())                        # nothing launched
    if Lk == 0:
        a[2] = torch.zeros(B, 0, 2 * D, device="cuda")
    with pytest.raises(ValueError):
        train.vla_layer(*[t.requires_grad_() for t in a])


def test_work_buffer_overlapping_an_output_is_refused():
    case = (2, 5, 16, 256, 0.25)
    c = vc.case(*case)
    B, L, Lk, d_ff = dims = case[:4]
    a = [t.cuda() for t in c["args"]]
    n = _lib.lib().hcm_op_vla_train_work_floats(*dims)
    big = torch.full((n + B * L * D,), float("nan"), device="cuda")
    rc, fw = _raw_forward(a, None, 0.0, dims)
    assert rc == 0
    l = _lib.lib()
    out_in_work = big[n - 256:n - 256 + B * L * D]                                   # starts inside the work buffer's last 1 KB
    rc = l.hcm_op_vla_layer_train(*[_p(t) for t in a], None, None, None, 0.0, _p(out_in_work), _p(fw["a"]), _p(fw["x1"]), _p(fw["x1hat"]), _p(fw["h"]),
                                  _p(fw["x2hat"]), _p(fw["rstd"]), _p(big), B, L, Lk, d_ff, None)
    assert rc == -1
    q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = a
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    rc = l.hcm_op_vla_layer_bwd(_p(c["cot"].cuda()), _p(q), _p(kv), _p(wo), _p(w1), _p(w2), _p(g1), _p(g2), None, None, None, 0.0, _p(fw["x1hat"]), _p(fw["h"]),
                                _p(fw["x2hat"]), _p(fw["rstd"]), _p(big), _p(f(B * L, D)), _p(out_in_work), _p(f(B, Lk, 2 * D)), _p(f(B * L, D)),
                                _p(f(B * L, d_ff)), _p(f(B * L, D)), _p(f(4, D)), B, L, Lk, d_ff, None)
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.isnan(big).all()


def test_host_tensor_is_refused_at_the_python_level():
    c = vc.case(2, 5, 16, 256, 0.25)
    a = [t.cuda() for t in c["args"]]
    for i in (1, 3, 12):
        mixed = list(a)
        mixed[i] = c["args"][i]
        with pytest.raises(ValueError):
            train.vla_layer(*mixed)
    with pytest.raises(ValueError):
        train.vla_layer(*a, keep=c["keep"], p=0.25)                               # keep masks on the host
    with pytest.raises(ValueError):
        train.vla_layer(*c["args"])
