"""The differentiable instruction encoder on the GPU: robo_vln_amd.train.instr_scan (hcm_op_instr_scan_train + hcm_op_instr_scan_bwd) against
float64 CPU autograd through train.instr_encoder_ref, exact zeros at padding, the training forward against the engines' one-launch scans bit
for bit, the saved tensors, determinism, the InstructionEncoder module against its CPU path, an optimizer step between two calls, a
non-default stream, and the refusals.

Gradient bound: per tensor max|g - g64| / max|g64| <= 1e-5 with exact zero where the reference is identically zero (`rel` / BOUND, the rule of
tests/test_state_scan_train_gpu.py); forward outputs 1e-5 absolute.  torch's own float32 CPU path lies within 7.1e-7 (forward 1.7e-7) of float64
on the first five shapes with these input distributions.  No element is excluded from any comparison.  The edge cases of
tests/instr_train_cases.py (lengths of 0, below 0 and past L, a workgroup of empty rows, 200 tokens, eight samples per workgroup in one direction)
and the saturated ones run under the same bounds; tests/test_train_coverage_cpu.py holds the float32 CPU restatement to half of them there.

Samples per workgroup: the launcher takes the fewest of 2, 4, 8 that keep the launch within 128 workgroups (instr_scan_sb of csrc/instr_scan.hip,
one rule for the engines' scans, the training forward and the reverse scan); with two directions (130, 3) reaches 4 and (260, 2) reaches 8, with
one direction (260, 2) reaches 4 and (513, 2) reaches 8, every other case runs at 2 (tests/test_train_coverage_cpu.py computes this from the case
lists).  The engines' scans and the training forward are one kernel, instr_scan_kernel<SB, GRU, FORM>, whose FORM only selects stores: the bitwise
comparison of the two guards that, and tests/golden/instr_scan_parent_bits.json holds all of them to the bits of the three separate kernels that
kernel replaced.  These tests load the shipped library."""
import ctypes as C
import functools
import json
import os

import pytest
import torch

from robo_vln_amd import _lib, train
from tests import instr_train_cases as cases
from tests.instr_train_cases import BOUND, rel

pytestmark = pytest.mark.gpu

H, E = 256, 50
SHAPES, CASES = cases.GPU_SHAPES, cases.GPU_CASES


def _gpu(rnn, dirs, final, B, L, emb_grad=True, lengths=None, ih_scale=1.0):
    c = cases.case(rnn, dirs, final, B, L, ih_scale=ih_scale)
    emb = c["emb"].cuda().requires_grad_(emb_grad)
    params = [tuple(t.cuda().requires_grad_() for t in p) for p in c["params"]]
    y = train.instr_scan(emb, (c["lengths"] if lengths is None else lengths).cuda(), params, final)
    leaves = ([emb] if emb_grad else []) + [t for p in params for t in p]
    grads = torch.autograd.grad(y, leaves, c["cot"].cuda())
    torch.cuda.synchronize()
    names = cases.grad_names(dirs)[0 if emb_grad else 1:]
    return y.detach().cpu(), dict(zip(names, (g.cpu() for g in grads)))


def _check_against_float64(c, y, grads, tag, dirs, final, L):
    e_y = (y.double() - c["y64"]).abs().max().item()
    print(f"{tag} forward {e_y:.3e}")
    assert y.shape == c["y64"].shape and e_y <= 1e-5
    active = torch.arange(L)[None, :] < c["lengths"][:, None]
    empty = ~active.any(1)
    if not final:
        assert (y[~active] == 0).all()                                   # exact zeros at every inactive token
    else:
        assert (y[empty] == 0).all()                                     # the zero state of a row without a token
    errs = {k: rel(grads[k], c["ref"][k], f"{tag} {k}") for k in cases.grad_names(dirs)}
    # an inactive token, and so every token of an empty sample, receives exactly nothing (as in the reference)
    assert (c["ref"]["d_emb"][~active] == 0).all() and (grads["d_emb"][~active] == 0).all()
    assert (grads["d_emb"][empty] == 0).all()
    assert max(errs.values()) <= BOUND, errs


@pytest.mark.parametrize("rnn,dirs,final,B,L", CASES + cases.EDGE_CASES)
def test_gradients_match_float64_autograd(rnn, dirs, final, B, L):
    c = cases.case(rnn, dirs, final, B, L)
    y, grads = _gpu(rnn, dirs, final, B, L)
    _check_against_float64(c, y, grads, f"[{rnn} dirs={dirs} final={final} B={B} L={L}]", dirs, final, L)


@pytest.mark.parametrize("rnn,dirs,final,B,L", cases.SATURATED_CASES)
def test_gradients_match_float64_autograd_with_saturated_gates(rnn, dirs, final, B, L):
    """weight_ih times 20: about a fifth of the input-side pre-activations pass +-6, so g (1 - g) and 1 - n^2 round towards zero.  The bound is the
    one above; tests/test_train_coverage_cpu.py holds the float32 CPU restatement to half of it on the same inputs."""
    c = cases.case(rnn, dirs, final, B, L, ih_scale=cases.SATURATED_IH_SCALE)
    y, grads = _gpu(rnn, dirs, final, B, L, ih_scale=cases.SATURATED_IH_SCALE)
    _check_against_float64(c, y, grads, f"[{rnn} dirs={dirs} final={final} B={B} L={L} saturated]", dirs, final, L)


OUT_OF_RANGE = [(*s, B, L) for B, L in ((6, 9), (4, 5)) for s in cases.SETTINGS]


@pytest.mark.parametrize("rnn,dirs,final,B,L", OUT_OF_RANGE)
def test_out_of_range_lengths_are_the_clamped_lengths_bitwise(rnn, dirs, final, B, L):
    """a length below 0 is 0 and one past L is L: the scans' own results -- the output through the autograd function, and out, final, d_pre and
    d_gh through the C ABI -- carry the bits of a call whose lengths were clamped on the host.  (The parameter gradients end in torch GEMMs over
    those d_pre / d_gh, the BLAS library's business, and are held to float64 above.)"""
    raw_lengths = cases.case(rnn, dirs, final, B, L)["lengths"]
    host = cases.clamped(raw_lengths, L)
    assert not torch.equal(host, raw_lengths) and host.min() >= 0 and host.max() <= L
    y, grads = _gpu(rnn, dirs, final, B, L)
    y_c, grads_c = _gpu(rnn, dirs, final, B, L, lengths=host)
    assert torch.equal(y, y_c)
    for k in grads:
        assert rel(grads[k], grads_c[k].double(), f"clamped on the host {k}") <= 1e-6
    a, _ = _raw(rnn, dirs, final, B, L)
    b, _ = _raw(rnn, dirs, final, B, L, lengths=host)
    for k in ("out", "fin", "d_pre", "d_gh"):
        if a[k] is not None:
            assert not a[k].isnan().any() and torch.equal(a[k], b[k]), k


def _raw(rnn, dirs, final, B, L, nan_cot_at_padding=False, lengths=None, ih_scale=1.0):
    """hcm_op_instr_scan_train, hcm_op_instr_scan_bwd and the engines' inference scan through the C ABI on one case's inputs (or on `lengths` in
    place of the case's); every output starts as NaN"""
    c = cases.case(rnn, dirs, final, B, L, ih_scale=ih_scale)
    lstm = rnn == "LSTM"
    G = 4 if lstm else 3
    kind = _lib.HCM_LSTM if lstm else _lib.HCM_GRU
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pt = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    emb = c["emb"].cuda().reshape(B * L, E)
    params = [tuple(t.cuda() for t in p) for p in c["params"]]
    pre = torch.stack([torch.addmm(b_ih + b_hh if lstm else b_ih + torch.cat([b_hh[:2 * H], b_hh.new_zeros(H)]), emb, w_ih.t())
                       for w_ih, _, b_ih, b_hh in params])
    w_hh = torch.stack([p[1] for p in params])
    b_hn = None if lstm else torch.stack([p[3][2 * H:] for p in params])
    lens = (c["lengths"] if lengths is None else lengths).to(torch.int32).cuda()
    nan = float("nan")
    o = dict(out=torch.full((B, L, dirs * H), nan, device="cuda"), fin=torch.full((B, H), nan, device="cuda"),
             gates=torch.full((dirs, B, L, 4 * H), nan, device="cuda"), c_seq=torch.full((dirs, B, L, H), nan, device="cuda") if lstm else None,
             d_pre=torch.full((dirs, B, L, G * H), nan, device="cuda"), d_gh=None if lstm else torch.full((dirs, B, L, G * H), nan, device="cuda"))
    n_work = lib.hcm_op_instr_scan_work_floats(B, L, dirs, kind)
    assert n_work == dirs * 4 * H * H
    work, work_b = torch.empty(n_work, device="cuda"), torch.empty(n_work, device="cuda")
    assert lib.hcm_op_instr_scan_train(pt(pre), pt(w_hh), pt(b_hn), pt(lens), pt(o["out"]), pt(o["fin"]), pt(o["gates"]), pt(o["c_seq"]), pt(work),
                                       B, L, H, dirs, kind, st) == 0, _lib.last_error()
    cot = c["cot"].cuda()
    if nan_cot_at_padding:                                               # a cotangent at an inactive token must not be read
        cot = cot.clone()
        cot[~(torch.arange(L)[None, :] < c["lengths"][:, None]).cuda()] = nan
    assert lib.hcm_op_instr_scan_bwd(None if final else pt(cot), pt(cot) if final else None, pt(o["gates"]), pt(o["c_seq"]), pt(o["out"]), pt(w_hh),
                                     pt(lens), pt(work_b), pt(o["d_pre"]), pt(o["d_gh"]), B, L, H, dirs, kind, st) == 0, _lib.last_error()
    ref = None
    if final or lstm:                                                    # the engines' launch on the weights the training forward packed
        ref = torch.full((B, H) if final else (B, L, dirs * H), nan, device="cuda")
        assert lib.hcm_op_instr_scan_infer(pt(pre), pt(work), pt(b_hn), pt(lens), pt(ref), B, L, H, dirs, kind, int(final), st) == 0, _lib.last_error()
    torch.cuda.synchronize()
    return o, ref


RAW = [(*s, B, L) for s in cases.SETTINGS for B, L in ((3, 7), (5, 33))] + [("LSTM", 2, False, 130, 3), ("GRU", 2, False, 260, 2)] + cases.EDGE_CASES


@pytest.mark.parametrize("rnn,dirs,final,B,L", RAW)
def test_padding_is_exactly_zero_and_saved_tensors_are_written(rnn, dirs, final, B, L):
    c = cases.case(rnn, dirs, final, B, L)
    o, _ = _raw(rnn, dirs, final, B, L, nan_cot_at_padding=not final)
    g64, c64, active = cases.saved64(c["emb"], c["lengths"], c["params"])
    out, fin = o["out"].cpu(), o["fin"].cpu()
    assert (out[~active] == 0).all() and not out.isnan().any()
    assert not fin.isnan().any() and (fin[~active.any(1)] == 0).all()       # the zero state of a row without a token
    for k in ("d_pre", "d_gh"):
        if o[k] is not None:
            t = o[k].cpu()
            assert not t.isnan().any(), k                               # every element written, and the NaN cotangents at padding were not read
            assert (t[:, ~active] == 0).all(), k
    # saved tensors started as NaN: every active element was written, each within 1e-5 of float64, and as include/hcm.h says nothing was
    # written at an inactive token (GRU leaves nothing out of its four slots: r, z, n and hn)
    gates = o["gates"].cpu()
    e_g = (gates[:, active].double() - g64[:, active]).abs().max().item()
    assert not gates[:, active].isnan().any() and gates[:, ~active].isnan().all()
    e_c = 0.0
    if c64 is not None:
        cs = o["c_seq"].cpu()
        assert not cs[:, active].isnan().any() and cs[:, ~active].isnan().all()
        e_c = (cs[:, active].double() - c64[:, active]).abs().max().item()
    fin64 = c["y64"] if final else None
    e_f = (o["fin"].cpu().double() - fin64).abs().max().item() if final else 0.0
    print(f"[{rnn} dirs={dirs} final={final} B={B} L={L}] saved gates {e_g:.3e} c_seq {e_c:.3e} final {e_f:.3e}")
    assert e_g <= 1e-5 and e_c <= 1e-5 and e_f <= 1e-5


@pytest.mark.parametrize("rnn,dirs,final,B,L", cases.INFER_CASES)
def test_training_forward_is_the_inference_scan_bitwise(rnn, dirs, final, B, L):
    o, ref = _raw(rnn, dirs, final, B, L)
    assert not ref.isnan().any()
    assert torch.equal(o["fin"] if final else o["out"], ref)


@functools.lru_cache(maxsize=None)
def _parent_bits():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instr_scan_parent_bits.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("rnn,dirs,final,B,L", cases.PARENT_BITS_CASES)
def test_forward_scans_carry_the_parent_commits_bits(rnn, dirs, final, B, L):
    """out, fin, gates, c_seq of hcm_op_instr_scan_train and the output of hcm_op_instr_scan_infer, each pre-filled with NaN, carry the SHA-256
    that tools/record_instr_scan_bits.py recorded with the three separate scan kernels in front of csrc/instr_scan.hip's one kernel, on inputs drawn
    without a GEMM.  No case and no tensor is left out; a tensor the case does not have (c_seq of a GRU, the inference output of a per-token GRU) is
    recorded as null and must be absent."""
    want = _parent_bits()[cases.case_id(rnn, dirs, final, B, L)]
    inputs, outputs = cases.forward_scan_digests(_lib.lib(), rnn, dirs, final, B, L)
    assert inputs == want["inputs"], "the inputs drawn here are not the recorded ones: re-record the fixture at the parent commit (tools/record_instr_scan_bits.py)"
    assert set(outputs) == set(want["outputs"]) == {"out", "fin", "gates", "c_seq", "infer_out"}
    for k, v in want["outputs"].items():
        assert outputs[k] == v, k


@pytest.mark.parametrize("rnn,dirs,final", [("LSTM", 2, False), ("GRU", 2, False), ("LSTM", 1, True), ("GRU", 1, True)])
def test_empty_rows_and_an_empty_workgroup_leave_zeros_and_untouched_saved_tensors(rnn, dirs, final):
    """(6, 9): rows of length 0, a workgroup whose two samples are both empty (it runs no step) and a negative length, one call each of
    hcm_op_instr_scan_train and hcm_op_instr_scan_bwd with every output pre-filled with NaN.  out, final, d_pre and d_gh come back without a NaN
    and zero at every inactive token, the idle workgroup's rows included; gates and c_seq are written at active tokens only."""
    B, L = 6, 9
    c = cases.case(rnn, dirs, final, B, L)
    o, _ = _raw(rnn, dirs, final, B, L, nan_cot_at_padding=not final)
    active = torch.arange(L)[None, :] < c["lengths"][:, None]
    empty = ~active.any(1)
    assert empty.tolist() == [False, True, True, True, False, True] and active.sum().item() == 13
    for k in ("out", "fin", "d_pre", "d_gh", "gates", "c_seq"):
        if o[k] is None:
            continue
        t = o[k].cpu()
        if k == "fin":
            assert not t.isnan().any() and (t[empty] == 0).all() and (t[~empty] != 0).any(1).all()
        elif k == "out":
            assert not t.isnan().any() and (t[~active] == 0).all() and (t[active] != 0).any(1).all()
        elif k in ("d_pre", "d_gh"):
            assert not t.isnan().any() and (t[:, ~active] == 0).all() and (t[:, active] != 0).any(2).all(), k
        else:
            assert t[:, ~active].isnan().all() and t[:, active].isfinite().all(), k


def test_the_final_state_is_the_last_active_output():
    for rnn in ("LSTM", "GRU"):
        o, _ = _raw(rnn, 1, True, 5, 33)
        idx = cases.case(rnn, 1, True, 5, 33)["lengths"].cuda() - 1
        assert torch.equal(o["fin"], o["out"][torch.arange(5, device="cuda"), idx])


@pytest.mark.parametrize("rnn,dirs,final,B,L", [("LSTM", 2, False, 5, 33), ("GRU", 2, False, 5, 33), ("LSTM", 1, True, 9, 12), ("GRU", 1, True, 9, 12),
                                                ("GRU", 2, False, 130, 3), ("LSTM", 2, False, 6, 9), ("GRU", 1, True, 6, 9), ("GRU", 2, False, 4, 5),
                                                ("LSTM", 2, False, 3, 200), ("GRU", 2, False, 3, 200), ("LSTM", 1, True, 513, 2),
                                                ("GRU", 1, True, 513, 2), ("LSTM", 1, False, 513, 2)])
def test_two_runs_give_the_same_bits(rnn, dirs, final, B, L):
    a, _ = _raw(rnn, dirs, final, B, L)
    b, _ = _raw(rnn, dirs, final, B, L)
    active = (torch.arange(L)[None, :] < cases.case(rnn, dirs, final, B, L)["lengths"][:, None]).cuda()
    for k in ("d_pre", "d_gh", "out", "fin"):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["gates"][:, active], b["gates"][:, active])


@pytest.mark.parametrize("rnn,dirs,final,B,L", cases.SATURATED_CASES)
def test_saturated_gates_are_saved_and_two_runs_give_the_same_bits(rnn, dirs, final, B, L):
    """the saturated cases through the C ABI: the saved gates (many within rounding of 0 or 1) and c within 1e-5 of float64, untouched at inactive
    tokens, and every output of a second run bitwise equal"""
    c = cases.case(rnn, dirs, final, B, L, ih_scale=cases.SATURATED_IH_SCALE)
    a, _ = _raw(rnn, dirs, final, B, L, nan_cot_at_padding=True, ih_scale=cases.SATURATED_IH_SCALE)
    b, _ = _raw(rnn, dirs, final, B, L, nan_cot_at_padding=True, ih_scale=cases.SATURATED_IH_SCALE)
    g64, c64, active = cases.saved64(c["emb"], c["lengths"], c["params"])
    gates = a["gates"].cpu()
    assert gates[:, ~active].isnan().all()
    e_g = (gates[:, active].double() - g64[:, active]).abs().max().item()
    e_c = (a["c_seq"].cpu()[:, active].double() - c64[:, active]).abs().max().item() if c64 is not None else 0.0
    sat = ((g64[:, active][..., :2 * H] < 1e-3) | (g64[:, active][..., :2 * H] > 1 - 1e-3)).double().mean().item()
    print(f"[{rnn} dirs={dirs} final={final} B={B} L={L} saturated] saved gates {e_g:.3e} c_seq {e_c:.3e}; {sat:.3f} of the first two gates within 1e-3 of 0 or 1")
    assert e_g <= 1e-5 and e_c <= 1e-5 and sat > 0.1
    for k in ("out", "fin", "d_pre", "d_gh"):
        if a[k] is not None:
            assert not a[k].isnan().any() and torch.equal(a[k], b[k]), k
    assert torch.equal(a["gates"][:, active.cuda()], b["gates"][:, active.cuda()])


def test_d_emb_is_absent_when_the_input_does_not_require_it():
    want_y, want = _gpu("GRU", 2, False, 3, 7)
    y, grads = _gpu("GRU", 2, False, 3, 7, emb_grad=False)
    assert "d_emb" not in grads and torch.equal(y, want_y)
    for k, g in grads.items():
        assert rel(g, want[k].double(), f"without d_emb {k}") <= 1e-6
    # and the function hands autograd None for it
    c = cases.case("GRU", 2, False, 3, 7)
    emb = c["emb"].cuda()
    params = [tuple(t.cuda().requires_grad_() for t in p) for p in c["params"]]
    y = train.instr_scan(emb, c["lengths"].cuda(), params, False)
    (y * c["cot"].cuda()).sum().backward()
    assert emb.grad is None and all(t.grad is not None for p in params for t in p)


def _modules(rnn, bidir, final, fine_tune, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.rand(23, E, generator=g) * 2 - 1
    table[0] = 0
    kw = dict(embeddings=table, hidden_size=H, rnn_type=rnn, bidirectional=bidir, final_state_only=final, fine_tune_embeddings=fine_tune)
    cpu = train.InstructionEncoder(**kw)
    with torch.no_grad():
        for p in cpu.encoder_rnn.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    dev = train.InstructionEncoder(**kw)
    dev.load_state_dict(cpu.state_dict())
    return cpu.double(), dev.cuda(), g


def _ids(B, L, lengths, g):
    ids = torch.randint(1, 23, (B, L), generator=g)
    ids[torch.arange(L)[None, :] >= torch.tensor(lengths)[:, None]] = 0
    return ids


@pytest.mark.parametrize("fine_tune", [False, True])
@pytest.mark.parametrize("rnn,bidir,final", [("LSTM", True, False), ("GRU", False, True), ("GRU", True, False), ("LSTM", False, True)])
def test_module_matches_its_cpu_path(rnn, bidir, final, fine_tune):
    cpu, dev, g = _modules(rnn, bidir, final, fine_tune, 5)
    B, L = 5, 9
    ids = _ids(B, L, [9, 1, 4, 0, 6], g)                                  # one all-padding row
    y64 = cpu(ids)
    cot = torch.rand(y64.shape, generator=g) * 2 - 1
    (y64 * cot.double()).sum().backward()
    y = dev(ids.cuda())
    (y * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert y.shape == ((B, H) if final else (B, (2 if bidir else 1) * H, L))
    e = (y.detach().cpu().double() - y64.detach()).abs().max().item()
    print(f"module [{rnn} bidir={bidir} final={final} fine_tune={fine_tune}]: forward {e:.3e}")
    assert e <= 1e-5 and (y[3] == 0).all()
    assert (dev.embedding_layer.weight.grad is not None) == fine_tune == (cpu.embedding_layer.weight.grad is not None)
    errs = [rel(pd.grad.cpu(), pc.grad, f"module [{rnn}] {n}") for (n, pc), pd in zip(cpu.named_parameters(), dev.parameters()) if pc.grad is not None]
    assert len(errs) == (4 * (2 if bidir else 1) + fine_tune) and max(errs) <= BOUND


@pytest.mark.parametrize("rnn,bidir,final", [("LSTM", True, False), ("GRU", False, True)])
def test_an_optimizer_step_is_seen_by_the_next_call(rnn, bidir, final):
    """Adam with eps = 1e-3: with the default 1e-8 the first update is lr * sign(g) for every element, so an element whose float64 gradient
    is below float32 rounding noise could move by +lr on one side and -lr on the other; 1e-3 makes the update continuous in g."""
    cpu, dev, g = _modules(rnn, bidir, final, True, 9)
    ids = _ids(4, 8, [8, 3, 1, 5], g)
    outs = []
    for mod, to in ((cpu, lambda t: t), (dev, lambda t: t.cuda())):
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3, eps=1e-3)
        y1 = mod(to(ids))
        y1.square().sum().backward()
        opt.step()
        with torch.no_grad():
            y2 = mod(to(ids))
        outs.append((y1.detach().cpu().double(), y2.cpu().double()))
    (c1, c2), (d1, d2) = outs
    moved, e1, e2 = (d2 - d1).abs().max().item(), (d1 - c1).abs().max().item(), (d2 - c2).abs().max().item()
    print(f"optimizer step [{rnn}]: output moved by {moved:.3e}; vs CPU before {e1:.3e} after {e2:.3e}")
    assert moved > 1e-4 and e1 <= 1e-5 and e2 <= 1e-5


@pytest.mark.parametrize("rnn,dirs,final", [("LSTM", 2, False), ("GRU", 1, True)])
def test_calls_enqueue_on_the_current_stream(rnn, dirs, final):
    B, L = 5, 33
    want_y, want = _gpu(rnn, dirs, final, B, L)
    c = cases.case(rnn, dirs, final, B, L)
    emb = c["emb"].cuda().requires_grad_()
    params = [tuple(t.cuda().requires_grad_() for t in p) for p in c["params"]]
    lens, cot = c["lengths"].cuda(), c["cot"].cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    before, after = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s):
        before.record()
        y = train.instr_scan(emb, lens, params, final)
        grads = torch.autograd.grad(y, [emb] + [t for p in params for t in p], cot)
        after.record()
    after.synchronize()                                                  # only the side stream's work is waited for
    assert before.query() and after.query()
    # the scan's own output: the same bits.  The gradients end in a torch GEMM or sum, whose reduction order is the BLAS library's: float32 rounding
    assert torch.equal(y.detach().cpu(), want_y)
    for k, gk in zip(cases.grad_names(dirs), grads):
        assert rel(gk.cpu(), want[k].double(), f"side stream [{rnn}] {k}") <= 1e-6


@pytest.mark.parametrize("host", ["weight_hh", "lengths"])
def test_a_host_tensor_beside_device_rows_is_refused(host):
    """the kernels take raw pointers: a tensor left on the CPU must raise before any launch"""
    c = cases.case("GRU", 1, True, 3, 7)
    w_ih, w_hh, b_ih, b_hh = (t.cuda() for t in c["params"][0])
    lens = c["lengths"].cuda()
    if host == "weight_hh":
        w_hh = w_hh.cpu()
    else:
        lens = lens.cpu()
    with pytest.raises(ValueError, match=host):
        train.instr_scan(c["emb"].cuda(), lens, [(w_ih, w_hh, b_ih, b_hh)], True)


def test_limits_are_named():
    mod = train.InstructionEncoder(vocab_size=9, embedding_size=E, hidden_size=128, rnn_type="LSTM", bidirectional=False, final_state_only=True).cuda()
    with pytest.raises(ValueError, match="256"):
        mod(torch.tensor([[1, 2, 0]], device="cuda"))
    emb, params, _ = cases.make_inputs("LSTM", 1, True, 2, 3, 128, E, 0)
    with pytest.raises(ValueError, match="256"):
        train.instr_scan(emb.cuda(), torch.tensor([3, 1], device="cuda"), [tuple(t.cuda() for t in params[0])], True)
    with pytest.raises(ValueError, match="one direction"):
        emb, params, _ = cases.make_inputs("LSTM", 2, False, 2, 3, H, E, 0)
        train.instr_scan(emb.cuda(), torch.tensor([3, 1], device="cuda"), [tuple(t.cuda() for t in p) for p in params], True)


def test_the_c_abi_refuses_bad_arguments_with_a_message():
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pt = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    B, L = 2, 3
    pre, w_hh = torch.zeros(1, B * L, 4 * H, device="cuda"), torch.zeros(1, 4 * H, H, device="cuda")
    lens = torch.ones(B, dtype=torch.int32, device="cuda")
    out, fin, gates, c_seq = (torch.zeros(n, device="cuda") for n in (B * L * H, B * H, B * L * 4 * H, B * L * H))
    work = torch.zeros(4 * H * H + 4, device="cuda")

    def call(pre=pre, w_hh=w_hh, out=out, work=work, hidden=H, dirs=1):
        return lib.hcm_op_instr_scan_train(pt(pre), pt(w_hh), None, pt(lens), pt(out), pt(fin), pt(gates), pt(c_seq), pt(work), B, L, hidden, dirs,
                                           _lib.HCM_LSTM, st)

    assert call() == 0, _lib.last_error()
    for kw, word in ((dict(hidden=128), "256"), (dict(dirs=3), "dirs"), (dict(w_hh=None), "NULL"), (dict(out=work[:B * L * H]), "overlaps"),
                     (dict(work=work[1:]), "aligned")):
        assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.hcm_op_instr_scan_work_floats(B, L, 3, _lib.HCM_LSTM) == 0
    torch.cuda.synchronize()
