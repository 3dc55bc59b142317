"""What the case lists of the four training ops reach, and whether their bound means anything where they reach it -- without a GPU.

Coverage: the launch forms, run-time branches and sequence edges of csrc/vla_train.hip, csrc/embed_train.hip, csrc/instr_scan.hip and
csrc/state_scan*.hip are chosen from the shapes alone, so the set a case list reaches can be computed here (the precedent is
test_cases_straddle_the_row_block_and_the_k_slices of tests/test_embed_train_cpu.py).  Each assertion names a set that must be complete; a case
taken out of a list leaves one of them short.

Reference alone: the GPU tests hold the kernels to 1e-5 of float64 (per tensor max|g - g64| / max|g64|, forward values 1e-5 absolute).  That bound
was set where every gate sits near the middle of its range and every softmax is close to uniform.  For each recurrent case at an edge or at the
horizon, each saturated case and each peaked case, the project's own pure-torch restatement is run here in float32 on the CPU against its
float64 run and must stay within HALF the bound, forward and every gradient: if float32 arithmetic in torch's order could not do that, the bound
would say nothing about a kernel in that regime.  This is a condition on the cases, not a tolerance on the code under test."""
import math

import pytest
import torch

from robo_vln_amd import train
from tests import embed_train_cases as ec
from tests import instr_train_cases as ic
from tests import state_scan_train_cases as sc
from tests import vla_train_cases as vc

HALF = 0.5 * 1e-5


# ---- coverage ----
def test_cross_modal_cases_reach_every_key_block_count_chunk_count_and_edge():
    lks = {c[2] for c in vc.CASES}
    assert {math.ceil(lk / 16) for lk in lks} == {1, 2, 3, 4}                     # vla_train_attn_bwd_kernel<KB>, KB = ceil(Lk / 16)
    for kb in (1, 2, 3, 4):                                                       # either edge of every instantiation
        assert {16 * (kb - 1) + 1, 16 * kb} <= lks, kb
    assert {15, 31} <= lks                                                        # one idle key lane in the last block, KB 1 and KB 2
    assert {c[3] // 256 for c in vc.CASES} == {1, 2, 3, 4}                        # d_ff chunks of 256
    rows = {c[0] * c[1] for c in vc.CASES}
    assert max(rows) > 128 and max(rows) % 64 != 0                                # three row blocks, the last one ragged
    assert any(c[1] > 128 for c in vc.CASES)                                      # ... of ONE sample: three 64-row chunks of the attention forward
    assert any(c[1] > 128 and math.ceil(c[2] / 16) == 2 for c in vc.CASES)        # three LayerNorm partials behind a KB 2 backward
    assert any(c[4] == 0 for c in vc.CASES) and any(c[4] > 0 for c in vc.CASES)
    assert set(vc.SEEDS) == set(vc.CASES) and len(set(vc.CASES)) == len(vc.CASES)
    # the peaked variant: the first three of the cases behind the original seven, as KB 2 at both edges (one with three chunks) and KB 3
    assert vc.PEAKED_CASES == vc.CASES[7:10] and set(vc.PEAKED_SEEDS) == set(vc.PEAKED_CASES)
    assert {math.ceil(c[2] / 16) for c in vc.PEAKED_CASES} == {2, 3} and {c[3] // 256 for c in vc.PEAKED_CASES} == {1, 3}


def test_prologue_cases_reach_every_k_slice_form_and_d_x_panel():
    ks = {c[1] for c in ec.CASES}
    # the forward walks K in slices of 256 with a ragged last one; every tail, alone and behind a full slice.  K is a multiple of 64 up to 1024,
    # which reaches all eight combinations: none is left out
    assert {(k > 256, k % 256) for k in ks} == {(full, tail) for full in (False, True) for tail in (0, 64, 128, 192)}
    # the backward's last d_x panel has 2, 4 or 6 tiles (K % 256 = 64, 128, 192); the ragged ones behind the fewest and the most full panels that
    # fit, and one behind exactly two: the panel's offset into the packed weight is 256 times that count
    with_dx = {(c[1] // 256, c[1] % 256) for c in ec.CASES if c[4]}
    assert {(1, 64), (2, 64), (1, 128), (0, 192), (1, 192), (3, 192)} <= with_dx
    assert any((c[1] // 256, c[1] % 256) == (3, 64) and not c[4] and c[0] > 128 for c in ec.CASES)    # three row blocks, no d_x: the pack is skipped
    rows = {c[0] for c in ec.CASES}
    assert {1, 63, 64, 65, 128} <= rows and any(r > 128 and r % 64 for r in rows)
    assert any(c[0] > 64 and c[2] and 64 % c[2] and c[2] % 64 for c in ec.CASES)                      # a table whose period does not divide the block
    assert set(ec.SEEDS) == set(ec.CASES) and len(set(ec.CASES)) == len(ec.CASES)


def _samples_per_workgroup(B, dirs):
    """instr_scan_sb of csrc/instr_scan.hip, the one rule of the forward scan in every form and of the reverse scan, restated: the smallest of
    2, 4, 8 that keeps ceil(B / SB) * dirs within 128 workgroups (8 where none does).  A change to that rule must change this function, and the cases with it."""
    for sb in (2, 4):
        if math.ceil(B / sb) * dirs <= 128:
            return sb
    return 8


def _instr_cases():
    return ic.GPU_CASES + ic.EDGE_CASES + ic.SATURATED_CASES


def test_instruction_cases_reach_every_samples_per_workgroup_count_in_either_direction_count():
    assert [_samples_per_workgroup(B, d) for B, d in ((256, 1), (257, 1), (512, 1), (513, 1), (128, 2), (129, 2), (256, 2), (257, 2))] == \
        [2, 4, 4, 8, 2, 4, 4, 8]
    reached = {(dirs, _samples_per_workgroup(B, dirs)) for _, dirs, _, B, _ in _instr_cases()}
    assert reached == {(dirs, sb) for dirs in (1, 2) for sb in (2, 4, 8)}
    # with one direction, either cell at each count, and both the per-token output and the final state (the d_final entry point)
    for sb in (4, 8):
        one = [(rnn, final) for rnn, dirs, final, B, _ in _instr_cases() if dirs == 1 and _samples_per_workgroup(B, dirs) == sb]
        assert {rnn for rnn, _ in one} == {"LSTM", "GRU"} and {final for _, final in one} == {False, True}, sb
    # at eight per workgroup: an idle workgroup and a last workgroup of one sample
    assert any(dirs == 1 and _samples_per_workgroup(B, 1) == 8 and B % 8 == 1 for _, dirs, _, B, _ in _instr_cases())
    for case in _instr_cases():
        assert (case[3], case[4]) in ic.LENGTHS and len(ic.LENGTHS[(case[3], case[4])]) == case[3], case
    assert len(set(_instr_cases())) == len(_instr_cases())


def test_instruction_cases_hold_every_packed_sequence_edge():
    """include/hcm.h: lengths are clamped to [0, L], a row of length 0 yields zeros and contributes nothing, and a workgroup whose samples are
    all empty runs no step"""
    seen = set()
    for _, dirs, _, B, L in _instr_cases():
        lengths = ic.LENGTHS[(B, L)]
        sb = _samples_per_workgroup(B, dirs)
        if 0 in lengths:
            seen.add("zero")
        if min(lengths) < 0:
            seen.add("negative")
        if max(lengths) > L:
            seen.add("past L")
        groups = [lengths[i:i + sb] for i in range(0, B, sb)]
        if any(max(g) <= 0 for g in groups) and any(max(g) > 0 for g in groups):
            seen.add(("idle workgroup", sb))
        if B % sb == 1 and B > sb:
            seen.add(("one sample in the last workgroup", sb))
        if L >= 200:
            seen.add(("horizon", dirs))
    assert {"zero", "negative", "past L", ("idle workgroup", 2), ("idle workgroup", 8), ("one sample in the last workgroup", 2),
            ("one sample in the last workgroup", 8), ("horizon", 1), ("horizon", 2)} <= seen
    # every setting meets the out-of-range lengths; at the horizon either cell, either direction count, with and without the final state
    for shape in ((6, 9), (4, 5)):
        assert ic.EDGE_SETTINGS[shape] == ic.SETTINGS
    assert set(ic.EDGE_SETTINGS[(3, 200)]) == {("LSTM", 2, False), ("GRU", 1, True), ("GRU", 2, False), ("LSTM", 1, True)}
    assert set(ic.EDGE_SETTINGS[(513, 2)]) == {("LSTM", 1, True), ("GRU", 1, True), ("LSTM", 1, False)}
    assert ic.EDGE_CASES == [(*s, B, L) for (B, L), settings in ic.EDGE_SETTINGS.items() for s in settings]
    horizon = [c for c in ic.EDGE_CASES if c[4] >= 200]
    assert {c[0] for c in horizon} == {"LSTM", "GRU"} and {c[1] for c in horizon} == {1, 2} and {c[2] for c in horizon} == {False, True}
    # the saturated regime: either cell, both directions, a scan long enough to carry a saturated state, an empty row beside it
    assert {c[0] for c in ic.SATURATED_CASES} == {"LSTM", "GRU"} and all(c[1] == 2 and c[4] >= 40 for c in ic.SATURATED_CASES)
    assert all(0 in ic.LENGTHS[(c[3], c[4])] for c in ic.SATURATED_CASES)
    t = torch.tensor([9, 0, -3, 4])
    assert ic.clamped(t, 5).tolist() == [5, 0, 0, 4]


def test_state_scan_cases_reach_the_horizon_the_sample_blocks_and_the_cut():
    shapes = {(T, N) for T, N, _ in sc.CASES}
    assert max(T for T, _ in shapes) >= 33 and any(T > 5 and T % 2 for T, _ in shapes)       # many uses of each ping-pong carry pair, an odd count
    assert any(N > 8 and T > 5 for T, N in shapes)                                          # forward sample blocks 8 + 5, backward 4 + 4 + 4 + 1
    assert any(N % 8 not in (0, 1) and N > 8 for _, N in shapes)
    assert any(N % 4 == 1 and N > 4 for _, N in shapes) and any(N < 4 for _, N in shapes) and any(N == 8 for _, N in shapes)
    assert {k for _, _, k in sc.CASES} == {"random", "ones", "zero0", "cut"}
    for T, N, kind in sc.CASES:
        if kind == "cut":
            assert T >= 4
            c = sc.case("GRU", T, N, kind)
            assert (c["m"][T // 2] == 0).all() and c["m"][T // 2 + 1:].sum() > 0 and c["m"][:T // 2].sum() > 0
            assert (c["cot"][:(T // 2) * N] == 0).all() and (c["cot"][(T // 2) * N:] != 0).any(1).all()
    assert sc.SATURATED_CASES and all(T >= 8 and kind == "random" for T, _, kind in sc.SATURATED_CASES)
    assert len(set(sc.CASES)) == len(sc.CASES)


def test_builders_leave_the_earlier_cases_bit_identical():
    """the keywords of the new regimes multiply behind the draws: without them a seed gives what it gave, with them only the named tensor moves"""
    a, _, cot = vc.make_inputs(2, 9, 17, 256, 0.25, 3)
    b, _, cot_b = vc.make_inputs(2, 9, 17, 256, 0.25, 3, q_scale=vc.PEAKED_Q_SCALE)
    assert torch.equal(b[0], a[0] * 16) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and torch.equal(cot, cot_b)
    emb, params, cot = ic.make_inputs("GRU", 2, False, 3, 4, 8, 5, 7)
    emb_s, params_s, cot_s = ic.make_inputs("GRU", 2, False, 3, 4, 8, 5, 7, ih_scale=ic.SATURATED_IH_SCALE)
    assert torch.equal(emb, emb_s) and torch.equal(cot, cot_s)
    for p, q in zip(params, params_s):
        assert torch.equal(q[0], p[0] * 20) and all(torch.equal(x, y) for x, y in zip(p[1:], q[1:]))
        assert p[0].abs().max() <= 0.1 and 1.9 < q[0].abs().max() <= 2.0
    c, s = sc.case("LSTM", 2, 1, "random"), sc.case("LSTM", 2, 1, "random", sc.SATURATED_IH_SCALE)
    assert torch.equal(s["p"][0], c["p"][0] * 20) and all(torch.equal(c[k], s[k]) for k in ("x", "h0", "m", "cot"))
    assert all(torch.equal(x, y) for x, y in zip(c["p"][1:], s["p"][1:]))


# ---- the restatements in float32 against themselves in float64 ----
def _within_half(got, want, what):
    """the project's rule (per tensor max|g - g64| / max|g64|, exact zero where the reference is identically zero) at half the bound"""
    e = vc.rel(got, want, what)
    assert e <= HALF, (what, e)
    return e


def _forward_within_half(y, y64, what):
    """forward values: the GPU tests ask 1e-5 absolute; here half of it, absolute and by the relative rule"""
    e = (y.double() - y64).abs().max().item()
    print(f"{what} forward, absolute: {e:.3e}")
    assert e <= HALF, (what, e)
    _within_half(y, y64, what + " forward")


def _instr_float32(rnn, dirs, final, B, L, ih_scale):
    c = ic.case(rnn, dirs, final, B, L, ih_scale=ih_scale)
    emb = c["emb"].clone().requires_grad_()
    params = [tuple(t.clone().requires_grad_() for t in p) for p in c["params"]]
    y = train.instr_encoder_ref(emb, c["lengths"], params, final)
    grads = torch.autograd.grad(y, [emb] + [t for p in params for t in p], c["cot"])
    return c, y.detach(), dict(zip(ic.grad_names(dirs), grads))


@pytest.mark.parametrize("rnn,dirs,final,B,L", ic.EDGE_CASES)
def test_instruction_edge_cases_are_well_conditioned_in_float32(rnn, dirs, final, B, L):
    c, y, grads = _instr_float32(rnn, dirs, final, B, L, 1.0)
    tag = f"float32 restatement [{rnn} dirs={dirs} final={final} B={B} L={L}]"
    _forward_within_half(y, c["y64"], tag)
    for k, g in grads.items():
        _within_half(g, c["ref"][k], f"{tag} {k}")
    # the reference itself at the edges: nothing at an inactive token, nothing for an empty row, and out-of-range lengths are the clamped ones
    active = torch.arange(L)[None, :] < c["lengths"][:, None]
    assert (c["ref"]["d_emb"][~active] == 0).all()
    if not final:
        assert (c["y64"][~active] == 0).all() and (c["y64"][active] != 0).any(1).all()
    else:
        assert (c["y64"][~active.any(1)] == 0).all()
    host = ic.clamped(c["lengths"], L)
    if not torch.equal(host, c["lengths"]):
        y_c, g_c = ic.reference(c["emb"], host, c["params"], final, c["cot"])
        assert torch.equal(y_c, c["y64"]) and all(torch.equal(a, b) for a, b in zip(g_c, c["ref"].values()))


def _saturated_share(pre):
    return (pre.abs() > 6).double().mean().item()


@pytest.mark.parametrize("rnn,dirs,final,B,L", ic.SATURATED_CASES)
def test_saturated_instruction_cases_are_well_conditioned_in_float32(rnn, dirs, final, B, L):
    c, y, grads = _instr_float32(rnn, dirs, final, B, L, ic.SATURATED_IH_SCALE)
    tag = f"float32 restatement [{rnn} dirs={dirs} final={final} B={B} L={L} saturated]"
    share = _saturated_share(torch.nn.functional.linear(c["emb"].double(), c["params"][0][0].double(), c["params"][0][2].double()))
    print(f"{tag}: {share:.3f} of the input-side pre-activations pass +-6")
    assert 0.15 <= share <= 0.25
    _forward_within_half(y, c["y64"], tag)
    for k, g in grads.items():
        _within_half(g, c["ref"][k], f"{tag} {k}")


def _state_float32(rnn, T, N, kind, ih_scale):
    c = sc.case(rnn, T, N, kind, ih_scale)
    leaves = [t.clone().requires_grad_() for t in (c["x"], *c["p"], c["h0"])]
    seq, hid = train.cell_loop(leaves[0], [tuple(leaves[1:5])], leaves[5], c["m"].reshape(-1), rnn)
    grads = torch.autograd.grad(seq, leaves, c["cot"])
    return c, seq.detach(), hid, dict(zip(sc.NAMES, grads))


@pytest.mark.parametrize("T,N,kind,ih_scale", [(*c, 1.0) for c in sc.CASES[7:]] + [(*c, sc.SATURATED_IH_SCALE) for c in sc.SATURATED_CASES])
@pytest.mark.parametrize("rnn", ["LSTM", "GRU"])
def test_state_scan_cases_are_well_conditioned_in_float32(rnn, T, N, kind, ih_scale):
    c, seq, hid, grads = _state_float32(rnn, T, N, kind, ih_scale)
    tag = f"float32 restatement [{rnn} T={T} N={N} {kind}{' saturated' if ih_scale != 1.0 else ''}]"
    if ih_scale != 1.0:
        share = _saturated_share(torch.nn.functional.linear(c["x"].double(), c["p"][0].double(), c["p"][2].double()))
        print(f"{tag}: {share:.3f} of the input-side pre-activations pass +-6")
        assert 0.10 <= share <= 0.25                   # (32 inputs: a standard deviation of 3.8, about 0.11; the instruction scan's 50 give 4.7)
    _forward_within_half(seq, c["seq64"], tag)
    _forward_within_half(hid, c["hid64"], tag + " hidden")
    for k, g in grads.items():
        _within_half(g, c["ref"][k], f"{tag} {k}")
    if kind == "cut":
        n = (T // 2) * N
        assert (c["ref"]["dx"][:n] == 0).all() and (c["ref"]["d_h_in"] == 0).all() and (c["ref"]["dx"][n:] != 0).any()


@pytest.mark.parametrize("case", vc.PEAKED_CASES)
def test_peaked_cross_modal_cases_are_well_conditioned_in_float32(case):
    c = vc.peaked_case(*case)
    plain = vc.case(*case)
    peak, flat = vc.mean_peak(c), vc.mean_peak(plain)
    print(f"{case}: mean largest probability {peak:.3f} with q times {vc.PEAKED_Q_SCALE:g}, {flat:.3f} without")
    assert peak >= 0.7 and flat <= 0.25
    assert c["kink"] >= vc.KINK and vc.PEAKED_SEEDS[case] == vc.first_seed(*case, q_scale=vc.PEAKED_Q_SCALE)
    leaves = [t.clone().requires_grad_() for t in c["args"]]
    out = train.vla_layer_ref(*leaves, keep=c["keep"], p=c["p"])
    grads = torch.autograd.grad(out, leaves, c["cot"])
    _forward_within_half(out.detach(), c["out64"], f"float32 restatement {case} peaked")
    for n, g in zip(vc.NAMES, grads):
        _within_half(g, c["ref"][n], f"float32 restatement {case} peaked {n}")
    # no fc1 pre-activation changes sign in float32
    k1 = c["keep"][0] if c["keep"] else None
    a32, a64 = c["args"], [t.double() for t in c["args"]]
    pre = [torch.nn.functional.linear(train.vla_attention_ref(a[0], a[1], a[2], a[3], a[4], a[9], a[10], k1, c["p"]), a[5], a[6]) for a in (a32, a64)]
    assert torch.equal(pre[0] > 0, pre[1] > 0)
