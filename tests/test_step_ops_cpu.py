"""tests/step_ops_cases.py on its own: the float64 references against the oracle's statements, the operator entries against the launchers of
csrc/elementwise.hip, and the inputs against what they were chosen for.  (The GPU side is tests/test_step_ops_gpu.py.)"""
import contextlib
import os
import re

import pytest
import torch

from oracle import hcm_oracle
from tests import step_ops_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robo-vln_amd", "csrc")


@contextlib.contextmanager
def float64_default():
    """the oracle builds its zero states with the default dtype"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ ties to the oracle (1e-12)
@pytest.mark.parametrize("kind,name", [(sc.LSTM, "LSTM"), (sc.GRU, "GRU")])
def test_cell_ref_equals_the_oracles_single_forward(kind, name):
    """cell_ref takes the gate products; the oracle takes x, the weights and the state: feed cell_ref the oracle's own products"""
    g = sc.gen(3)
    B, H, Fin, G = 5, 96, 40, 4 if kind == sc.LSTM else 3
    sd = {"rnn.weight_ih_l0": sc.uni(g, G * H, Fin).double(), "rnn.weight_hh_l0": sc.uni(g, G * H, H).double() / 8,
          "rnn.bias_ih_l0": sc.uni(g, G * H).double(), "rnn.bias_hh_l0": sc.uni(g, G * H).double()}
    w = hcm_oracle.Weights({k: v.numpy() for k, v in sd.items()})
    x, hidden = sc.uni(g, B, Fin).double(), sc.uni(g, 2 if kind == sc.LSTM else 1, B, H).double()
    mask = torch.tensor(sc.CELL_MASK).double()
    _, want = hcm_oracle.rnn_single_forward(x, hidden, mask, w, name)
    hm = hidden[0] * mask.view(-1, 1)
    gi = x @ sd["rnn.weight_ih_l0"].t() + sd["rnn.bias_ih_l0"]
    gh = hm @ sd["rnn.weight_hh_l0"].t() + sd["rnn.bias_hh_l0"]
    got = sc.cell_ref(kind, gi + gh, None, hidden, mask) if kind == sc.LSTM else sc.cell_ref(kind, gi, gh, hidden, mask)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("case", sc.ATTN_CASES, ids=sc.attn_id)
def test_attn_ref_equals_the_oracles_cma_attn(case):
    q, k, v, lens, scale = sc.make_attn(case)
    mask = None if lens is None else torch.arange(k.shape[1])[None] >= lens.long()[:, None]
    want = hcm_oracle.cma_attn(q.double(), k.double().transpose(1, 2), v.double().transpose(1, 2), scale, mask)
    assert (sc.attn_ref(q, k, v, lens, scale) - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("D", [768, 64])
def test_bert_embed_ref_equals_the_oracles_embedding_stage(D):
    """bert_encoder with no layers is its embedding stage; in-range ids (torch indexing wraps a negative id, the kernel clamps it)"""
    t = sc.make_bert_tables(D)
    sd = {"embeddings.word_embeddings.weight": t["word"], "embeddings.position_embeddings.weight": t["pos"],
          "embeddings.token_type_embeddings.weight": torch.stack([t["type0"], t["type0"] + 1]), "embeddings.LayerNorm.weight": t["gamma"],
          "embeddings.LayerNorm.bias": t["beta"]}
    w = hcm_oracle.Weights({k: v.double().numpy() for k, v in sd.items()})
    ids = torch.tensor(sc.BERT_IDS[7]).clamp(0, sc.BERT_VOCAB - 1)
    want = hcm_oracle.bert_encoder(ids, w, 0, 12)
    assert (sc.bert_embed_ref(ids, t) - want).abs().max().item() <= 1e-12


def test_bert_embed_ref_clamps():
    t = sc.make_bert_tables(64)
    ids = torch.tensor(sc.BERT_IDS[7])
    assert {0, sc.BERT_VOCAB - 1, -3, sc.BERT_VOCAB + 5} <= set(ids.flatten().tolist())
    assert torch.equal(sc.bert_embed_ref(ids, t), sc.bert_embed_ref(ids.clamp(0, sc.BERT_VOCAB - 1), t))


@pytest.mark.parametrize("kind,name", [(sc.LSTM, "LSTM"), (sc.GRU, "GRU")])
def test_instr_refs_equal_the_oracles_instruction_encoder(kind, name):
    """the length rule, the lookup and the packed step: instr_cell_ref stepped over the tokens against the oracle's forward direction"""
    g = sc.gen(5)
    H, E, G = 24, sc.INSTR_E, 4 if kind == sc.LSTM else 3
    ids = torch.tensor(sc.INSTR_IDS[9])
    table = sc.uni(g, sc.INSTR_VOCAB, E)
    sd = {"embedding_layer.weight": table.double(), "encoder_rnn.weight_ih_l0": sc.uni(g, G * H, E).double(),
          "encoder_rnn.weight_hh_l0": sc.uni(g, G * H, H).double(), "encoder_rnn.bias_ih_l0": sc.uni(g, G * H).double(),
          "encoder_rnn.bias_hh_l0": sc.uni(g, G * H).double()}
    w = hcm_oracle.Weights({k: v.numpy() for k, v in sd.items()})
    with float64_default():
        want, lengths = hcm_oracle.instruction_encoder(ids, w, H, False, name)
    mine = sc.instr_lengths_ref(ids)
    assert torch.equal(mine, lengths) and mine.tolist() == [4, 9, 1]           # row 0 has a zero in the middle
    x = sc.instr_embed_ref(ids, table, sc.INSTR_LDX).double()
    assert torch.equal(x[:, :, E:], torch.zeros(3, 9, sc.INSTR_LDX - E).double()) and torch.equal(x[:, :, :E], sd["embedding_layer.weight"][ids])
    h, c = torch.zeros(3, H).double(), (torch.zeros(3, H).double() if kind == sc.LSTM else None)
    lmax = int(mine.max())
    for t in range(lmax):
        pre = x[:, t, :E] @ sd["encoder_rnn.weight_ih_l0"].t() + sd["encoder_rnn.bias_ih_l0"]
        gh = h @ sd["encoder_rnn.weight_hh_l0"].t() + sd["encoder_rnn.bias_hh_l0"]
        h, c, out = sc.instr_cell_ref(kind, pre, gh, h, c, t < mine)
        assert (out - want[:, :, t]).abs().max().item() <= 1e-12, t


# ------------------------------------------------------------------------------------------------ every launcher has an entry
# launchers of elementwise.hip that no hcm_op_* entry calls, each with its reason
EXEMPT = {
    "launch_mark": "development aid: stores a clock value, nothing to compare",
    "launch_spin": "busy-wait of the stream-overlap probe: no output",
    "launch_convert_to_f32": "a type conversion: one rounding, pinned by every 16-bit operator test's read-back path and the feature export tests",
    "launch_convert": "a type conversion between storage types (or a device copy): one rounding",
}


def _launchers():
    decl = set(re.findall(r"^hipError_t (launch_\w+)\(", open(os.path.join(CSRC, "kernels.h")).read(), re.M))
    defs = set(re.findall(r"^hipError_t (launch_\w+)\(", open(os.path.join(CSRC, "elementwise.hip")).read(), re.M))
    return decl, defs


def _called_from_entries():
    api = open(os.path.join(CSRC, "api.cpp")).read()
    called = {}
    for m in re.finditer(r"^(?:int|int64_t) (hcm_op_\w+)\(", api, re.M):
        end = api.index("\n}", m.end())
        for name in re.findall(r"\b(launch_\w+)\(", api[m.end():end]):
            called.setdefault(name, set()).add(m.group(1))
    return called


def test_every_launcher_of_elementwise_hip_has_an_operator_entry():
    """Each launch_* that kernels.h declares and elementwise.hip defines is called from an hcm_op_* entry of api.cpp, or stands in EXEMPT with a
    reason.  Removing an entry, or adding a launcher without one, fails here."""
    decl, defs = _launchers()
    assert defs <= decl, defs - decl
    assert len(defs) >= 30
    called = _called_from_entries()
    missing = sorted(n for n in defs if n not in called and n not in EXEMPT)
    assert not missing, f"launchers of elementwise.hip without an hcm_op_* entry or an exemption: {missing}"
    stale = sorted(n for n in EXEMPT if n not in defs or n in called)
    assert not stale, f"exemptions that no longer apply: {stale}"
    assert all(len(r) > 10 for r in EXEMPT.values())
    # the entries this suite drives reach the launchers they are named for
    want = {"launch_rnn_prep": "hcm_op_rnn_cell", "launch_lstm_cell": "hcm_op_rnn_cell", "launch_gru_cell": "hcm_op_rnn_cell",
            "launch_heads_rows": "hcm_op_heads_rows", "launch_instr_lstm_cell": "hcm_op_instr_cell", "launch_instr_gru_cell": "hcm_op_instr_cell",
            "launch_attn1q": "hcm_op_attn1q", "launch_adaptive_avgpool": "hcm_op_adaptive_avgpool", "launch_mean_rows": "hcm_op_mean_rows",
            "launch_avgpool2_f32": "hcm_op_avgpool2", "launch_avgpool2_f32_padded": "hcm_op_avgpool2", "launch_bert_embed": "hcm_op_bert_embed",
            "launch_instr_embed": "hcm_op_instr_embed", "launch_layernorm_f32in": "hcm_op_layernorm_f32in", "launch_absmax": "hcm_op_absmax",
            "launch_argmax": "hcm_op_argmax", "launch_embed_rows": "hcm_op_embed_rows", "launch_val_subtask": "hcm_op_val_subtask",
            "launch_fill_cols": "hcm_op_fill_cols", "launch_copy_rows": "hcm_op_copy_rows"}
    for launcher, entry in want.items():
        assert entry in called.get(launcher, ()), (launcher, entry)


def test_entries_are_declared_with_matching_argument_counts():
    from robo_vln_amd import _lib
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    names = sorted({e for es in _called_from_entries().values() for e in es} & {
        "hcm_op_rnn_cell", "hcm_op_heads_rows", "hcm_op_instr_cell", "hcm_op_attn1q", "hcm_op_adaptive_avgpool", "hcm_op_mean_rows", "hcm_op_avgpool2",
        "hcm_op_bert_embed", "hcm_op_instr_embed", "hcm_op_layernorm_f32in", "hcm_op_absmax", "hcm_op_argmax", "hcm_op_embed_rows",
        "hcm_op_val_subtask", "hcm_op_fill_cols", "hcm_op_copy_rows"})
    assert len(names) == 16
    for name in names:
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", text, re.S)
        assert m, f"include/hcm.h does not declare {name}"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.EXPORTS[name][1]), name
    # hcm_op_heads: field for field
    m = re.search(r"typedef struct hcm_op_heads \{(.*?)\} hcm_op_heads;", text, re.S)
    fields = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert fields == [f[0] for f in _lib.HcmOpHeadsStruct._fields_], fields


# ------------------------------------------------------------------------------------------------ the inputs do what they are chosen for
@pytest.mark.parametrize("n", sc.ARGMAX_N)
def test_argmax_rows_tie_in_float32_and_cover_the_nan_positions(n):
    rows = sc.argmax_rows(n)
    assert rows.shape == (sc.ARGMAX_B, n) and rows.dtype == torch.float32
    want = torch.argmax(rows, dim=1)
    fin = ~torch.isnan(rows).any(1)
    mx = rows.max(1, keepdim=True).values
    ties = ((rows == mx).sum(1) >= 2) & fin
    if n == 1:
        assert bool(torch.isnan(rows[:, 0]).any())
        return
    # an exact tie of the maximum at every pair of positions, resolved to the first
    pairs = {tuple(torch.nonzero(rows[r] == mx[r]).flatten().tolist()) for r in torch.nonzero(ties).flatten().tolist()}
    assert {(i, j) for i in range(n) for j in range(i + 1, n)} <= pairs
    for r in torch.nonzero(ties).flatten().tolist():
        assert want[r].item() == torch.nonzero(rows[r] == mx[r]).flatten()[0].item()
    # a NaN at every position, alone and beside larger / infinite values: torch takes the first NaN
    nan_first = {int(torch.nonzero(torch.isnan(rows[r])).flatten()[0]) for r in range(rows.shape[0]) if bool(torch.isnan(rows[r]).any())}
    assert nan_first == set(range(n))
    for r in range(rows.shape[0]):
        if bool(torch.isnan(rows[r]).any()):
            assert want[r].item() == int(torch.nonzero(torch.isnan(rows[r])).flatten()[0])
    # rows on which `p[j] > best` alone (a NaN never compares greater) takes another index than torch: the NaN above index 0
    plain = []
    for r in rows.tolist():
        best = 0
        for j in range(1, n):
            if r[j] > r[best]:
                best = j
        plain.append(best)
    assert int((torch.tensor(plain) != want).sum()) >= n - 1
    assert bool((rows == float("inf")).any()) and bool((rows == float("-inf")).all(1).any())


def test_uneven_pool_windows_differ_in_size_and_overlap():
    wh, ww = sc.pool_windows(5, 4), sc.pool_windows(7, 4)
    assert wh == [(0, 2), (1, 3), (2, 4), (3, 5)] and ww == [(0, 2), (1, 4), (3, 6), (5, 7)]
    assert len({b - a for a, b in ww}) > 1 and any(ww[i][1] > ww[i + 1][0] for i in range(3))
    assert sc.pool_windows(2, 4) == [(0, 1), (0, 1), (1, 2), (1, 2)]            # the output larger than the input: windows of one
    assert sc.pool_windows(4, 4) == [(i, i + 1) for i in range(4)]              # the identity
    # the window rule is F.adaptive_avg_pool2d's
    _, x = sc.make_pool_input(2, 5, 7, 8, "fp32")
    ref = sc.adaptive_pool_ref(x, 4, 4)
    for oy, (y0, y1) in enumerate(wh):
        for ox, (x0, x1) in enumerate(ww):
            assert (ref[:, oy, ox] - x[:, y0:y1, x0:x1].mean((1, 2))).abs().max().item() <= 1e-15
    # dividing by a constant count instead (a 2 x 2 window everywhere) is far outside the bound
    wrong = torch.stack([torch.stack([x[:, y0:y1, x0:x1].sum((1, 2)) / 4 for x0, x1 in ww], 1) for y0, y1 in wh], 1)
    assert (wrong - ref).abs().max().item() > 100 * sc.f32_bound(ref)
    assert float((x == 0).double().mean()) > 0.2 and float(x.min()) >= 0


@pytest.mark.parametrize("case", [c for c in sc.ATTN_CASES if c[5]], ids=sc.attn_id)
def test_masked_attention_logits_underflow_to_zero_in_float64(case):
    q, k, v, lens, scale = sc.make_attn(case)
    p = sc.attn_ref(q, k, v, lens, scale, probs=True)
    masked = torch.arange(k.shape[1])[None] >= lens.long()[:, None]
    assert bool(masked.any()) and int(lens.min()) >= 1
    assert bool((p[masked] == 0.0).all())
    assert (p.sum(1) - 1).abs().max().item() <= 1e-12
    # ... so the masked result is the unmasked attention over the first length positions, and differs from ignoring the mask by far more than the bound
    full = sc.attn_ref(q, k, v, None, scale)
    ref = sc.attn_ref(q, k, v, lens, scale)
    for b in range(q.shape[0]):
        n = int(lens[b])
        cut = sc.attn_ref(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], None, scale)
        assert (cut - ref[b:b + 1]).abs().max().item() <= 1e-15
    short = [b for b in range(q.shape[0]) if int(lens[b]) < k.shape[1]]
    assert (full[short] - ref[short]).abs().max().item() > 100 * sc.f32_bound(ref)


def test_cell_cases_mix_masks_and_stale_states():
    for kind in (sc.LSTM, sc.GRU):
        c = sc.Cell(kind, 96, "r2_1")
        assert set(c.mask.tolist()) == {0.0, 1.0}
        ref = sc.cell_ref(kind, c.gates, c.gh, c.h_in, c.mask)
        assert bool(torch.isfinite(ref).all())
        # a masked sample's result is that of a zero state, whatever the stale state holds
        z = c.h_in.clone()
        z[:, c.mask == 0] = 0
        assert torch.equal(ref, sc.cell_ref(kind, c.gates, c.gh, z, c.mask))
        # ... and reading the stale state instead is far outside the bound
        wrong = sc.cell_ref(kind, c.gates, c.gh, c.h_in, torch.ones_like(c.mask))
        assert not bool(((wrong - ref).abs() <= sc.f32_bound(ref)).all())
        one = c.row(3)
        assert one.B == 1 and torch.equal(one.gates[0], c.gates[3]) and torch.equal(one.h_in[:, 0], c.h_in[:, 3])


def test_ulp_is_the_storage_spacing():
    for prec, tdt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        # at a representable value the bound is the distance to the next representable one above it
        for x in (1.0, 1.5, 0.75, 3.0, 2.0 ** -10, 96.0, -5.0):
            t = torch.tensor(abs(x), dtype=tdt)
            up = float((t.view(torch.int16) + 1).view(tdt))
            assert sc.ulp(torch.tensor([x]).double(), prec).item() == up - abs(x), (prec, x)
        # inside a binade it is that binade's spacing, and it never falls below the subnormal spacing
        assert sc.ulp(torch.tensor([1.9999]).double(), prec).item() == 2.0 ** -sc.MANT[prec]
        assert sc.ulp(torch.tensor([0.0, 1e-45, -1e-45]).double(), prec).tolist() == [sc.TINY[prec]] * 3
        assert float(torch.finfo(tdt).smallest_normal) * 2.0 ** -sc.MANT[prec] == sc.TINY[prec]


def test_layernorm_offset_case_is_a_hundred_standard_deviations():
    x, _, _ = sc.make_ln(7, 768, offset=100.0)
    assert (x.double().mean(1) / x.double().std(1)).min().item() > 90
    _, mean, rstd = sc.layernorm_ref(x, torch.ones(768), torch.zeros(768))
    assert (mean - 100).abs().max().item() < 0.2 and (rstd - 1).abs().max().item() < 0.1


def test_absmax_inputs_hold_every_special_value():
    for prec in ("fp32", "fp16", "bf16"):
        x = sc.make_absmax(3, 100, 128, prec, True)
        mx, bad = sc.absmax_ref(x, 100)
        assert mx == sc.FMAX[prec] and bad == 4
        assert bool(torch.isnan(x[:, 100:].float()).all())
        mx0, bad0 = sc.absmax_ref(sc.make_absmax(3, 100, 128, prec, False), 100)
        assert bad0 == 0 and 3.5 < mx0 <= 4.0
