"""The differentiable instruction encoder without a GPU: train.instr_encoder_ref against torch's own packed sequence in float64, the
InstructionEncoder module against the reference-captured goldens, its state dict, the gradient routing of frozen embeddings, its refusals
and a row of length 0."""
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from robo_vln_amd import synth, train
from robo_vln_amd.config import CMAConfig
from tests import instr_train_cases as cases
from tests import s2s_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
H, E = 16, 6                                         # the restatement serves any size
SHAPES = [(1, 1, (1,)), (3, 7, (7, 1, 4)), (5, 33, (33, 17, 1, 20, 32))]       # each holds a length-1 row


def _torch_packed(rnn, dirs, final, emb, lengths, params):
    """the reference's sequence (instruction_encoder.py:80-92) in float64, padded to L"""
    L = emb.shape[1]
    mod = getattr(nn, rnn)(input_size=emb.shape[2], hidden_size=params[0][1].shape[1], bidirectional=dirs == 2).double()
    leaves = []
    for sfx, p in zip(("", "_reverse"), params):
        for n, t in zip(cases.PARAM_NAMES, p):
            getattr(mod, f"{n}_l0{sfx}").data.copy_(t)
            leaves.append(getattr(mod, f"{n}_l0{sfx}"))
    e64 = emb.double().requires_grad_()
    packed = pack_padded_sequence(e64, lengths.cpu(), batch_first=True, enforce_sorted=False)
    output, final_state = mod(packed)
    if final:
        y = (final_state[0] if rnn == "LSTM" else final_state).squeeze(0)
    else:
        y = pad_packed_sequence(output, batch_first=True, total_length=L)[0].permute(0, 2, 1)
    return y, [e64] + leaves


@pytest.mark.parametrize("B,L,lengths", SHAPES)
@pytest.mark.parametrize("rnn,dirs,final", cases.SETTINGS)
def test_restatement_is_torchs_packed_sequence(rnn, dirs, final, B, L, lengths):
    lengths = torch.tensor(lengths)
    emb, params, cot = cases.make_inputs(rnn, dirs, final, B, L, H, E, seed=B + L)
    y64, g64 = cases.reference(emb, lengths, params, final, cot)
    y, leaves = _torch_packed(rnn, dirs, final, emb, lengths, params)
    want = y if final else y.permute(0, 2, 1)
    e = (y64 - want.detach()).abs().max().item()
    print(f"[{rnn} dirs={dirs} final={final} B={B} L={L}] forward {e:.3e}")
    assert y64.shape == want.shape and e <= 1e-12
    gt = torch.autograd.grad(want, leaves, cot.double())
    for name, a, b in zip(cases.grad_names(dirs), g64, gt):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(f"  {name}: {err:.3e} of {scale:.3e}")
        assert err <= 1e-10 * scale, name


def _s2s_module(cfg, sd):
    mod = train.InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden,
                                   rnn_type=cfg.instr_rnn, bidirectional=False, final_state_only=True)
    pre = "instruction_encoder."
    mod.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}, strict=True)
    return mod


@pytest.mark.parametrize("name", ["s2s_128_L20", "s2s_gru_128_L12"])
def test_module_reproduces_the_reference_golden(name):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, B, _, n_instr = s2s_ref.case_config(name)
    mod = _s2s_module(cfg, synth.make_s2s_weights(cfg, s2s_ref.SEED))
    obs = synth.make_s2s_observations(cfg, B, step=0, seed=s2s_ref.SEED, n_instr=n_instr)
    with torch.no_grad():
        y = mod(torch.from_numpy(obs["instruction"]).long())
    e = np.abs(y.numpy() - gold["tap.instruction"]).max()
    print(f"{name}: {e:.3e}")
    assert y.shape == gold["tap.instruction"].shape and e <= 1e-5


def test_state_dict_is_the_references():
    class Ref(nn.Module):                            # the reference's members, by its names (instruction_encoder.py:36-48)
        def __init__(self, vocab, emb, hid):
            super().__init__()
            self.embedding_layer = nn.Embedding(vocab, emb, padding_idx=0)
            self.encoder_rnn = nn.LSTM(input_size=emb, hidden_size=hid, bidirectional=True)

    cfg = CMAConfig(rgb_hw=128, depth_hw=128, instr_len=12).validate()
    assert cfg.bidirectional and cfg.instr_rnn == "LSTM"
    mod = train.InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden, rnn_type="LSTM",
                                   bidirectional=True, final_state_only=False)
    want = {k: tuple(v.shape) for k, v in Ref(cfg.vocab_size, cfg.embedding_size, cfg.instr_hidden).state_dict().items()}
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == want
    assert "encoder_rnn.weight_hh_l0_reverse" in want and "embedding_layer.weight" in want
    pre = "instruction_encoder."
    sd = {k[len(pre):]: torch.from_numpy(v) for k, v in synth.make_cma_weights(cfg, 0).items() if k.startswith(pre)}
    assert set(sd) == set(want)
    mod.load_state_dict(sd, strict=True)
    assert torch.equal(mod.encoder_rnn.weight_hh_l0_reverse, sd["encoder_rnn.weight_hh_l0_reverse"])
    ids = torch.from_numpy(synth.make_cma_observations(cfg, 2, step=0, seed=0)["instruction"]).long()
    y = mod(ids)
    assert y.shape == (2, 2 * cfg.instr_hidden, cfg.instr_len)
    # the reference's (B, D, max(lengths)) zero-padded to L
    lens = (ids != 0).sum(1)
    assert (y[0, :, lens[0]:] == 0).all() and (y[0, :, :lens[0]].abs().sum(0) > 0).all()


def _grad_module(fine_tune, **kw):
    g = torch.Generator().manual_seed(4)
    table = torch.rand(11, E, generator=g) - 0.5
    table[0] = 0
    mod = train.InstructionEncoder(embeddings=table, hidden_size=H, fine_tune_embeddings=fine_tune, **kw)
    with torch.no_grad():
        for p in mod.encoder_rnn.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
    return mod


@pytest.mark.parametrize("fine_tune", [False, True])
def test_frozen_embeddings_receive_no_gradient(fine_tune):
    mod = _grad_module(fine_tune, rnn_type="GRU", bidirectional=True, final_state_only=False)
    ids = torch.tensor([[3, 5, 7, 0], [2, 0, 0, 0], [9, 9, 1, 4]])
    mod(ids).square().sum().backward()
    assert (mod.embedding_layer.weight.grad is not None) == fine_tune
    assert mod.embedding_layer.weight.requires_grad == fine_tune
    for n, p in mod.encoder_rnn.named_parameters():
        assert p.grad is not None and p.grad.abs().max().item() > 0, n


def test_refusals():
    with pytest.raises(ValueError, match="final_state_only"):
        train.InstructionEncoder(vocab_size=5, embedding_size=E, hidden_size=H, rnn_type="LSTM", bidirectional=True, final_state_only=True)
    with pytest.raises(TypeError, match="dropout"):
        train.InstructionEncoder(vocab_size=5, embedding_size=E, hidden_size=H, rnn_type="LSTM", bidirectional=False, final_state_only=True, dropout=0.1)
    with pytest.raises(TypeError, match="missing"):
        train.InstructionEncoder(vocab_size=5, embedding_size=E, hidden_size=H)
    with pytest.raises(ValueError, match="rnn_type"):
        train.InstructionEncoder(vocab_size=5, embedding_size=E, hidden_size=H, rnn_type="RNN", bidirectional=False, final_state_only=True)

    class Cfg:                                       # a config object serves, and keyword arguments win
        vocab_size, embedding_size, hidden_size, rnn_type, bidirectional, final_state_only, fine_tune_embeddings = 5, E, H, "GRU", False, True, False

    mod = train.InstructionEncoder(Cfg(), hidden_size=2 * H)
    assert isinstance(mod.encoder_rnn, nn.GRU) and mod.encoder_rnn.hidden_size == 2 * H and mod.output_size == 2 * H


@pytest.mark.parametrize("rnn,dirs,final", cases.SETTINGS)
def test_a_row_of_length_zero_contributes_nothing(rnn, dirs, final):
    B, L = 3, 7
    lengths = torch.tensor([7, 1, 4])
    emb, params, cot = cases.make_inputs(rnn, dirs, final, B, L, H, E, seed=21)
    y, g = cases.reference(emb, lengths, params, final, cot)
    g_ = torch.Generator().manual_seed(5)
    emb2 = torch.cat([emb[:1], torch.rand(1, L, E, generator=g_), emb[1:]])          # an all-padding row between the valid ones
    cot2 = torch.cat([cot[:1], torch.rand(1, *cot.shape[1:], generator=g_), cot[1:]])
    y2, g2 = cases.reference(emb2, torch.tensor([7, 0, 1, 4]), params, final, cot2)
    # float64 on both sides; the extra row changes the row count of the batched products, so their summation order: 1e-12, not bit equality
    assert (y2[1] == 0).all() and (y2[[0, 2, 3]] - y).abs().max().item() <= 1e-12
    assert (g2[0][1] == 0).all()
    for name, a, b in zip(cases.grad_names(dirs), (g2[0][[0, 2, 3]], *g2[1:]), g):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), name


def test_the_recorded_scan_bits_belong_to_the_inputs_drawn_here():
    """tests/golden/instr_scan_parent_bits.json holds every case of PARENT_BITS_CASES, each with all five outputs, and the digests of the inputs it
    was recorded on are those of cases.scan_inputs on this machine (they are drawn on the CPU): a change to the draw shows here, without a GPU,
    and means recording again with the library of the commit whose bits are to be kept (tools/record_instr_scan_bits.py)."""
    import json
    with open(os.path.join(GOLD, "instr_scan_parent_bits.json")) as f:
        rec = json.load(f)["cases"]
    assert set(rec) == {cases.case_id(*c) for c in cases.PARENT_BITS_CASES} and len(rec) == len(cases.PARENT_BITS_CASES) == 20
    for rnn, dirs, final, B, L in cases.PARENT_BITS_CASES:
        want = rec[cases.case_id(rnn, dirs, final, B, L)]
        assert {k: cases.digest(v) for k, v in cases.scan_inputs(rnn, dirs, B, L).items()} == want["inputs"], (rnn, dirs, final, B, L)
        assert set(want["outputs"]) == {"out", "fin", "gates", "c_seq", "infer_out"}
        assert (want["outputs"]["c_seq"] is None) == (rnn == "GRU") and (want["outputs"]["infer_out"] is None) == (rnn == "GRU" and not final)
        assert all(want["outputs"][k] for k in ("out", "fin", "gates"))
