"""CPU side of the precomputed instruction stream: train.HighLevel's (N, L, D) form, the header / binding / library agreement on the new symbols, the
validator's stream cache against a stand-in engine, and the kernel cases' own expectations."""
import ctypes as C
import os
import re

import pytest
import torch

from robo_vln_amd import _lib, train
from robo_vln_amd.config import HCMConfig
from robo_vln_amd.validate import HCMValidator
from tests import instr_feature_cases as ic

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hcm.h")
NEW = ("hcm_encode_instruction", "hcm_op_instr_feat_ingest", "hcm_op_instr_feat_export")


def test_highlevel_takes_one_stream_per_trajectory():
    cfg = HCMConfig(instr_len=12, vla_layers=2, bert_layers=2, rnn_type="GRU", rgb_hw=128, depth_hw=128).validate()
    high = train.HighLevel(cfg)
    T, N, L = 4, 2, 5
    s = torch.randn(N, L, cfg.ins_in)
    got = high._instruction_stream({"instruction_features": s}, T * N)
    assert torch.equal(got, s.repeat(T, 1, 1)) and torch.equal(got[2 * N + 1], s[1])            # row t*N + n <- trajectory n
    # the forms it took before keep their behaviour
    assert torch.equal(high._instruction_stream({"instruction_features": s[:1]}, T * N), s[:1].expand(T * N, L, cfg.ins_in))
    full = torch.randn(T * N, L, cfg.ins_in)
    assert torch.equal(high._instruction_stream({"instruction_features": full}, T * N), full)
    for bad in (torch.randn(3, L, cfg.ins_in), torch.randn(N, L, cfg.ins_in + 1), torch.randn(N, L), torch.randn(0, L, cfg.ins_in)):
        with pytest.raises(ValueError, match="instruction_features"):
            high._instruction_stream({"instruction_features": bad}, T * N)


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = open(HEADER).read()
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m, f"{name} is not declared in include/hcm.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.EXPORTS[name][1]), name
        assert _lib.EXPORTS[name][0] is C.c_int and getattr(lib, name) is not None
    assert re.search(r"HCM_INSTR_FEATURES\s*=\s*7\b", text) and _lib.HCM_INSTR_FEATURES == 7
    m = re.search(r"typedef struct hcm_instr_features\s*\{([^}]*)\}", text)
    assert m and [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == [n for n, _ in _lib.HcmInstrFeaturesStruct._fields_]
    assert C.sizeof(_lib.HcmInstrFeaturesStruct) == 16


def test_kernel_case_expectations_are_what_they_claim():
    for name, (B, S, L, D, lens, off) in ic.CASES.items():
        x = ic.source(name)
        assert tuple(x.shape) == (S, L, D) and B % S == 0 and (lens is None or len(lens) == B)
        assert torch.isinf(x).any() and (x == 65504.0).any() and (x == -65504.0).any() and ((x != 0) & (x.abs() < 1.2e-38)).any()
        for dt in ic.DTYPES:
            y = ic.expected(x, B, dt, lens)
            assert tuple(y.shape) == (B, L, D) and torch.equal(ic.bits(y[B - 1, : (lens[B - 1] if lens else L)]),
                                                               ic.bits(x[(B - 1) % S, : (lens[B - 1] if lens else L)].to(ic.DTYPES[dt])))
            if lens:
                assert all(bool((ic.bits(y[r, k:]) == 0).all()) for r, k in enumerate(lens))
    a, b = torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -11]).half().float(), torch.tensor([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -11]).bfloat16().float()
    assert a[0] != b[0] and a[1] == 1.0 and b[1] == 1.0              # the two formats round these apart


class _StandIn:
    """what HCMValidator needs of an engine, on the CPU: val_step records which observation keys and stream rows it was handed"""
    num_recurrent_layers = 1
    device = torch.device("cpu")

    class cfg:
        hidden = 4

    def __init__(self):
        self.encoded, self.calls = [], []

    def encode_instruction(self, ids, lens=None):
        self.encoded.append(tuple(ids.shape))
        return ids.float()[:, :, None].expand(-1, -1, 3).contiguous()

    def val_step(self, obs, corrected, stop, hh, lh, masks, result=None):
        self.calls.append((sorted(obs), None if obs.get("instruction_features") is None else obs["instruction_features"].clone()))
        result.copy_(torch.arange(8.0))
        result[6] = 0
        return result, hh, lh

    @staticmethod
    def check_val_result(r):
        return torch.as_tensor(r).reshape(-1, 8)


def _batch(T, N, L, chunks, shift=0):
    rows = chunks * T * N
    ids = (torch.arange(N * L).view(N, L) + shift)
    return ({"rgb": torch.zeros(rows, 1), "instruction": ids}, None, torch.ones(rows, 1), torch.zeros(rows, 2), torch.zeros(rows, 1))


def test_validator_stream_cache_on_a_stand_in_engine():
    T, N, L = 3, 2, 4
    eng = _StandIn()
    batches = [_batch(T, N, L, 2), _batch(T, N, L, 1, shift=100)]
    v = HCMValidator(eng, T * N, N, cache_instruction=True)
    v.run(batches)
    assert eng.encoded == [(N, L)] * 3                                  # the first N rows of each chunk, once
    assert all(keys == ["instruction_features", "rgb"] for keys, _ in eng.calls)
    assert torch.equal(eng.calls[2][1][:, :, 0], batches[1][0]["instruction"].float())
    v.run(batches)
    assert len(eng.encoded) == 3 and len(eng.calls) == 6
    with pytest.raises(ValueError, match="not part of the cached run"):
        v.run(batches + [_batch(T, N, L, 1)])
    v.clear_cache()
    v.run(batches[:1])
    assert len(eng.encoded) == 5
    # off by default: nothing changes
    eng2 = _StandIn()
    HCMValidator(eng2, T * N, N).run(batches)
    assert eng2.encoded == [] and all("instruction" in keys and "instruction_features" not in keys for keys, _ in eng2.calls)
    # an instruction that changes along T
    obs, prev, m, c, s = _batch(T, N, L, 1)
    ids = obs["instruction"].repeat(T, 1)
    ids[N] += 1
    with pytest.raises(ValueError, match="changes along"):
        HCMValidator(_StandIn(), T * N, N, cache_instruction=True).run([(dict(obs, instruction=ids), prev, m, c, s)])
    HCMValidator(_StandIn(), T * N, N, cache_instruction=True, check_instruction=False).run([(dict(obs, instruction=ids), prev, m, c, s)])
