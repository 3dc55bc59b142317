"""Precomputed trunk features without a GPU: the C ABI's declarations and bindings, the validators' feature cache against stub engines, and the
golden captured from the imported reference models on observations that hold only the feature keys (tests/golden/features_128_L12.npz,
tools/gen_features_golden.py) against the CPU oracle fed the same features through tests/features_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import hcm_oracle
from robo_vln_amd import _lib, synth
from robo_vln_amd.config import HCMConfig
from robo_vln_amd.policy import HCMEngine
from robo_vln_amd.validate import FlatValidator, HCMValidator
from tests import features_cases as fc
from tests import features_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5      # fp32 CPU restatement vs fp32 CPU reference (different op order only), as tests/test_val_cpu.py


# ---------------------------------------------------------------- declaration, export, binding
def test_header_declares_and_library_exports_the_features_abi():
    text = open(os.path.join(ROOT, "include", "hcm.h")).read()
    for name in ("hcm_encode_features", "hcm_encode_features_ex"):
        m = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.EXPORTS[name][1])
        assert hasattr(_lib.lib(), name)
    assert re.search(r"HCM_FEATURES = %d\b" % _lib.HCM_FEATURES, text)
    for sel in ("HCM_FEAT_RGB_HI", "HCM_FEAT_RGB_LO", "HCM_FEAT_DEPTH_HI", "HCM_FEAT_DEPTH_LO", "HCM_FEAT_SHARED"):
        assert re.search(r"%s = %d\b" % (sel, getattr(_lib, sel)), text), sel
    # the struct: two pointers around an int32, then 2 + 2 pointers
    assert C.sizeof(_lib.HcmFeaturesStruct) == 7 * C.sizeof(C.c_void_p)
    for line in ("resnet_encoders.py:83-86", ":207-214", "(rows, 2048, 4, 4)", "(rows, 2048, 1, 1)"):
        assert line in text, line


def test_feature_queries_and_argument_errors_need_no_device():
    from robo_vln_amd.policy import _to_struct
    l = _lib.lib()
    st = _to_struct(HCMConfig(rgb_hw=128, depth_hw=192, instr_len=12, bert_layers=2).validate(), 4, "fp32", True, True)
    h = C.c_void_p()
    assert l.hcm_create(C.byref(st), C.byref(h)) == 0
    try:
        out = C.c_int64()
        want = {_lib.HCM_FEAT_RGB_HI: 2048 * 16, _lib.HCM_FEAT_RGB_LO: 2048, _lib.HCM_FEAT_DEPTH_HI: 228 * 9, _lib.HCM_FEAT_DEPTH_LO: 228 * 9}
        for sel, n in want.items():
            assert l.hcm_query(h, sel, C.byref(out)) == 0 and out.value == n, (sel, out.value)
        f = _lib.HcmFeaturesStruct()
        assert l.hcm_encode_features(h, None, _lib.HCM_F32, None, 1, C.byref(f), None) == -2          # not finalized
        assert l.hcm_encode_features(None, None, _lib.HCM_F32, None, 1, C.byref(f), None) == -1
    finally:
        l.hcm_destroy(h)


# ---------------------------------------------------------------- the validators' feature cache
class _Stub:
    """A val_step whose result is a function of the trunk OUTPUTS only: rgb * 2 and depth + 1 stand for the trunks."""
    device = "cpu"
    num_recurrent_layers = 1
    cfg = HCMConfig(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2, rnn_type="GRU").validate()
    check_val_result = staticmethod(HCMEngine.check_val_result)

    def __init__(self, flat):
        self.flat, self.encoded, self.seen = flat, [], []

    def encode_features(self, observations):
        self.encoded.append(int(observations["rgb"].shape[0]))
        r, d = observations["rgb"] * 2, observations["depth"] + 1
        return {"rgb_features": r if self.flat else (r, r[:, :1]), "depth_features": d if self.flat else (d, None)}

    def _value(self, observations):
        self.seen.append(sorted(observations))
        if "rgb_features" in observations:
            r, d = observations["rgb_features"], observations["depth_features"]
            r, d = (r, d) if self.flat else (r[0], d[0])
        else:
            r, d = observations["rgb"] * 2, observations["depth"] + 1
        return float(r.sum() + 3 * d.sum())

    def val_step(self, observations, corrected_actions, oracle_stop, *rest, result=None, return_outputs=False):
        result.copy_(torch.tensor([self._value(observations), 0.5, 0.25, 1, 2, 2, 0, 0]))
        return (result,) + tuple(rest[:1 if self.flat else 2])


def _batch(rows, seed):
    g = torch.Generator().manual_seed(seed)
    obs = {"rgb": torch.rand(rows, 3, generator=g), "depth": torch.rand(rows, 2, generator=g), "instruction": torch.zeros(1, 5),
           "vln_oracle_action_sensor": torch.ones(rows, 1)}
    return obs, torch.zeros(rows, 2), torch.ones(rows, 2), torch.zeros(rows, 2), torch.zeros(rows, 1)


@pytest.mark.parametrize("flat", [False, True])
def test_validator_feature_cache(flat):
    V = FlatValidator if flat else HCMValidator
    batches = [_batch(8, 1), _batch(6, 2)]                       # chunks of 4, 4 and 4, 2 rows
    plain_eng = _Stub(flat)
    plain = V(plain_eng, tbptt_steps=4, batch_size=2).run(batches)
    assert plain_eng.encoded == [] and all("rgb" in k and "rgb_features" not in k for k in plain_eng.seen)      # the default never encodes

    eng = _Stub(flat)
    val = V(eng, tbptt_steps=4, batch_size=2, cache_features=True)
    first = val.run(batches)
    assert eng.encoded == [4, 4, 4, 2]                           # once per chunk
    eng.seen.clear()
    second = val.run(batches)
    assert eng.encoded == [4, 4, 4, 2]                           # not again
    assert len(eng.seen) == 4 and all("rgb_features" in k and "depth_features" in k and "rgb" not in k and "depth" not in k for k in eng.seen)
    assert torch.equal(first["table"], plain["table"]) and torch.equal(second["table"], plain["table"])
    # other batches: refused until the cache is cleared
    with pytest.raises(ValueError, match="rows"):
        val.run([_batch(8, 1), _batch(8, 2)])
    with pytest.raises(ValueError, match="clear_cache"):
        val.run(batches + [_batch(4, 3)])
    with pytest.raises(ValueError, match="clear_cache"):
        val.run(batches[:1])
    val.clear_cache()
    third = val.run([_batch(8, 1), _batch(8, 2)])
    assert eng.encoded == [4, 4, 4, 2, 4, 4, 4, 4] and third["chunks"] == 4
    with pytest.raises(ValueError, match="cache_device"):
        V(eng, 4, 2, cache_features=True, cache_device="disk")
    host = V(_Stub(flat), 4, 2, cache_features=True, cache_device="cpu")
    assert torch.equal(host.run(batches)["table"], plain["table"]) and torch.equal(host.run(batches)["table"], plain["table"])


# ---------------------------------------------------------------- the golden from the imported reference
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "features_128_L12.npz")))


def _check(what, got, ref):
    e = float(np.abs(np.asarray(got) - ref).max())
    print(f"{what}: oracle through features_ref vs the reference on feature keys, max-abs {e:.2e} (<= {TOL:.0e})")
    assert e <= TOL


def test_golden_features_are_the_seeded_draws(gold):
    for k, v in fc.draw_features(fc.hcm_cfg()).items():
        assert np.array_equal(gold[k], v), k


def test_oracle_through_features_ref_matches_the_reference_on_feature_keys(gold):
    cfg, ccfg = fc.hcm_cfg(), fc.cma_cfg()
    hi_sd, lo_sd = synth.make_weights(cfg, fc.SEED)
    frames1 = {"rgb": np.zeros((1, 128, 128, 3), np.float32), "depth": np.zeros((1, 128, 128, 1), np.float32)}
    frames2 = {"rgb": np.zeros((2, 128, 128, 3), np.float32), "depth": np.zeros((2, 128, 128, 1), np.float32)}
    ids, h0, m = fc.hi_inputs(cfg)
    with features_ref.given(gold["rgb_spatial"], gold["depth"][:1]):
        logits, hid = hcm_oracle.HighLevelOracle(cfg, hi_sd).forward(dict(frames1, instruction=ids), h0.clone(), m)
    _check("high-level logits", logits, gold["hi_logits"])
    _check("high-level hidden", hid, gold["hi_hidden"])
    h0, m, sub = fc.lo_inputs(cfg)
    with features_ref.given(gold["rgb_flat"], gold["depth"]):
        vel, stop, hid = hcm_oracle.LowLevelOracle(cfg, lo_sd).forward(frames2, h0.clone(), m, sub)
    _check("low-level vel", vel, gold["lo_vel"])
    _check("low-level stop", stop, gold["lo_stop"])
    _check("low-level hidden", hid, gold["lo_hidden"])
    ids, h0, m = fc.cma_inputs(ccfg)
    with features_ref.given(gold["rgb_spatial"], gold["depth"][:1]):
        out, stop, hid = hcm_oracle.CMAOracle(ccfg, synth.make_cma_weights(ccfg, fc.SEED)).forward(dict(frames1, instruction=ids), h0.clone(), m)
    _check("CMANet out", out, gold["cma_out"])
    _check("CMANet stop", stop, gold["cma_stop"])
    _check("CMANet hidden", hid, gold["cma_hidden"])
    # outside the context the oracle's trunks are its own again
    assert hcm_oracle.tv_resnet50_trunk.__name__ == "tv_resnet50_trunk" and hcm_oracle.habitat_resnet_encoder.__name__ == "habitat_resnet_encoder"
