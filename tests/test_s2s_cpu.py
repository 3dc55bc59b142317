"""Seq2SeqNet flat baseline without a GPU: the torch-CPU restatement (tests/s2s_ref.py) against the goldens captured from the imported
reference (tests/golden/s2s_*.npz, tools/gen_s2s_golden.py), and the library's boundary -- the refused settings, the argument checks and the
strict state_dict loader (none of which touches the device)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import cases
from robo_vln_amd import _lib, synth
from robo_vln_amd.config import S2SConfig
from robo_vln_amd.seq2seq import _to_struct
from tests import s2s_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5      # fp32 CPU restatement vs fp32 CPU reference (different op order only)


@pytest.mark.parametrize("name", list(s2s_ref.S2S_CASES))
def test_restatement_matches_reference_golden(name):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, B, T, n_instr = s2s_ref.case_config(name)
    orc = s2s_ref.S2SOracle(cfg, synth.make_s2s_weights(cfg, s2s_ref.SEED))
    hid = torch.zeros(cfg.num_recurrent_layers, B, cfg.hidden)
    for t in range(T):
        obs = synth.make_s2s_observations(cfg, B, step=t, seed=s2s_ref.SEED, n_instr=n_instr)
        lens = (obs["instruction"] != 0).sum(1)
        assert B == 1 or n_instr == 1 or len(set(lens.tolist())) > 1          # ragged batch
        taps = {}
        out, stop, prog, hid = orc.forward(obs, hid, cases.step_masks(B, t), taps)
        np.testing.assert_allclose(out.numpy(), gold["out"][t], atol=TOL, rtol=0)
        np.testing.assert_allclose(stop.numpy(), gold["stop"][t], atol=TOL, rtol=0)
        if cfg.progress_monitor:
            np.testing.assert_allclose(prog.numpy(), gold["progress"][t], atol=TOL, rtol=0)
        else:
            assert prog is None and "progress" not in gold
        if t == 0:
            np.testing.assert_allclose(taps["instruction"].numpy(), gold["tap.instruction"], atol=TOL, rtol=0)
            np.testing.assert_allclose(taps["rnn_in"].numpy(), gold["tap.rnn_in"], atol=TOL, rtol=0)
    np.testing.assert_allclose(hid.numpy(), gold["hidden"], atol=TOL, rtol=0)


@pytest.mark.parametrize("name", list(s2s_ref.S2S_SEQ_CASES))
def test_restatement_matches_reference_seq_golden(name):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, T, N = s2s_ref.seq_case(name)
    orc = s2s_ref.S2SOracle(cfg, synth.make_s2s_weights(cfg, s2s_ref.SEED))
    m = cases.seq_masks(T, N)
    assert (m.reshape(T, N)[1:] == 0).any()                                   # an episode reset inside T
    out, stop, _, hid = orc.forward(s2s_ref.seq_observations(cfg, T, N), torch.from_numpy(gold["h0"]), m)
    np.testing.assert_allclose(out.numpy(), gold["out"], atol=TOL, rtol=0)
    np.testing.assert_allclose(stop.numpy(), gold["stop"], atol=TOL, rtol=0)
    np.testing.assert_allclose(hid.numpy(), gold["hidden"], atol=TOL, rtol=0)


def _create(cfg=None, **over):
    l = _lib.lib()
    st = _to_struct(cfg or S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12), 4, "fp32")
    for k, v in over.items():
        setattr(st, k, v)
    h = C.c_void_p()
    rc = l.hcm_s2s_create(C.byref(st), C.byref(h))
    return l, rc, h


@pytest.mark.parametrize("field,py_kw,ref_line", [
    ("bidirectional", dict(bidirectional=True), "seq2seq.py:163"),
    ("use_prev_action", dict(use_prev_action=True), "default.py:202"),
    ("is_bert", dict(is_bert=True), "seq2seq.py:45"),
])
def test_refused_settings_cite_the_reference(field, py_kw, ref_line):
    with pytest.raises(ValueError, match=ref_line.replace(".", r"\.")):
        S2SConfig(**py_kw).validate()
    l, rc, h = _create(**{field: 1})
    assert rc == -6 and not h.value
    assert ref_line.encode() in l.hcm_last_error(None), l.hcm_last_error(None)


def test_create_checks_struct_size_and_sizes():
    l, rc, h = _create(struct_size=8)
    assert rc == -1 and b"struct_size" in l.hcm_last_error(None)
    l, rc, h = _create(instr_hidden=100)
    assert rc == -6
    with pytest.raises(ValueError):
        S2SConfig(instr_hidden=100).validate()
    with pytest.raises(ValueError):
        S2SConfig(final_state_only=False).validate()
    for kw in (dict(progress_monitor=True), dict(instr_rnn="GRU", rnn_type="GRU"), dict(depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN"),
               dict(instr_hidden=128), dict(ablate_instruction=True), dict(ablate_depth=True), dict(ablate_rgb=True)):
        l, rc, h = _create(S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, **kw).validate())
        assert rc == 0, l.hcm_last_error(None)
        out = C.c_int64()
        assert l.hcm_query(h, _lib.HCM_NUM_RECURRENT_LAYERS, C.byref(out)) == 0
        assert out.value == (1 if kw.get("rnn_type") == "GRU" else 2)
        l.hcm_destroy(h)


def test_forward_argument_errors():
    """`progress` with the flag clear and B_instr outside {1, B} are the caller's mistakes: HCM_ERR_ARG, whatever else is wrong."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    l, rc, h = _create()
    assert rc == 0
    try:
        args = lambda B, Bi, prog: (h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, B, Bi, 12, p, p, p, p, prog, p, None)
        assert l.hcm_s2s_forward(*args(2, 2, p)) == -1 and b"progress" in l.hcm_last_error(h)
        assert l.hcm_s2s_forward(*args(3, 2, None)) == -1 and b"B_instr" in l.hcm_last_error(h)
        assert l.hcm_s2s_forward(*args(3, 0, None)) == -1
        assert l.hcm_s2s_forward_seq(h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, 2, 2, 3, 12, p, p, p, p, None, p, None) == -1
        assert l.hcm_s2s_forward(*args(2, 2, None)) == -2          # well-formed, but the handle is not finalized
        assert l.hcm_s2s_forward(*args(2, 1, None)) == -2
        # a handle of another kind
        assert l.hcm_load_tensor(h, _lib.HCM_LOW, b"linear.bias", p, _lib.HCM_F32, (C.c_int64 * 1)(2), 1) == -1
    finally:
        l.hcm_destroy(h)
    l, rc, h = _create(S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, progress_monitor=True))
    assert rc == 0
    try:
        assert l.hcm_s2s_forward(h, p, _lib.HCM_F32, p, p, _lib.HCM_I64, 2, 2, 12, p, p, p, p, p, p, None) == -2     # progress accepted
    finally:
        l.hcm_destroy(h)


def _load(l, h, key, shape, kind):
    a = np.zeros(shape, np.int64 if kind == "nbt" else np.float32)
    shp = (C.c_int64 * max(1, len(shape)))(*shape)
    return l.hcm_load_tensor(h, _lib.HCM_S2S, key.encode(), a.ctypes.data_as(C.c_void_p), _lib.HCM_I64 if kind == "nbt" else _lib.HCM_F32, shp, len(shape))


@pytest.mark.parametrize("kw", [dict(), dict(instr_rnn="GRU", rnn_type="GRU"), dict(depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN"),
                                dict(instr_hidden=128, progress_monitor=True), dict(depth_encoder="SimpleDepthCNN", rnn_type="GRU")])
def test_every_synth_key_is_accepted_by_the_library(kw):
    """The C++ spec (weights.cpp build_spec_s2s) and the Python spec (synth.seq2seq_spec, validated against the imported reference by
    tools/gen_s2s_golden.py with strict=True) agree key for key and shape for shape; a missing and an unknown key are refused."""
    cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, **kw).validate()
    l, rc, h = _create(cfg)
    assert rc == 0, l.hcm_last_error(None)
    try:
        spec = synth.seq2seq_spec(cfg)
        keys = [k for k, *_ in spec]
        assert "sub_goal_linear.weight" in keys and "progress_monitor.bias" in keys and "sub_task_embedding.weight" not in keys
        assert _load(l, h, "sub_task_embedding.weight", (5, 32), "emb") == -3 and b"Unexpected key" in l.hcm_last_error(h)
        assert _load(l, h, "linear.weight", (3, cfg.hidden), "w") == -4
        for key, shape, kind, aux in spec[:-1]:
            assert _load(l, h, key, shape, kind) == 0, (key, l.hcm_last_error(h))
        assert l.hcm_finalize(h) == -3 and spec[-1][0].encode() in l.hcm_last_error(h)          # strict: the last key is missing
        key, shape, kind, aux = spec[-1]
        assert _load(l, h, key, shape, kind) == 0
    finally:
        l.hcm_destroy(h)


def test_flat_checkpoint_reader_round_trip(tmp_path):
    from robo_vln_amd import checkpoint
    cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN").validate()
    sd = synth.make_s2s_weights(cfg, 1)
    path = str(tmp_path / "ckpt.0.pth")
    torch.save({"state_dict": {k: torch.as_tensor(v) for k, v in sd.items()}, "config": None}, path)      # robo_vln_trainer.py:367-372
    got, _ = checkpoint.load_flat_checkpoint(path)
    assert list(got) == list(sd)
    assert all(np.array_equal(got[k].numpy(), sd[k]) for k in sd)
    with pytest.raises(KeyError):
        torch.save({"high_level_state_dict": {}}, path)
        checkpoint.load_flat_checkpoint(path)
