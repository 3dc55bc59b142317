"""The case behind tests/golden/features_128_L12.npz (tools/gen_features_golden.py): configurations, the drawn features and the other inputs,
all rebuilt from the seed."""
import numpy as np
import torch

from robo_vln_amd.config import CMAConfig, HCMConfig

SEED = 0


def hcm_cfg():
    return HCMConfig(rgb_hw=128, depth_hw=128, instr_len=12, vla_layers=2, bert_layers=2).validate()


def cma_cfg():
    return CMAConfig(rgb_hw=128, depth_hw=128, instr_len=12).validate()


def draw_features(cfg):
    """rgb_spatial (1,2048,4,4) for the spatial encoders, rgb_flat (2,2048,1,1) for the flat one, depth (2,C,s,s): half-normal draws that fp16
    holds exactly"""
    rng = np.random.RandomState(7)
    s, c = cfg.depth_final_spatial(), cfg.depth_compress_channels()

    def draw(*shape):
        return np.abs(rng.standard_normal(shape)).astype(np.float16).astype(np.float32)
    return {"rgb_spatial": draw(1, 2048, 4, 4), "rgb_flat": draw(2, 2048, 1, 1), "depth": draw(2, c, s, s)}


def _ids(rows, L, vocab, first):
    rng = np.random.RandomState(11)
    ids = rng.randint(1000 if first else 1, vocab, size=(rows, L)).astype(np.int64)
    if first:
        ids[:, 0], ids[:, -1] = 101, 102
    else:
        ids[:, L - 3:] = 0                                       # a padded tail
    return ids


def _h0(R, rows, hidden):
    return torch.rand(R, rows, hidden, generator=torch.Generator().manual_seed(3)) - 0.5


def hi_inputs(cfg):
    return _ids(1, cfg.instr_len, cfg.bert_vocab, True), _h0(cfg.num_recurrent_layers, 1, cfg.hidden), np.ones(1, np.float32)


def cma_inputs(cfg):
    return _ids(1, cfg.instr_len, cfg.vocab_size, False), _h0(cfg.num_recurrent_layers, 1, cfg.hidden), np.ones(1, np.float32)


def lo_inputs(cfg):
    return _h0(cfg.num_recurrent_layers, 2, cfg.hidden), np.array([1.0, 0.0], np.float32), np.array([1, 3], np.int64)
