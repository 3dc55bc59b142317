"""CMANet sequence-forward test helpers: the case table shared by tools/gen_cma_seq_golden.py (which runs the imported reference) and the
tests, and the seeded inputs (observations, masks, h0) every side rebuilds.  Test infrastructure only."""
import numpy as np
import torch

from oracle import cases
from robo_vln_amd import synth
from robo_vln_amd.config import CMAConfig

SEED = cases.SEED
_S = dict(rgb_hw=128, depth_hw=128)

# Training / validation path (RNNStateEncoder.seq_forward for both state encoders): name -> (CMAConfig kwargs, T, N).
# GRU state encoders: the reference's in-tree seq_forward raises for LSTM (`hidden_states.detach()` on a tuple, state_encoder.py:131), so only
# these have a golden from the reference.
CMA_SEQ_CASES = {
    # bidirectional LSTM instruction encoder (paper_configs/cma_robo.yaml)
    "cma_seq_T4_N2_L12": (dict(_S, instr_len=12, rnn_type="GRU"), 4, 2),
    # unidirectional GRU instruction encoder
    "cma_seq_gru_instr_T3_N3_L9": (dict(_S, instr_len=9, instr_rnn="GRU", bidirectional=False, rnn_type="GRU"), 3, 3),
    # cma.py:236-237
    "cma_seq_ablate_instr_T2_N2": (dict(_S, instr_len=12, ablate_instruction=True, rnn_type="GRU"), 2, 2),
}
# LSTM state encoders: pinned by oracle.hcm_oracle.CMAOracle (its LSTM cell by the single-step goldens, its sequence branch by the cases above)
CMA_SEQ_CASES_ORACLE_ONLY = {
    "cma_seq_T4_N3_lstm": (dict(_S, instr_len=12), 4, 3),
}


def seq_case(name):
    kw, T, N = {**CMA_SEQ_CASES, **CMA_SEQ_CASES_ORACLE_ONLY}[name]
    return CMAConfig(**kw).validate(), T, N


def seq_observations(cfg, T, N):
    """T*N frames, time-major (row t*N + n); the padded instruction of env n (lengths differ between envs) repeated at every step, as the
    trainer's collate does."""
    obs = synth.make_cma_observations(cfg, T * N, step=7, seed=SEED)
    ids = synth.make_cma_observations(cfg, N, step=0, seed=SEED)["instruction"]
    obs["instruction"] = np.tile(ids, (T, 1))
    return obs


def seq_masks(T, N):
    """(T*N,) time-major.  At t = 0 every env starts an episode except the last one, whose chunk continues an episode (mask 1 on a non-zero
    h0); env 1 % N is reset at t = 1 and, when the chunk is long enough, env 0 at t = 2 (segment boundaries for seq_forward)."""
    m = np.ones((T, N), dtype=np.float32)
    m[0, :] = 0
    m[0, N - 1] = 1
    if T > 1:
        m[1, 1 % N] = 0
    if T > 2:
        m[2, 0] = 0
    return m.reshape(-1)


def seq_h0(cfg, N):
    g = torch.Generator().manual_seed(3)
    return torch.rand(cfg.num_recurrent_layers, N, cfg.hidden, generator=g) - 0.5
