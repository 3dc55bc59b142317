"""Seq2SeqNet test helpers: the golden case table shared by tools/gen_s2s_golden.py (which runs the imported reference) and the tests, and
a torch-CPU restatement of `Seq2SeqNet.forward` (models/seq2seq.py:140-189) composed from the pieces of oracle/hcm_oracle.py, for the
batches the goldens do not cover.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import cases, hcm_oracle
from robo_vln_amd import synth
from robo_vln_amd.config import S2SConfig

SEED = cases.SEED
_S = dict(rgb_hw=128, depth_hw=128)

# name -> (S2SConfig kwargs, frames B, steps T, instructions: None = one per frame, 1 = ONE for all frames)
# every batch is ragged (synth.make_s2s_observations draws each row's length from [L/2, L]); cases.step_masks starts every episode at step 0
# and resets one environment at step 2
S2S_CASES = {
    # paper_configs/seq2seq_robo.yaml: LSTM instruction encoder, LSTM state encoder
    "s2s_128_L20": (dict(_S, instr_len=20), 2, 3, None),
    # paper_configs/seq2seq_robo_pm.yaml: PROGRESS_MONITOR.use
    "s2s_pm_128_L12": (dict(_S, instr_len=12, progress_monitor=True), 2, 2, None),
    # GRU instruction encoder and GRU state encoder
    "s2s_gru_128_L12": (dict(_S, instr_len=12, instr_rnn="GRU", rnn_type="GRU"), 3, 3, None),
    # full frame size, L = 80
    "s2s_256_L80": (dict(), 1, 2, None),
    # one instruction, three frames (seq2seq.py:163 `.expand`)
    "s2s_bcast_128_L12": (dict(_S, instr_len=12), 3, 2, 1),
    # both SimpleCNN encoders (seq2seq.py:54-57,:72-75)
    "s2s_simplecnn_L12": (dict(_S, instr_len=12, depth_encoder="SimpleDepthCNN", rgb_encoder="SimpleRGBCNN"), 2, 2, None),
    # INSTRUCTION_ENCODER.hidden_size = 128: the per-token launches
    "s2s_ih128_L12": (dict(_S, instr_len=12, instr_hidden=128), 2, 2, None),
    # seq2seq.py:156-161
    "s2s_ablate_instr_128_L12": (dict(_S, instr_len=12, ablate_instruction=True), 2, 2, None),
    "s2s_ablate_depth_128_L12": (dict(_S, instr_len=12, ablate_depth=True), 2, 2, None),
    "s2s_ablate_rgb_128_L12": (dict(_S, instr_len=12, ablate_rgb=True), 2, 2, None),
}
# training path (RNNStateEncoder.seq_forward): name -> (kwargs, T, N).  GRU state encoder: the reference's in-tree seq_forward raises for LSTM
# (oracle/cases.py, SEQ_CASES)
S2S_SEQ_CASES = {
    "s2s_seq_T4_N2_gru": (dict(_S, instr_len=12, rnn_type="GRU"), 4, 2),
}


def case_config(name):
    kw, B, T, n_instr = S2S_CASES[name]
    return S2SConfig(**kw).validate(), B, T, n_instr


def seq_case(name):
    kw, T, N = S2S_SEQ_CASES[name]
    return S2SConfig(**kw).validate(), T, N


def seq_observations(cfg, T, N):
    """T*N frames, time-major (row t*N + n); the instruction of env n repeated at every step."""
    obs = synth.make_s2s_observations(cfg, T * N, step=7, seed=SEED)
    ids = synth.make_s2s_observations(cfg, N, step=0, seed=SEED)["instruction"]
    obs["instruction"] = np.tile(ids, (T, 1))
    return obs


def seq_h0(cfg, N):
    g = torch.Generator().manual_seed(3)
    return torch.rand(cfg.num_recurrent_layers, N, cfg.hidden, generator=g) - 0.5


def instruction_final_state(ids, w, hidden, rnn_type):
    """InstructionEncoder.forward with final_state_only=True (instruction_encoder.py:70-90): the hidden state of the packed RNN at each
    row's own last token = the last non-zero column of the all-outputs restatement (zeros for an all-padding row)."""
    seq, lengths = hcm_oracle.instruction_encoder(ids, w, hidden, False, rnn_type)      # (B, H, Lmax)
    B = seq.shape[0]
    idx = (lengths - 1).clamp(min=0)
    fin = seq[torch.arange(B), :, idx]
    return fin * (lengths > 0).float().view(B, 1)


class S2SOracle:
    """Seq2SeqNet.forward (models/seq2seq.py:140-189)."""

    def __init__(self, cfg, sd):
        self.cfg = cfg
        self.w = hcm_oracle.Weights(sd)

    @torch.no_grad()
    def forward(self, obs, hidden, mask, taps=None):
        cfg, w = self.cfg, self.w
        rgb = torch.as_tensor(np.asarray(obs["rgb"])).float()
        depth = torch.as_tensor(np.asarray(obs["depth"])).float()
        ids = torch.as_tensor(np.asarray(obs["instruction"])).long()
        hidden = torch.as_tensor(hidden).float()
        B = rgb.shape[0]
        mask = torch.as_tensor(mask).float().reshape(B, -1)[:, 0]                                          # :172
        ins = instruction_final_state(ids, w.sub("instruction_encoder."), cfg.instr_hidden, cfg.instr_rnn)  # :153
        if cfg.depth_encoder == "VlnResnetDepthEncoder":
            d = hcm_oracle.depth_resnet_flat(depth, w.sub("depth_encoder."), cfg.depth_baseplanes // 2)     # :154
        else:
            d = hcm_oracle.simple_depth_cnn(depth, w.sub("depth_encoder."))
        if cfg.rgb_encoder == "TorchVisionResNet50":
            r = hcm_oracle.rgb_resnet_flat(rgb, w.sub("rgb_encoder."))                                      # :155
        else:
            r = hcm_oracle.simple_rgb_cnn(rgb, w.sub("rgb_encoder."))
        ins_enc = ins
        if cfg.ablate_instruction:
            ins = ins * 0                                                                                   # :156-157
        if cfg.ablate_depth:
            d = d * 0                                                                                       # :158-159
        if cfg.ablate_rgb:
            r = r * 0                                                                                       # :160-161
        ins = ins.expand(B, ins.shape[1])                                                                   # :163
        x = torch.cat([ins, d, r], dim=1)                                                                   # :164
        h, hid = hcm_oracle.rnn_forward(x, hidden, mask, w.sub("state_encoder."), cfg.rnn_type)             # :174
        prog = torch.tanh(F.linear(h, w("progress_monitor.weight"), w("progress_monitor.bias"))) if cfg.progress_monitor else None   # :177
        out = F.linear(h, w("linear.weight"), w("linear.bias"))                                             # :187
        stop = F.linear(h, w("stop_linear.weight"), w("stop_linear.bias"))                                  # :188
        if taps is not None:
            taps.update(instruction=ins_enc, depth_flat=d, rgb_flat=r, rnn_in=x, rnn_out=h)
        return out, stop, prog, hid
