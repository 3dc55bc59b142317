"""Host-side mirror of the reference's `CMANet` flat baseline (robo_vln_baselines/models/cma.py:19-333): the same
tuple-in / tuple-out `forward(batch)` contract and properties, all arithmetic in libhcm.so (HIP, gfx950).

    net = CMANet(CMAEngine(cfg, state_dict, max_batch=...))
    output, stop_out, rnn_hidden_states = net((observations, rnn_hidden_states, prev_actions, masks))    # robo_vln_trainer.py:1096
"""
import ctypes as C

import torch

from . import _lib
from ._engine import _TORCH_DT, _FlatEngine, _ptr, _val_labels       # noqa: F401  (_val_labels: importable from here as before)
from .config import CMAConfig


def _to_struct(cfg: CMAConfig, max_batch, precision):
    s = _lib.HcmCmaConfigStruct()
    s.struct_size = C.sizeof(_lib.HcmCmaConfigStruct)
    s.precision = _lib.PRECISIONS[precision]
    s.max_batch = max_batch
    s.rgb_h, s.rgb_w = cfg.rgb_shape
    s.depth_h = s.depth_w = cfg.depth_hw
    s.instr_len = cfg.instr_len
    s.vocab_size, s.embedding_size, s.instr_hidden = cfg.vocab_size, cfg.embedding_size, cfg.instr_hidden
    s.bidirectional = int(cfg.bidirectional)
    s.rgb_out, s.depth_out, s.depth_baseplanes = cfg.rgb_out, cfg.depth_out, cfg.depth_baseplanes
    s.hidden = cfg.hidden
    s.rnn_type = _lib.HCM_LSTM if cfg.rnn_type == "LSTM" else _lib.HCM_GRU
    s.num_actions = cfg.num_actions
    s.use_prev_action, s.rcm_state_encoder = int(cfg.use_prev_action), int(cfg.rcm_state_encoder)
    s.progress_monitor = int(cfg.progress_monitor)
    s.instr_rnn = _lib.HCM_LSTM if cfg.instr_rnn == "LSTM" else _lib.HCM_GRU
    s.ablate_instruction, s.ablate_depth, s.ablate_rgb = int(cfg.ablate_instruction), int(cfg.ablate_depth), int(cfg.ablate_rgb)
    return s


class CMAEngine(_FlatEngine):
    """Owns one libhcm CMANet handle (weights + workspace) on one GPU."""

    def __init__(self, cfg: CMAConfig, state_dict, max_batch=64, precision="fp16", device=None, graph=False):
        """graph=True: forward() runs on an engine-owned stream with engine-owned static I/O buffers so that libhcm replays one
        captured hipGraph per step; the returned tensors then alias those buffers and stay valid until the second-next call."""
        cfg.validate()
        self._open(cfg, max_batch, device, graph, "hcm_cma_create", _to_struct(cfg, max_batch, precision),
                   ((_lib.HCM_CMA, k, v) for k, v in state_dict.items()))

    def _inputs(self, observations, rows, lead="B"):
        """-> (rgb, depth, ids expanded to one row per frame (cma.py:226), B); `lead` names the leading dimension in the messages"""
        c = self.cfg
        rgb, depth, B = self._frames(observations, (0,), lambda r, d: self._frame_check(r, d, lead))      # (or rgb_features / depth_features)
        if rows is not None and B != rows:
            raise ValueError(f"expected {rows} frames (T*N), got {B}")
        self._no_instr_stream(observations)
        ids = self._dev(observations["instruction"], (torch.int64, torch.int32, torch.float32))
        # cfg.instr_len is the longest padded instruction the workspace is sized for; every call brings its own L
        if ids.dim() != 2 or ids.shape[0] not in (1, B) or not 1 <= ids.shape[1] <= c.instr_len:
            raise ValueError(f"instruction must be ({lead} or 1, L <= {c.instr_len}), got {tuple(ids.shape)}")
        return rgb, depth, ids.expand(B, ids.shape[1]).contiguous(), B

    def _frame_check(self, rgb, depth, lead="B"):
        c = self.cfg
        rgb = self._dev(rgb, (torch.float32, torch.uint8))
        depth = self._dev(depth, (torch.float32,))
        if rgb.dim() != 4 or tuple(rgb.shape[1:]) != (*c.rgb_shape, 3):
            raise ValueError(f"rgb must be ({lead},{c.rgb_shape[0]},{c.rgb_shape[1]},3), got {tuple(rgb.shape)}")
        if tuple(depth.shape) != (rgb.shape[0], c.depth_hw, c.depth_hw, 1):
            raise ValueError(f"depth must be ({lead},{c.depth_hw},{c.depth_hw},1), got {tuple(depth.shape)}")
        return rgb, depth

    def _enc_frames(self, observations):
        return self._frame_check(observations["rgb"], observations["depth"])

    def _outputs(self, B):
        c = self.cfg
        return (torch.empty(B, c.num_actions, device=self.device, dtype=torch.float32),
                torch.empty(B, 1, device=self.device, dtype=torch.float32))

    def forward(self, observations, hidden, masks):
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, None)
            h_in, m = self._state_mask(hidden, masks, B, B)

            def call(rgb_, depth_, ids_, h_in_, m_, out, stop, _, h_out, st):
                _lib.check(self._lib.hcm_cma_forward(self._h, rgb_.data_ptr(), _TORCH_DT[rgb.dtype], depth_.data_ptr(), ids_.data_ptr(),
                                                     _TORCH_DT[ids.dtype], B, ids.shape[1], h_in_.data_ptr(), m_.data_ptr(), out.data_ptr(),
                                                     stop.data_ptr(), h_out.data_ptr(), st), self._h)
            if self._graph:
                out, stop, _, h_out = self._forward_graph(call, rgb, depth, ids, h_in, m, B)
                return out, stop, h_out
            out, stop = self._outputs(B)
            h_out = torch.empty_like(h_in)
            call(rgb, depth, ids, h_in, m, out, stop, None, h_out, self._stream())
        return out, stop, h_out

    def forward_seq(self, observations, hidden, masks, T, N):
        """Training / validation path (RNNStateEncoder.seq_forward for both state encoders): observations hold T*N rows, time-major (the
        instruction repeated at every step, as the trainer's collate does; a (1, L) instruction is expanded); hidden (R,N,hidden); masks (T*N,).
        -> (output (T*N,num_actions), stop_out (T*N,1), rnn_hidden_states (R,N,hidden))"""
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, T * N, "T*N")
            h_in, m = self._state_mask(hidden, masks, B, N)
            out, stop = self._outputs(B)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_cma_forward_seq(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(),
                                                     _TORCH_DT[ids.dtype], T, N, ids.shape[1], h_in.data_ptr(), m.data_ptr(), out.data_ptr(),
                                                     stop.data_ptr(), h_out.data_ptr(), self._stream()), self._h)
        return out, stop, h_out

    def val_step(self, observations, corrected_actions, oracle_stop, hidden, masks, result=None, return_outputs=False):
        """The flat trainer's validation step, `_update_agent_val` (robo_vln_trainer.py:544-575), in one library call (hcm_flat_val_step): the
        model on the chunk's T*N time-major rows of `observations` (N = hidden.shape[1]) and the criteria.  Returns (result, hidden'), plus
        (out, stop, None) BEFORE any masking with return_outputs=True -- the third place is Seq2SeqNet's progress_hat; CMANet has no progress
        monitor.  result is the (8,) f32 device tensor of include/hcm.h: [action loss, stop loss, aux loss (0 here), stop rows, aux rows (0), 0, 0,
        0]; it is written into `result` when given, so that a caller can keep a table of them and read once.  Does not synchronise."""
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, None, "T*N")
            h_in, N, ca, os_, m, result = _val_labels(self, B, hidden, corrected_actions, oracle_stop, masks, result)
            h_out = torch.empty_like(h_in)
            out, stop = self._outputs(B) if return_outputs else (None, None)
            _lib.check(self._lib.hcm_flat_val_step(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(), _TORCH_DT[ids.dtype],
                                                   B // N, N, B, ids.shape[1], ca.data_ptr(), os_.data_ptr(), None, h_in.data_ptr(), m.data_ptr(),
                                                   result.data_ptr(), h_out.data_ptr(), _ptr(out), _ptr(stop), None, self._stream()), self._h)
        if return_outputs:
            return result, h_out, (out, stop, None)
        return result, h_out


class CMANet:
    """`CMANet.forward(batch)` (models/cma.py:211-333): batch = (observations, rnn_hidden_states, prev_actions, masks) ->
    (output (B,2), stop_out (B,1), rnn_hidden_states).  Like the reference it deletes observations['instruction'] (:228);
    prev_actions is ignored (CMA.use_prev_action = False)."""

    def __init__(self, engine: CMAEngine):
        self.engine = engine

    @property
    def output_size(self):
        return self.engine.cfg.hidden

    @property
    def is_blind(self):
        return False

    @property
    def num_recurrent_layers(self):
        return self.engine.num_recurrent_layers

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def forward(self, batch):
        observations, rnn_hidden_states, prev_actions, masks = batch
        out, stop, hidden = self.engine.forward(observations, rnn_hidden_states, masks)
        if isinstance(observations, dict) and "instruction" in observations:
            del observations["instruction"]
        return out, stop, hidden

    def seq_forward(self, batch, T, N):
        """The training / validation call (robo_vln_trainer.py:516-518, :553-555): T*N frames at once with an (R,N,hidden) state."""
        observations, rnn_hidden_states, prev_actions, masks = batch
        out, stop, hidden = self.engine.forward_seq(observations, rnn_hidden_states, masks, T, N)
        if isinstance(observations, dict) and "instruction" in observations:
            del observations["instruction"]
        return out, stop, hidden

    __call__ = forward
