"""Host-side mirror of the reference's `Seq2SeqNet` flat baseline (robo_vln_baselines/models/seq2seq.py:21-189; the model of
paper_configs/seq2seq_robo.yaml and seq2seq_robo_pm.yaml): the same tuple-in / tuple-out `forward(batch)` contract and properties, all
arithmetic in libhcm.so (HIP, gfx950).

    net = Seq2SeqNet(S2SEngine(cfg, state_dict, max_batch=...))
    output, stop_out, rnn_hidden_states = net((observations, rnn_hidden_states, prev_actions, masks))    # robo_vln_trainer.py:1096

The reference's GRU instruction encoder raises IndexError at batch 1 (`final_state[0].squeeze(0)` squeezes the batch axis, then
seq2seq.py:163 indexes shape[1]); the library serves batch 1 with the value a larger batch gives for that row.
"""
import ctypes as C

import torch

from . import _lib
from ._engine import _TORCH_DT, _FlatEngine, _ptr, _val_labels
from .config import S2SConfig


def _to_struct(cfg: S2SConfig, max_batch, precision):
    s = _lib.HcmS2sConfigStruct()
    s.struct_size = C.sizeof(_lib.HcmS2sConfigStruct)
    s.precision = _lib.PRECISIONS[precision]
    s.max_batch = max_batch
    s.rgb_h, s.rgb_w = cfg.rgb_shape
    s.depth_h, s.depth_w = cfg.depth_shape
    s.instr_len = cfg.instr_len
    s.vocab_size, s.embedding_size, s.instr_hidden = cfg.vocab_size, cfg.embedding_size, cfg.instr_hidden
    s.instr_rnn = _lib.HCM_LSTM if cfg.instr_rnn == "LSTM" else _lib.HCM_GRU
    s.bidirectional = int(cfg.bidirectional)
    s.rgb_encoder = _lib.HCM_ENC_RESNET if cfg.rgb_encoder == "TorchVisionResNet50" else _lib.HCM_ENC_SIMPLECNN
    s.depth_encoder = _lib.HCM_ENC_RESNET if cfg.depth_encoder == "VlnResnetDepthEncoder" else _lib.HCM_ENC_SIMPLECNN
    s.rgb_out, s.depth_out, s.depth_baseplanes = cfg.rgb_out, cfg.depth_out, cfg.depth_baseplanes
    s.hidden = cfg.hidden
    s.rnn_type = _lib.HCM_LSTM if cfg.rnn_type == "LSTM" else _lib.HCM_GRU
    s.num_actions, s.num_sub_tasks = cfg.num_actions, cfg.num_sub_tasks
    s.use_prev_action, s.is_bert, s.progress_monitor = int(cfg.use_prev_action), int(cfg.is_bert), int(cfg.progress_monitor)
    s.ablate_instruction, s.ablate_depth, s.ablate_rgb = int(cfg.ablate_instruction), int(cfg.ablate_depth), int(cfg.ablate_rgb)
    return s


class S2SEngine(_FlatEngine):
    """Owns one libhcm Seq2SeqNet handle (weights + workspace) on one GPU."""

    def __init__(self, cfg: S2SConfig, state_dict, max_batch=64, precision="fp16", device=None, graph=False):
        """graph=True: forward() runs on an engine-owned stream with engine-owned static I/O buffers so that libhcm replays one
        captured hipGraph per step; the returned tensors then alias those buffers and stay valid until the second-next call."""
        cfg.validate()
        self._open(cfg, max_batch, device, graph, "hcm_s2s_create", _to_struct(cfg, max_batch, precision),
                   ((_lib.HCM_S2S, k, v) for k, v in state_dict.items()))

    def _inputs(self, observations, rows):
        c = self.cfg
        rgb, depth, B = self._frames(observations, (0,), self._frame_check)      # (or rgb_features / depth_features)
        if rows is not None and B != rows:
            raise ValueError(f"expected {rows} frames, got {B}")
        self._no_instr_stream(observations)
        ids = self._dev(observations["instruction"], (torch.int64, torch.int32, torch.float32))
        # cfg.instr_len is the longest padded instruction the workspace is sized for; every call brings its own L.  A (1, L) instruction is NOT
        # expanded here: the library encodes it once and writes the vector to all B rows (seq2seq.py:163)
        if ids.dim() != 2 or ids.shape[0] not in (1, B) or not 1 <= ids.shape[1] <= c.instr_len:
            raise ValueError(f"instruction must be (B or 1, L <= {c.instr_len}), got {tuple(ids.shape)}")
        return rgb, depth, ids, B

    def _frame_check(self, rgb, depth):
        c = self.cfg
        rgb = self._dev(rgb, (torch.float32, torch.uint8))
        depth = self._dev(depth, (torch.float32,))
        if tuple(rgb.shape[1:]) != (*c.rgb_shape, 3):
            raise ValueError(f"rgb must be (B,{c.rgb_shape[0]},{c.rgb_shape[1]},3), got {tuple(rgb.shape)}")
        if tuple(depth.shape) != (rgb.shape[0], *c.depth_shape, 1):
            raise ValueError(f"depth must be (B,{c.depth_shape[0]},{c.depth_shape[1]},1), got {tuple(depth.shape)}")
        return rgb, depth

    def _enc_frames(self, observations):
        return self._frame_check(observations["rgb"], observations["depth"])

    def _outputs(self, B):
        c = self.cfg
        out = torch.empty(B, c.num_actions, device=self.device, dtype=torch.float32)
        stop = torch.empty(B, 1, device=self.device, dtype=torch.float32)
        prog = torch.empty(B, 1, device=self.device, dtype=torch.float32) if c.progress_monitor else None
        return out, stop, prog

    def forward(self, observations, hidden, masks):
        """-> (output (B,num_actions), stop_out (B,1), progress_hat (B,1) or None, rnn_hidden_states)"""
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, None)
            h_in, m = self._state_mask(hidden, masks, B, B)

            def call(rgb_, depth_, ids_, h_in_, m_, out, stop, prog, h_out, st):
                _lib.check(self._lib.hcm_s2s_forward(self._h, rgb_.data_ptr(), _TORCH_DT[rgb.dtype], depth_.data_ptr(), ids_.data_ptr(),
                                                     _TORCH_DT[ids.dtype], B, ids.shape[0], ids.shape[1], h_in_.data_ptr(), m_.data_ptr(),
                                                     out.data_ptr(), stop.data_ptr(), _ptr(prog), h_out.data_ptr(), st), self._h)
            if self._graph:
                return self._forward_graph(call, rgb, depth, ids, h_in, m, B, progress=self.cfg.progress_monitor)
            out, stop, prog = self._outputs(B)
            h_out = torch.empty_like(h_in)
            call(rgb, depth, ids, h_in, m, out, stop, prog, h_out, self._stream())
        return out, stop, prog, h_out

    def forward_seq(self, observations, hidden, masks, T, N):
        """Training / validation path (RNNStateEncoder.seq_forward): observations hold T*N rows, time-major; hidden (R,N,hidden); masks (T*N,)."""
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, T * N)
            h_in, m = self._state_mask(hidden, masks, B, N)
            out, stop, prog = self._outputs(B)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_s2s_forward_seq(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(),
                                                     _TORCH_DT[ids.dtype], T, N, ids.shape[0], ids.shape[1], h_in.data_ptr(), m.data_ptr(),
                                                     out.data_ptr(), stop.data_ptr(), _ptr(prog), h_out.data_ptr(), self._stream()), self._h)
        return out, stop, prog, h_out

    def val_step(self, observations, corrected_actions, oracle_stop, hidden, masks, result=None, return_outputs=False):
        """The flat trainer's validation step, `_update_agent_val` (robo_vln_trainer.py:544-575), in one library call (hcm_flat_val_step): the
        model on the chunk's T*N time-major rows of `observations` (N = hidden.shape[1]) and the criteria.  With PROGRESS_MONITOR.use,
        observations["progress"] ((T*N,) or (T*N,1)) is the target of the auxiliary loss the reference registers at seq2seq.py:176-185.  Returns
        (result, hidden'), plus (out, stop, progress_hat or None) BEFORE any masking with return_outputs=True.  result is the (8,) f32 device
        tensor of include/hcm.h: [action loss, stop loss, aux loss, stop rows, aux rows, 0, 0, 0]; it is written into `result` when given, so
        that a caller can keep a table of them and read once.  Does not synchronise."""
        c = self.cfg
        with torch.cuda.device(self.device):
            rgb, depth, ids, B = self._inputs(observations, None)
            h_in, N, ca, os_, m, result = _val_labels(self, B, hidden, corrected_actions, oracle_stop, masks, result)
            prog = None
            if c.progress_monitor:
                if "progress" not in observations:
                    raise ValueError("observations['progress'] is missing: the engine was built with progress_monitor=True")
                prog = self._dev(observations["progress"], (torch.float32,))
                if tuple(prog.shape) not in ((B,), (B, 1)):
                    raise ValueError(f"observations['progress'] must be ({B},) or ({B},1), got {tuple(prog.shape)}")
            h_out = torch.empty_like(h_in)
            out, stop, prog_hat = self._outputs(B) if return_outputs else (None, None, None)
            st = self._stream()
            _lib.check(self._lib.hcm_flat_val_step(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(), _TORCH_DT[ids.dtype],
                                                   B // N, N, ids.shape[0], ids.shape[1], ca.data_ptr(), os_.data_ptr(), _ptr(prog), h_in.data_ptr(),
                                                   m.data_ptr(), result.data_ptr(), h_out.data_ptr(), _ptr(out), _ptr(stop), _ptr(prog_hat), st), self._h)
        if return_outputs:
            return result, h_out, (out, stop, prog_hat)
        return result, h_out


class Seq2SeqNet:
    """`Seq2SeqNet.forward(batch)` (models/seq2seq.py:140-189): batch = (observations, rnn_hidden_states, prev_actions, masks) ->
    (output (B,2), stop_out (B,1), rnn_hidden_states).  observations['instruction'] stays in place (the reference's `del` is commented
    out, seq2seq.py:150-151); prev_actions is ignored (SEQ2SEQ.use_prev_action = False).  With PROGRESS_MONITOR.use the last
    tanh(progress_monitor(x)) (seq2seq.py:177) is kept in `progress_hat`; the loss against observations['progress'] is the caller's."""

    def __init__(self, engine: S2SEngine):
        self.engine = engine
        self.progress_hat = None

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
        out, stop, self.progress_hat, hidden = self.engine.forward(observations, rnn_hidden_states, masks)
        return out, stop, hidden

    def seq_forward(self, batch, T, N):
        """The training / validation call: T*N frames at once with an (R,N,hidden) state (RNNStateEncoder.seq_forward)."""
        observations, rnn_hidden_states, prev_actions, masks = batch
        out, stop, self.progress_hat, hidden = self.engine.forward_seq(observations, rnn_hidden_states, masks, T, N)
        return out, stop, hidden

    __call__ = forward
