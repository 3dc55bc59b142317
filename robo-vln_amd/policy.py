"""Host-side mirror of the reference's model-call interface for the HCM hot path.

`Seq2Seq_HighLevel_CMA` / `Seq2Seq_LowLevel` keep the reference's tuple-in / tuple-out `forward(batch)`
contracts (robo_vln_baselines/models/seq2seq_highlevel_cma.py:170-233, seq2seq_lowlevel.py:116-162) and
properties, so the eval loop of hierarchical_trainer.py:1088-1197 can call them unchanged; `Policy.act()` is
the fused step (hi -> argmax -> lo) of :1095-1101.  All arithmetic happens in libhcm.so (HIP, gfx950);
torch is used only for device buffers and streams.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._engine import INSTR_KEY, _TORCH_DT, _EngineBase, _FeatureFrames, _InstrStream, _np32, _ptr, obs_rows       # noqa: F401  (_np32: importable from here as before)
from .config import HCMConfig

_SUB_SLOTS = {"depth": 0, "bert": 1, "vla": 2, "rgb": 3}
_SUB_DT = {"fp32": _lib.HCM_F32, "bf16": _lib.HCM_BF16, "fp16": _lib.HCM_F16}


def _to_struct(cfg: HCMConfig, max_batch, precision, build_high, build_low, sub_precision=None, max_instr_len=None, keep_host_weights=False,
               share_trunks=True):
    s = _lib.HcmConfigStruct()
    for name, p in (sub_precision or {}).items():
        s.reserved[_SUB_SLOTS[name]] = _SUB_DT[p] + 1
    s.reserved[4] = int(bool(keep_host_weights))
    s.reserved[5] = int(not share_trunks)
    s.struct_size = C.sizeof(_lib.HcmConfigStruct)
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
    s.precision = _lib.PRECISIONS[precision]
    s.max_batch = max_batch
    s.rgb_h, s.rgb_w = cfg.rgb_shape
    s.depth_h, s.depth_w = cfg.depth_shape
    s.instr_len = max_instr_len or cfg.instr_len           # the library's instr_len is the MAXIMUM L of a call
    s.rgb_encoder = _lib.HCM_ENC_RESNET if cfg.rgb_encoder == "TorchVisionResNet50" else _lib.HCM_ENC_SIMPLECNN
    s.depth_encoder = _lib.HCM_ENC_RESNET if cfg.depth_encoder == "VlnResnetDepthEncoder" else _lib.HCM_ENC_SIMPLECNN
    s.rgb_out, s.depth_out, s.depth_baseplanes = cfg.rgb_out, cfg.depth_out, cfg.depth_baseplanes
    s.vla_layers, s.d_model, s.vla_heads, s.d_ff = cfg.vla_layers, cfg.d_model, cfg.vla_heads, cfg.d_ff
    s.vis_in, s.ins_in = cfg.vis_in, cfg.ins_in
    s.hidden = cfg.hidden
    s.rnn_type = _lib.HCM_LSTM if cfg.rnn_type == "LSTM" else _lib.HCM_GRU
    s.num_actions, s.num_sub_tasks, s.lo_actions = cfg.num_actions, cfg.num_sub_tasks, cfg.lo_actions
    s.bert_layers, s.bert_hidden, s.bert_heads = cfg.bert_layers, cfg.bert_hidden, cfg.bert_heads
    s.bert_inter, s.bert_vocab, s.bert_max_pos = cfg.bert_inter, cfg.bert_vocab, cfg.bert_max_pos
    s.build_high, s.build_low = int(build_high), int(build_low)
    s.use_prev_action, s.ablate_instruction = int(cfg.use_prev_action), int(cfg.ablate_instruction)
    s.progress_monitor = int(cfg.progress_monitor)
    s.ablate_depth, s.ablate_rgb = int(cfg.ablate_depth), int(cfg.ablate_rgb)
    return s


class HCMEngine(_EngineBase):
    """Owns one libhcm handle (weights + workspace) on one GPU.  One engine per device per thread."""

    def __init__(self, cfg: HCMConfig, high_level_state_dict=None, low_level_state_dict=None, max_batch=64,
                 precision="fp16", device=None, sub_precision=None, graph=False, max_instr_len=None, keep_host_weights=False, guard_every=64,
                 share_trunks=True, chain_graphs="auto"):
        """precision (fp32 accumulation, fp32 recurrent cells / heads in every mode):
          "fp16"  fp16 storage + fp16 MFMA tiles in every sub-network, behind the range calibration of hcm_finalize (the measured 16-bit mode:
                  record error 2.6e-3 at B = 64).  A trunk that leaves the fp16 range gets an exact power-of-two range fold (`range_fold`),
                  BERT / the cross-modal block fall back to bf16 tiles (`fp16_fallback`);
          "bf16"  bf16 storage + bf16 MFMA tiles in BERT, the RGB trunks and the cross-modal block; the GroupNorm depth trunks stay on
                  range-folded fp16 tiles (on bf16 that trunk alone costs 1.9e-2 of the 1e-2 record tolerance);
          "fp32"  fp32 storage + fp32 MFMA.
        `sub_precision` overrides the storage type per sub-network, e.g. {"depth": "bf16"} or {"bert": "fp16"} (keys: depth, bert, vla, rgb).
        share_trunks: when the two models' trunk weights are bit-identical (frozen pretrained encoders in both state_dicts) the trunk runs once per
        step and feeds both heads; False runs it per model (test aid).
        guard_every: act() polls the run-time overflow guard every this many steps without synchronising (hcm_guard_poll) and raises
        FloatingPointError once a recurrent cell has seen non-finite gate pre-activations; 0 disables.
        graph=True: act() runs on an engine-owned stream with engine-owned static I/O buffers, so that libhcm replays
        one captured hipGraph per step; the returned record / hidden tensors then alias those buffers and stay valid
        until the second-next act() call (ping-pong), which is what a rollout loop that rebinds them every step needs.
        chain_graphs (with graph=True): replay the step as one LINEAR hipGraph per encoder chain instead of one graph captured across the forked
        streams (HCM_ACT_CHAIN_GRAPHS, include/hcm.h): 0.18 ms of host time per step instead of 0.5-0.8 ms and a lower synchronous latency at B = 1,
        2-4 % less pipelined throughput.  "auto" = for calls of one or two environments (the reference's own evaluation loop, one policy call per
        simulator step), and for host_frames=True calls whose frame tensors are at least 4 MB each (the copies then overlap BERT: +5-12 % PCIe-inclusive
        throughput from B = 24 up); True / False force it.  Bit-identical either way.
        max_instr_len: the longest instruction (tokens) a call may carry; sizes the workspace.  Every call takes its own
        (B or 1, L <= max_instr_len) ids, as the reference model does (its eval loop feeds the unpadded tokens of the episode's
        instruction, common/utils.py:18-20).  Default: cfg.instr_len.  BERT's position table allows up to 512."""
        self.max_instr_len = int(max_instr_len or cfg.instr_len)
        # fp16 range safety: hcm_finalize checks the fp16 sub-networks on a synthetic batch and repairs what would overflow (`range_fold`,
        # `fp16_fallback`); keep_host_weights=True keeps the f32 host copies so that `calibrate(observations)` can repeat the check -- and
        # the repair -- on real observations
        if chain_graphs not in ("auto", True, False):
            raise ValueError('chain_graphs must be "auto", True or False')
        self._chain_graphs = chain_graphs
        self.comm_world, self.comm_rank = 0, 0          # > 0 once comm_init() has created the RCCL communicator
        self._guard_every = int(guard_every)
        self._guard_tick = 0
        self._guard_seen = 0
        self._gather_B = 0                              # per-rank batch of the library collective (act(gather=True)), 0 before the first such call
        self._gather_called = False
        self.guard_alarm = 0                            # deferred alarms of act(gather=True) steps, see guard_check()
        cfg.validate()
        self.precision = precision
        self.has_high = high_level_state_dict is not None
        self.has_low = low_level_state_dict is not None
        st = _to_struct(cfg, max_batch, precision, self.has_high, self.has_low, sub_precision, self.max_instr_len, keep_host_weights, share_trunks)
        # load_state_dict(strict=True) semantics (hierarchical_trainer.py:343-345); BertEmbeddings' position_ids / token_type_ids are buffers of
        # some transformers versions, not parameters
        self._open(cfg, max_batch, device, graph, "hcm_create", st,
                   ((model, k, v) for model, sd in ((_lib.HCM_HIGH, high_level_state_dict), (_lib.HCM_LOW, low_level_state_dict)) if sd is not None
                    for k, v in sd.items() if not k.endswith(("embeddings.position_ids", "embeddings.token_type_ids"))))

    def _guard_poll(self, stream, defer=False):
        """Every `guard_every` act() calls: non-blocking read of the overflow guard (the value is the one an EARLIER poll enqueued).
        defer=True (act(gather=True): env-sharded ranks): the alarm is only RECORDED (self.guard_alarm) -- a rank that raised on its own in
        the middle of a rollout would leave its peers blocked in the next step's all-gather; guard_check() agrees on it across ranks."""
        if self._guard_every <= 0:
            return
        self._guard_tick += 1
        if self._guard_tick % self._guard_every:
            return
        out = C.c_int64()
        _lib.check(self._lib.hcm_guard_poll(self._h, stream, C.byref(out)), self._h)
        if out.value > self._guard_seen:
            new, self._guard_seen = out.value - self._guard_seen, out.value
            if defer:
                self.guard_alarm += new
                return
            raise FloatingPointError(f"overflow guard: {new} (environment, recurrent step) pairs had non-finite activations in front of a recurrent "
                                     "cell since the last check -- broken sensor frames, or a sub-network outside its fp16 range "
                                     "(engine.calibrate(observations) on real observations; engine.calibration_report())")

    def guard_check(self, group=None):
        """Env-sharded ranks: agree on the deferred overflow-guard alarms (MAX over the ranks of `group`, one tiny all-reduce) and raise
        FloatingPointError on EVERY rank when any rank has one -- all ranks leave the rollout at the same step, nobody is left inside a
        collective.  rollout() calls it every `guard_every` steps; a single-process engine raises from act() directly and needs no call."""
        alarm = int(self.guard_alarm)
        if self.comm_world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            t = torch.tensor([alarm], device=self.device, dtype=torch.int64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=group)
            alarm = int(t.item())
        if alarm:
            self.guard_alarm = 0
            raise FloatingPointError(f"overflow guard: up to {alarm} (environment, recurrent step) pairs on one rank had non-finite activations in "
                                     "front of a recurrent cell since the last check (engine.calibrate(observations); engine.calibration_report())")

    def comm_abort(self):
        """Tear the library's communicator down (hcm_comm_abort): for a rank that is going to stop stepping outside an agreed point."""
        _lib.check(self._lib.hcm_comm_abort(self._h), self._h)
        self.comm_world, self.comm_rank = 0, 0
        self._gather_B = 0

    @property
    def fp16_fallback(self):
        """Sub-networks the range calibration moved from fp16 to bf16 storage: subset of {"bert", "depth", "rgb", "vla"}."""
        bits = self.query(_lib.HCM_FP16_FALLBACK)
        return {n for b, n in ((1, "bert"), (2, "depth"), (4, "rgb"), (8, "vla")) if bits & b}

    @property
    def range_fold(self):
        """Trunks the range calibration kept on fp16 by folding a power of two into their weights (exact): subset of {"depth", "rgb"}."""
        bits = self.query(_lib.HCM_RANGE_FOLD)
        return {n for b, n in ((2, "depth"), (4, "rgb")) if bits & b}

    def calibration_report(self):
        return {"bert_max_abs": self.query(_lib.HCM_CALIB_MAX_BERT), "depth_max_abs": self.query(_lib.HCM_CALIB_MAX_DEPTH),
                "rgb_max_abs": self.query(_lib.HCM_CALIB_MAX_RGB), "vla_max_abs": self.query(_lib.HCM_CALIB_MAX_VLA),
                "non_finite": self.query(_lib.HCM_CALIB_NONFINITE), "fp16_fallback": sorted(self.fp16_fallback),
                "range_fold": sorted(self.range_fold)}

    def comm_init(self, group=None):
        """Create the library's own RCCL communicator over the ranks of a torch.distributed process group (one process per GPU): rank 0 draws the
        ncclUniqueId (hcm_comm_unique_id), the existing group broadcasts its 128 bytes, every rank calls hcm_comm_init.  Afterwards
        act(..., gather=True) returns the all-gathered (world * B, 7) record of the whole rollout batch, the collective being enqueued by the
        library behind the step on the step's stream (hcm_act_gather) -- no torch.distributed call per step."""
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        ident = (C.c_char * 128)()
        ok = 1
        if rank == 0:
            ok = 1 if self._lib.hcm_comm_unique_id(ident) == 0 else 0
        # 128 id bytes + one status byte: a rank-0 failure (no librccl to dlopen) reaches every rank as an exception, not as a hang in the broadcast
        t = torch.tensor(list(bytes(ident)) + [ok], dtype=torch.uint8)
        on_dev = dist.get_backend(group) == "nccl"
        if on_dev:
            t = t.to(self.device)
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = bytes(t.cpu().numpy().tobytes())
        if raw[128] != 1:
            raise RuntimeError("hcm_comm_unique_id failed on rank 0 (librccl not loadable?)")
        with torch.cuda.device(self.device):
            rc = self._lib.hcm_comm_init(self._h, C.c_char_p(raw[:128]), rank, world)
        # every rank learns whether ALL ranks have a communicator (a rank that failed would otherwise leave the others in their first collective)
        flag = torch.tensor([1 if rc == 0 else 0], dtype=torch.int32, device=self.device if on_dev else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) != 1:
            raise RuntimeError("hcm_comm_init failed on at least one rank" + (": " + _lib.last_error(self._h) if rc != 0 else ""))
        self.comm_world, self.comm_rank = world, rank
        return world

    def calibrate(self, observations, release_host_weights=True):
        """Range-check the fp16 sub-networks on these observations (hcm_calibrate); returns calibration_report().  Needs
        keep_host_weights=True at construction to be able to re-build a sub-network on bf16 tiles."""
        with torch.cuda.device(self.device):
            rgb, depth, ids, _, B = self._obs(observations, self.has_high)
            _lib.check(self._lib.hcm_calibrate(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), _ptr(ids),
                                               _TORCH_DT[ids.dtype] if ids is not None else _lib.HCM_I64, B, ids.shape[1] if ids is not None else 1,
                                               self._stream()), self._h)
            if release_host_weights:
                _lib.check(self._lib.hcm_release_host_weights(self._h), self._h)
        # hcm_calibrate re-synchronised the library's polled view of the overflow guard with the device word (zeroed by a re-build, possibly
        # raised by the measuring passes): alarms are counted from THAT value on -- neither a stale count (which would hide new alarms) nor a
        # cached earlier one (which would raise again for steps already reported)
        self._guard_seen = self.query(_lib.HCM_STEP_NONFINITE)
        self._guard_tick = 0
        return self.calibration_report()

    # ---- helpers
    def _host_frame(self, t, dtypes, name):
        # HCM_ACT_HOST_FRAMES: the library copies the frames itself, chain by chain -- they must be page-locked host tensors as they are
        if not isinstance(t, torch.Tensor) or t.device.type != "cpu" or not t.is_pinned() or not t.is_contiguous() or t.dtype not in dtypes:
            raise ValueError(f"host_frames=True: {name} must be a contiguous pinned CPU tensor of dtype {' / '.join(str(d) for d in dtypes)}")
        return t

    def _has_slot(self, slot):
        return self.has_high if slot == 0 else self.has_low

    def _frame_check(self, rgb, depth, host_frames=False):
        if host_frames:
            rgb = self._host_frame(rgb, (torch.float32, torch.uint8), "rgb")
            depth = self._host_frame(depth, (torch.float32,), "depth")
        else:
            rgb = self._dev(rgb, (torch.float32, torch.uint8))
            depth = self._dev(depth, (torch.float32,))
        B = rgb.shape[0]
        c = self.cfg
        if tuple(rgb.shape[1:]) != (*c.rgb_shape, 3):
            raise ValueError(f"rgb must be (B,{c.rgb_shape[0]},{c.rgb_shape[1]},3), got {tuple(rgb.shape)}")
        if tuple(depth.shape) != (B, *c.depth_shape, 1):
            raise ValueError(f"depth must be (B,{c.depth_shape[0]},{c.depth_shape[1]},1), got {tuple(depth.shape)}")
        return rgb, depth

    def _enc_frames(self, observations):
        return self._frame_check(observations["rgb"], observations["depth"])

    def _instr_stream(self, t, B, seq):
        """observations["instruction_features"] of a call of B rows, checked: f32 (B or 1, L, bert_hidden) on the engine's device -- or, in a
        sequence / validation call (seq), any row count that divides B; the call narrows it to (B, 1 or N) once it knows N (_InstrStream.check_envs)"""
        c = self.cfg
        if not self.has_high:
            raise ValueError(f"{INSTR_KEY}: this engine holds no high-level model, and only that one reads the instruction")
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"{INSTR_KEY} must be a tensor on the engine's device {self.device} (encode_instruction returns one); a host copy of a cache "
                             "is brought over with .to(device) by its owner, not silently per call")
        if t.device != self.device and (t.device.index is not None and self.device.index is not None):
            raise ValueError(f"{INSTR_KEY} lives on {t.device}, the engine on {self.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"{INSTR_KEY} must be float32, got {t.dtype}")
        if t.dim() != 3 or t.shape[2] != c.bert_hidden:
            raise ValueError(f"{INSTR_KEY} must be (rows, L, {c.bert_hidden}), got {tuple(t.shape)}")
        if not 1 <= t.shape[1] <= self.max_instr_len:
            raise ValueError(f"{INSTR_KEY}: L = {t.shape[1]} outside [1, {self.max_instr_len}] (max_instr_len)")
        rows = t.shape[0]
        if rows < 1 or B % rows or (not seq and rows not in (1, B)):
            raise ValueError(f"{INSTR_KEY} must hold {B} rows or 1" + (f", or one row per environment (a divisor of {B})" if seq else "") + f", got {rows}")
        return t.contiguous()

    def _obs(self, observations, need_ids, host_frames=False, slots=(0, 1), seq=False):
        """slots: the models the call runs (0 high-level, 1 low-level) -- whose rgb_features / depth_features it takes (_EngineBase._frames).
        ids comes back as the (B, L) token tensor, or as an _InstrStream when the observations carry `instruction_features`.
        seq: a sequence / validation call, whose stream may hold one row per environment"""
        rgb, depth, B = self._frames(observations, tuple(s for s in slots if self._has_slot(s)) or slots,
                                     lambda r, d: self._frame_check(r, d, host_frames), host_frames)
        ids = lens = None
        if need_ids:
            if observations.get(INSTR_KEY) is not None:
                # the frozen BERT stream instead of the ids: given together with `instruction` the feature wins and the ids are not read, as with the
                # trunk features; `instruction` may be absent
                ids = _InstrStream(self._instr_stream(observations[INSTR_KEY], B, seq), B)
            else:
                ids = self._dev(observations["instruction"], (torch.int64, torch.int32, torch.float32))
                if ids.dim() != 2 or ids.shape[0] not in (1, B) or not 1 <= ids.shape[1] <= self.max_instr_len:
                    raise ValueError(f"instruction must be (B or 1, L) with 1 <= L <= {self.max_instr_len} (max_instr_len), got {tuple(ids.shape)}")
                # instruction.expand(B, L) (seq2seq_highlevel_cma.py:189-190)
                ids = ids.expand(B, ids.shape[1]).contiguous()
            # extension for batched rollouts (not a reference key): per-environment token counts of a padded ragged batch
            if observations.get("instruction_lengths") is not None:
                lens = self._dev(observations["instruction_lengths"], (torch.int32,)).reshape(-1)
                if lens.numel() != B:
                    raise ValueError(f"instruction_lengths must hold {B} entries, got {lens.numel()}")
        return rgb, depth, ids, lens, B

    def _mask(self, masks, B):
        m = self._dev(masks, (torch.float32,))
        # the reference reads masks[:,0] (seq2seq_highlevel_cma.py:208); accept (B,), (B,1), (B,2), (B,2,1)
        m = m.reshape(B, -1)[:, 0].contiguous()
        return m

    def _hidden(self, h, B=None):
        h = self._dev(h, (torch.float32,))
        R = self.num_recurrent_layers
        if h.dim() != 3 or h.shape[0] != R or h.shape[2] != self.cfg.hidden or (B is not None and h.shape[1] != B):
            raise ValueError(f"hidden state must be ({R},{B if B is not None else 'N'},{self.cfg.hidden}), got {tuple(h.shape)}")
        return h

    # ---- the three calls
    def high_forward(self, observations, hidden, masks):
        with torch.cuda.device(self.device):
            rgb, depth, ids, lens, B = self._obs(observations, True, slots=(0,))
            h_in, m = self._hidden(hidden, B), self._mask(masks, B)
            logits = torch.empty(B, self.cfg.num_actions, device=self.device, dtype=torch.float32)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_high_forward(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(),
                                                  ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(lens), B, ids.shape[1], h_in.data_ptr(), m.data_ptr(),
                                                  logits.data_ptr(), h_out.data_ptr(), self._stream()), self._h)
        return logits, h_out

    def low_forward(self, observations, hidden, masks, subtask):
        with torch.cuda.device(self.device):
            rgb, depth, _, _, B = self._obs(observations, False, slots=(1,))
            h_in, m = self._hidden(hidden, B), self._mask(masks, B)
            st = self._dev(subtask, (torch.int64,)).reshape(B)
            vel = torch.empty(B, self.cfg.lo_actions, device=self.device, dtype=torch.float32)
            stop = torch.empty(B, 1, device=self.device, dtype=torch.float32)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_low_forward(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), B,
                                                 h_in.data_ptr(), m.data_ptr(), st.data_ptr(), vel.data_ptr(),
                                                 stop.data_ptr(), h_out.data_ptr(), self._stream()), self._h)
        return vel, stop, h_out

    def _act_graph(self, observations, hi_hidden, lo_hidden, masks, flags=0, gather=False):
        host_frames = bool(flags & _lib.HCM_ACT_HOST_FRAMES)
        with torch.cuda.device(self.device):
            rgb, depth, ids, lens, B = self._obs(observations, True, host_frames)
            if gather:
                self._gather_B = B
            L = ids.shape[1]
            hh, lh, m = self._hidden(hi_hidden, B), self._hidden(lo_hidden, B), self._mask(masks, B)
            if self._gstream is None:
                self._gstream = torch.cuda.Stream(device=self.device)
            st = self._static
            feat = isinstance(rgb, _FeatureFrames)      # features are read in place: the graph is keyed by the pointers in the struct
            instr = isinstance(ids, _InstrStream)       # ... and so is the instruction stream (no static copy: the graph is keyed by its address and rows)
            if st is None or st["B"] != B or st["rgb"].dtype != rgb.dtype or (not instr and st["ids"].dtype != ids.dtype) or st["rgb"].device != rgb.device:
                # the static ids buffer holds the longest instruction; a call uses its first B*L elements, so the graph of a new L
                # differs by its key only, not by the buffer address
                st = {"B": B, "tick": 0, "rgb": rgb if feat else torch.empty_like(rgb), "depth": depth if feat else torch.empty_like(depth),
                      "ids": torch.empty(B * self.max_instr_len, device=self.device, dtype=torch.int64 if instr else ids.dtype),
                      "lens": torch.empty(B, device=self.device, dtype=torch.int32),
                      "mask": torch.empty_like(m), "rec": [torch.empty(B, 7, device=self.device) for _ in range(2)],
                      "hh": [torch.zeros_like(hh) for _ in range(2)], "lh": [torch.zeros_like(lh) for _ in range(2)]}
                self._static = st
            cur = torch.cuda.current_stream()
            gs = self._gstream
            gs.wait_stream(cur)
            # Observation buffers the caller re-uses from step to step (an ObsStager's device tensors, a vectorised simulator's
            # output buffers) are read in place: the captured graph is keyed by their addresses like by any other argument.
            # Tensors seen for the first time go through the engine's static copies, so that fresh allocations every step
            # do not force a new capture every step.
            ptrs = (rgb.pointers() if feat else (rgb.data_ptr(), depth.data_ptr())) + (ids.pointers() if instr else (ids.data_ptr(),)) \
                + (m.data_ptr(), L, lens.data_ptr() if lens is not None else 0)
            # (a caller that rotates a few buffer sets -- double-buffered staging -- is recognised as well: the last four sets)
            seen = st.setdefault("seen_ptrs", [])
            direct = ptrs in seen and not os.environ.get("HCM_NO_DIRECT_OBS")
            if ptrs in seen:
                seen.remove(ptrs)
            seen.append(ptrs)
            del seen[:-4]
            st["hold"] = (rgb, depth, ids, m, lens)        # keep the caller's tensors alive while the graph may read them
            s_ids = ids if instr else st["ids"][:B * L].view(B, L)
            g_rgb, g_depth, g_ids, g_m = (rgb, depth, ids, m) if direct else (st["rgb"], st["depth"], s_ids, st["mask"])
            if host_frames or feat:                        # pinned host frames are always read in place (the library stages them); so are features
                g_rgb, g_depth = rgb, depth
            g_lens = None if lens is None else lens if direct else st["lens"]
            with torch.cuda.stream(gs):
                i = st["tick"] & 1
                for dst, src in ((g_rgb, rgb), (g_depth, depth), (g_ids, ids), (g_m, m), (g_lens, lens),
                                 (st["hh"][1 - i], hh), (st["lh"][1 - i], lh)):
                    if dst is not None and dst.data_ptr() != src.data_ptr():
                        dst.copy_(src, non_blocking=True)
                if gather:
                    if "gat" not in st:
                        st["gat"] = [torch.empty(self.comm_world * B, 7, device=self.device) for _ in range(2)]
                    self._gather_called = True
                    _lib.check(self._lib.hcm_act_gather(self._h, g_rgb.data_ptr(), _TORCH_DT[rgb.dtype], g_depth.data_ptr(),
                                                        g_ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(g_lens), B, L, st["hh"][1 - i].data_ptr(),
                                                        st["lh"][1 - i].data_ptr(), g_m.data_ptr(), st["rec"][i].data_ptr(),
                                                        st["hh"][i].data_ptr(), st["lh"][i].data_ptr(), flags, st["gat"][i].data_ptr(),
                                                        C.c_void_p(gs.cuda_stream)), self._h)
                else:
                    _lib.check(self._lib.hcm_act_ex(self._h, g_rgb.data_ptr(), _TORCH_DT[rgb.dtype], g_depth.data_ptr(),
                                                    g_ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(g_lens), B, L, st["hh"][1 - i].data_ptr(),
                                                    st["lh"][1 - i].data_ptr(), g_m.data_ptr(), st["rec"][i].data_ptr(),
                                                    st["hh"][i].data_ptr(), st["lh"][i].data_ptr(), flags, C.c_void_p(gs.cuda_stream)), self._h)
                st["tick"] += 1
            cur.wait_stream(gs)
            # (after the join: an alarm raised from here leaves the caller's stream ordered behind the step it interrupts)
            self._guard_poll(C.c_void_p(gs.cuda_stream), defer=gather)
        return (st["gat"][i] if gather else st["rec"][i]), st["hh"][i], st["lh"][i]

    # ---- training / validation path: T*N frames per call, RNNStateEncoder.seq_forward (state_encoder.py:83-133)
    def high_forward_seq(self, observations, hidden, masks):
        with torch.cuda.device(self.device):
            rgb, depth, ids, lens, TN = self._obs(observations, True, slots=(0,), seq=True)
            h_in = self._hidden(hidden)
            N = h_in.shape[1]
            if TN % N:
                raise ValueError(f"{TN} frames is not a multiple of the hidden batch {N}")
            if isinstance(ids, _InstrStream):
                ids.check_envs(TN, N)
            m = self._mask(masks, TN)
            logits = torch.empty(TN, self.cfg.num_actions, device=self.device, dtype=torch.float32)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_high_forward_seq(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(),
                                                      _TORCH_DT[ids.dtype], _ptr(lens), TN // N, N, ids.shape[1], h_in.data_ptr(), m.data_ptr(), logits.data_ptr(),
                                                      h_out.data_ptr(), self._stream()), self._h)
        return logits, h_out

    def low_forward_seq(self, observations, hidden, masks, subtask):
        with torch.cuda.device(self.device):
            rgb, depth, _, _, TN = self._obs(observations, False, slots=(1,))
            h_in = self._hidden(hidden)
            N = h_in.shape[1]
            if TN % N:
                raise ValueError(f"{TN} frames is not a multiple of the hidden batch {N}")
            m = self._mask(masks, TN)
            st = self._dev(subtask, (torch.int64,)).reshape(TN)
            vel = torch.empty(TN, self.cfg.lo_actions, device=self.device, dtype=torch.float32)
            stop = torch.empty(TN, 1, device=self.device, dtype=torch.float32)
            h_out = torch.empty_like(h_in)
            _lib.check(self._lib.hcm_low_forward_seq(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), TN // N, N,
                                                     h_in.data_ptr(), m.data_ptr(), st.data_ptr(), vel.data_ptr(), stop.data_ptr(),
                                                     h_out.data_ptr(), self._stream()), self._h)
        return vel, stop, h_out

    def val_step(self, observations, corrected_actions, oracle_stop, hi_hidden, lo_hidden, masks, result=None, return_outputs=False):
        """The teacher-forced validation step, HierarchicalTrainer._update_agent_val (hierarchical_trainer.py:562-631), in one library
        call (hcm_val_step): both models on the T*N frames of `observations` -- the low-level one fed the oracle's sub-task
        observations["vln_oracle_action_sensor"] (0 = padded row, k = sub-task k - 1; any integer or float dtype, (T*N,) or (T*N,1) as the
        trainer carries it, :580) -- and the criteria.  Returns (result, hi_hidden', lo_hidden'), plus (logits, vel, stop) BEFORE any masking
        with return_outputs=True.  result is the (8,) f32 device tensor of include/hcm.h: [high-level loss, action loss, stop loss, correct,
        total, stop rows, out-of-range labels, 0]; it is written into `result` when given, so that a caller can keep a table of them and
        read once (check_val_result).  Does not synchronise."""
        with torch.cuda.device(self.device):
            rgb, depth, ids, lens, TN = self._obs(observations, True, seq=True)
            hh = self._hidden(hi_hidden)
            N = hh.shape[1]
            lh = self._hidden(lo_hidden, N)
            if TN % N:
                raise ValueError(f"{TN} frames is not a multiple of the hidden batch {N}")
            if isinstance(ids, _InstrStream):
                ids.check_envs(TN, N)
            m = self._mask(masks, TN)
            oracle = observations["vln_oracle_action_sensor"]
            if not isinstance(oracle, torch.Tensor):
                oracle = torch.as_tensor(np.asarray(oracle))
            if oracle.numel() != TN:
                raise ValueError(f"vln_oracle_action_sensor must hold {TN} entries, got {tuple(oracle.shape)}")
            oracle = oracle.to(self.device, non_blocking=True).reshape(TN).to(torch.int64).contiguous()      # .squeeze(1).to(dtype=torch.int64), :580
            ca = self._dev(corrected_actions, (torch.float32,))
            os_ = self._dev(oracle_stop, (torch.float32,))
            if tuple(ca.shape) != (TN, self.cfg.lo_actions) or os_.numel() != TN:
                raise ValueError(f"corrected_actions must be ({TN},{self.cfg.lo_actions}) and oracle_stop ({TN},1), got {tuple(ca.shape)} and {tuple(os_.shape)}")
            result = self._result(result)
            hh2, lh2 = torch.empty_like(hh), torch.empty_like(lh)
            logits = vel = stop = None
            if return_outputs:
                logits = torch.empty(TN, self.cfg.num_actions, device=self.device, dtype=torch.float32)
                vel = torch.empty(TN, self.cfg.lo_actions, device=self.device, dtype=torch.float32)
                stop = torch.empty(TN, 1, device=self.device, dtype=torch.float32)
            _lib.check(self._lib.hcm_val_step(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(), _TORCH_DT[ids.dtype],
                                              _ptr(lens), TN // N, N, ids.shape[1], oracle.data_ptr(), ca.data_ptr(), os_.data_ptr(),
                                              hh.data_ptr(), lh.data_ptr(), m.data_ptr(), result.data_ptr(), hh2.data_ptr(), lh2.data_ptr(),
                                              _ptr(logits), _ptr(vel), _ptr(stop), self._stream()), self._h)
        if return_outputs:
            return result, hh2, lh2, (logits, vel, stop)
        return result, hh2, lh2

    @staticmethod
    def check_val_result(result):
        """Host-side check of one or more val_step results ((8,) or (n,8), any device; synchronises if on the GPU): raises ValueError when a call
        saw vln_oracle_action_sensor values outside [0, num_sub_tasks] (result[6]).  Returns the results as a CPU tensor."""
        r = _EngineBase.check_val_result(result)
        bad = r[:, 6]
        if bool((bad != 0).any()):
            where = [int(i) for i in torch.nonzero(bad).reshape(-1)]
            raise ValueError(f"vln_oracle_action_sensor holds {int(bad.sum())} value(s) outside [0, num_sub_tasks] (val_step call(s) {where}): "
                             "such rows were treated as padded")
        return r

    def act(self, observations, hi_hidden, lo_hidden, masks, out=None, reuse_instruction=False, host_frames=False, gather=False):
        """reuse_instruction=True: the caller asserts that every environment's instruction is the one of the previous act() call
        (no episode ended): BERT and the instruction stream of the cross-modal block are not recomputed (hcm_act_ex).  Off in
        every parity test and in bench.py's headline number.
        host_frames=True: observations["rgb"] / ["depth"] are PINNED CPU tensors (an ObsStager's host side) and stay there: the
        library copies each to the device at the head of the encoder chain that reads it (HCM_ACT_HOST_FRAMES), overlapping the copies
        with BERT and with each other's compute; bit-identical to copying first.
        gather=True (after comm_init()): the returned record is the all-gathered (world * B, 7) record of every rank's environments, rank-major
        (hcm_act_gather: one ncclAllGather enqueued by the library behind the step).
        observations["instruction_features"] (encode_instruction's output, f32 (B or 1, L, bert_hidden)) replaces BERT; it wins over `instruction`,
        which may then be left out; `instruction_lengths` still applies.  In graph mode the stream is read IN PLACE, as the trunk features are:
        there is no static copy, the captured graph is keyed by the stream's address and row count, so keep the tensor alive and at one address
        over an episode (a new address costs one eager step and one capture)."""
        if reuse_instruction and isinstance(observations, dict) and observations.get(INSTR_KEY) is not None:
            raise ValueError(f"reuse_instruction=True together with observations[{INSTR_KEY!r}]: the flag says `keep the previous step's instruction`, "
                             "the key hands one over -- drop one of them")
        if gather and not self.comm_world:
            raise RuntimeError("act(gather=True) needs comm_init() first")
        if not gather:
            return self._act_impl(observations, hi_hidden, lo_hidden, masks, out, reuse_instruction, host_frames, False)
        # env-sharded ranks: whatever fails on THIS rank in front of the library (a malformed observation, a shape error) must not leave the peers
        # alone inside this step's all-gather -- the rank joins it with an all-NaN block (hcm_gather_poison) and raises afterwards; the peers see
        # its NaN rows and leave at the same step (rollout()).  Failures inside hcm_act_gather take the same path in the library itself.
        self._gather_called = False
        try:
            return self._act_impl(observations, hi_hidden, lo_hidden, masks, out, reuse_instruction, host_frames, True)
        except Exception:
            # did this rank's all-gather go out?  Only the library knows: hcm_act_gather returns pure argument errors (a batch beyond this engine's
            # max_batch, a communicator aborted locally) WITHOUT joining, and such a cause can be rank-local (round-5 advisor)
            joined = self._gather_called and self.query(_lib.HCM_GATHER_JOINED) == 1
            if not joined and self._gather_B and self.comm_world:
                with torch.cuda.device(self.device):
                    B = self._gather_B
                    scratch = torch.empty((1 + self.comm_world) * B, 7, device=self.device, dtype=torch.float32)
                    self._lib.hcm_gather_poison(self._h, B, scratch.data_ptr(), scratch[B:].data_ptr(), self._stream())
                    torch.cuda.current_stream().synchronize()
            raise

    def _act_impl(self, observations, hi_hidden, lo_hidden, masks, out, reuse_instruction, host_frames, gather):
        # (the per-rank batch of the collective -- every rank passes the same B -- is recorded from the VALIDATED observation of every gather call,
        #  _obs() below, so that a later call that cannot even read its observations still knows how many rows its peers expect, and a job that
        #  changes its agreed B between steps does not poison with a stale count: round-5 advisor)
        flags = (_lib.HCM_ACT_REUSE_INSTRUCTION if reuse_instruction else 0) | (_lib.HCM_ACT_HOST_FRAMES if host_frames else 0)
        if self._graph:
            cg = self._chain_graphs
            if cg == "auto":
                if host_frames:
                    # the replay enqueues the two frame copies itself, at once and outside the graphs, so they run beside BERT (B = 64: 4.87 -> 4.40 ms
                    # PCIe-inclusive); below ~4 MB a pinned host -> device copy is carried out by the calling thread behind the stream's earlier work
                    cg = min(observations["rgb"].numel() * observations["rgb"].element_size(),
                             observations["depth"].numel() * observations["depth"].element_size()) >= (4 << 20)
                else:
                    cg = obs_rows(observations) <= 2
            if cg:
                flags |= _lib.HCM_ACT_CHAIN_GRAPHS
        if self._graph:
            rec, hh2, lh2 = self._act_graph(observations, hi_hidden, lo_hidden, masks, flags, gather)
            if out is not None:
                out.copy_(rec)
                rec = out
            return rec, hh2, lh2
        with torch.cuda.device(self.device):
            rgb, depth, ids, lens, B = self._obs(observations, True, host_frames)
            if gather:
                self._gather_B = B
            hh, lh, m = self._hidden(hi_hidden, B), self._hidden(lo_hidden, B), self._mask(masks, B)
            hh2, lh2 = torch.empty_like(hh), torch.empty_like(lh)
            if gather:
                local = torch.empty(B, 7, device=self.device, dtype=torch.float32)
                rec = out if out is not None else torch.empty(self.comm_world * B, 7, device=self.device, dtype=torch.float32)
                self._gather_called = True
                _lib.check(self._lib.hcm_act_gather(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(),
                                                    _TORCH_DT[ids.dtype], _ptr(lens), B, ids.shape[1], hh.data_ptr(), lh.data_ptr(), m.data_ptr(),
                                                    local.data_ptr(), hh2.data_ptr(), lh2.data_ptr(), flags, rec.data_ptr(), self._stream()), self._h)
            else:
                rec = out if out is not None else torch.empty(B, 7, device=self.device, dtype=torch.float32)
                _lib.check(self._lib.hcm_act_ex(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), ids.data_ptr(),
                                                _TORCH_DT[ids.dtype], _ptr(lens), B, ids.shape[1], hh.data_ptr(), lh.data_ptr(), m.data_ptr(),
                                                rec.data_ptr(), hh2.data_ptr(), lh2.data_ptr(), flags, self._stream()), self._h)
            self._guard_poll(self._stream(), defer=gather)
        return rec, hh2, lh2

    def encode_instruction(self, instruction, instruction_lengths=None):
        """BERT alone (hcm_encode_instruction): instruction (rows, L) ids -> f32 (rows, L, bert_hidden) on the engine's device, the tensor the calls
        take as observations["instruction_features"] in place of the ids; zeros behind instruction_lengths[r] where lengths are given.  BERT is
        frozen and runs under no_grad in the reference (seq2seq_highlevel_cma.py:192-195), so once per episode is enough: a call fed the stream
        returns the bits of the call fed the ids when the stream was encoded at the call's own row count (include/hcm.h, hcm_instr_features), and
        agrees to the precision mode's round-off otherwise.  The values carry the engine's precision: precision="fp32" gives the stream within
        the fp32 contract (what train.HighLevel should be fed).  Invalidates a reuse_instruction cache, like every entry point but act()."""
        with torch.cuda.device(self.device):
            ids = self._dev(instruction, (torch.int64, torch.int32, torch.float32))
            if ids.dim() != 2 or not 1 <= ids.shape[0] <= self.max_batch or not 1 <= ids.shape[1] <= self.max_instr_len:
                raise ValueError(f"instruction must be (rows <= {self.max_batch}, L <= {self.max_instr_len}), got {tuple(ids.shape)}")
            rows, L = ids.shape
            lens = None
            if instruction_lengths is not None:
                lens = self._dev(instruction_lengths, (torch.int32,)).reshape(-1)
                if lens.numel() != rows:
                    raise ValueError(f"instruction_lengths must hold {rows} entries, got {lens.numel()}")
            out = torch.empty(rows, L, self.cfg.bert_hidden, device=self.device, dtype=torch.float32)
            _lib.check(self._lib.hcm_encode_instruction(self._h, ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(lens), rows, L, out.data_ptr(),
                                                        self._stream()), self._h)
        return out

    def refresh_instruction(self, instruction, env_indices, instruction_lengths=None):
        """Recompute the cached instruction stream of the listed environments (those that started a new episode) from
        `instruction` (B, L) -- same L as the cached step; afterwards act(..., reuse_instruction=True) is valid again
        (hcm_refresh_instruction)."""
        idx = np.ascontiguousarray(np.asarray(env_indices, dtype=np.int32).reshape(-1))
        with torch.cuda.device(self.device):
            ids = self._dev(instruction, (torch.int64, torch.int32, torch.float32))
            B, L = ids.shape
            lens = None if instruction_lengths is None else self._dev(instruction_lengths, (torch.int32,)).reshape(-1)
            if self._graph and self._static is not None and self._static["B"] == B and self._static["ids"].dtype == ids.dtype:
                gs = self._gstream
                gs.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(gs):
                    s_ids = self._static["ids"][:B * L].view(B, L)
                    s_ids.copy_(ids, non_blocking=True)
                    if lens is not None:
                        self._static["lens"].copy_(lens, non_blocking=True)
                        lens = self._static["lens"]
                    _lib.check(self._lib.hcm_refresh_instruction(self._h, s_ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(lens), B, L,
                                                                 idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size, C.c_void_p(gs.cuda_stream)), self._h)
                torch.cuda.current_stream().wait_stream(gs)
            else:
                _lib.check(self._lib.hcm_refresh_instruction(self._h, ids.data_ptr(), _TORCH_DT[ids.dtype], _ptr(lens), B, L,
                                                             idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size, self._stream()), self._h)


class _ModelBase:
    def __init__(self, engine: HCMEngine):
        self.engine = engine
        self.model_config = engine.cfg

    def __call__(self, batch):
        return self.forward(batch)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    @property
    def output_size(self):
        return self.engine.cfg.hidden

    @property
    def is_blind(self):
        return False

    @property
    def num_recurrent_layers(self):
        return self.engine.num_recurrent_layers


class Seq2Seq_HighLevel_CMA(_ModelBase):
    """Drop-in for robo_vln_baselines.models.seq2seq_highlevel_cma.Seq2Seq_HighLevel_CMA (inference)."""

    def forward(self, batch):
        observations, rnn_hidden_states, prev_actions, masks = batch   # prev_actions unused (use_prev_action=False)
        # RNNStateEncoder.forward dispatch (state_encoder.py:135-137): frames == hidden batch -> single step, else sequence
        # (observations["instruction_features"], the frozen BERT stream, is taken in place of the ids by both calls: HCMEngine.encode_instruction)
        if obs_rows(observations) == rnn_hidden_states.shape[1]:
            logits, hidden = self.engine.high_forward(observations, rnn_hidden_states, masks)
        else:
            logits, hidden = self.engine.high_forward_seq(observations, rnn_hidden_states, masks)
        # the reference mutates the caller's dict (seq2seq_highlevel_cma.py:196)
        if isinstance(observations, dict) and "instruction" in observations:
            del observations["instruction"]
        return logits, hidden


class Seq2Seq_LowLevel(_ModelBase):
    """Drop-in for robo_vln_baselines.models.seq2seq_lowlevel.Seq2Seq_LowLevel (inference)."""

    def forward(self, batch):
        observations, rnn_hidden_states, prev_actions, masks, discrete_actions = batch
        if obs_rows(observations) == rnn_hidden_states.shape[1]:
            return self.engine.low_forward(observations, rnn_hidden_states, masks, discrete_actions)
        return self.engine.low_forward_seq(observations, rnn_hidden_states, masks, discrete_actions)


class Policy:
    """`act()`-shaped wrapper over the fused step (the reference has no Policy class)."""

    def __init__(self, engine: HCMEngine):
        self.engine = engine
        self.high_level = Seq2Seq_HighLevel_CMA(engine)
        self.low_level = Seq2Seq_LowLevel(engine)

    def act(self, observations, hi_hidden, lo_hidden, prev_actions, masks, deterministic=True, reuse_instruction=False, host_frames=False, gather=False):
        """-> (record (B,7) = [4 sub-task logits, lin_vel, ang_vel, stop logit], hi_hidden', lo_hidden'); gather=True (env-sharded ranks, after
        engine.comm_init()): the record of ALL ranks' environments, (world * B, 7)."""
        return self.engine.act(observations, hi_hidden, lo_hidden, masks, reuse_instruction=reuse_instruction, host_frames=host_frames, gather=gather)

    def get_value(self, *a, **k):
        """Imitation-learned agent: the reference has no critic / value head anywhere."""
        return None
