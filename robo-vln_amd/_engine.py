"""What the three engines share: the ctypes helpers, the handle and its lifecycle (`_EngineBase`), and the hipGraph step of the two flat
baselines (`_FlatEngine`).  HCMEngine (policy.py), CMAEngine (cma.py) and S2SEngine (seq2seq.py) keep only what is their own."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

_TORCH_DT = {torch.float32: _lib.HCM_F32, torch.uint8: _lib.HCM_U8, torch.int32: _lib.HCM_I32, torch.int64: _lib.HCM_I64,
             "hcm_features": _lib.HCM_FEATURES, "hcm_instr_features": _lib.HCM_INSTR_FEATURES}
FEATURE_KEYS = ("rgb_features", "depth_features")       # the reference's key names (resnet_encoders.py:207-208, :83-84)
INSTR_KEY = "instruction_features"                      # the frozen BERT stream, under the name train.HighLevel reads it by


class _FeatureFrames:
    """Stands where the RGB frame tensor stands in a library call when the observations carry feature keys: data_ptr() is the address of an
    hcm_features struct (include/hcm.h) and `dtype` selects HCM_FEATURES in _TORCH_DT, so the call sites read as they do for frames.  Holds the
    tensors the struct points to."""
    dtype = "hcm_features"

    def __init__(self, rows, rgb, depth, rgb_feat, depth_feat):
        self.shape = (rows,)
        self.device = next(t for t in (*rgb_feat, *depth_feat) if t is not None).device
        self.keep = (rgb, depth, tuple(rgb_feat), tuple(depth_feat))
        st = self.struct = _lib.HcmFeaturesStruct()
        st.rgb, st.rgb_dtype, st.depth = _ptr(rgb), _TORCH_DT[rgb.dtype] if rgb is not None else _lib.HCM_F32, _ptr(depth)
        for m in range(2):
            st.rgb_feat[m], st.depth_feat[m] = _ptr(rgb_feat[m]), _ptr(depth_feat[m])

    def data_ptr(self):
        return C.addressof(self.struct)

    def pointers(self):
        """what a captured graph of the call is keyed by"""
        st = self.struct
        return (st.rgb, st.depth, st.rgb_feat[0], st.rgb_feat[1], st.depth_feat[0], st.depth_feat[1])


class _InstrStream:
    """Stands where the ids tensor stands in a library call when the observations carry `instruction_features`: data_ptr() is the address of an
    hcm_instr_features struct (include/hcm.h), `dtype` selects HCM_INSTR_FEATURES in _TORCH_DT and shape is (call rows, L), so the call sites read
    as they do for ids.  Holds the stream tensor the struct points to."""
    dtype = "hcm_instr_features"

    def __init__(self, stream, call_rows):
        self.stream = stream
        self.shape = (call_rows, stream.shape[1])
        st = self.struct = _lib.HcmInstrFeaturesStruct()
        st.stream, st.rows, st.reserved = stream.data_ptr(), stream.shape[0], 0

    def data_ptr(self):
        return C.addressof(self.struct)

    def pointers(self):
        """what a captured graph of the call is keyed by"""
        return (self.struct.stream, self.struct.rows)

    def check_envs(self, rows, N):
        """a sequence / validation call, once it knows N: the stream holds one row per frame, one for all, or one per environment"""
        if self.stream.shape[0] not in (1, N, rows):
            raise ValueError(f"{INSTR_KEY} must hold {rows} rows (one per frame), 1, or {N} (one per environment, time-major), got {self.stream.shape[0]}")


class _NoDepth:
    """the `depth` argument beside a _FeatureFrames: NULL (the depth frames travel in the struct)"""
    @staticmethod
    def data_ptr():
        return None


def _ptr(t):
    """device pointer of an optional tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


def obs_rows(observations):
    """leading dimension of an observation dict's frames, or of its feature keys when it carries no frames"""
    for k in ("rgb", "depth") + FEATURE_KEYS:
        v = observations.get(k)
        for t in (v if isinstance(v, (tuple, list)) else (v,)):
            if t is not None:
                return int(t.shape[0])
    raise KeyError("observations hold neither frames nor rgb_features / depth_features")


def _np32(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    if v.dtype == np.int64:
        return np.require(v, requirements="C"), _lib.HCM_I64          # keeps 0-d (num_batches_tracked) 0-d
    return np.require(v, dtype=np.float32, requirements="C"), _lib.HCM_F32


def _val_labels(eng, rows, hidden, corrected_actions, oracle_stop, masks, result):
    """Argument handling shared by CMAEngine.val_step and S2SEngine.val_step: the state (R,N,hidden), the labels as the trainer's collate carries
    them -- corrected_actions (rows,num_actions), oracle_stop (rows,) or (rows,1), masks (rows,) or (rows,2) -- and the caller's result row.
    -> (h_in, N, corrected, oracle_stop, masks[:,0], result), all contiguous f32 on the engine's device."""
    c = eng.cfg
    h_in = eng._dev(hidden, (torch.float32,))
    R = eng.num_recurrent_layers
    if h_in.dim() != 3 or h_in.shape[0] != R or h_in.shape[2] != c.hidden or h_in.shape[1] < 1:
        raise ValueError(f"hidden must be ({R},N,{c.hidden}), got {tuple(h_in.shape)}")
    N = h_in.shape[1]
    if rows % N:
        raise ValueError(f"{rows} frames is not a multiple of the hidden batch {N}")
    ca = eng._dev(corrected_actions, (torch.float32,))
    if tuple(ca.shape) != (rows, c.num_actions):
        raise ValueError(f"corrected_actions must be ({rows},{c.num_actions}), got {tuple(ca.shape)}")
    os_ = eng._dev(oracle_stop, (torch.float32,))
    if tuple(os_.shape) not in ((rows,), (rows, 1)):
        raise ValueError(f"oracle_stop must be ({rows},) or ({rows},1), got {tuple(os_.shape)}")
    m = eng._dev(masks, (torch.float32,))
    if tuple(m.shape) not in ((rows,), (rows, 1), (rows, 2)):
        raise ValueError(f"masks must be ({rows},) or ({rows},2), got {tuple(m.shape)}")
    m = m.reshape(rows, -1)[:, 0].contiguous()                  # masks[:,0] (cma.py:219, seq2seq.py:172)
    return h_in, N, ca, os_, m, eng._result(result)


class _EngineBase:
    """One libhcm handle (weights + workspace) on one GPU: created, loaded and finalized here, destroyed by close()."""

    def _open(self, cfg, max_batch, device, graph, create, struct, tensors):
        """`create` (the kind's hcm_*create call) on `struct`, then hcm_load_tensor of every (model id, key, value) of `tensors` -- the library
        applies load_state_dict(strict=True) semantics -- then hcm_finalize; a failure destroys the handle."""
        self._graph = bool(graph)
        self._gstream = None
        self._static = None
        self.cfg = cfg
        self.max_batch = max_batch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._lib = _lib.lib()
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, create)(C.byref(struct), C.byref(self._h)))
            try:
                for model, k, v in tensors:
                    a, dt = _np32(v)
                    shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
                    _lib.check(self._lib.hcm_load_tensor(self._h, model, k.encode(), a.ctypes.data_as(C.c_void_p), dt, shape, a.ndim), self._h)
                _lib.check(self._lib.hcm_finalize(self._h), self._h)
            except Exception:
                self._lib.hcm_destroy(self._h)
                self._h = C.c_void_p()
                raise

    def close(self):
        if self._h:
            self._lib.hcm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- observations: frames and the reference's feature keys, for all three engine kinds
    def _feat_elems(self):
        """[[rgb, depth] of slot 0 (the high-level model / a flat engine's model), [rgb, depth] of slot 1 (the low-level model)]: f32 elements per
        row of the feature that (model, modality) takes, 0 = none (hcm_query(HCM_FEAT_*))"""
        if getattr(self, "_feat_elems_", None) is None:
            self._feat_elems_ = [[self.query(_lib.HCM_FEAT_RGB_HI), self.query(_lib.HCM_FEAT_DEPTH_HI)],
                                 [self.query(_lib.HCM_FEAT_RGB_LO), self.query(_lib.HCM_FEAT_DEPTH_LO)]]
        return self._feat_elems_

    def feature_shape(self, slot, key):
        """Shape behind the leading dimension of observations[key] for model slot 0 / 1, the reference's layout: rgb_features (2048,4,4) for a
        spatial encoder and (2048,1,1) for a flat one, depth_features (C,s,s); None where that encoder takes no features."""
        mod = FEATURE_KEYS.index(key)
        n = self._feat_elems()[slot][mod]
        if not n:
            return None
        if mod == 0:
            return (2048, 4, 4) if n == 2048 * 16 else (2048, 1, 1)
        s = self.cfg.depth_final_spatial()
        return (n // (s * s), s, s)

    def _frames(self, observations, slots, frame_check, host_frames=False):
        """The frame / feature part of an observation dict for a call that runs the models of `slots` -> (rgb, depth, rows).
        Without feature keys: the frames, through frame_check(rgb, depth) (the engine's own dtype / shape rules).  With `rgb_features` /
        `depth_features` (resnet_encoders.py:207-214, :83-86): a feature replaces that model's trunk and wins over a frame given beside it, as in
        the reference; `rgb` / `depth` are read only when some model of the call has no feature for them, and may be absent otherwise.  rgb then
        comes back as a _FeatureFrames and depth as _NoDepth, which the call sites pass on like tensors.
        A key holds one tensor for the one model of the call, or a (high, low) pair -- either may be None -- when the call runs both; a single
        tensor for both is accepted for depth_features only (the two depth encoders give equal shapes; the caller vouches that the trunks are
        one, as the reference does when it hands one dict to both models) -- the two RGB encoders' features differ in shape."""
        has = [k for k in FEATURE_KEYS if observations.get(k) is not None]
        if not has:
            rgb, depth = frame_check(observations["rgb"], observations["depth"])
            return rgb, depth, rgb.shape[0]
        if host_frames:
            raise ValueError("host_frames=True cannot be combined with rgb_features / depth_features: features are device tensors "
                             "(HCM_ACT_HOST_FRAMES, include/hcm.h)")
        feats = [[None, None], [None, None]]                        # [modality][slot]
        rows = None
        for mod, key in enumerate(FEATURE_KEYS):
            v = observations.get(key)
            if v is None:
                continue
            if isinstance(v, (tuple, list)):
                if len(v) != 2:
                    raise ValueError(f"{key} must be one tensor or a (high, low) pair, got {len(v)} entries")
                per = {0: v[0], 1: v[1]}
            elif len(slots) == 1:
                per = {slots[0]: v}
            elif mod == 1:
                per = {0: v, 1: v}
            else:
                raise ValueError("rgb_features must be a (high, low) pair for a call that runs both models: the high-level encoder takes "
                                 "(rows,2048,4,4) and the low-level one (rows,2048,1,1) (resnet_encoders.py:225-236)")
            for slot in slots:
                t = per.get(slot)
                if t is None:
                    continue
                t = self._dev(t, (torch.float32,))
                want = self.feature_shape(slot, key)
                # (an encoder that takes no features -- SimpleCNN, ablated -- is refused by the library, with the reference line)
                if want is not None and (t.dim() != 4 or tuple(t.shape[1:]) != want):
                    raise ValueError(f"{key} must be (rows,{','.join(map(str, want))}) for model slot {slot}, got {tuple(t.shape)}")
                if t.dim() < 1 or (rows is not None and t.shape[0] != rows):
                    raise ValueError(f"{key}: {tuple(t.shape)} does not hold {rows} rows like the other features")
                rows = t.shape[0]
                feats[mod][slot] = t
        if rows is None:
            rgb, depth = frame_check(observations["rgb"], observations["depth"])
            return rgb, depth, rgb.shape[0]
        # frames only for the trunks that still run (a frame beside a feature is not read: the feature wins)
        need = [any(feats[mod][s] is None and self._runs_trunk(s, mod) for s in slots) for mod in range(2)]
        rgb = depth = None
        if need[0] or need[1]:
            for k, n in zip(("rgb", "depth"), need):
                if n and observations.get(k) is None:
                    raise ValueError(f"observations[{k!r}] is missing: a model of this call has no {k}_features and still runs its {k} encoder")
            # (frame_check wants both: the frame that is not needed is checked when it is there and dropped)
            r_in = observations.get("rgb") if need[0] else None
            d_in = observations.get("depth") if need[1] else None
            rgb, depth = self._check_some(frame_check, r_in, d_in, rows)
        return _FeatureFrames(rows, rgb, depth, feats[0], feats[1]), _NoDepth, rows

    def _runs_trunk(self, slot, mod):
        """does model `slot` read the rgb (mod 0) / depth (mod 1) frames: it exists and that modality is not ablated"""
        c = self.cfg
        if getattr(c, "ablate_rgb" if mod == 0 else "ablate_depth", False):
            return False
        return self._has_slot(slot)

    def _has_slot(self, slot):
        return slot == 0

    def _check_some(self, frame_check, rgb, depth, rows):
        """frame_check on the frames that are there; a missing one is replaced by an empty stand-in of the right shape for the check and dropped"""
        c = self.cfg
        dshape = tuple(c.depth_shape) if hasattr(c, "depth_shape") else (c.depth_hw, c.depth_hw)
        r = rgb if rgb is not None else torch.empty(rows, *c.rgb_shape, 3, device=self.device, dtype=torch.uint8)
        d = depth if depth is not None else torch.empty(rows, *dshape, 1, device=self.device, dtype=torch.float32)
        r2, d2 = frame_check(r, d)
        if r2.shape[0] != rows:
            raise ValueError(f"the frames hold {r2.shape[0]} rows, the features {rows}")
        return (r2 if rgb is not None else None), (d2 if depth is not None else None)

    def _no_instr_stream(self, observations):
        """the flat engines: their instruction encoder is a recurrent InstructionEncoder behind an embedding (cma.py:50-52, seq2seq.py:45-48), not BERT"""
        if observations.get(INSTR_KEY) is not None:
            raise ValueError(f"observations[{INSTR_KEY!r}] is the frozen BERT stream of the hierarchical pair's high-level model (HCMEngine); "
                             f"{type(self).__name__}'s instruction encoder is recurrent and trained, there is no such stream to take")

    def encode_features(self, observations, for_act=False):
        """The trunks alone (hcm_encode_features): observations["rgb"] / ["depth"] -> {"rgb_features": ..., "depth_features": ...} in the
        reference's layouts (resnet_encoders.py:207-214, :83-86), ready to be fed back under the same keys in place of the frames -- the calls
        then give the same bits as from the frames.  An engine with two models returns (high, low) pairs (None where an encoder takes no
        features: SimpleCNN); an ablated modality has no key.  for_act=True: the trunk launches of act(), which runs two models' unequal trunks
        as one paired network (the default reproduces every other call; the two agree to round-off, and exactly when the trunks are shared)."""
        with torch.cuda.device(self.device):
            rgb, depth = self._enc_frames(observations)
            rows = rgb.shape[0]
            out = _lib.HcmFeaturesStruct()
            slots = [s for s in (0, 1) if self._has_slot(s)]
            res = {}
            for mod, key in enumerate(FEATURE_KEYS):
                per = [None, None]
                for s in slots:
                    shape = self.feature_shape(s, key)
                    if shape is None:
                        continue
                    per[s] = torch.empty(rows, *shape, device=self.device, dtype=torch.float32)
                    (out.rgb_feat if mod == 0 else out.depth_feat)[s] = per[s].data_ptr()
                if any(t is not None for t in per):
                    res[key] = per[slots[0]] if len(slots) == 1 else tuple(per)
            if not res:
                raise ValueError("this engine has no encoder that takes features (SimpleCNN encoders / ablated modalities)")
            _lib.check(self._lib.hcm_encode_features_ex(self._h, rgb.data_ptr(), _TORCH_DT[rgb.dtype], depth.data_ptr(), rows, C.byref(out),
                                                        _lib.HCM_ENCODE_ACT if for_act else 0, self._stream()), self._h)
        return res

    def query(self, what):
        out = C.c_int64()
        with torch.cuda.device(self.device):       # (HCM_STEP_NONFINITE waits for the handle's device)
            _lib.check(self._lib.hcm_query(self._h, what, C.byref(out)), self._h)
        return out.value

    def nonfinite_steps(self):
        """Overflow guard (hcm_query(HCM_STEP_NONFINITE)): number of (sample, recurrent step) pairs since construction whose gate
        pre-activations were not all finite -- an fp16 overflow or a NaN anywhere upstream of the state encoders ends up there, and the
        squashing cell would otherwise turn it into finite garbage.  0 on a healthy engine.  Synchronises the device: call it per episode
        or per evaluation, not per step."""
        return self.query(_lib.HCM_STEP_NONFINITE)

    @property
    def num_recurrent_layers(self):
        return self.query(_lib.HCM_NUM_RECURRENT_LAYERS)

    def _dev(self, t, dtypes):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        if t.dtype not in dtypes:
            t = t.to(dtypes[0])
        return t.to(self.device, non_blocking=True).contiguous()

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _result(self, result):
        """the (8,) result row of a val_step: the caller's, checked, or a fresh one"""
        if result is None:
            return torch.empty(8, device=self.device, dtype=torch.float32)
        if (not isinstance(result, torch.Tensor) or result.dtype != torch.float32 or result.numel() != 8 or not result.is_contiguous()
                or result.device.type != self.device.type or (self.device.index is not None and result.device.index != self.device.index)):
            raise ValueError("result must be a contiguous (8,) float32 tensor on the engine's device")
        return result

    @staticmethod
    def check_val_result(result):
        """One or more val_step results ((8,) or (n,8), any device; synchronises if on the GPU) as a CPU tensor: the one read of an epoch."""
        return torch.as_tensor(result).detach().to("cpu", torch.float32).reshape(-1, 8)

    # debug taps (tests)
    def enable_taps(self, on=True):
        _lib.check(self._lib.hcm_debug_enable_taps(self._h, int(on)), self._h)

    def get_tap(self, name):
        n = C.c_int64()
        shape = (C.c_int64 * 4)()
        _lib.check(self._lib.hcm_debug_get_tap(self._h, name.encode(), None, 0, C.byref(n), shape), self._h)
        buf = np.empty(n.value, dtype=np.float32)
        _lib.check(self._lib.hcm_debug_get_tap(self._h, name.encode(), buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n), shape), self._h)
        return buf.reshape([d for d in shape if d > 0])


class _FlatEngine(_EngineBase):
    """The two flat baselines: one model per handle, forward(graph=True) through engine-owned static buffers."""

    def _state_mask(self, hidden, masks, B, N):
        """-> (rnn_hidden_states checked against (R,N,hidden), masks[:,0] of the B rows)"""
        h_in = self._dev(hidden, (torch.float32,))
        R = self.num_recurrent_layers
        if tuple(h_in.shape) != (R, N, self.cfg.hidden):
            raise ValueError(f"rnn_hidden_states must be ({R},{N},{self.cfg.hidden}), got {tuple(h_in.shape)}")
        return h_in, self._dev(masks, (torch.float32,)).reshape(B, -1)[:, 0].contiguous()      # masks[:,0] (cma.py:219, seq2seq.py:172)

    def _forward_graph(self, call, rgb, depth, ids, h_in, m, B, progress=False):
        """One step on the engine's stream with static I/O buffers, so that libhcm replays one captured hipGraph per step.
        call(rgb, depth, ids, h_in, mask, out, stop, progress, h_out, stream) makes the library call; ids is (Bi, L) with Bi = B or 1;
        progress: keep progress_hat buffers.  -> (out, stop, progress_hat or None, h_out), valid until the second-next call (ping-pong)."""
        c = self.cfg
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(device=self.device)
        st = self._static
        Bi, L = ids.shape
        feat = isinstance(rgb, _FeatureFrames)          # features are read in place: the graph is keyed by the pointers in the struct
        if st is None or st["B"] != B or st["Bi"] != Bi or st["rgb"].dtype != rgb.dtype or st["ids"].dtype != ids.dtype:
            st = {"B": B, "Bi": Bi, "tick": 0, "rgb": rgb if feat else torch.empty_like(rgb), "depth": depth if feat else torch.empty_like(depth),
                  "ids": torch.empty(Bi * c.instr_len, device=self.device, dtype=ids.dtype),
                  "mask": torch.empty_like(m), "h": [torch.zeros_like(h_in) for _ in range(2)],
                  "out": [torch.empty(B, c.num_actions, device=self.device) for _ in range(2)],
                  "stop": [torch.empty(B, 1, device=self.device) for _ in range(2)],
                  "prog": [torch.empty(B, 1, device=self.device) if progress else None for _ in range(2)]}
            self._static = st
        cur, gs = torch.cuda.current_stream(), self._gstream
        gs.wait_stream(cur)
        # observation buffers whose addresses repeat from the previous call are read in place (see HCMEngine._act_graph)
        ptrs = (rgb.pointers() if feat else (rgb.data_ptr(), depth.data_ptr())) + (ids.data_ptr(),)
        seen = st.setdefault("seen_ptrs", [])
        direct = ptrs in seen and not os.environ.get("HCM_NO_DIRECT_OBS")
        if ptrs in seen:
            seen.remove(ptrs)
        seen.append(ptrs)
        del seen[:-4]
        st["hold"] = (rgb, depth, ids)
        g_rgb, g_depth, g_ids = (rgb, depth, ids) if direct else (st["rgb"], st["depth"], st["ids"][:Bi * L].view(Bi, L))
        if feat:
            g_rgb, g_depth = rgb, depth
        with torch.cuda.stream(gs):
            i = st["tick"] & 1
            for dst, src in ((g_rgb, rgb), (g_depth, depth), (g_ids, ids), (st["mask"], m), (st["h"][1 - i], h_in)):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
            call(g_rgb, g_depth, g_ids, st["h"][1 - i], st["mask"], st["out"][i], st["stop"][i], st["prog"][i], st["h"][i], C.c_void_p(gs.cuda_stream))
            st["tick"] += 1
        cur.wait_stream(gs)
        return st["out"][i], st["stop"][i], st["prog"][i], st["h"][i]
