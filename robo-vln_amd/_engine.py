"""What the three engines share: the ctypes helpers, the handle and its lifecycle (`_EngineBase`), and the hipGraph step of the two flat
baselines (`_FlatEngine`).  HCMEngine (policy.py), CMAEngine (cma.py) and S2SEngine (seq2seq.py) keep only what is their own."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

_TORCH_DT = {torch.float32: _lib.HCM_F32, torch.uint8: _lib.HCM_U8, torch.int32: _lib.HCM_I32, torch.int64: _lib.HCM_I64}


def _ptr(t):
    """device pointer of an optional tensor (None -> NULL)"""
    return None if t is None else t.data_ptr()


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
        if st is None or st["B"] != B or st["Bi"] != Bi or st["rgb"].dtype != rgb.dtype or st["ids"].dtype != ids.dtype:
            st = {"B": B, "Bi": Bi, "tick": 0, "rgb": torch.empty_like(rgb), "depth": torch.empty_like(depth),
                  "ids": torch.empty(Bi * c.instr_len, device=self.device, dtype=ids.dtype),
                  "mask": torch.empty_like(m), "h": [torch.zeros_like(h_in) for _ in range(2)],
                  "out": [torch.empty(B, c.num_actions, device=self.device) for _ in range(2)],
                  "stop": [torch.empty(B, 1, device=self.device) for _ in range(2)],
                  "prog": [torch.empty(B, 1, device=self.device) if progress else None for _ in range(2)]}
            self._static = st
        cur, gs = torch.cuda.current_stream(), self._gstream
        gs.wait_stream(cur)
        # observation buffers whose addresses repeat from the previous call are read in place (see HCMEngine._act_graph)
        ptrs = (rgb.data_ptr(), depth.data_ptr(), ids.data_ptr())
        seen = st.setdefault("seen_ptrs", [])
        direct = ptrs in seen and not os.environ.get("HCM_NO_DIRECT_OBS")
        if ptrs in seen:
            seen.remove(ptrs)
        seen.append(ptrs)
        del seen[:-4]
        st["hold"] = (rgb, depth, ids)
        g_rgb, g_depth, g_ids = (rgb, depth, ids) if direct else (st["rgb"], st["depth"], st["ids"][:Bi * L].view(Bi, L))
        with torch.cuda.stream(gs):
            i = st["tick"] & 1
            for dst, src in ((g_rgb, rgb), (g_depth, depth), (g_ids, ids), (st["mask"], m), (st["h"][1 - i], h_in)):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
            call(g_rgb, g_depth, g_ids, st["h"][1 - i], st["mask"], st["out"][i], st["stop"][i], st["prog"][i], st["h"][i], C.c_void_p(gs.cuda_stream))
            st["tick"] += 1
        cur.wait_stream(gs)
        return st["out"][i], st["stop"][i], st["prog"][i], st["h"][i]
