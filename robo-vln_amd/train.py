"""Differentiable state encoder: the reference's RNNStateEncoder (models/decoder/state_encoder.py) with the time-serial part of forward and
backward on the HIP scan kernels (csrc/state_scan.hip, csrc/state_scan_bwd.hip).

`state_scan` is the autograd function; `RNNStateEncoder` is the drop-in module (same parameters, same state-dict keys, same argument shapes).
Device tensors go through the kernels -- hidden size 512, one layer, float32, the sizes the kernels are built for -- and anything else on
the device raises.  CPU tensors go through `cell_loop`, a pure-torch restatement (a per-step cell loop with h * mask in front of every step):
it is what the GPU tests compare against, not a fallback for a missing kernel."""
import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

SCAN_HIDDEN = 512


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


class _StateScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_ih, weight_hh, bias_ih, bias_hh, hidden_states, masks):
        H = weight_hh.shape[1]
        G = weight_hh.shape[0] // H
        if not x.is_cuda:
            raise ValueError("state_scan runs on the device; CPU tensors go through cell_loop")
        for name, t in (("weight_ih", weight_ih), ("weight_hh", weight_hh), ("bias_ih", bias_ih), ("bias_hh", bias_hh),
                        ("hidden_states", hidden_states), ("masks", masks)):
            if t.device != x.device:                 # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"state_scan: {name} is on {t.device}, x on {x.device}")
        if H != SCAN_HIDDEN or G not in (3, 4) or weight_hh.shape[0] != G * H:
            raise ValueError(f"state_scan serves hidden size {SCAN_HIDDEN} with LSTM (4) or GRU (3) gates, got weight_hh {tuple(weight_hh.shape)}")
        lstm = G == 4
        R, N = hidden_states.shape[0], hidden_states.shape[1]
        if R != (2 if lstm else 1) or x.shape[0] % N or hidden_states.shape[2] != H:
            raise ValueError(f"hidden_states {tuple(hidden_states.shape)} does not fit {x.shape[0]} rows of a one-layer {'LSTM' if lstm else 'GRU'}")
        T = x.shape[0] // N
        x, w_ih, w_hh, b_ih, b_hh, h_in = (_f32c(t) for t in (x, weight_ih, weight_hh, bias_ih, bias_hh, hidden_states))
        m = _f32c(masks).reshape(-1)
        if m.numel() != T * N:
            raise ValueError(f"masks has {m.numel()} elements for {T * N} rows")
        # the convention of include/hcm.h: LSTM adds both biases to `pre`; GRU keeps b_hh for the kernel (it sits inside r * (W_hn h + b_hn))
        pre = torch.addmm(b_ih + b_hh if lstm else b_ih, x, w_ih.t())
        seq = torch.empty(T * N, H, device=x.device)
        h_out = torch.empty_like(h_in)
        gates = torch.empty(T * N, 4 * H, device=x.device)
        c_seq = torch.empty(T * N, H, device=x.device) if lstm else None
        work = torch.empty(4 * H * H, device=x.device)
        _lib.check(_lib.lib().hcm_op_state_scan_train(_ptr(pre), _ptr(w_hh), None if lstm else _ptr(b_hh), _ptr(h_in), _ptr(m), _ptr(seq), _ptr(h_out),
                                                      _ptr(gates), _ptr(c_seq), _ptr(work), T, N, H, _lib.HCM_LSTM if lstm else _lib.HCM_GRU, _stream()))
        ctx.save_for_backward(x, w_ih, w_hh, h_in, m, seq, gates, c_seq)
        ctx.dims = (T, N, H, lstm)
        ctx.mark_non_differentiable(h_out)
        return seq, h_out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_seq, _d_h_out):
        x, w_ih, w_hh, h_in, m, seq, gates, c_seq = ctx.saved_tensors
        T, N, H, lstm = ctx.dims
        G = 4 if lstm else 3
        d_seq = _f32c(d_seq)
        d_pre = torch.empty(T * N, G * H, device=x.device)
        d_gh = None if lstm else torch.empty(T * N, G * H, device=x.device)
        d_h_in = torch.empty_like(h_in)
        work = torch.empty(4 * H * H + 4 * N * H, device=x.device)
        _lib.check(_lib.lib().hcm_op_state_scan_bwd(_ptr(d_seq), _ptr(gates), _ptr(c_seq), _ptr(seq), _ptr(h_in), _ptr(m), _ptr(w_hh), _ptr(work),
                                                    _ptr(d_pre), _ptr(d_gh), _ptr(d_h_in), T, N, H, _lib.HCM_LSTM if lstm else _lib.HCM_GRU, _stream()))
        if lstm:
            d_gh = d_pre
        need = ctx.needs_input_grad
        h_prev = torch.cat([h_in[0], seq[:-N]], 0) * m[:, None] if T > 1 else h_in[0] * m[:, None]
        dx = d_pre @ w_ih if need[0] else None
        dw_ih = d_pre.t() @ x if need[1] else None
        dw_hh = d_gh.t() @ h_prev if need[2] else None
        db_ih = d_pre.sum(0) if need[3] else None
        db_hh = d_gh.sum(0) if need[4] else None
        return dx, dw_ih, dw_hh, db_ih, db_hh, (d_h_in if need[5] else None), None


def state_scan(x, weight_ih, weight_hh, bias_ih, bias_hh, hidden_states, masks):
    """T masked steps of a one-layer nn.LSTM / nn.GRU (hidden 512, float32, on the device) with gradients: x (T*N, in), torch's parameter
    tensors, hidden_states packed (R, N, 512) with R = 2 (h, c) for LSTM / 1 for GRU, masks (T*N,) multiplied onto the state in front of every
    step.  Returns (seq (T*N, 512), hidden_out (R, N, 512)); hidden_out is non-differentiable, as the reference detaches it
    (state_encoder.py:131) and the trainers detach the state they carry.  LSTM or GRU is read off weight_hh's row count.

    Forward: `pre` by torch.addmm, then hcm_op_state_scan_train, one launch per step on the current stream.  Backward: hcm_op_state_scan_bwd,
    one launch per step in reverse, gives d_pre, d_gh and d_h_in; the batched reductions behind it -- dx = d_pre @ W_ih, dW_ih = d_pre.T @ x,
    db_ih = d_pre.sum(0), dW_hh = d_gh.T @ h', db_hh = d_gh.sum(0), with h' = cat(h_in[0], seq[:-N]) * masks[:, None] and d_gh = d_pre for
    LSTM -- are dense float32 GEMMs and sums over all rows, not the serial path, and stay in torch.  Nothing is cached between calls: the
    weights are packed for the kernels on the device in every call."""
    return _StateScan.apply(x, weight_ih, weight_hh, bias_ih, bias_hh, hidden_states, masks)


def cell_loop(x, params, hidden_states, masks, rnn_type):
    """Pure-torch restatement for any size, layer count and dtype: a per-step cell loop with h * mask (and c * mask) in front of every step.
    params: per layer (weight_ih, weight_hh, bias_ih, bias_hh); hidden_states packed (R, N, H) as the reference packs it (LSTM: the h of every
    layer, then the c of every layer).  Returns (seq (T*N, H), hidden_out (R, N, H), detached)."""
    lstm = rnn_type == "LSTM"
    L = len(params)
    N = hidden_states.shape[1]
    T = x.shape[0] // N
    m = masks.reshape(T, N, 1).to(x.dtype)
    h = [hidden_states[l] for l in range(L)]
    c = [hidden_states[L + l] for l in range(L)] if lstm else None
    out = []
    for t in range(T):
        inp = x[t * N:(t + 1) * N]
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
            hp = h[l] * m[t]
            gi = torch.nn.functional.linear(inp, w_ih, b_ih)
            gh = torch.nn.functional.linear(hp, w_hh, b_hh)
            if lstm:
                i, f, g, o = (gi + gh).chunk(4, 1)
                c[l] = torch.sigmoid(f) * (c[l] * m[t]) + torch.sigmoid(i) * torch.tanh(g)
                h[l] = torch.sigmoid(o) * torch.tanh(c[l])
            else:
                i_r, i_z, i_n = gi.chunk(3, 1)
                h_r, h_z, h_n = gh.chunk(3, 1)
                r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
                n = torch.tanh(i_n + r * h_n)
                h[l] = (1 - z) * n + z * hp
            inp = h[l]
        out.append(inp)
    return torch.cat(out, 0), torch.stack(h + c if lstm else h, 0).detach()


class RNNStateEncoder(nn.Module):
    """Drop-in for the reference's RNNStateEncoder: parameters under rnn.weight_ih_l0 / rnn.weight_hh_l0 / rnn.bias_ih_l0 / rnn.bias_hh_l0 in
    a real nn.GRU / nn.LSTM (storage and initialisation only: orthogonal weights, zero biases), so load_state_dict takes a reference
    checkpoint's keys unchanged.  Unlike the reference's, seq_forward also serves LSTM."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, rnn_type: str = "GRU"):
        super().__init__()
        if rnn_type not in ("GRU", "LSTM"):
            raise ValueError(f"rnn_type must be GRU or LSTM, got {rnn_type!r}")
        self._num_recurrent_layers = num_layers
        self._rnn_type = rnn_type
        self._hidden_size = hidden_size
        self.rnn = getattr(nn, rnn_type)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.layer_init()

    def layer_init(self):
        for name, param in self.rnn.named_parameters():
            if "weight" in name:
                nn.init.orthogonal_(param)
            elif "bias" in name:
                nn.init.constant_(param, 0)

    @property
    def num_recurrent_layers(self):
        return self._num_recurrent_layers * (2 if "LSTM" in self._rnn_type else 1)

    def _params(self):
        return [tuple(getattr(self.rnn, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for l in range(self._num_recurrent_layers)]

    def _run(self, x, hidden_states, masks):
        masks = masks.reshape(-1)
        if not x.is_cuda:
            return cell_loop(x, self._params(), hidden_states, masks, self._rnn_type)
        if self._hidden_size != SCAN_HIDDEN or self._num_recurrent_layers != 1:
            raise ValueError(f"on the device RNNStateEncoder serves hidden_size {SCAN_HIDDEN} with one layer "
                             f"(got hidden_size {self._hidden_size}, num_layers {self._num_recurrent_layers})")
        return state_scan(x, *self._params()[0], hidden_states, masks)

    def single_forward(self, x, hidden_states, masks):
        """x (N, in), hidden_states (R, N, H), masks (N,) or (N, 1): one step (T = 1)"""
        if x.size(0) != hidden_states.size(1):
            raise ValueError(f"single_forward takes one row per state, got {x.size(0)} rows for {hidden_states.size(1)} states")
        return self._run(x, hidden_states, masks)

    def seq_forward(self, x, hidden_states, masks):
        """x (T*N, in) flattened from (T, N, in), hidden_states (R, N, H), masks (T*N,) or (T*N, 1)"""
        if x.size(0) % hidden_states.size(1):
            raise ValueError(f"{x.size(0)} rows are not a whole number of steps of {hidden_states.size(1)} states")
        return self._run(x, hidden_states, masks)

    def forward(self, x, hidden_states, masks):
        if x.size(0) == hidden_states.size(1):
            return self.single_forward(x, hidden_states, masks)
        return self.seq_forward(x, hidden_states, masks)
