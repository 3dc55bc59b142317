"""Differentiable state encoder: the reference's RNNStateEncoder (models/decoder/state_encoder.py) with the time-serial part of forward and
backward on the HIP scan kernels (csrc/state_scan.hip, csrc/state_scan_bwd.hip).

`state_scan` is the autograd function; `RNNStateEncoder` is the drop-in module (same parameters, same state-dict keys, same argument shapes).
Device tensors go through the kernels -- hidden size 512, one layer, float32, the sizes the kernels are built for -- and anything else on
the device raises.  CPU tensors go through `cell_loop`, a pure-torch restatement (a per-step cell loop with h * mask in front of every step):
it is what the GPU tests compare against, not a fallback for a missing kernel.

Differentiable cross-modal layer: the reference's InterModuleAttnLayer (models/transformer/transformer.py:209-221) with everything behind the
three projections -- attention, fc_o, dropout, LayerNorm, the feed-forward block, dropout, LayerNorm -- on the float32 HIP kernels of
csrc/vla_train.hip, forward and backward.  `vla_layer` is the autograd function, `InterModuleAttnLayer` the drop-in module, `vla_layer_ref` the
pure-torch restatement (CPU path of the module, and what the tests compare against).

Differentiable Visual_Ling_Attn: the reference's whole cross-modal encoder (transformer.py:250-282).  Its prologue -- Linear, ReLU, dropout, the
shared LayerNorm, and for the instruction half the sinusoid table -- is `embed_ln` on the float32 HIP kernels of csrc/embed_train.hip, one launch
forward and one backward per half; `embed_ln_ref` is the pure-torch restatement, `sinusoid_table` the reference's table, `Visual_Ling_Attn` the
drop-in module around `InterModuleAttnLayer`.

Differentiable instruction encoder: the reference's InstructionEncoder (models/encoders/instruction_encoder.py:70-92), a packed nn.LSTM / nn.GRU
with hidden size 256 in one or two directions, with the whole scan forward and the whole scan backward one launch each (csrc/instr_scan.hip)
and the lengths read on the device.  `instr_scan` is the autograd function, `instr_encoder_ref` the pure-torch restatement, `InstructionEncoder`
the drop-in module.

Differentiable CMANet: the reference's flat baseline (models/cma.py) from cached trunk features.  Its attention stage (cma.py:271-311) has one query
per sample and keys that are a 1x1 convolution of the raw tokens, so the key projection folds into the query (qt = q W_k; q.b_k cancels in the
softmax) and K and V are never formed: `attn1q` is the autograd function over csrc/cma_attn_train.hip, `attn1q_ref` the pure-torch restatement,
`CMANet` the trainable model around it, `InstructionEncoder` and two `RNNStateEncoder`s.

The flat trainer's update step: the reference's `_update_agent` (robo_vln_trainer.py:505-542).  Its end -- `linear`, `stop_linear`,
tanh(`progress_monitor`) and the masked criteria -- is `flat_heads_loss`, the autograd function over csrc/flat_heads_train.hip (two launches forward,
two backward), with `flat_heads_loss_ref` the pure-torch restatement; `Seq2SeqNet` is the second flat baseline (models/seq2seq.py) as a trainable
model from cached trunk features, both models have `update_loss`, and `flat_update` is `_update_agent` around it.

The hierarchical trainer's update step: the reference's `_update_agent` (hierarchical_trainer.py:492-560).  The high-level criterion -- `linear`,
masked_fill_, CrossEntropyLoss(ignore_index=-1) -- is `subtask_ce`, the autograd function over csrc/subtask_ce_train.hip (two launches forward, two
backward), with `subtask_ce_ref` the pure-torch restatement; `HighLevel` (models/seq2seq_highlevel_cma.py, the frozen BERT's output entering as a
tensor) and `LowLevel` (models/seq2seq_lowlevel.py, its heads on `flat_heads_loss`) are the pair as trainable models from cached trunk features,
and `hier_update` is `_update_agent` around them."""
import ctypes as C
import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

SCAN_HIDDEN = 512
INSTR_HIDDEN = 256
VLA_D_MODEL, VLA_HEADS, VLA_MAX_KEYS, VLA_MAX_D_FF = 256, 4, 64, 1024
EMBED_K_STEP, EMBED_MAX_K = 64, 1024


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


def mask_dropout(x, keep, p):
    """Dropout with the keep mask given: x * keep / (1 - p); keep None = identity.  keep has x's element count (the kernels take it as (rows, n))."""
    return x if keep is None else x * keep.reshape(x.shape).to(x.dtype) / (1.0 - p)


def vla_attention_ref(q, I, kv, wo, bo, g1, be1, keep1=None, p=0.0, heads=VLA_HEADS):
    """The first half of vla_layer_ref, MultiHeadAttention behind its projections (transformer.py:111-126): x1 = LN1(I + dropout(fc_o(attention)))"""
    B, L, _ = q.shape
    Lk = kv.shape[1]
    d_k = q.shape[2] // heads
    qh = q.reshape(B, L, heads, d_k).permute(0, 2, 1, 3)
    kh = kv[..., :heads * d_k].reshape(B, Lk, heads, d_k).permute(0, 2, 3, 1)
    vh = kv[..., heads * d_k:].reshape(B, Lk, heads, -1).permute(0, 2, 1, 3)
    att = torch.softmax(torch.matmul(qh, kh) / math.sqrt(d_k), -1)
    a = torch.matmul(att, vh).permute(0, 2, 1, 3).reshape(B, L, -1)
    u = torch.nn.functional.linear(a, wo, bo)
    return torch.nn.functional.layer_norm(I + mask_dropout(u, keep1, p), I.shape[-1:], g1, be1, 1e-5)


def vla_layer_ref(q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, keep=None, p=0.0, heads=VLA_HEADS):
    """Pure-torch restatement of the layer behind its projections, any dtype, CPU or device: q = fc_q(input_1) (B, L, h*d_k), I = input_1
    (B, L, d_model), kv = fc_k(input_2) | fc_v(input_2) (B, Lk, h*d_k + h*d_v); keep = None or the three keep masks of the dropouts behind
    fc_o, behind the ReLU and behind fc2 (element counts B*L*d_model, B*L*d_ff, B*L*d_model), p the dropout probability they were drawn with.
    MultiHeadAttention (vla_attention_ref) and PositionWiseFeedForward (transformer.py:25-43)."""
    k1, k2, k3 = keep if keep is not None else (None, None, None)
    x1 = vla_attention_ref(q, I, kv, wo, bo, g1, be1, k1, p, heads)
    h = mask_dropout(torch.relu(torch.nn.functional.linear(x1, w1, b1)), k2, p)
    z = torch.nn.functional.linear(h, w2, b2)
    return torch.nn.functional.layer_norm(x1 + mask_dropout(z, k3, p), I.shape[-1:], g2, be2, 1e-5)


class _VlaLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, keep1, keep2, keep3, p):
        if not q.is_cuda:
            raise ValueError("vla_layer runs on the device; CPU tensors go through vla_layer_ref")
        named = (("I", I), ("kv", kv), ("wo", wo), ("bo", bo), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("g1", g1), ("be1", be1),
                 ("g2", g2), ("be2", be2), ("keep[0]", keep1), ("keep[1]", keep2), ("keep[2]", keep3))
        for name, t in named:
            if t is not None and t.device != q.device:    # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"vla_layer: {name} is on {t.device}, q on {q.device}")
        D = VLA_D_MODEL
        if q.dim() != 3 or q.shape[2] != D or I.shape != q.shape or kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * D:
            raise ValueError(f"vla_layer serves q, I (B, L, {D}) and kv (B, Lk, {2 * D}), got {tuple(q.shape)}, {tuple(I.shape)}, {tuple(kv.shape)}")
        B, L, Lk, d_ff = q.shape[0], q.shape[1], kv.shape[1], w1.shape[0]
        if B < 1 or L < 1 or not 1 <= Lk <= VLA_MAX_KEYS or d_ff % 256 or not 256 <= d_ff <= VLA_MAX_D_FF:
            raise ValueError(f"vla_layer serves B, L >= 1, 1..{VLA_MAX_KEYS} keys and d_ff a multiple of 256 up to {VLA_MAX_D_FF}, got B {B}, L {L}, Lk {Lk}, d_ff {d_ff}")
        for name, t, shape in (("wo", wo, (D, D)), ("bo", bo, (D,)), ("w1", w1, (d_ff, D)), ("b1", b1, (d_ff,)), ("w2", w2, (D, d_ff)), ("b2", b2, (D,)),
                               ("g1", g1, (D,)), ("be1", be1, (D,)), ("g2", g2, (D,)), ("be2", be2, (D,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"vla_layer: {name} has shape {tuple(t.shape)}, expected {shape}")
        if not 0.0 <= p < 1.0:
            raise ValueError(f"vla_layer: p must be in [0, 1), got {p}")
        rows = B * L
        keeps = []
        for name, t, n in (("keep[0]", keep1, D), ("keep[1]", keep2, d_ff), ("keep[2]", keep3, D)):
            if t is not None and (t.dtype != torch.uint8 or t.numel() != rows * n):
                raise ValueError(f"vla_layer: {name} must be uint8 with {rows} x {n} elements, got {t.dtype} {tuple(t.shape)}")
            keeps.append(None if t is None else t.contiguous())
        q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = (_f32c(t) for t in (q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2))
        dev = q.device
        out, a, x1, x1hat, x2hat = (torch.empty(B, L, D, device=dev) for _ in range(5))
        h = torch.empty(rows, d_ff, device=dev)
        rstd = torch.empty(rows, 2, device=dev)
        work = torch.empty(_lib.lib().hcm_op_vla_train_work_floats(B, L, Lk, d_ff), device=dev)
        _lib.check(_lib.lib().hcm_op_vla_layer_train(_ptr(q), _ptr(I), _ptr(kv), _ptr(wo), _ptr(bo), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(g1),
                                                     _ptr(be1), _ptr(g2), _ptr(be2), _ptr(keeps[0]), _ptr(keeps[1]), _ptr(keeps[2]), p, _ptr(out), _ptr(a),
                                                     _ptr(x1), _ptr(x1hat), _ptr(h), _ptr(x2hat), _ptr(rstd), _ptr(work), B, L, Lk, d_ff, _stream()))
        ctx.save_for_backward(q, kv, wo, w1, w2, g1, g2, a, x1, x1hat, h, x2hat, rstd, *keeps)
        ctx.dims = (B, L, Lk, d_ff, p)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        q, kv, wo, w1, w2, g1, g2, a, x1, x1hat, h, x2hat, rstd, keep1, keep2, keep3 = ctx.saved_tensors
        B, L, Lk, d_ff, p = ctx.dims
        D, rows, dev = VLA_D_MODEL, B * L, q.device
        d_out = _f32c(d_out)
        d_q, d_I = torch.empty_like(q), torch.empty_like(q)
        d_kv = torch.empty_like(kv)
        d_u, d_z = torch.empty(rows, D, device=dev), torch.empty(rows, D, device=dev)
        d_hpre = torch.empty(rows, d_ff, device=dev)
        d_ln = torch.empty(4, D, device=dev)
        work = torch.empty(_lib.lib().hcm_op_vla_train_work_floats(B, L, Lk, d_ff), device=dev)
        _lib.check(_lib.lib().hcm_op_vla_layer_bwd(_ptr(d_out), _ptr(q), _ptr(kv), _ptr(wo), _ptr(w1), _ptr(w2), _ptr(g1), _ptr(g2), _ptr(keep1), _ptr(keep2),
                                                   _ptr(keep3), p, _ptr(x1hat), _ptr(h), _ptr(x2hat), _ptr(rstd), _ptr(work), _ptr(d_q), _ptr(d_I), _ptr(d_kv),
                                                   _ptr(d_u), _ptr(d_hpre), _ptr(d_z), _ptr(d_ln), B, L, Lk, d_ff, _stream()))
        need = ctx.needs_input_grad
        return (d_q if need[0] else None, d_I if need[1] else None, d_kv if need[2] else None,
                d_u.t() @ a.reshape(rows, D) if need[3] else None, d_u.sum(0) if need[4] else None,
                d_hpre.t() @ x1.reshape(rows, D) if need[5] else None, d_hpre.sum(0) if need[6] else None,
                d_z.t() @ h if need[7] else None, d_z.sum(0) if need[8] else None,
                d_ln[0] if need[9] else None, d_ln[1] if need[10] else None, d_ln[2] if need[11] else None, d_ln[3] if need[12] else None,
                None, None, None, None)


def vla_layer(q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, keep=None, p=0.0):
    """The cross-modal layer behind its three projections (float32, on the device) with gradients to the first thirteen arguments: arguments as
    vla_layer_ref; d_model 256, 4 heads of 64, 1..64 keys, d_ff a multiple of 256 up to 1024, any B, L >= 1; keep = None or three uint8 keep masks.

    Forward: hcm_op_vla_layer_train (weight pack, attention, one fused launch for the rest) saves a, x1, h, the two normalised rows and their
    reciprocal standard deviations.  Backward: hcm_op_vla_layer_bwd gives d_q, d_I, d_kv, the four LayerNorm parameter gradients and the row-local
    d_u, d_hpre, d_z; the dense reductions over all rows -- dWo = d_u.T @ a, dW1 = d_hpre.T @ x1, dW2 = d_z.T @ h and the three bias column
    sums -- stay in torch, the split state_scan's backward made.  Nothing is cached between calls: the weights are packed for the kernels on the
    device in every call."""
    k1, k2, k3 = keep if keep is not None else (None, None, None)
    return _VlaLayer.apply(q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, k1, k2, k3, float(p))


class _ScaledDotProductAttention(nn.Module):
    """Parameters and initialisation of the reference's ScaledDotProductAttention (transformer.py:46-79): xavier_normal_ weights, zero biases"""

    def __init__(self, d_model, d_k, d_v, h):
        super().__init__()
        self.fc_q = nn.Linear(d_model, h * d_k)
        self.fc_k = nn.Linear(d_model, h * d_k)
        self.fc_v = nn.Linear(d_model, h * d_v)
        self.fc_o = nn.Linear(h * d_v, d_model)
        for fc in (self.fc_q, self.fc_k, self.fc_v, self.fc_o):
            nn.init.xavier_normal_(fc.weight, gain=1.0)
        for fc in (self.fc_q, self.fc_k, self.fc_v, self.fc_o):
            nn.init.constant_(fc.bias, 0)


class _MultiHeadAttention(nn.Module):
    def __init__(self, d_model, d_k, d_v, h):
        super().__init__()
        self.attention = _ScaledDotProductAttention(d_model, d_k, d_v, h)
        self.layer_norm = nn.LayerNorm(d_model)


class _PositionWiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff):
        super().__init__()
        self.fc1 = nn.Linear(d_model, d_ff)
        self.fc2 = nn.Linear(d_ff, d_model)
        self.layer_norm = nn.LayerNorm(d_model)


class InterModuleAttnLayer(nn.Module):
    """Drop-in for the reference's InterModuleAttnLayer (transformer.py:209-221): the same sixteen state-dict keys (enc_att.attention.fc_{q,k,v,o},
    enc_att.layer_norm, pwff.fc1, pwff.fc2, pwff.layer_norm), the same initialisation and forward signature.  fc_q / fc_k / fc_v are ordinary
    nn.Linear through torch autograd; everything behind them is vla_layer on the device and vla_layer_ref on the CPU.  In train mode with
    dropout > 0 the three keep masks are drawn with torch's generator on the input's device (draw_keep), so torch.manual_seed governs them."""

    def __init__(self, d_model=256, d_k=64, d_v=64, h=4, d_ff=1024, dropout=.1):
        super().__init__()
        self.enc_att = _MultiHeadAttention(d_model, d_k, d_v, h)
        self.pwff = _PositionWiseFeedForward(d_model, d_ff)
        self.d_model, self.d_k, self.d_v, self.h, self.d_ff, self.dropout = d_model, d_k, d_v, h, d_ff, float(dropout)

    def draw_keep(self, rows, device):
        """The three uint8 keep masks of one call: (rows, d_model), (rows, d_ff), (rows, d_model), each element kept with probability 1 - dropout"""
        return tuple((torch.rand(rows, n, device=device) >= self.dropout).to(torch.uint8) for n in (self.d_model, self.d_ff, self.d_model))

    def forward(self, input_1, input_2, mask_self_att, mask_enc_att, pos_embed=None, _keep=None):
        if mask_enc_att is not None:
            raise ValueError("InterModuleAttnLayer serves mask_enc_att = None, as the high-level model calls it (seq2seq_highlevel_cma.py:200-201)")
        att, ln1, ff = self.enc_att.attention, self.enc_att.layer_norm, self.pwff
        p = self.dropout if self.training else 0.0
        keep = _keep
        if keep is None and p > 0:
            keep = self.draw_keep(input_1.shape[0] * input_1.shape[1], input_1.device)
        q = att.fc_q(input_1)
        kv = torch.cat([att.fc_k(input_2), att.fc_v(input_2)], -1)
        args = (q, input_1, kv, att.fc_o.weight, att.fc_o.bias, ff.fc1.weight, ff.fc1.bias, ff.fc2.weight, ff.fc2.bias,
                ln1.weight, ln1.bias, ff.layer_norm.weight, ff.layer_norm.bias)
        if not input_1.is_cuda:
            return vla_layer_ref(*args, keep=keep, p=p, heads=self.h)
        if (self.d_model, self.d_k, self.d_v, self.h) != (VLA_D_MODEL, 64, 64, VLA_HEADS) or self.d_ff % 256 or not 256 <= self.d_ff <= VLA_MAX_D_FF:
            raise ValueError(f"on the device InterModuleAttnLayer serves d_model {VLA_D_MODEL}, {VLA_HEADS} heads of 64 and d_ff a multiple of 256 up to "
                             f"{VLA_MAX_D_FF} (got d_model {self.d_model}, d_k {self.d_k}, d_v {self.d_v}, h {self.h}, d_ff {self.d_ff})")
        return vla_layer(*args, keep=keep, p=p)


def sinusoid_table(L, d):
    """The reference's sinusoid_encoding_table(L, d) (common/utils.py:167-185): float32 on the CPU, by the reference's own expression"""
    pos = torch.arange(L, dtype=torch.float32).view(-1, 1)
    dim = torch.arange(d // 2, dtype=torch.float32).view(1, -1)
    out = torch.zeros((L, d))
    out[:, ::2] = torch.sin(pos / 10000 ** (2 * dim / d))
    out[:, 1::2] = torch.cos(pos / 10000 ** (2 * dim / d))
    return out


def embed_ln_ref(x, w, b, gamma, beta, keep=None, p=0.0, post=None):
    """Pure-torch restatement of one half of Visual_Ling_Attn's prologue, any width, dtype and device: LayerNorm(dropout(relu(x W^T + b))) with
    the dropout's keep mask given (None = no dropout), plus post[row % period] for an additive table post (period, width), rows counted over
    all leading dimensions of x."""
    r = mask_dropout(torch.relu(torch.nn.functional.linear(x, w, b)), keep, p)
    y = torch.nn.functional.layer_norm(r, r.shape[-1:], gamma, beta, 1e-5)
    if post is not None:
        rows = y.numel() // y.shape[-1]
        y = y + post[torch.arange(rows, device=post.device) % post.shape[0]].reshape(y.shape)
    return y


def embed_k_ok(K):
    return EMBED_K_STEP <= K <= EMBED_MAX_K and K % EMBED_K_STEP == 0


class _EmbedLn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, keep, p, post):
        if not x.is_cuda:
            raise ValueError("embed_ln runs on the device; CPU tensors go through embed_ln_ref")
        for name, t in (("w", w), ("b", b), ("gamma", gamma), ("beta", beta), ("keep", keep), ("post", post)):
            if t is not None and t.device != x.device:    # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"embed_ln: {name} is on {t.device}, x on {x.device}")
        D, K = VLA_D_MODEL, x.shape[-1] if x.dim() else 0
        if x.dim() < 2 or not embed_k_ok(K):
            raise ValueError(f"embed_ln serves x (..., K) with K a multiple of {EMBED_K_STEP} from {EMBED_K_STEP} to {EMBED_MAX_K}, got {tuple(x.shape)}")
        for name, t, shape in (("w", w, (D, K)), ("b", b, (D,)), ("gamma", gamma, (D,)), ("beta", beta, (D,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"embed_ln: {name} has shape {tuple(t.shape)}, expected {shape}")
        if not 0.0 <= p < 1.0:
            raise ValueError(f"embed_ln: p must be in [0, 1), got {p}")
        rows = x.numel() // K
        if keep is not None and (keep.dtype != torch.uint8 or keep.numel() != rows * D):
            raise ValueError(f"embed_ln: keep must be uint8 with {rows} x {D} elements, got {keep.dtype} {tuple(keep.shape)}")
        if post is not None and (post.dim() != 2 or post.shape[0] < 1 or post.shape[1] != D):
            raise ValueError(f"embed_ln: post must be (period >= 1, {D}), got {tuple(post.shape)}")
        if keep is None:
            p = 0.0                                       # no mask, no scaling: the backward's s must be 1 as well
        x2, w, b, gamma, beta = (_f32c(t) for t in (x.reshape(rows, K), w, b, gamma, beta))
        keep = None if keep is None else keep.contiguous()
        post = None if post is None else _f32c(post)
        dev = x.device
        y, xhat = torch.empty(rows, D, device=dev), torch.empty(rows, D, device=dev)
        rstd = torch.empty(rows, device=dev)
        gate = torch.empty(rows, D, dtype=torch.uint8, device=dev)
        work = torch.empty(_lib.lib().hcm_op_embed_ln_work_floats(rows, K), device=dev)
        _lib.check(_lib.lib().hcm_op_embed_ln_train(_ptr(x2), _ptr(w), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(keep), p, _ptr(post),
                                                    post.shape[0] if post is not None else 0, _ptr(y), _ptr(xhat), _ptr(rstd), _ptr(gate), _ptr(work),
                                                    rows, K, _stream()))
        ctx.save_for_backward(x2, w, gamma, xhat, rstd, gate)
        ctx.dims = (rows, K, p, tuple(x.shape))
        return y.reshape(*x.shape[:-1], D)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x2, w, gamma, xhat, rstd, gate = ctx.saved_tensors
        rows, K, p, shape = ctx.dims
        D, dev = VLA_D_MODEL, x2.device
        need = ctx.needs_input_grad
        d_y = _f32c(d_y).reshape(rows, D)
        d_pre = torch.empty(rows, D, device=dev)
        d_x = torch.empty(rows, K, device=dev) if need[0] else None
        d_ln = torch.empty(2, D, device=dev)
        work = torch.empty(_lib.lib().hcm_op_embed_ln_work_floats(rows, K), device=dev)
        _lib.check(_lib.lib().hcm_op_embed_ln_bwd(_ptr(d_y), _ptr(w), _ptr(gamma), _ptr(xhat), _ptr(rstd), _ptr(gate), p, _ptr(work), _ptr(d_pre),
                                                  _ptr(d_x), _ptr(d_ln), rows, K, _stream()))
        return (d_x.reshape(shape) if need[0] else None, d_pre.t() @ x2 if need[1] else None, d_pre.sum(0) if need[2] else None,
                d_ln[0] if need[3] else None, d_ln[1] if need[4] else None, None, None, None)


def embed_ln(x, w, b, gamma, beta, keep=None, p=0.0, post=None):
    """One half of Visual_Ling_Attn's prologue (float32, on the device) with gradients to x, w, b, gamma, beta: arguments as embed_ln_ref; x
    (..., K) with K a multiple of 64 from 64 to 1024, w (256, K), keep None or a uint8 keep mask with rows x 256 elements, post None or a
    (period, 256) table added behind the LayerNorm.

    Forward: hcm_op_embed_ln_train (weight pack and one fused launch) saves the normalised rows, their reciprocal standard deviations and one
    gate byte per element.  Backward: hcm_op_embed_ln_bwd gives the row-local d_pre, the two LayerNorm parameter gradients, and d_x = d_pre W
    only when x requires a gradient; dW = d_pre.T @ x and db = d_pre.sum(0) are dense reductions over all rows and stay in torch, the split
    vla_layer's backward made.  Nothing is cached between calls."""
    return _EmbedLn.apply(x, w, b, gamma, beta, keep, float(p), post)


class Visual_Ling_Attn(nn.Module):
    """Drop-in for the reference's Visual_Ling_Attn (transformer.py:250-282), `image_cm_encoder` of the high-level model: the reference's state-dict
    keys (layers.{i}.<the sixteen keys of InterModuleAttnLayer>, vis_fc.*, ins_fc.*, layer_norm.*), initialisation and forward signature.  Takes the
    reference's config object (N, vis_in_features, ins_in_features, d_model, h, d_ff, dropout) or the same names as keyword arguments, which win.

    Both prologue halves are embed_ln on the device and embed_ln_ref on the CPU; one layer_norm serves both, and its gradient accumulates
    through autograd.  The sinusoid table is kept per (L, device) in the plain dict `_tables` -- no buffer, not in the state dict -- so the device
    path copies nothing per call.  In train mode with dropout > 0 the keep masks are drawn by draw_keep with torch's generator on the input's
    device, in the order vis half, ins half, then each layer's three, so torch.manual_seed governs them; `_keep` takes them explicitly."""

    def __init__(self, config=None, **kw):
        super().__init__()
        names = ("N", "vis_in_features", "ins_in_features", "d_model", "h", "d_ff", "dropout")
        unknown = set(kw) - set(names)
        if unknown:
            raise TypeError(f"Visual_Ling_Attn: unknown arguments {sorted(unknown)}")
        missing = [n for n in names if n not in kw and not hasattr(config, n)]
        if missing:
            raise TypeError(f"Visual_Ling_Attn: missing {missing}")
        N, vis_in, ins_in, d_model, h, d_ff, dropout = (kw[n] if n in kw else getattr(config, n) for n in names)
        self.d_model, self.d_att, self.p = d_model, int(d_model / h), float(dropout)
        self.layers = nn.ModuleList([InterModuleAttnLayer(d_model, self.d_att, self.d_att, h, d_ff, dropout) for _ in range(N)])
        self.vis_fc = nn.Linear(vis_in, d_model)
        self.ins_fc = nn.Linear(ins_in, d_model)
        self.layer_norm = nn.LayerNorm(d_model)
        self._tables = {}

    def table(self, L, device):
        key = (L, torch.device(device))
        if key not in self._tables:
            self._tables[key] = sinusoid_table(L, self.d_model).to(device)
        return self._tables[key]

    def draw_keep(self, B, L, Lk, device):
        """The uint8 keep masks of one call in their fixed order: (vis half (B*Lk, d_model), ins half (B*L, d_model), layer 0's three, layer 1's three, ...)"""
        def draw(rows):
            return (torch.rand(rows, self.d_model, device=device) >= self.p).to(torch.uint8)
        vis, ins = draw(B * Lk), draw(B * L)
        return (vis, ins, *(layer.draw_keep(B * L, device) for layer in self.layers))

    def _embed(self, x, fc, keep, p, post):
        args = (x, fc.weight, fc.bias, self.layer_norm.weight, self.layer_norm.bias)
        if not x.is_cuda:
            return embed_ln_ref(*args, keep=keep, p=p, post=post)
        if self.d_model != VLA_D_MODEL or not embed_k_ok(fc.in_features):
            raise ValueError(f"on the device Visual_Ling_Attn serves d_model {VLA_D_MODEL} and input widths that are multiples of {EMBED_K_STEP} from "
                             f"{EMBED_K_STEP} to {EMBED_MAX_K} (got d_model {self.d_model}, in_features {fc.in_features})")
        return embed_ln(*args, keep=keep, p=p, post=post)

    def forward(self, input, input_2, self_att_mask, enc_att_mask, _keep=None):
        if self_att_mask is not None or enc_att_mask is not None:
            raise ValueError("Visual_Ling_Attn serves self_att_mask = enc_att_mask = None, as the high-level model calls it (seq2seq_highlevel_cma.py:200-201)")
        if input.dim() != 3 or input_2.dim() != 3 or input.shape[0] != input_2.shape[0]:
            raise ValueError(f"Visual_Ling_Attn takes input (B, L, ins_in) and input_2 (B, Lk, vis_in), got {tuple(input.shape)}, {tuple(input_2.shape)}")
        B, L, Lk = input.shape[0], input.shape[1], input_2.shape[1]
        p = self.p if self.training else 0.0
        keep = _keep
        if keep is None:
            keep = self.draw_keep(B, L, Lk, input.device) if p > 0 else (None, None) + (None,) * len(self.layers)
        out = self._embed(input_2, self.vis_fc, keep[0], p, None)
        inp = self._embed(input, self.ins_fc, keep[1], p, self.table(L, input.device))
        for layer, k in zip(self.layers, keep[2:]):
            out = layer(inp, out, None, None, _keep=k)
        return out


def _instr_params(params):
    """params: per direction (weight_ih, weight_hh, bias_ih, bias_hh), one or two directions -> (list of 4-tuples, H, G, E)"""
    params = [tuple(p) for p in params]
    if len(params) not in (1, 2) or any(len(p) != 4 for p in params):
        raise ValueError(f"instruction scan: params holds (weight_ih, weight_hh, bias_ih, bias_hh) for one or two directions, got {len(params)} entries")
    w_ih, w_hh = params[0][0], params[0][1]
    if w_hh.dim() != 2 or w_ih.dim() != 2 or w_hh.shape[1] < 1 or w_hh.shape[0] % w_hh.shape[1] or w_hh.shape[0] // w_hh.shape[1] not in (3, 4):
        raise ValueError(f"instruction scan: weight_hh must be (G*H, H) with G = 4 (LSTM) or 3 (GRU), got {tuple(w_hh.shape)}")
    H, G, E = w_hh.shape[1], w_hh.shape[0] // w_hh.shape[1], w_ih.shape[1]
    for d, p in enumerate(params):
        for name, t, shape in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), p, ((G * H, E), (G * H, H), (G * H,), (G * H,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"instruction scan: {name} of direction {d} has shape {tuple(t.shape)}, expected {shape}")
    return params, H, G, E


def instr_encoder_ref(embedded, lengths, params, final_state_only):
    """Pure-torch restatement of the packed instruction scan for any size, dtype and device: a per-token cell loop with each row frozen beyond its
    length -- row b is active at tokens t < lengths[b]; the forward direction walks t = 0 .. L-1 and the reverse t = L-1 .. 0, each from the zero
    state, and an inactive token neither changes the state nor produces output.  That is pack_padded_sequence(enforce_sorted=False) -> nn.LSTM /
    nn.GRU -> pad_packed_sequence(total_length=L) without the packing.  embedded (B, L, E), lengths (B,), params as instr_scan.  Returns
    (B, L, dirs*H), zeros at inactive tokens, or with final_state_only (B, H): the forward direction's state at each row's own last token (zeros
    for a row of length 0)."""
    params, H, G, _ = _instr_params(params)
    if final_state_only and len(params) != 1:
        raise ValueError("instruction scan: final_state_only serves one direction")
    B, L = embedded.shape[0], embedded.shape[1]
    lstm = G == 4
    outs, fin = [], None
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        gi_all = torch.nn.functional.linear(embedded, w_ih, b_ih)
        h = embedded.new_zeros(B, H)
        c = embedded.new_zeros(B, H)
        seq = [None] * L
        for t in (range(L - 1, -1, -1) if d else range(L)):
            act = (t < lengths).reshape(B, 1)
            gi, gh = gi_all[:, t], torch.nn.functional.linear(h, w_hh, b_hh)
            if lstm:
                i, f, g, o = (gi + gh).chunk(4, 1)
                c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h2 = torch.sigmoid(o) * torch.tanh(c2)
                c = torch.where(act, c2, c)
            else:
                (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3, 1), gh.chunk(3, 1)
                r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
                h2 = (1 - z) * torch.tanh(i_n + r * h_n) + z * h
            h = torch.where(act, h2, h)
            seq[t] = torch.where(act, h2, torch.zeros_like(h2))
        outs.append(torch.stack(seq, 1))
        if d == 0:
            fin = h
    return fin if final_state_only else torch.cat(outs, 2)


class _InstrScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embedded, lengths, final_state_only, *flat):
        params, H, G, E = _instr_params([flat[i:i + 4] for i in range(0, len(flat), 4)])
        if not embedded.is_cuda:
            raise ValueError("instr_scan runs on the device; CPU tensors go through instr_encoder_ref")
        for d, p in enumerate(params):
            for name, t in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), p):
                if t.device != embedded.device:       # the kernels take raw pointers: a host pointer would fault on the device
                    raise ValueError(f"instr_scan: {name} of direction {d} is on {t.device}, embedded on {embedded.device}")
        if lengths.device != embedded.device:
            raise ValueError(f"instr_scan: lengths is on {lengths.device}, embedded on {embedded.device}")
        if H != INSTR_HIDDEN:
            raise ValueError(f"instr_scan serves hidden size {INSTR_HIDDEN} (256 units x 4 partitions = 1024 threads), got weight_hh {tuple(params[0][1].shape)}")
        dirs, lstm = len(params), G == 4
        if final_state_only and dirs != 1:
            raise ValueError("instr_scan: final_state_only serves one direction")
        if embedded.dim() != 3 or embedded.shape[0] < 1 or embedded.shape[1] < 1 or embedded.shape[2] != E:
            raise ValueError(f"instr_scan takes embedded (B >= 1, L >= 1, {E}), got {tuple(embedded.shape)}")
        B, L = embedded.shape[0], embedded.shape[1]
        if tuple(lengths.shape) != (B,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError(f"instr_scan: lengths must be an integer tensor of shape ({B},), got {lengths.dtype} {tuple(lengths.shape)}")
        dev = embedded.device
        emb = _f32c(embedded).reshape(B * L, E)
        len32 = lengths.detach().to(torch.int32).contiguous()
        params = [tuple(_f32c(t) for t in p) for p in params]
        # the convention of include/hcm.h: LSTM adds both biases to `pre`; GRU adds (b_hr, b_hz, 0) and hands b_hn to the kernel
        pre = torch.empty(dirs, B * L, G * H, device=dev)
        for d, (w_ih, _, b_ih, b_hh) in enumerate(params):
            bias = b_ih + b_hh if lstm else b_ih + torch.cat([b_hh[:2 * H], b_hh.new_zeros(H)])
            torch.addmm(bias, emb, w_ih.t(), out=pre[d])
        w_hh = torch.stack([p[1] for p in params])
        b_hn = None if lstm else torch.stack([p[3][2 * H:] for p in params])
        out = torch.empty(B, L, dirs * H, device=dev)
        fin = torch.empty(B, H, device=dev) if final_state_only else None
        gates = torch.empty(dirs, B * L, 4 * H, device=dev)
        c_seq = torch.empty(dirs, B * L, H, device=dev) if lstm else None
        kind = _lib.HCM_LSTM if lstm else _lib.HCM_GRU
        work = torch.empty(_lib.lib().hcm_op_instr_scan_work_floats(B, L, dirs, kind), device=dev)
        _lib.check(_lib.lib().hcm_op_instr_scan_train(_ptr(pre), _ptr(w_hh), _ptr(b_hn), _ptr(len32), _ptr(out), _ptr(fin), _ptr(gates), _ptr(c_seq),
                                                      _ptr(work), B, L, H, dirs, kind, _stream()))
        ctx.save_for_backward(emb, len32, w_hh, out, gates, c_seq, *(p[0] for p in params))
        ctx.dims = (B, L, E, dirs, lstm, bool(final_state_only))
        return fin if final_state_only else out

    @staticmethod
    @once_differentiable
    def backward(ctx, d):
        emb, len32, w_hh, out, gates, c_seq, *w_ih = ctx.saved_tensors
        B, L, E, dirs, lstm, final = ctx.dims
        H, G, dev = INSTR_HIDDEN, 4 if lstm else 3, emb.device
        d = _f32c(d)
        d_pre = torch.empty(dirs, B * L, G * H, device=dev)
        d_gh = None if lstm else torch.empty(dirs, B * L, G * H, device=dev)
        kind = _lib.HCM_LSTM if lstm else _lib.HCM_GRU
        work = torch.empty(_lib.lib().hcm_op_instr_scan_work_floats(B, L, dirs, kind), device=dev)
        _lib.check(_lib.lib().hcm_op_instr_scan_bwd(None if final else _ptr(d), _ptr(d) if final else None, _ptr(gates), _ptr(c_seq), _ptr(out), _ptr(w_hh),
                                                    _ptr(len32), _ptr(work), _ptr(d_pre), _ptr(d_gh), B, L, H, dirs, kind, _stream()))
        if lstm:
            d_gh = d_pre
        need = ctx.needs_input_grad
        grads = []
        for k in range(dirs):
            n = need[3 + 4 * k:7 + 4 * k]
            dw_hh = None
            if n[1]:
                # h' is `out` shifted by one token against the direction (zero at each end, and `out` is zero at inactive tokens)
                g3, o3 = d_gh[k].view(B, L, G * H), out[:, :, k * H:(k + 1) * H]
                if L == 1:
                    dw_hh = torch.zeros(G * H, H, device=dev)
                elif k == 0:
                    dw_hh = g3[:, 1:].reshape(-1, G * H).t() @ o3[:, :-1].reshape(-1, H)
                else:
                    dw_hh = g3[:, :-1].reshape(-1, G * H).t() @ o3[:, 1:].reshape(-1, H)
            grads += [d_pre[k].t() @ emb if n[0] else None, dw_hh, d_pre[k].sum(0) if n[2] else None, d_gh[k].sum(0) if n[3] else None]
        d_emb = None
        if need[0]:
            d_emb = d_pre[0] @ w_ih[0]
            if dirs == 2:
                d_emb = torch.addmm(d_emb, d_pre[1], w_ih[1])
            d_emb = d_emb.reshape(B, L, E)
        return (d_emb, None, None, *grads)


def instr_scan(embedded, lengths, params, final_state_only):
    """The packed instruction scan (hidden 256, one layer, float32, on the device) with gradients to `embedded` and the parameters: embedded
    (B, L, E), lengths (B,) integer on the device (row b is active at tokens t < lengths[b]; nothing is read back to the host), params per
    direction torch's (weight_ih, weight_hh, bias_ih, bias_hh) -- one entry, or two for a bidirectional encoder (the second is the `_reverse`
    set); LSTM or GRU is read off weight_hh's row count.  Returns (B, L, dirs*256) with zeros at inactive tokens, or with final_state_only
    (one direction) the (B, 256) state at each row's own last token.  The semantics are instr_encoder_ref's.

    Forward: `pre` by torch.addmm over all B*L rows, then hcm_op_instr_scan_train, one launch for the whole scan on the current stream, which
    saves the gates, c_t and h_t.  Backward: hcm_op_instr_scan_bwd, one launch for the whole reverse scan, gives d_pre and d_gh; the dense
    reductions behind it -- dW_ih = d_pre.T @ emb, db_ih = d_pre.sum(0), dW_hh = d_gh.T @ h', db_hh = d_gh.sum(0) with h' the output shifted by
    one token against the direction and d_gh = d_pre for LSTM -- stay in torch, the split state_scan made; d_emb = d_pre @ W_ih is computed
    only when `embedded` requires a gradient (with frozen embeddings it never runs).  Nothing is cached between calls: the weights are packed
    for the kernels on the device in every call."""
    return _InstrScan.apply(embedded, lengths, bool(final_state_only), *(t for p in params for t in p))


class InstructionEncoder(nn.Module):
    """Drop-in for the reference's InstructionEncoder (models/encoders/instruction_encoder.py): the reference's state-dict keys --
    embedding_layer.weight and encoder_rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l0, with the _reverse suffix for the second direction -- in a
    real nn.Embedding and a real nn.LSTM / nn.GRU (storage and initialisation only), so load_state_dict takes a reference checkpoint's keys
    unchanged.  Takes the reference's config object (vocab_size, embedding_size, hidden_size, rnn_type, bidirectional, final_state_only,
    fine_tune_embeddings) or the same names as keyword arguments, which win.  `embeddings=` (vocab, E) stands in for the reference's file load:
    the table is nn.Embedding.from_pretrained(embeddings, freeze=not fine_tune_embeddings), as with use_pretrained_embeddings; without it the
    table is a trainable nn.Embedding(vocab_size, embedding_size, padding_idx=0), as in the reference.

    forward(instruction) takes (B, L) token ids, 0 = padding, and derives lengths = (instruction != 0).sum(1) on the device: nothing is read
    back to the host.  With final_state_only it returns (B, hidden); otherwise (B, D, L), D = hidden * directions: the reference's
    (B, D, max(lengths)) zero-padded to L -- trimming to max(lengths) would need the host read this module exists to remove.  CMANet masks
    all-zero columns (cma.py:273), so the model's outputs are unchanged.

    Device tensors go through instr_scan (hidden size 256; anything else raises), CPU tensors through instr_encoder_ref.  final_state_only
    together with bidirectional is refused: the reference returns a (2, B, H) tensor there that no model can consume."""

    NAMES = ("vocab_size", "embedding_size", "hidden_size", "rnn_type", "bidirectional", "final_state_only", "fine_tune_embeddings")

    def __init__(self, config=None, embeddings=None, **kw):
        super().__init__()
        unknown = set(kw) - set(self.NAMES)
        if unknown:
            raise TypeError(f"InstructionEncoder: unknown arguments {sorted(unknown)}")
        given = dict(fine_tune_embeddings=False)
        if embeddings is not None:
            given.update(vocab_size=embeddings.shape[0], embedding_size=embeddings.shape[1])
        given.update({n: getattr(config, n) for n in self.NAMES if hasattr(config, n)})
        given.update(kw)
        missing = [n for n in self.NAMES if n not in given]
        if missing:
            raise TypeError(f"InstructionEncoder: missing {missing}")
        vocab, E, H, rnn_type, bidir, final, fine_tune = (given[n] for n in self.NAMES)
        if rnn_type not in ("GRU", "LSTM"):
            raise ValueError(f"rnn_type must be GRU or LSTM, got {rnn_type!r}")
        if final and bidir:
            raise ValueError("InstructionEncoder: final_state_only with bidirectional is refused (the reference returns a (2, B, H) tensor no model consumes)")
        if embeddings is not None:
            if tuple(embeddings.shape) != (vocab, E):
                raise ValueError(f"InstructionEncoder: embeddings has shape {tuple(embeddings.shape)}, expected {(vocab, E)}")
            self.embedding_layer = nn.Embedding.from_pretrained(embeddings.detach().clone().float(), freeze=not fine_tune)
        else:
            self.embedding_layer = nn.Embedding(num_embeddings=vocab, embedding_dim=E, padding_idx=0)
        self.encoder_rnn = getattr(nn, rnn_type)(input_size=E, hidden_size=H, bidirectional=bool(bidir))
        self.rnn_type, self.hidden_size, self.bidir, self.final_state_only = rnn_type, H, bool(bidir), bool(final)

    @property
    def output_size(self):
        return self.hidden_size * (2 if self.bidir else 1)

    def _params(self):
        return [tuple(getattr(self.encoder_rnn, f"{n}_l0{sfx}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for sfx in (("", "_reverse") if self.bidir else ("",))]

    def forward(self, instruction):
        if instruction.dim() != 2:
            raise ValueError(f"InstructionEncoder takes instruction (B, L), got {tuple(instruction.shape)}")
        lengths = (instruction != 0).sum(1)
        embedded = self.embedding_layer(instruction.long())
        if not instruction.is_cuda:
            y = instr_encoder_ref(embedded, lengths, self._params(), self.final_state_only)
        else:
            if self.hidden_size != INSTR_HIDDEN:
                raise ValueError(f"on the device InstructionEncoder serves hidden_size {INSTR_HIDDEN} (got {self.hidden_size})")
            y = instr_scan(embedded, lengths, self._params(), self.final_state_only)
        return y if self.final_state_only else y.permute(0, 2, 1)


TOKEN_MAJOR, CHANNEL_MAJOR = _lib.HCM_ATTN_TOKEN_MAJOR, _lib.HCM_ATTN_CHANNEL_MAJOR
ATTN1Q_MAX_I, ATTN1Q_MAX_C = 256, 4096


def attn1q_access(layout, C0, I):
    """Bytes per lane the kernels move for x of this shape (the launcher's rule, csrc/cma_attn_train.hip): 16 where the shape keeps every access on a
    16-byte boundary -- token-major rows with C0 % 4 == 0, channel-major rows with I % 4 == 0 -- and 4 otherwise"""
    return 16 if (C0 if layout == TOKEN_MAJOR else I) % 4 == 0 else 4


def attn1q_ref(qt, x, e, mask_zero, scale, layout, _taps=None):
    """Pure-torch restatement of CMANet's attention with the key projection folded into the query, any dtype and device: qt (B, C0 + Ce) = q W_k;
    x (B, I, C0) with layout TOKEN_MAJOR or (B, C0, I) with CHANNEL_MAJOR; e (I, Ce), a tail of further channels shared by all samples, or None.
    a = softmax(scale (X^T qt - 1e8 mask)) and the result is xbar = X a (B, C0 + Ce); with mask_zero a position is masked exactly when all its
    channels compare == 0 (cma.py:273), and 1e8 leaves the logit before the scale, as the reference writes it (cma.py:205-207)."""
    X = x if layout == TOKEN_MAJOR else x.transpose(1, 2)
    C0 = X.shape[2]
    logits = torch.einsum("bic,bc->bi", X, qt[:, :C0])
    if e is not None:
        logits = logits + qt[:, C0:] @ e.t()
    if mask_zero:
        mask = (X == 0).all(2)
        if e is not None:
            mask = mask & (e == 0).all(1)[None]
        logits = logits - mask.to(logits.dtype) * 1e8
    a = torch.softmax(logits * scale, 1)
    if _taps is not None:
        _taps["a"] = a
    xbar = torch.einsum("bi,bic->bc", a, X)
    return xbar if e is None else torch.cat([xbar, a @ e], 1)


class _Attn1q(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qt, x, e, mask_zero, scale, layout):
        if not qt.is_cuda:
            raise ValueError("attn1q runs on the device; CPU tensors go through attn1q_ref")
        for name, t in (("x", x), ("e", e)):
            if t is not None and t.device != qt.device:   # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"attn1q: {name} is on {t.device}, qt on {qt.device}")
        if layout not in (TOKEN_MAJOR, CHANNEL_MAJOR):
            raise ValueError(f"attn1q: layout must be TOKEN_MAJOR or CHANNEL_MAJOR, got {layout!r}")
        if x.dim() != 3 or qt.dim() != 2 or x.shape[0] != qt.shape[0] or (e is not None and e.dim() != 2):
            raise ValueError(f"attn1q takes qt (B, C), x (B, I, C0) or (B, C0, I) and e (I, Ce), got {tuple(qt.shape)}, {tuple(x.shape)}, "
                             f"{None if e is None else tuple(e.shape)}")
        B = x.shape[0]
        I, C0 = (x.shape[1], x.shape[2]) if layout == TOKEN_MAJOR else (x.shape[2], x.shape[1])
        Ce = 0 if e is None else e.shape[1]
        if B < 1 or C0 < 1 or not 1 <= I <= ATTN1Q_MAX_I or C0 + Ce > ATTN1Q_MAX_C or Ce % 4 or (e is not None and (Ce < 1 or e.shape[0] != I)) \
                or qt.shape[1] != C0 + Ce:
            raise ValueError(f"attn1q serves B >= 1, 1..{ATTN1Q_MAX_I} positions, C0 + Ce <= {ATTN1Q_MAX_C} channels with Ce a multiple of 4, e (I, Ce) and "
                             f"qt (B, C0 + Ce), got B {B}, I {I}, C0 {C0}, e {None if e is None else tuple(e.shape)}, qt {tuple(qt.shape)}")
        qt, x = _f32c(qt), _f32c(x)
        e = None if e is None else _f32c(e)
        a = torch.empty(B, I, device=qt.device)
        xbar = torch.empty(B, C0 + Ce, device=qt.device)
        _lib.check(_lib.lib().hcm_op_attn1q_train(_ptr(qt), _ptr(x), _ptr(e), layout, int(bool(mask_zero)), scale, _ptr(a), _ptr(xbar), None,
                                                  B, C0, Ce, I, _stream()))
        ctx.save_for_backward(qt, x, e, a)
        ctx.dims = (B, C0, Ce, I, layout, scale)
        return xbar

    @staticmethod
    @once_differentiable
    def backward(ctx, d_xbar):
        qt, x, e, a = ctx.saved_tensors
        B, C0, Ce, I, layout, scale = ctx.dims
        need = ctx.needs_input_grad
        d_xbar = _f32c(d_xbar)
        d_qt = torch.empty_like(qt)
        d_x = torch.empty_like(x) if need[1] else None
        d_e = torch.empty_like(e) if e is not None else None
        n = _lib.lib().hcm_op_attn1q_work_floats(B, C0, Ce, I)
        work = torch.empty(n, device=qt.device) if n else None
        _lib.check(_lib.lib().hcm_op_attn1q_bwd(_ptr(d_xbar), _ptr(qt), _ptr(x), _ptr(e), _ptr(a), layout, scale, _ptr(d_qt), _ptr(d_x), _ptr(d_e),
                                                _ptr(work), B, C0, Ce, I, _stream()))
        return d_qt if need[0] else None, d_x, d_e if need[2] else None, None, None, None


def attn1q(qt, x, e, mask_zero, scale, layout):
    """CMANet's attention with one query per sample (float32, on the device) with gradients to qt, x and e: arguments and result as attn1q_ref;
    1..256 positions, at most 4096 channels, Ce a multiple of 4; x in either layout is read where it lies, and so is e: no (B, C0 + Ce, I) tensor
    is formed.

    Forward: hcm_op_attn1q_train, one launch with one workgroup per sample, derives the mask in the pass that forms the logits and saves the
    weights a (B, I); K and V do not exist.  Backward: hcm_op_attn1q_bwd, one launch for d_qt (and d_x, computed only when x requires a gradient:
    with frozen trunk features it never is) plus an ordered reduce over the samples for d_e.  The projections around it -- qt = q W_k,
    xbar W_v^T + b_v -- are dense products and stay in torch.  Nothing is cached between calls."""
    return _Attn1q.apply(qt, x, e, bool(mask_zero), float(scale), int(layout))


FLAT_HEADS_HIDDEN, FLAT_HEADS_MAX_ACTIONS = 512, 4
# the launch rules of csrc/flat_heads_train.hip: rows per workgroup of the heads launch, the backward's row block and its two halves, and the
# thread count of the criterion launch (flat_val_loss_kernel: thread t adds the rows t, t + 256, ...)
FLAT_HEADS_FWD_ROWS, FLAT_HEADS_BWD_ROWS, FLAT_HEADS_BWD_HALF, FLAT_LOSS_THREADS = 4, 32, 16, 256


def flat_heads_ok(rows, hidden, num_actions):
    """the sizes the kernels serve (include/hcm.h); rows == 0 is legal at the C ABI and writes nothing, so the wrapper leaves it to the restatement"""
    return rows >= 1 and hidden == FLAT_HEADS_HIDDEN and 1 <= num_actions <= FLAT_HEADS_MAX_ACTIONS


def flat_heads_loss_ref(x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected_actions, oracle_stop, progress):
    """Pure-torch restatement, any dtype and device, of the three heads of the flat baselines (seq2seq.py:176-188, cma.py's last lines) and the
    criterion of `_update_agent` (robo_vln_trainer.py:521-533), statement by statement, AuxLosses.reduce (common/aux_losses.py:27-33) included.
    x (rows, hidden); the weights as nn.Linear stores them; w_pm / b_pm / progress None = no progress monitor (nothing is registered and reduce
    returns 0.0).  The model passes PROGRESS_MONITOR.alpha in the `masks` slot of register_loss, so the weight of the registered loss is the
    default 1.0; reproduced here.  Returns (result (8,), out, stop, progress_hat or None): result as hcm_flat_val_step writes it -- [action loss,
    stop loss, aux loss, stop rows, aux rows, 0, 0, 0] -- differentiable in its first three entries; out and stop are the raw head outputs."""
    F = torch.nn.functional
    losses, alphas = {}, {}                                                   # AuxLosses.clear()
    progress_hat = None
    if w_pm is not None:
        progress_hat = torch.tanh(F.linear(x, w_pm, b_pm))                     # seq2seq.py:177
        losses["progress_monitor"] = F.mse_loss(progress_hat.squeeze(1), progress.reshape(-1).to(x.dtype), reduction="none")
        alphas["progress_monitor"] = 1.0                                       # register_loss(name, loss, alpha): alpha lands in `masks`
    output = F.linear(x, w_lin, b_lin)                                         # seq2seq.py:187
    stop_out = F.linear(x, w_stop, b_stop)                                     # seq2seq.py:188
    corrected_actions = corrected_actions.to(x.dtype).reshape(output.shape)
    action_mask = corrected_actions == 0                                       # :521
    masked = output.masked_fill(action_mask, 0)                                # :522, out of place: `output` is returned as the model gave it
    action_loss = F.mse_loss(masked, corrected_actions)                        # :525
    oracle_stop = oracle_stop.to(x.dtype).reshape(stop_out.shape)
    mask = oracle_stop != -1                                                   # :527
    stop_loss = F.binary_cross_entropy_with_logits(torch.masked_select(stop_out, mask), torch.masked_select(oracle_stop, mask))    # :528-530
    aux_mask = ~action_mask[:, 0]                                              # :531
    aux_loss = 0.0                                                             # AuxLosses.reduce
    for k in losses:
        aux_loss = aux_loss + alphas[k] * torch.masked_select(losses[k], aux_mask).mean()
    zero = x.new_zeros(())
    n_aux = aux_mask.sum().to(x.dtype) if losses else zero
    aux_loss = aux_loss if losses else zero
    result = torch.stack([action_loss, stop_loss, aux_loss, mask.sum().to(x.dtype), n_aux, zero, zero, zero])
    return result, output, stop_out, progress_hat


class _FlatHeadsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected_actions, oracle_stop, progress):
        if not x.is_cuda:
            raise ValueError("flat_heads_loss runs on the device; CPU tensors go through flat_heads_loss_ref")
        named = (("w_lin", w_lin), ("b_lin", b_lin), ("w_stop", w_stop), ("b_stop", b_stop), ("w_pm", w_pm), ("b_pm", b_pm),
                 ("corrected_actions", corrected_actions), ("oracle_stop", oracle_stop), ("progress", progress))
        for name, t in named:
            if t is not None and t.device != x.device:    # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"flat_heads_loss: {name} is on {t.device}, x on {x.device}")
        monitor = w_pm is not None
        if (b_pm is not None) != monitor or (progress is not None) != monitor:
            raise ValueError("flat_heads_loss: w_pm, b_pm and progress are given together or not at all")
        if x.dim() != 2 or w_lin.dim() != 2 or not flat_heads_ok(x.shape[0], x.shape[1], w_lin.shape[0]):
            raise ValueError(f"flat_heads_loss serves x (rows >= 1, {FLAT_HEADS_HIDDEN}) and 1..{FLAT_HEADS_MAX_ACTIONS} actions, got x {tuple(x.shape)}, "
                             f"w_lin {tuple(w_lin.shape)}")
        rows, H, A = x.shape[0], x.shape[1], w_lin.shape[0]
        shapes = [("w_lin", w_lin, (A, H)), ("b_lin", b_lin, (A,)), ("w_stop", w_stop, (1, H)), ("b_stop", b_stop, (1,))]
        if monitor:
            shapes += [("w_pm", w_pm, (1, H)), ("b_pm", b_pm, (1,))]
        for name, t, shape in shapes:
            if tuple(t.shape) != shape:
                raise ValueError(f"flat_heads_loss: {name} has shape {tuple(t.shape)}, expected {shape}")
        for name, t, n in (("corrected_actions", corrected_actions, rows * A), ("oracle_stop", oracle_stop, rows), ("progress", progress, rows)):
            if t is not None and t.numel() != n:
                raise ValueError(f"flat_heads_loss: {name} has {t.numel()} elements, expected {n}")
        x, w_lin, b_lin, w_stop, b_stop, corrected_actions, oracle_stop = (_f32c(t) for t in (x, w_lin, b_lin, w_stop, b_stop, corrected_actions,
                                                                                             oracle_stop))
        w_pm, b_pm, progress = (_f32c(t) if monitor else None for t in (w_pm, b_pm, progress))
        dev = x.device
        out, stop = torch.empty(rows, A, device=dev), torch.empty(rows, 1, device=dev)
        progress_hat = torch.empty(rows, 1, device=dev) if monitor else None
        result = torch.empty(8, device=dev)
        _lib.check(_lib.lib().hcm_op_flat_heads_loss_train(_ptr(x), _ptr(w_lin), _ptr(b_lin), _ptr(w_stop), _ptr(b_stop), _ptr(w_pm), _ptr(b_pm),
                                                           _ptr(corrected_actions), _ptr(oracle_stop), _ptr(progress), _ptr(out), _ptr(stop),
                                                           _ptr(progress_hat), _ptr(result), rows, H, A, _stream()))
        ctx.save_for_backward(x, w_lin, w_stop, w_pm, out, stop, progress_hat, corrected_actions, oracle_stop, progress, result)
        ctx.dims = (rows, H, A)
        ctx.mark_non_differentiable(out, stop)
        if monitor:
            ctx.mark_non_differentiable(progress_hat)
        return result, out, stop, progress_hat

    @staticmethod
    @once_differentiable
    def backward(ctx, d_result, _d_out, _d_stop, _d_progress_hat):
        x, w_lin, w_stop, w_pm, out, stop, progress_hat, corrected_actions, oracle_stop, progress, result = ctx.saved_tensors
        rows, H, A = ctx.dims
        need, dev, monitor = ctx.needs_input_grad, x.device, w_pm is not None
        d_result = _f32c(d_result)
        d_x = torch.empty(rows, H, device=dev) if need[0] else None
        d_w_lin, d_b_lin = torch.empty(A, H, device=dev), torch.empty(A, device=dev)
        d_w_stop, d_b_stop = torch.empty(1, H, device=dev), torch.empty(1, device=dev)
        d_w_pm, d_b_pm = (torch.empty(1, H, device=dev), torch.empty(1, device=dev)) if monitor else (None, None)
        work = torch.empty(_lib.lib().hcm_op_flat_heads_work_floats(rows, H, A), device=dev)
        _lib.check(_lib.lib().hcm_op_flat_heads_loss_bwd(_ptr(d_result), _ptr(x), _ptr(w_lin), _ptr(w_stop), _ptr(w_pm), _ptr(out), _ptr(stop),
                                                         _ptr(progress_hat), _ptr(corrected_actions), _ptr(oracle_stop), _ptr(progress), _ptr(result),
                                                         _ptr(d_x), _ptr(d_w_lin), _ptr(d_b_lin), _ptr(d_w_stop), _ptr(d_b_stop), _ptr(d_w_pm),
                                                         _ptr(d_b_pm), _ptr(work), rows, H, A, _stream()))
        return (d_x, d_w_lin if need[1] else None, d_b_lin if need[2] else None, d_w_stop if need[3] else None, d_b_stop if need[4] else None,
                d_w_pm if monitor and need[5] else None, d_b_pm if monitor and need[6] else None, None, None, None)


def flat_heads_loss(x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected_actions, oracle_stop, progress):
    """The heads and the criterion of the flat trainer's update step with gradients to x and the six head parameters: arguments and the returned
    (result, out, stop, progress_hat) as flat_heads_loss_ref; `result` is the differentiable output, out / stop / progress_hat are marked
    non-differentiable (the trainer forms its loss from the criterion alone).

    Float32 device tensors with hidden 512, 1..4 actions and at least one row go through hcm_op_flat_heads_loss_train -- the heads launch and
    flat_val_loss_kernel behind it, so `result` has the bits of hcm_op_flat_val_loss on this call's outputs -- and hcm_op_flat_heads_loss_bwd: one
    launch for d_x (only when x requires a gradient) and the row blocks' shares of the parameter gradients, one ordered reduce.  The cotangent and
    the counts are read on the device: nothing is read back to the host.  CPU tensors, other dtypes and unsupported sizes go through
    flat_heads_loss_ref.  Nothing is cached between calls."""
    args = (x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected_actions, oracle_stop, progress)
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or w_lin.dim() != 2 or not flat_heads_ok(x.shape[0], x.shape[1], w_lin.shape[0]):
        return flat_heads_loss_ref(*args)
    return _FlatHeadsLoss.apply(*args)


def _progress_target(observations, monitor):
    """observations["progress"] when the model has the monitor (a missing key raises, as S2SEngine.val_step does), None otherwise"""
    if not monitor:
        return None
    if "progress" not in observations:
        raise ValueError("observations['progress'] is missing: the model was built with the progress monitor")
    return observations["progress"]


def _heads_loss(model, x, corrected_actions, oracle_stop, progress):
    """model._flat_heads (flat_heads_loss; tools/bench_flat_update.py swaps in the restatement) over a model's heads; the labels are brought to
    x's device and dtype"""
    rows = x.shape[0]
    labels = [t.to(device=x.device, dtype=x.dtype) for t in (corrected_actions, oracle_stop)]
    if labels[0].numel() != rows * model.linear.out_features or labels[1].numel() != rows:
        raise ValueError(f"update_loss takes corrected_actions ({rows}, {model.linear.out_features}) and oracle_stop ({rows}, 1), got "
                         f"{tuple(corrected_actions.shape)}, {tuple(oracle_stop.shape)}")
    pm_w = pm_b = None
    if progress is not None:
        progress = progress.to(device=x.device, dtype=x.dtype)
        if tuple(progress.shape) not in ((rows,), (rows, 1)):
            raise ValueError(f"observations['progress'] must be ({rows},) or ({rows}, 1), got {tuple(progress.shape)}")
        pm_w, pm_b = model.progress_monitor.weight, model.progress_monitor.bias
    return model._flat_heads(x, model.linear.weight, model.linear.bias, model.stop_linear.weight, model.stop_linear.bias, pm_w, pm_b,
                             labels[0], labels[1], progress)[0]


class _ZeroGrad(torch.autograd.Function):
    """y unchanged; `param` -- a parameter that takes no part in the forward here but has an exact zero gradient in the reference: a key
    projection's bias, which cancels in the softmax, or a weight the reference multiplies by an ablated, all-zero embedding -- receives a
    gradient of exact zeros, not None, so that an optimizer treats it as the reference's does"""

    @staticmethod
    def forward(ctx, y, param):
        ctx.save_for_backward(param)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return g, torch.zeros_like(ctx.saved_tensors[0])


def _zero_grads(y, *params):
    """_ZeroGrad for every tensor of `params`"""
    for p in params:
        y = _ZeroGrad.apply(y, p)
    return y


class _SpatialEncoder(nn.Module):
    """What a spatial encoder of the reference keeps outside its frozen trunk: the (positions, 64) table under `spatial_embeddings.weight`"""

    def __init__(self, positions):
        super().__init__()
        self.spatial_embeddings = nn.Embedding(positions, 64)

    def tail(self):
        """(channels-major (64, I), kernel operand (I, 64)): the reference appends the table as `.view(1, -1, h, w)` (resnet_encoders.py:91-104,
        :218-231) -- a raw reinterpretation of the (I, 64) storage as 64 channels of I positions, not a transpose -- so channel c of position i
        is element c * I + i of the table"""
        w = self.spatial_embeddings.weight
        cm = w.view(64, w.shape[0])
        return cm, cm.t().contiguous()


CMA_TRUNK_PREFIXES = ("rgb_encoder.cnn.", "depth_encoder.visual_encoder.")


class CMANet(nn.Module):
    """The reference's CMANet (models/cma.py:28-333) as a trainable model from cached trunk features: the reference's parameters, buffer, state-dict
    keys and shapes outside the two frozen trunks (robo_vln_amd.synth.cma_spec lists them), and its forward signature.  Takes a
    robo_vln_amd.config.CMAConfig; `embeddings=` goes to InstructionEncoder.

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (output, stop_out, rnn_hidden_states) as cma.py:211-333, with
    observations["rgb_features"] (rows, 2048, 4, 4) and ["depth_features"] (rows, C, s, s) -- what CMAEngine.encode_features returns; an ablated
    modality needs no key -- and ["instruction"] (rows, L) or (1, L).  The returned state is a new tensor (the reference writes into its argument).

    The three attention stages are attn1q on the device and attn1q_ref on the CPU: text attention with qt = state_q(state) W_text_k over the
    instruction encoder's (rows, L, D) output, token-major and masked; RGB and depth attention with qt = text_q(text) W_k over the trunk feature,
    channel-major, with the spatial embedding as the shared tail, and the value projection xbar W_v^T + b_v behind it.  The instruction encoder is
    train.InstructionEncoder and both state encoders train.RNNStateEncoder; the linear layers around them are torch.  rgb_linear and depth_linear
    take the feature and the embedding as two operands, so no (rows, C + 64, I) tensor exists.  The key biases -- text_k.bias and the first
    hidden/2 entries of rgb_kv.bias and depth_kv.bias -- cancel and receive exact zero gradients.  `_scale` is kept as the reference's buffer; the
    stages use its constructor value 1 / sqrt(hidden / 2) as a host number, so nothing is read back from the device.

    update_loss(batch, corrected_actions, oracle_stop) is the model and the criterion of the trainer's update step; progress_monitor=True adds the
    auxiliary progress loss to it (CMAConfig.validate keeps refusing its own flag: that is the engine's configuration).  forward is the same
    either way, and without the keyword progress_monitor.* takes part in nothing."""

    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg, embeddings=None, progress_monitor=False):
        super().__init__()
        cfg.validate()
        self.cfg = cfg
        self.monitor = bool(progress_monitor)
        hh, fs, cc = cfg.hidden // 2, cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.hh, self.depth_shape = hh, (cc, fs * fs)
        self.instruction_encoder = InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden,
                                                      rnn_type=cfg.instr_rnn, bidirectional=cfg.bidirectional, final_state_only=False,
                                                      fine_tune_embeddings=True, embeddings=embeddings)
        self.depth_encoder = _SpatialEncoder(fs * fs)
        self.rgb_encoder = _SpatialEncoder(16)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2048 + 64, cfg.rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear((cc + 64) * fs * fs, cfg.depth_out), nn.ReLU(True))
        self.state_encoder = RNNStateEncoder(cfg.rgb_out + cfg.depth_out, cfg.hidden, 1, cfg.rnn_type)
        self.rgb_kv = nn.Conv1d(2048 + 64, hh + cfg.rgb_out, 1)
        self.depth_kv = nn.Conv1d(cc + 64, hh + cfg.depth_out, 1)
        self.state_q = nn.Linear(cfg.hidden, hh)
        self.text_k = nn.Conv1d(cfg.instr_out, hh, 1)
        self.text_q = nn.Linear(cfg.instr_out, hh)
        self.scale = 1.0 / (hh ** 0.5)
        self.register_buffer("_scale", torch.tensor(self.scale))
        self.second_state_compress = nn.Sequential(nn.Linear(cfg.hidden + cfg.rgb_out + cfg.depth_out + cfg.instr_out, cfg.hidden), nn.ReLU(True))
        self.second_state_encoder = RNNStateEncoder(cfg.hidden, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)      # read by update_loss with progress_monitor=True; parameters only otherwise
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        self.stop_linear = nn.Linear(cfg.hidden, 1)

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers + self.second_state_encoder.num_recurrent_layers

    def load_reference_state_dict(self, sd):
        """Load a reference CMANet state dict (tensors or arrays): the keys of the two frozen trunks are dropped, everything else is strict --
        a missing, unexpected or misshapen key raises"""
        kept = {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(CMA_TRUNK_PREFIXES)}
        return self.load_state_dict(kept, strict=True)

    def _attend(self, q, w_k, x, e, mask_zero, layout, kernel=True):
        fn = attn1q if kernel and x.is_cuda else attn1q_ref
        return fn(q @ w_k, x, e, mask_zero, self.scale, layout)

    def _visual(self, name, feat, enc, fc, pooled, ablated, rows, C0, I, like):
        """One modality's operands: (x (rows, C0, I), e (I, 64), input of the first state encoder (rows, out)) from the trunk feature.  The
        visual FC takes the feature and the embedding as two operands: rgb_linear pools over the positions first (AdaptiveAvgPool1d(1)),
        depth_linear flattens in NCHW order.  Ablated: zeros for the whole embedding, the spatial tail included (cma.py:238-241)."""
        if ablated:
            return (like.new_zeros(rows, C0, I), like.new_zeros(I, 64),
                    _zero_grads(torch.relu(fc.bias).expand(rows, -1), fc.weight, enc.spatial_embeddings.weight))
        s = int(round(I ** 0.5))
        if feat is None:
            raise ValueError(f"CMANet trains from cached trunk features: observations['{name}_features'] is missing; CMAEngine.encode_features "
                             "returns it from the frames")
        if feat.dim() != 4 or tuple(feat.shape) != (rows, C0, s, s):
            raise ValueError(f"CMANet takes {name}_features ({rows}, {C0}, {s}, {s}) as CMAEngine.encode_features returns them, got {tuple(feat.shape)}")
        x = feat.flatten(2)
        cm, e = enc.tail()
        if pooled:
            x_in = torch.addmm(torch.nn.functional.linear(cm.mean(1), fc.weight[:, C0:], fc.bias), x.mean(2), fc.weight[:, :C0].t())
        else:
            x_in = torch.addmm(torch.nn.functional.linear(cm.reshape(-1), fc.weight[:, C0 * I:], fc.bias), x.flatten(1), fc.weight[:, :C0 * I].t())
        return x, e, torch.relu(x_in)

    def forward(self, batch, taps=None):
        x, hidden = self._encode(batch, taps)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of `_update_agent` (robo_vln_trainer.py:515-533): the model up to the second state encoder, then
        flat_heads_loss.  -> (result (8,), rnn_hidden_states); result[0] + result[1] + result[2] is the trainer's loss.  With progress_monitor=True
        the auxiliary loss Seq2SeqNet registers (seq2seq.py:176-185) is formed on CMANet's progress_monitor against observations["progress"]."""
        progress = _progress_target(batch[0], self.monitor)
        x, hidden = self._encode(batch, None)
        return _heads_loss(self, x, corrected_actions, oracle_stop, progress), hidden

    def _encode(self, batch, taps):
        """forward up to the second state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg, hh = self.cfg, self.hh
        masks = masks.reshape(masks.shape[0], -1)[:, 0]
        rows = masks.shape[0]
        R = self.state_encoder.num_recurrent_layers
        instruction = observations["instruction"].long()
        instruction = instruction.expand(rows, instruction.shape[1])
        ins = self.instruction_encoder(instruction).permute(0, 2, 1)            # (rows, L, D): the encoder's own storage order
        if cfg.ablate_instruction:
            ins = ins * 0                                                       # every position masked: uniform weights, text = exact zeros
        cc, I_d = self.depth_shape
        rgb_x, rgb_e, rgb_in = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder, self.rgb_linear[2], True, cfg.ablate_rgb,
                                            rows, 2048, 16, ins)
        dep_x, dep_e, dep_in = self._visual("depth", observations.get("depth_features"), self.depth_encoder, self.depth_linear[1], False,
                                            cfg.ablate_depth, rows, cc, I_d, ins)
        state, h1 = self.state_encoder(torch.cat([rgb_in, dep_in], 1), rnn_hidden_states[:R], masks)

        text = self._attend(self.state_q(state), self.text_k.weight[:, :, 0], ins, None, True, TOKEN_MAJOR)
        text = _ZeroGrad.apply(text, self.text_k.bias)
        text_q = self.text_q(text)
        att = []
        for x, e, kv, ablated in ((rgb_x, rgb_e, self.rgb_kv, cfg.ablate_rgb), (dep_x, dep_e, self.depth_kv, cfg.ablate_depth)):
            xbar = self._attend(text_q, kv.weight[:hh, :, 0], x, e, False, CHANNEL_MAJOR, kernel=not ablated)
            att.append(torch.nn.functional.linear(xbar, kv.weight[hh:, :, 0], kv.bias[hh:]))

        x = self.second_state_compress(torch.cat([state, text, att[0], att[1]], 1))
        x, h2 = self.second_state_encoder(x, rnn_hidden_states[R:], masks)
        if taps is not None:
            taps.update(state=state, text=text, rgb_att=att[0], depth_att=att[1], rnn2_out=x)
        return x, torch.cat([h1, h2], 0)


S2S_TRUNK_PREFIXES = CMA_TRUNK_PREFIXES


class _FlatRgbEncoder(nn.Module):
    """What TorchVisionResNet50 in flat mode keeps outside its frozen trunk (resnet_encoders.py:189-237): `fc`, 2048 -> output_size, ReLU behind it"""

    def __init__(self, out):
        super().__init__()
        self.fc = nn.Linear(2048, out)


class _FlatDepthEncoder(nn.Module):
    """What VlnResnetDepthEncoder in flat mode keeps outside its frozen trunk (resnet_encoders.py:56-62): visual_fc = Flatten, Linear, ReLU"""

    def __init__(self, in_features, out):
        super().__init__()
        self.visual_fc = nn.Sequential(nn.Flatten(), nn.Linear(in_features, out), nn.ReLU(True))


class Seq2SeqNet(nn.Module):
    """The reference's Seq2SeqNet (models/seq2seq.py:21-189) as a trainable model from cached trunk features: the reference's parameters, state-dict
    keys and shapes outside the two frozen trunks (robo_vln_amd.synth.seq2seq_spec lists them), and its forward signature.  Takes a
    robo_vln_amd.config.S2SConfig; `embeddings=` goes to InstructionEncoder.  The progress monitor is on when cfg.progress_monitor is set.

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (output, stop_out, rnn_hidden_states) as seq2seq.py:140-189, with
    observations["rgb_features"] (rows, 2048, 1, 1) and ["depth_features"] (rows, C, s, s) -- what S2SEngine.encode_features returns; an ablated
    modality needs no key -- and ["instruction"] (rows, L) or (1, L): one instruction is encoded once and expanded (seq2seq.py:163).  The
    instruction encoder is train.InstructionEncoder with final_state_only, the state encoder train.RNNStateEncoder; rgb_encoder.fc and
    depth_encoder.visual_fc.1 with their ReLUs are torch; the cat is the reference's [instruction | depth | rgb].  sub_goal_linear holds
    parameters only, as in the reference.  update_loss(batch, corrected_actions, oracle_stop) is the model and the criterion of the trainer's
    update step, with the auxiliary progress loss against observations["progress"] when the monitor is on.

    The SimpleCNN encoders are trunks that train with the model: there is nothing to cache, and they are refused."""

    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg, embeddings=None):
        super().__init__()
        cfg.validate()
        if cfg.rgb_encoder != "TorchVisionResNet50" or cfg.depth_encoder != "VlnResnetDepthEncoder":
            raise ValueError("train.Seq2SeqNet trains from cached features of the two frozen ResNet trunks; SimpleRGBCNN / SimpleDepthCNN are trainable "
                             f"trunks with nothing to cache (got rgb_encoder {cfg.rgb_encoder!r}, depth_encoder {cfg.depth_encoder!r})")
        self.cfg = cfg
        self.monitor = bool(cfg.progress_monitor)
        fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.depth_shape = (cc, fs)
        self.instruction_encoder = InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden,
                                                      rnn_type=cfg.instr_rnn, bidirectional=False, final_state_only=True,
                                                      fine_tune_embeddings=True, embeddings=embeddings)
        self.depth_encoder = _FlatDepthEncoder(cc * fs * fs, cfg.depth_out)
        self.rgb_encoder = _FlatRgbEncoder(cfg.rgb_out)
        self.state_encoder = RNNStateEncoder(cfg.rnn_input_size, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        self.sub_goal_linear = nn.Linear(cfg.hidden, cfg.num_sub_tasks)      # parameters only (seq2seq.py:108): no forward reads it
        self.stop_linear = nn.Linear(cfg.hidden, 1)
        nn.init.kaiming_normal_(self.progress_monitor.weight, nonlinearity="tanh")     # _init_layers, seq2seq.py:136-138
        nn.init.constant_(self.progress_monitor.bias, 0)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def load_reference_state_dict(self, sd):
        """Load a reference Seq2SeqNet state dict (tensors or arrays): the keys of the two frozen trunks are dropped, everything else is strict --
        a missing, unexpected or misshapen key raises"""
        kept = {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(S2S_TRUNK_PREFIXES)}
        return self.load_state_dict(kept, strict=True)

    def _visual(self, name, feat, fc, ablated, rows, shape, like):
        """One modality's embedding relu(fc(flatten(feature))) (rows, out) from the trunk feature; ablated: times 0 (seq2seq.py:158-161), and
        exact zeros without the key"""
        if feat is None:
            if ablated:
                return _zero_grads(like.new_zeros(rows, fc.out_features), fc.weight, fc.bias)
            raise ValueError(f"Seq2SeqNet trains from cached trunk features: observations['{name}_features'] is missing; S2SEngine.encode_features "
                             "returns it from the frames")
        if tuple(feat.shape) != (rows, *shape):
            raise ValueError(f"Seq2SeqNet takes {name}_features {(rows, *shape)} as S2SEngine.encode_features returns them, got {tuple(feat.shape)}")
        y = torch.relu(fc(feat.flatten(1)))                                   # Flatten in NCHW order
        return y * 0 if ablated else y

    def _encode(self, batch):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                       # :172
        rows = masks.shape[0]
        instruction = observations["instruction"].long()
        if instruction.dim() != 2 or instruction.shape[0] not in (1, rows):
            raise ValueError(f"Seq2SeqNet takes instruction ({rows} or 1, L), got {tuple(instruction.shape)}")
        ins = self.instruction_encoder(instruction)                           # :153
        cc, fs = self.depth_shape
        depth = self._visual("depth", observations.get("depth_features"), self.depth_encoder.visual_fc[1], cfg.ablate_depth, rows, (cc, fs, fs), ins)
        rgb = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder.fc, cfg.ablate_rgb, rows, (2048, 1, 1), ins)
        if cfg.ablate_instruction:
            ins = ins * 0                                                     # :156-157
        ins = ins.expand(rows, ins.shape[1])                                  # :163
        x = torch.cat([ins, depth, rgb], 1)                                   # :164
        return self.state_encoder(x, rnn_hidden_states, masks)                # :174

    def forward(self, batch):
        x, hidden = self._encode(batch)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of `_update_agent` (robo_vln_trainer.py:515-533): the model up to the state encoder, then flat_heads_loss.
        -> (result (8,), rnn_hidden_states); result[0] + result[1] + result[2] is the trainer's loss."""
        progress = _progress_target(batch[0], self.monitor)
        x, hidden = self._encode(batch)
        return _heads_loss(self, x, corrected_actions, oracle_stop, progress), hidden


def flat_update(model, optimizer, observations, prev_actions, not_done_masks, corrected_actions, oracle_stop, rnn_hidden_states):
    """The reference's `_update_agent` (robo_vln_trainer.py:505-542) for train.CMANet / train.Seq2SeqNet: zero_grad, detach the carried state
    (repackage_hidden), model.update_loss, loss = result[0] + result[1] + result[2], backward, optimizer.step().  Returns (result, rnn_hidden_states)
    with `result` the detached (8,) tensor on the model's device -- [action loss, stop loss, aux loss, stop rows, aux rows, 0, 0, 0] -- where the
    reference returns three host numbers: nothing is read back and nothing synchronises, so a caller keeps the results of an epoch and reads once,
    as FlatValidator does."""
    optimizer.zero_grad()
    rnn_hidden_states = rnn_hidden_states.detach()
    result, rnn_hidden_states = model.update_loss((observations, rnn_hidden_states, prev_actions, not_done_masks), corrected_actions, oracle_stop)
    loss = result[0] + result[1] + result[2]
    loss.backward()
    optimizer.step()
    return result.detach(), rnn_hidden_states


SUBTASK_CE_HIDDEN, SUBTASK_CE_MAX_CLASSES = 512, 6
# the launch rules of csrc/subtask_ce_train.hip: rows per workgroup of the head launch, the backward's row block and its two halves, and the
# thread count of the criterion launch (thread t adds the rows t, t + 256, ...: val_loss_kernel's shape)
SUBTASK_CE_FWD_ROWS, SUBTASK_CE_BWD_ROWS, SUBTASK_CE_BWD_HALF, SUBTASK_CE_LOSS_THREADS = 4, 32, 16, 256


def subtask_ce_ok(rows, hidden, A, num_sub_tasks):
    """the sizes the kernels serve (include/hcm.h); rows == 0 is legal at the C ABI and writes nothing, so the wrapper leaves it to the restatement"""
    return rows >= 1 and hidden == SUBTASK_CE_HIDDEN and 1 <= num_sub_tasks <= A <= SUBTASK_CE_MAX_CLASSES


def _subtask_labels(oracle_subtask, rows, device):
    """the label tensor as the collate function carries it -- (rows, 1) float, or any integer tensor of rows elements -- as (rows,) int64 on
    `device`: moved first, converted there"""
    if oracle_subtask.numel() != rows:
        raise ValueError(f"subtask_ce takes one sub-task label per row: {rows} rows, oracle_subtask {tuple(oracle_subtask.shape)}")
    return oracle_subtask.detach().to(device).reshape(-1).to(torch.int64).contiguous()


def subtask_ce_ref(x, w, b, oracle_subtask, num_sub_tasks=None):
    """Pure-torch restatement, any dtype and device, of the high-level model's head (seq2seq_highlevel_cma.py:232) and the criterion of
    `_update_agent` (hierarchical_trainer.py:506-511), statement by statement.  x (rows, hidden); w, b as nn.Linear stores them (A classes);
    oracle_subtask (rows,) or (rows, 1), float or integer: 0 = padded row, 1..num_sub_tasks = the target class plus one (num_sub_tasks = A
    when not given); a label outside [0, num_sub_tasks] is counted and treated as padded, as tests/val_ref.criteria does.  Returns
    (result (8,), logits): result in the index positions of hcm_val_step -- [0] the cross-entropy, [3] correct, [4] total, [6] out-of-range rows,
    the rest 0 -- differentiable in its first entry; logits is the raw head output."""
    F = torch.nn.functional
    A = w.shape[0]
    num_sub_tasks = A if num_sub_tasks is None else int(num_sub_tasks)
    if not 1 <= num_sub_tasks <= A:
        raise ValueError(f"subtask_ce: num_sub_tasks must be in 1..{A} (the head's classes), got {num_sub_tasks}")
    output = F.linear(x, w, b)                                                 # :506, the model's `self.linear(x)`
    oracle = _subtask_labels(oracle_subtask, output.shape[0], x.device)
    bad = (oracle < 0) | (oracle > num_sub_tasks)
    oracle = oracle.masked_fill(bad, 0)                                        # counted, then treated as padded
    high_level_action_mask = (oracle == 0).view(-1, 1)                         # :508
    masked = output.masked_fill(high_level_action_mask, 0)                     # :509, out of place: `output` is returned as the model gave it
    target = oracle - 1                                                        # :510-511; -1 on the padded rows: ignore_index
    loss = F.cross_entropy(masked, target, ignore_index=-1, reduction="mean")  # :498, :511
    valid = ~high_level_action_mask[:, 0]
    correct = ((torch.argmax(output.detach(), 1) == target) & valid).sum().to(x.dtype)
    zero = x.new_zeros(())
    result = torch.stack([loss, zero, zero, correct, valid.sum().to(x.dtype), zero, bad.sum().to(x.dtype), zero])
    return result, output


class _SubtaskCe(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, oracle, num_sub_tasks):
        if not x.is_cuda:
            raise ValueError("subtask_ce runs on the device; CPU tensors go through subtask_ce_ref")
        for name, t in (("w", w), ("b", b), ("oracle_subtask", oracle)):
            if t.device != x.device:                      # the kernels take raw pointers: a host pointer would fault on the device
                raise ValueError(f"subtask_ce: {name} is on {t.device}, x on {x.device}")
        if x.dim() != 2 or w.dim() != 2 or not subtask_ce_ok(x.shape[0], x.shape[1], w.shape[0], num_sub_tasks):
            raise ValueError(f"subtask_ce serves x (rows >= 1, {SUBTASK_CE_HIDDEN}) and 1 <= num_sub_tasks <= A <= {SUBTASK_CE_MAX_CLASSES} classes, got "
                             f"x {tuple(x.shape)}, w {tuple(w.shape)}, num_sub_tasks {num_sub_tasks}")
        rows, H, A = x.shape[0], x.shape[1], w.shape[0]
        for name, t, shape in (("w", w, (A, H)), ("b", b, (A,)), ("oracle_subtask", oracle, (rows,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"subtask_ce: {name} has shape {tuple(t.shape)}, expected {shape}")
        if oracle.dtype != torch.int64:
            raise ValueError(f"subtask_ce: the labels reach the kernels as int64, got {oracle.dtype}")
        x, w, b = (_f32c(t) for t in (x, w, b))
        oracle = oracle.contiguous()
        logits, result = torch.empty(rows, A, device=x.device), torch.empty(8, device=x.device)
        _lib.check(_lib.lib().hcm_op_subtask_ce_train(_ptr(x), _ptr(w), _ptr(b), _ptr(oracle), _ptr(logits), _ptr(result), rows, H, A, num_sub_tasks,
                                                      _stream()))
        ctx.save_for_backward(x, w, logits, oracle, result)
        ctx.dims = (rows, H, A, num_sub_tasks)
        ctx.mark_non_differentiable(logits)
        return result, logits

    @staticmethod
    @once_differentiable
    def backward(ctx, d_result, _d_logits):
        x, w, logits, oracle, result = ctx.saved_tensors
        rows, H, A, num_sub_tasks = ctx.dims
        need, dev = ctx.needs_input_grad, x.device
        d_result = _f32c(d_result)
        d_x = torch.empty(rows, H, device=dev) if need[0] else None
        d_w, d_b = torch.empty(A, H, device=dev), torch.empty(A, device=dev)
        work = torch.empty(_lib.lib().hcm_op_subtask_ce_work_floats(rows, H, A), device=dev)
        _lib.check(_lib.lib().hcm_op_subtask_ce_bwd(_ptr(d_result), _ptr(x), _ptr(w), _ptr(logits), _ptr(oracle), _ptr(result), _ptr(d_x), _ptr(d_w),
                                                    _ptr(d_b), _ptr(work), rows, H, A, num_sub_tasks, _stream()))
        return d_x, d_w if need[1] else None, d_b if need[2] else None, None, None


def subtask_ce(x, w, b, oracle_subtask, num_sub_tasks=None):
    """The head and the criterion of the hierarchical trainer's high-level update step with gradients to x, w and b: arguments and the returned
    (result, logits) as subtask_ce_ref; `result` is the differentiable output, logits is marked non-differentiable (the trainer forms its loss from
    the criterion alone).

    Float32 device tensors with hidden 512, 1 <= num_sub_tasks <= A <= 6 classes and at least one row go through hcm_op_subtask_ce_train -- the
    head launch and the criterion launch behind it, so result[0], [3], [4], [6] have the bits of hcm_op_val_loss on this call's logits -- and
    hcm_op_subtask_ce_bwd: one launch for d_x (only when x requires a gradient) and the row blocks' shares of d_w and d_b, one ordered reduce.  The
    labels are converted to int64 on the device; the cotangent and the count are read there: nothing is read back to the host.  CPU tensors,
    other dtypes and unsupported sizes go through subtask_ce_ref.  Nothing is cached between calls."""
    nst = w.shape[0] if num_sub_tasks is None else int(num_sub_tasks)
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or w.dim() != 2 or not subtask_ce_ok(x.shape[0], x.shape[1], w.shape[0], nst):
        return subtask_ce_ref(x, w, b, oracle_subtask, num_sub_tasks)
    return _SubtaskCe.apply(x, w, b, _subtask_labels(oracle_subtask, x.shape[0], x.device), nst)


def _model_slot(feat, slot):
    """one model's entry of a feature HCMEngine.encode_features returned for both: (high, low) pairs -> entry `slot`; a tensor is taken as it is"""
    return feat[slot] if isinstance(feat, (tuple, list)) else feat


HCM_HIGH_FROZEN_PREFIXES = ("rgb_encoder.cnn.", "depth_encoder.visual_encoder.", "embedding_layer.")
HCM_LOW_FROZEN_PREFIXES = CMA_TRUNK_PREFIXES


def _refuse_simple_cnn(cls, cfg):
    if cfg.rgb_encoder != "TorchVisionResNet50" or cfg.depth_encoder != "VlnResnetDepthEncoder":
        raise ValueError(f"train.{cls} trains from cached features of the two frozen ResNet trunks; SimpleRGBCNN / SimpleDepthCNN are trainable "
                         f"trunks with nothing to cache (got rgb_encoder {cfg.rgb_encoder!r}, depth_encoder {cfg.depth_encoder!r})")


class HighLevel(nn.Module):
    """The reference's Seq2Seq_HighLevel_CMA (models/seq2seq_highlevel_cma.py:29-233) as a trainable model from cached trunk features and a cached
    instruction stream: the reference's parameters, state-dict keys and shapes outside its three frozen parts -- the two trunks and BERT
    (robo_vln_amd.synth.high_level_spec lists them all) -- and its forward signature.  Takes a robo_vln_amd.config.HCMConfig; `dropout` is
    VISUAL_LING_ATTN.dropout (config/default.py:164); `embedder`, optional, maps token ids (B, L) to BERT's last hidden state (B, L, ins_in).

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (logits, rnn_hidden_states) as :170-233, with
    observations["rgb_features"] (rows, 2048, 4, 4) and ["depth_features"] (rows, C, s, s) -- the high entries of HCMEngine.encode_features' pairs;
    a pair is accepted and its entry 0 taken; an ablated modality needs no key -- and ["instruction_features"] (rows or 1 or N | rows, L, ins_in): BERT is
    frozen and runs under no_grad in the reference (:192-195), so its output enters as a tensor.  Without that key the stream is
    embedder(observations["instruction"]) under no_grad; with neither a ValueError names the key.

    rgb_kv / depth_kv are 1x1 convolutions of [feature | spatial embedding]: the tokens are x^T W[:, :C0]^T plus a row-independent (I, vis_in)
    tail from the spatial table and the bias, computed once per call -- no (rows, C0 + 64, I) tensor is formed -- and rgb_linear / depth_linear
    take the two operands as train.CMANet's do.  Then the two Visual_Ling_Attn calls on the one image_cm_encoder, the token mean over all L
    positions (cross_pooler), the cat [rgb_in | depth_in | ins_rgb | ins_depth], train.RNNStateEncoder and `linear`.  ablate_rgb / ablate_depth zero
    the whole embedding, the spatial tail included (:185-188); ablate_instruction and use_prev_action are branches the reference cannot run and
    HCMConfig.validate refuses them.  ins_fc and progress_monitor hold parameters only: no forward of the reference reads the first, the
    monitor's branch reads an undefined name (:221-224) and the trainer adds no aux loss.

    update_loss(batch, oracle_subtask) -> (result (8,), rnn_hidden_states) is the model and the criterion of the trainer's high-level step through
    subtask_ce; result[0] is the loss."""

    _subtask_ce = staticmethod(subtask_ce)

    def __init__(self, cfg, embedder=None, dropout=0.25):
        super().__init__()
        cfg.validate()
        _refuse_simple_cnn("HighLevel", cfg)
        self.cfg = cfg
        object.__setattr__(self, "embedder", embedder)        # frozen and the caller's: not a submodule, so no key of it enters the state dict
        fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.depth_shape = (cc, fs * fs)
        self.ins_fc = nn.Linear(768, 256)                     # TRANSFORMER_INSTRUCTION_ENCODER d_in / d_model (:46): parameters only
        self.depth_encoder = _SpatialEncoder(fs * fs)
        self.rgb_encoder = _SpatialEncoder(16)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2048 + 64, cfg.rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear((cc + 64) * fs * fs, cfg.depth_out), nn.ReLU(True))
        self.rgb_kv = nn.Conv1d(2048 + 64, cfg.vis_in, 1)
        self.depth_kv = nn.Conv1d(cc + 64, cfg.vis_in, 1)
        self.image_cm_encoder = Visual_Ling_Attn(N=cfg.vla_layers, vis_in_features=cfg.vis_in, ins_in_features=cfg.ins_in, d_model=cfg.d_model,
                                                 h=cfg.vla_heads, d_ff=cfg.d_ff, dropout=dropout)
        self.state_encoder = RNNStateEncoder(cfg.cm_d_model * 2 + cfg.depth_out + cfg.rgb_out, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        nn.init.kaiming_normal_(self.progress_monitor.weight, nonlinearity="tanh")     # _init_layers, :166-168
        nn.init.constant_(self.progress_monitor.bias, 0)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def load_reference_state_dict(self, sd):
        """Load a reference Seq2Seq_HighLevel_CMA state dict (tensors or arrays): the keys of the two frozen trunks and of BERT are dropped,
        everything else is strict -- a missing, unexpected or misshapen key raises"""
        kept = {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(HCM_HIGH_FROZEN_PREFIXES)}
        return self.load_state_dict(kept, strict=True)

    def _instruction_stream(self, observations, rows):
        stream = observations.get("instruction_features")
        if stream is None:
            if self.embedder is None or "instruction" not in observations:
                raise ValueError("HighLevel trains from the frozen BERT's output: observations['instruction_features'] (rows or 1, L, "
                                 f"{self.cfg.ins_in}) is missing, and there is no embedder with observations['instruction'] to compute it from")
            with torch.no_grad():                                              # :192-195
                stream = self.embedder(observations["instruction"].long())
        if stream.dim() != 3 or stream.shape[0] < 1 or rows % stream.shape[0] or stream.shape[2] != self.cfg.ins_in:
            raise ValueError(f"HighLevel takes instruction_features ({rows} or 1, L, {self.cfg.ins_in}) -- or (N, L, {self.cfg.ins_in}) with N dividing "
                             f"the {rows} time-major rows, one stream per trajectory -- got {tuple(stream.shape)}")
        if stream.shape[0] not in (1, rows):
            # one stream per trajectory (HCMEngine.encode_instruction of the N instructions): row t*N + n takes trajectory n's, as the collate repeats the ids
            return stream.detach().repeat(rows // stream.shape[0], 1, 1)
        return stream.detach().expand(rows, stream.shape[1], stream.shape[2])  # :190

    def _visual(self, name, feat, enc, fc, kv, pooled, ablated, rows, C0, I, like):
        """One modality: (tokens (rows, I, vis_in) = the 1x1 convolution of [feature | spatial embedding], transposed as the cross-modal encoder
        takes it; input of the state encoder (rows, out)).  Ablated: zeros for the whole embedding, so the tokens are the bias alone."""
        if ablated:
            return (_zero_grads(kv.bias.expand(rows, I, -1), kv.weight),
                    _zero_grads(torch.relu(fc.bias).expand(rows, -1), fc.weight, enc.spatial_embeddings.weight))
        feat = _model_slot(feat, 0)
        s = int(round(I ** 0.5))
        if feat is None:
            raise ValueError(f"HighLevel trains from cached trunk features: observations['{name}_features'] is missing; HCMEngine.encode_features "
                             "returns it from the frames")
        if feat.dim() != 4 or tuple(feat.shape) != (rows, C0, s, s):
            raise ValueError(f"HighLevel takes {name}_features ({rows}, {C0}, {s}, {s}) as HCMEngine.encode_features returns them, got {tuple(feat.shape)}")
        x = feat.flatten(2)
        cm, e = enc.tail()
        w = kv.weight[:, :, 0]
        tail = torch.addmm(kv.bias, e, w[:, C0:].t())                          # (I, vis_in): the same for every row
        tokens = torch.matmul(x.transpose(1, 2), w[:, :C0].t()) + tail
        if pooled:
            x_in = torch.addmm(torch.nn.functional.linear(cm.mean(1), fc.weight[:, C0:], fc.bias), x.mean(2), fc.weight[:, :C0].t())
        else:
            x_in = torch.addmm(torch.nn.functional.linear(cm.reshape(-1), fc.weight[:, C0 * I:], fc.bias), x.flatten(1), fc.weight[:, :C0 * I].t())
        return tokens, torch.relu(x_in)

    def _encode(self, batch, taps=None):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                        # :208
        rows = masks.shape[0]
        embedded = self._instruction_stream(observations, rows)
        cc, I_d = self.depth_shape
        rgb_tok, rgb_in = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder, self.rgb_linear[2], self.rgb_kv, True,
                                       cfg.ablate_rgb, rows, 2048, 16, embedded)
        dep_tok, dep_in = self._visual("depth", observations.get("depth_features"), self.depth_encoder, self.depth_linear[1], self.depth_kv, False,
                                       cfg.ablate_depth, rows, cc, I_d, embedded)
        ins_rgb = self.image_cm_encoder(embedded, rgb_tok, None, None).mean(1)      # :200, :209
        ins_dep = self.image_cm_encoder(embedded, dep_tok, None, None).mean(1)      # :201, :210
        x = torch.cat((rgb_in, dep_in, ins_rgb, ins_dep), 1)                   # :215
        if taps is not None:
            taps.update(rgb_kv=rgb_tok, depth_kv=dep_tok, rnn_in=x)
        return self.state_encoder(x, rnn_hidden_states, masks)                 # :219

    def forward(self, batch, taps=None):
        x, hidden = self._encode(batch, taps)
        return self.linear(x), hidden

    def update_loss(self, batch, oracle_subtask):
        """The forward and the criterion of the high-level half of `_update_agent` (hierarchical_trainer.py:505-511): the model up to the state
        encoder, then subtask_ce with oracle_subtask as the collate function carries it ((rows, 1) float, converted on the device).
        -> (result (8,), rnn_hidden_states); result[0] is the trainer's high-level loss."""
        x, hidden = self._encode(batch)
        if oracle_subtask.numel() != x.shape[0]:
            raise ValueError(f"update_loss takes oracle_subtask ({x.shape[0]}, 1), got {tuple(oracle_subtask.shape)}")
        return self._subtask_ce(x, self.linear.weight, self.linear.bias, oracle_subtask.to(x.device), self.cfg.num_sub_tasks)[0], hidden


class LowLevel(nn.Module):
    """The reference's Seq2Seq_LowLevel (models/seq2seq_lowlevel.py:21-162) as a trainable model from cached trunk features: the reference's
    parameters, state-dict keys and shapes outside the two frozen trunks (robo_vln_amd.synth.low_level_spec lists them), and its forward signature.
    Takes a robo_vln_amd.config.HCMConfig.

    forward((observations, rnn_hidden_states, prev_actions, masks, discrete_actions)) -> (output, stop_out, rnn_hidden_states) as :116-162, with
    observations["rgb_features"] (rows, 2048, 1, 1) and ["depth_features"] (rows, C, s, s) -- the low entries of HCMEngine.encode_features' pairs;
    a pair is accepted and its entry 1 taken; an ablated modality needs no key -- and discrete_actions (rows,) the sub-task of every row,
    num_sub_tasks on the padded ones.  rgb_encoder.fc and depth_encoder.visual_fc.1 with their ReLUs are torch, as in train.Seq2SeqNet;
    sub_task_embedding has padding_idx = num_sub_tasks (the reference writes 4, its num_sub_tasks): that row is zero at construction and gets
    no gradient; the cat is the reference's [depth | rgb | sub_task]; the state encoder is train.RNNStateEncoder.  progress_monitor holds
    parameters only (the trainer clears AuxLosses and adds no aux loss).

    update_loss(batch, corrected_actions, oracle_stop) -> (result (8,), rnn_hidden_states) is the model and the criterion of the trainer's
    low-level step through flat_heads_loss without the monitor; result[0] + result[1] is the loss.

    The SimpleCNN encoders are trunks that train with the model: there is nothing to cache, and they are refused."""

    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg):
        super().__init__()
        cfg.validate()
        _refuse_simple_cnn("LowLevel", cfg)
        self.cfg = cfg
        fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.depth_shape = (cc, fs)
        self.depth_encoder = _FlatDepthEncoder(cc * fs * fs, cfg.depth_out)
        self.rgb_encoder = _FlatRgbEncoder(cfg.rgb_out)
        self.sub_task_embedding = nn.Embedding(cfg.num_sub_tasks + 1, 32, padding_idx=cfg.num_sub_tasks)
        self.state_encoder = RNNStateEncoder(cfg.depth_out + cfg.rgb_out + 32, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        nn.init.kaiming_normal_(self.progress_monitor.weight, nonlinearity="tanh")     # _init_layers, :112-114
        nn.init.constant_(self.progress_monitor.bias, 0)
        self.linear = nn.Linear(cfg.hidden, cfg.lo_actions)
        self.stop_linear = nn.Linear(cfg.hidden, 1)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def load_reference_state_dict(self, sd):
        """Load a reference Seq2Seq_LowLevel state dict (tensors or arrays): the keys of the two frozen trunks are dropped, everything else is
        strict -- a missing, unexpected or misshapen key raises"""
        kept = {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(HCM_LOW_FROZEN_PREFIXES)}
        return self.load_state_dict(kept, strict=True)

    def _visual(self, name, feat, fc, ablated, rows, shape, like):
        """One modality's embedding relu(fc(flatten(feature))) (rows, out) from the trunk feature; ablated: times 0 (:132-135), and exact zeros
        without the key"""
        feat = _model_slot(feat, 1)
        if feat is None:
            if ablated:
                return _zero_grads(like.new_zeros(rows, fc.out_features), fc.weight, fc.bias)
            raise ValueError(f"LowLevel trains from cached trunk features: observations['{name}_features'] is missing; HCMEngine.encode_features "
                             "returns it from the frames")
        if tuple(feat.shape) != (rows, *shape):
            raise ValueError(f"LowLevel takes {name}_features {(rows, *shape)} as HCMEngine.encode_features returns them, got {tuple(feat.shape)}")
        y = torch.relu(fc(feat.flatten(1)))                                    # Flatten in NCHW order
        return y * 0 if ablated else y

    def _encode(self, batch):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks, discrete_actions = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                        # :145
        rows = masks.shape[0]
        if discrete_actions.numel() != rows or discrete_actions.dtype.is_floating_point:
            raise ValueError(f"LowLevel takes discrete_actions ({rows},) as an integer tensor, got {discrete_actions.dtype} {tuple(discrete_actions.shape)}")
        cc, fs = self.depth_shape
        depth = self._visual("depth", observations.get("depth_features"), self.depth_encoder.visual_fc[1], cfg.ablate_depth, rows, (cc, fs, fs),
                             rnn_hidden_states)
        rgb = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder.fc, cfg.ablate_rgb, rows, (2048, 1, 1), rnn_hidden_states)
        sub_task = self.sub_task_embedding(discrete_actions.reshape(-1).long())    # :141
        x = torch.cat([depth, rgb, sub_task], 1)                               # :143
        return self.state_encoder(x, rnn_hidden_states, masks)                 # :147

    def forward(self, batch):
        x, hidden = self._encode(batch)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of the low-level half of `_update_agent` (hierarchical_trainer.py:539-553): the model up to the state
        encoder, then flat_heads_loss without the monitor.  -> (result (8,), rnn_hidden_states); result[0] + result[1] is the trainer's loss."""
        x, hidden = self._encode(batch)
        return _heads_loss(self, x, corrected_actions, oracle_stop, None), hidden


def hier_update(high, low, opt_high, opt_low, observations, prev_actions, not_done_masks, corrected_actions, oracle_stop, hi_hidden, lo_hidden):
    """The reference's `_update_agent` (hierarchical_trainer.py:492-560) for train.HighLevel / train.LowLevel, in its order: zero both optimizers,
    detach both carried states (repackage_hidden), the high-level loss with its backward and step, then the low-level model teacher-forced with
    oracle - 1 -- num_sub_tasks where the label is 0 or out of range, formed by torch.where on the device -- with loss = result[0] + result[1],
    backward and step.  observations["vln_oracle_action_sensor"] is the label tensor as the collate function carries it, (rows, 1) float; it is
    converted on the device and `observations` is left as it was (the reference deletes keys from it).  Both models run on one device (the
    reference moves the low-level model's inputs to a second one).

    Returns (result_high, result_low, hi_hidden, lo_hidden), all detached and on the device: result_high (8,) as subtask_ce writes it, result_low
    (8,) as flat_heads_loss does, where the reference returns four host numbers: nothing is read back and nothing synchronises."""
    opt_high.zero_grad()
    opt_low.zero_grad()
    hi_hidden, lo_hidden = hi_hidden.detach(), lo_hidden.detach()
    if "vln_oracle_action_sensor" not in observations:
        raise ValueError("observations['vln_oracle_action_sensor'] is missing: the oracle sub-task of every row, (rows, 1)")
    oracle = observations["vln_oracle_action_sensor"]
    result_high, hi_hidden = high.update_loss((observations, hi_hidden, prev_actions, not_done_masks), oracle)
    result_high[0].backward()
    opt_high.step()

    n = low.cfg.num_sub_tasks
    o = oracle.to(lo_hidden.device).reshape(-1).to(torch.int64)
    discrete_actions = torch.where((o >= 1) & (o <= n), o - 1, torch.full_like(o, n))      # :522-524
    result_low, lo_hidden = low.update_loss((observations, lo_hidden, prev_actions, not_done_masks, discrete_actions), corrected_actions, oracle_stop)
    (result_low[0] + result_low[1]).backward()
    opt_low.step()
    return result_high.detach(), result_low.detach(), hi_hidden.detach(), lo_hidden.detach()
