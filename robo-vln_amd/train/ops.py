"""The training ops: eight autograd functions over the HIP training kernels, each with its public wrapper and its pure-torch restatement.  Device
tensors go through the kernels, at the sizes the kernels are built for, and anything else on the device raises; the restatement is the CPU
path of the drop-in modules (train/modules.py) and what the GPU tests compare against, not a fallback for a missing kernel.

`state_scan`: the time-serial part of the reference's RNNStateEncoder (models/decoder/state_encoder.py), forward and backward, on the scan kernels
(csrc/state_scan.hip, csrc/state_scan_bwd.hip) -- hidden size 512, one layer, float32; `cell_loop` is the restatement, a per-step cell loop with
h * mask in front of every step.

`vla_layer`: the reference's InterModuleAttnLayer (models/transformer/transformer.py:209-221) behind its three projections -- attention, fc_o,
dropout, LayerNorm, the feed-forward block, dropout, LayerNorm -- on the float32 kernels of csrc/vla_train.hip, forward and backward;
`vla_layer_ref` is the restatement.

`embed_ln`: one half of the prologue of the reference's Visual_Ling_Attn (transformer.py:250-282) -- Linear, ReLU, dropout, the shared LayerNorm,
and for the instruction half the sinusoid table -- on the float32 kernels of csrc/embed_train.hip, one launch forward and one backward per half;
`embed_ln_ref` is the restatement, `sinusoid_table` the reference's table.

`instr_scan`: the packed nn.LSTM / nn.GRU of the reference's InstructionEncoder (models/encoders/instruction_encoder.py:70-92), hidden size 256 in
one or two directions, with the whole scan forward and the whole scan backward one launch each (csrc/instr_scan.hip) and the lengths read on
the device; `instr_encoder_ref` is the restatement.

`attn1q`: the attention stage of the reference's CMANet (models/cma.py:271-311).  It has one query per sample and keys that are a 1x1 convolution of
the raw tokens, so the key projection folds into the query (qt = q W_k; q.b_k cancels in the softmax) and K and V are never formed; the kernels
are csrc/cma_attn_train.hip, `attn1q_ref` is the restatement.

`flat_heads_loss`: the end of the flat trainer's `_update_agent` (robo_vln_trainer.py:505-542) -- `linear`, `stop_linear`, tanh(`progress_monitor`)
and the masked criteria -- over csrc/flat_heads_train.hip (two launches forward, two backward); `flat_heads_loss_ref` is the restatement.

`subtask_ce`: the high-level criterion of the hierarchical trainer's `_update_agent` (hierarchical_trainer.py:492-560) -- `linear`, masked_fill_,
CrossEntropyLoss(ignore_index=-1) -- over csrc/subtask_ce_train.hip (two launches forward, two backward); `subtask_ce_ref` is the restatement.

`simple_cnn`: the convolutional part of the reference's SimpleAllCNN.cnn (models/encoders/simple_cnns.py:76-95) -- Conv2d(Cin, 32, 8, 4), ReLU,
Conv2d(32, 64, 4, 2), ReLU, Conv2d(64, 32, 3, 1) over depth or RGB frames -- on the float32 kernels of csrc/simplecnn_train.hip, one launch per
convolution forward, and backward a weight-gradient launch with its ordered reduce, a bias sum and a data-gradient launch per layer;
`simple_cnn_ref` is the restatement."""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from .. import _lib

SCAN_HIDDEN = 512
INSTR_HIDDEN = 256
VLA_D_MODEL, VLA_HEADS, VLA_MAX_KEYS, VLA_MAX_D_FF = 256, 4, 64, 1024
EMBED_K_STEP, EMBED_MAX_K = 64, 1024
SIMPLE_CNN_MIN_HW, SIMPLE_CNN_CHANNELS = 36, (1, 3)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _on_device(op, ref, anchor_name, anchor, named):
    """The kernels take raw pointers, and a host pointer would fault on the device: `anchor` must be a device tensor (CPU tensors go through the
    restatement `ref`) and every tensor of `named`, (name, tensor or None) pairs, must lie where it does"""
    if not anchor.is_cuda:
        raise ValueError(f"{op} runs on the device; CPU tensors go through {ref}")
    for name, t in named:
        if t is not None and t.device != anchor.device:
            raise ValueError(f"{op}: {name} is on {t.device}, {anchor_name} on {anchor.device}")


def _check_shapes(op, shapes):
    """shapes: (name, tensor, expected shape) triples"""
    for name, t, shape in shapes:
        if tuple(t.shape) != shape:
            raise ValueError(f"{op}: {name} has shape {tuple(t.shape)}, expected {shape}")


class _StateScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight_ih, weight_hh, bias_ih, bias_hh, hidden_states, masks):
        H = weight_hh.shape[1]
        G = weight_hh.shape[0] // H
        _on_device("state_scan", "cell_loop", "x", x, (("weight_ih", weight_ih), ("weight_hh", weight_hh), ("bias_ih", bias_ih), ("bias_hh", bias_hh),
                                                       ("hidden_states", hidden_states), ("masks", masks)))
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
        named = (("I", I), ("kv", kv), ("wo", wo), ("bo", bo), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("g1", g1), ("be1", be1),
                 ("g2", g2), ("be2", be2), ("keep[0]", keep1), ("keep[1]", keep2), ("keep[2]", keep3))
        _on_device("vla_layer", "vla_layer_ref", "q", q, named)
        D = VLA_D_MODEL
        if q.dim() != 3 or q.shape[2] != D or I.shape != q.shape or kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * D:
            raise ValueError(f"vla_layer serves q, I (B, L, {D}) and kv (B, Lk, {2 * D}), got {tuple(q.shape)}, {tuple(I.shape)}, {tuple(kv.shape)}")
        B, L, Lk, d_ff = q.shape[0], q.shape[1], kv.shape[1], w1.shape[0]
        if B < 1 or L < 1 or not 1 <= Lk <= VLA_MAX_KEYS or d_ff % 256 or not 256 <= d_ff <= VLA_MAX_D_FF:
            raise ValueError(f"vla_layer serves B, L >= 1, 1..{VLA_MAX_KEYS} keys and d_ff a multiple of 256 up to {VLA_MAX_D_FF}, got B {B}, L {L}, Lk {Lk}, d_ff {d_ff}")
        _check_shapes("vla_layer", (("wo", wo, (D, D)), ("bo", bo, (D,)), ("w1", w1, (d_ff, D)), ("b1", b1, (d_ff,)), ("w2", w2, (D, d_ff)),
                                    ("b2", b2, (D,)), ("g1", g1, (D,)), ("be1", be1, (D,)), ("g2", g2, (D,)), ("be2", be2, (D,))))
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
        _on_device("embed_ln", "embed_ln_ref", "x", x, (("w", w), ("b", b), ("gamma", gamma), ("beta", beta), ("keep", keep), ("post", post)))
        D, K = VLA_D_MODEL, x.shape[-1] if x.dim() else 0
        if x.dim() < 2 or not embed_k_ok(K):
            raise ValueError(f"embed_ln serves x (..., K) with K a multiple of {EMBED_K_STEP} from {EMBED_K_STEP} to {EMBED_MAX_K}, got {tuple(x.shape)}")
        _check_shapes("embed_ln", (("w", w, (D, K)), ("b", b, (D,)), ("gamma", gamma, (D,)), ("beta", beta, (D,))))
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


def _instr_names(d):
    return [f"{n} of direction {d}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


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
        _check_shapes("instruction scan", zip(_instr_names(d), p, ((G * H, E), (G * H, H), (G * H,), (G * H,))))
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
        named = [pair for d, p in enumerate(params) for pair in zip(_instr_names(d), p)] + [("lengths", lengths)]
        _on_device("instr_scan", "instr_encoder_ref", "embedded", embedded, named)
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
        _on_device("attn1q", "attn1q_ref", "qt", qt, (("x", x), ("e", e)))
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
        named = (("w_lin", w_lin), ("b_lin", b_lin), ("w_stop", w_stop), ("b_stop", b_stop), ("w_pm", w_pm), ("b_pm", b_pm),
                 ("corrected_actions", corrected_actions), ("oracle_stop", oracle_stop), ("progress", progress))
        _on_device("flat_heads_loss", "flat_heads_loss_ref", "x", x, named)
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
        _check_shapes("flat_heads_loss", shapes)
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
        _on_device("subtask_ce", "subtask_ce_ref", "x", x, (("w", w), ("b", b), ("oracle_subtask", oracle)))
        if x.dim() != 2 or w.dim() != 2 or not subtask_ce_ok(x.shape[0], x.shape[1], w.shape[0], num_sub_tasks):
            raise ValueError(f"subtask_ce serves x (rows >= 1, {SUBTASK_CE_HIDDEN}) and 1 <= num_sub_tasks <= A <= {SUBTASK_CE_MAX_CLASSES} classes, got "
                             f"x {tuple(x.shape)}, w {tuple(w.shape)}, num_sub_tasks {num_sub_tasks}")
        rows, H, A = x.shape[0], x.shape[1], w.shape[0]
        _check_shapes("subtask_ce", (("w", w, (A, H)), ("b", b, (A,)), ("oracle_subtask", oracle, (rows,))))
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


def simple_cnn_out_hw(H, W):
    """(h3, w3) of the last map for an H x W frame: three unpadded convolutions, 8/4, 4/2, 3/1 (simple_cnns.py:63-73)"""
    for k, st in ((8, 4), (4, 2), (3, 1)):
        H, W = (H - k) // st + 1, (W - k) // st + 1
    return H, W


def simple_cnn_ref(x, w1, b1, w2, b2, w3, b3, scale=1.0, _taps=None):
    """Pure-torch restatement of the convolutional part of SimpleAllCNN.cnn, any dtype and device: x (B, H, W, Cin) as the observations carry the
    frames, permuted to NCHW and multiplied by `scale` (simple_cnns.py:122-125, :144-147: 1/255 for RGB); the weights as nn.Conv2d stores them.
    Returns (B, 32, h3, w3); .flatten(1) is the reference's Flatten order in front of cnn.7."""
    F = torch.nn.functional
    x = x.to(w1.dtype).permute(0, 3, 1, 2) * scale
    p1 = F.conv2d(x, w1, b1, stride=4)
    p2 = F.conv2d(torch.relu(p1), w2, b2, stride=2)
    if _taps is not None:
        _taps.update(pre1=p1, pre2=p2)
    return F.conv2d(torch.relu(p2), w3, b3, stride=1)


def _simple_cnn_check(x, w1, b1, w2, b2, w3, b3):
    """the refusals of simple_cnn that need no device"""
    if x.requires_grad:
        raise ValueError("simple_cnn: the frames must not require a gradient (there is no frame gradient)")
    if x.dim() != 4 or x.shape[3] not in SIMPLE_CNN_CHANNELS:
        raise ValueError(f"simple_cnn takes frames (B, H, W, Cin) with Cin in {SIMPLE_CNN_CHANNELS}, got {tuple(x.shape)}")
    B, H, W, Cin = x.shape
    if H < SIMPLE_CNN_MIN_HW or W < SIMPLE_CNN_MIN_HW:
        raise ValueError(f"simple_cnn: frames must be at least {SIMPLE_CNN_MIN_HW} x {SIMPLE_CNN_MIN_HW}, got {H} x {W}")
    if x.dtype != torch.float32 and not (x.dtype == torch.uint8 and Cin == 3):
        raise ValueError(f"simple_cnn takes float32 frames, or uint8 RGB frames, got {x.dtype} with {Cin} channel(s)")
    _check_shapes("simple_cnn", (("w1", w1, (32, Cin, 8, 8)), ("b1", b1, (32,)), ("w2", w2, (64, 32, 4, 4)), ("b2", b2, (64,)),
                                 ("w3", w3, (32, 64, 3, 3)), ("b3", b3, (32,))))
    return B, H, W, Cin


class _SimpleCnn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, scale):
        _on_device("simple_cnn", "simple_cnn_ref", "x", x, (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("w3", w3), ("b3", b3)))
        B, H, W, Cin = _simple_cnn_check(x, w1, b1, w2, b2, w3, b3)
        n = _lib.lib().hcm_op_simplecnn_work_floats(B, H, W, Cin)
        if B < 1 or not n:
            raise ValueError(f"simple_cnn serves B >= 1 and calls whose element offsets fit 31 bits, got frames {tuple(x.shape)}")
        x = x.detach().contiguous()
        w1, b1, w2, b2, w3, b3 = (_f32c(t) for t in (w1, b1, w2, b2, w3, b3))
        dt = _lib.HCM_U8 if x.dtype == torch.uint8 else _lib.HCM_F32
        h3, w3_ = simple_cnn_out_hw(H, W)
        y = torch.empty(B, 32, h3, w3_, device=x.device)
        work = torch.empty(n, device=x.device)
        _lib.check(_lib.lib().hcm_op_simplecnn_train(_ptr(x), dt, scale, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(y), _ptr(work),
                                                     B, H, W, Cin, _stream()))
        ctx.save_for_backward(x, w2, w3, work)
        ctx.dims = (B, H, W, Cin, dt, scale)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        x, w2, w3, work = ctx.saved_tensors
        B, H, W, Cin, dt, scale = ctx.dims
        dev = x.device
        d_y = _f32c(d_y)
        d_w1, d_b1 = torch.empty(32, Cin, 8, 8, device=dev), torch.empty(32, device=dev)
        d_w2, d_b2 = torch.empty(64, 32, 4, 4, device=dev), torch.empty(64, device=dev)
        d_w3, d_b3 = torch.empty(32, 64, 3, 3, device=dev), torch.empty(32, device=dev)
        _lib.check(_lib.lib().hcm_op_simplecnn_bwd(_ptr(d_y), _ptr(x), dt, scale, _ptr(w2), _ptr(w3), _ptr(work), _ptr(d_w1), _ptr(d_b1), _ptr(d_w2),
                                                   _ptr(d_b2), _ptr(d_w3), _ptr(d_b3), B, H, W, Cin, _stream()))
        need = ctx.needs_input_grad
        return (None, *(g if need[1 + i] else None for i, g in enumerate((d_w1, d_b1, d_w2, d_b2, d_w3, d_b3))), None)


def simple_cnn(x, w1, b1, w2, b2, w3, b3, scale=1.0):
    """The convolutional part of SimpleAllCNN.cnn (float32, on the device) with gradients to the six parameters: arguments and result as
    simple_cnn_ref; frames (B >= 1, H, W, Cin) with Cin 1 or 3 and H, W >= 36 (non-square and any remainder allowed), float32 or, for RGB, uint8;
    a frame that requires a gradient, another Cin, a smaller frame or another dtype raises ValueError.

    Forward: hcm_op_simplecnn_train packs the weights and runs one launch per convolution; the two post-ReLU maps stay in the call's work
    buffer, which the autograd node keeps.  Backward: hcm_op_simplecnn_bwd on that buffer -- per layer a weight-gradient launch over chunks of
    pixels with an ordered reduce, a bias sum, and for conv3 and conv2 a data-gradient launch gated by `stored value > 0`.  There is no frame
    gradient.  A row's forward bits depend on that row and the weights alone, and two runs give the same bits.  cnn.7 behind it is a dense
    product and stays in torch.  Nothing is cached between calls: the weights are packed on the device in every call."""
    _simple_cnn_check(x, w1, b1, w2, b2, w3, b3)
    return _SimpleCnn.apply(x, w1, b1, w2, b2, w3, b3, float(scale))
