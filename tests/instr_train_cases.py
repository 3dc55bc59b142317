"""Shared cases of the differentiable instruction encoder (robo_vln_amd.train.instr_scan): inputs from a seeded generator and the float64
CPU-autograd reference through train.instr_encoder_ref, computed once per case and never modified.

Inputs: weights and biases uniform in +-0.1, embedded rows and the cotangent uniform in +-1.  A case is (rnn, dirs, final, B, L): the lengths
come from LENGTHS, the cotangent has the shape of the result -- (B, L, dirs*H), or (B, H) for the final state."""
import functools

import torch

from robo_vln_amd import train
from tests.vla_train_cases import rel  # noqa: F401  (the project's bound rule, shared)

BOUND = 1e-5
# (rnn_type, directions, final_state_only)
SETTINGS = [("LSTM", 2, False), ("LSTM", 1, False), ("LSTM", 1, True), ("GRU", 2, False), ("GRU", 1, False), ("GRU", 1, True)]
# lengths per (B, L): one row of one token; a length-1 row beside a full one (one workgroup, partly filled); a row of full length, a row of
# length 1 and lengths either side of 32; nine rows (an odd count: the last workgroup holds one sample); and the two shapes at which two
# directions pass 128 workgroups at two and at four samples per workgroup
LENGTHS = {
    (1, 1): (1,),
    (3, 7): (7, 1, 4),
    (5, 33): (33, 17, 1, 20, 32),
    (9, 12): (12, 3, 7, 1, 9, 12, 5, 10, 2),
    (130, 3): tuple(1 + (3 * b + b // 7) % 3 for b in range(130)),
    (260, 2): tuple(1 + (b + b // 5) % 2 for b in range(260)),
}
PARAM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def grad_names(dirs):
    return ["d_emb"] + [f"d_{n}{sfx}" for sfx in ("", "_reverse")[:dirs] for n in PARAM_NAMES]


def make_inputs(rnn, dirs, final, B, L, H, E, seed):
    """(embedded (B, L, E), params per direction, cotangent), float32 on the CPU"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, scale=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale

    G = 4 if rnn == "LSTM" else 3
    params = [(u(G * H, E, scale=0.1), u(G * H, H, scale=0.1), u(G * H, scale=0.1), u(G * H, scale=0.1)) for _ in range(dirs)]
    emb = u(B, L, E)
    cot = u(B, H) if final else u(B, L, dirs * H)
    return emb, params, cot


def reference(emb, lengths, params, final, cot):
    """float64 CPU autograd through instr_encoder_ref: (result, gradients in grad_names order)"""
    e64 = emb.double().requires_grad_()
    p64 = [tuple(t.double().requires_grad_() for t in p) for p in params]
    y = train.instr_encoder_ref(e64, lengths, p64, final)
    leaves = [e64] + [t for p in p64 for t in p]
    return y.detach(), torch.autograd.grad(y, leaves, cot.double())


@functools.lru_cache(maxsize=None)
def case(rnn, dirs, final, B, L, H=256, E=50):
    lengths = torch.tensor(LENGTHS[(B, L)])
    emb, params, cot = make_inputs(rnn, dirs, final, B, L, H, E, 10000 * B + 100 * L + 10 * dirs + 2 * final + (rnn == "GRU"))
    y64, g64 = reference(emb, lengths, params, final, cot)
    return dict(emb=emb, params=params, cot=cot, lengths=lengths, y64=y64, ref=dict(zip(grad_names(dirs), g64)))


def saved64(emb, lengths, params):
    """What the training forward saves, from a float64 cell loop: gates (dirs, B, L, 4H) -- LSTM i,f,g,o; GRU r,z,n and hn = W_hn h + b_hn -- and
    c (dirs, B, L, H) (LSTM; None for GRU), NaN at inactive tokens; and the boolean activity mask (B, L)."""
    B, L = emb.shape[0], emb.shape[1]
    H = params[0][1].shape[1]
    lstm = params[0][1].shape[0] == 4 * H
    x = emb.double()
    gates = torch.full((len(params), B, L, 4 * H), float("nan"), dtype=torch.float64)
    cs = torch.full((len(params), B, L, H), float("nan"), dtype=torch.float64) if lstm else None
    for d, p in enumerate(params):
        w_ih, w_hh, b_ih, b_hh = (t.double() for t in p)
        for b in range(B):
            h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            n = int(lengths[b])
            for t in (range(n - 1, -1, -1) if d else range(n)):
                gi, gh = w_ih @ x[b, t] + b_ih, w_hh @ h + b_hh
                if lstm:
                    i, f, g, o = (gi + gh).chunk(4)
                    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                    c = f * c + i * g
                    h = o * torch.tanh(c)
                    gates[d, b, t] = torch.cat([i, f, g, o])
                    cs[d, b, t] = c
                else:
                    (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3), gh.chunk(3)
                    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
                    nn_ = torch.tanh(i_n + r * h_n)
                    h = (1 - z) * nn_ + z * h
                    gates[d, b, t] = torch.cat([r, z, nn_, h_n])
    active = torch.arange(L)[None, :] < lengths[:, None]
    return gates, cs, active
