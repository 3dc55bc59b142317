"""Shared cases of CMANet's differentiable attention (robo_vln_amd.train.attn1q): inputs from a seeded generator and the float64 CPU-autograd
reference through train.attn1q_ref, computed once per case and never modified.

A case is (layout, B, C0, Ce, I, mask_zero, want_dx, q_scale).  x, e and the cotangent are uniform in +-1, qt uniform in +-q_scale.  A masked case
zeroes the tail positions of each sample to differing lengths (MASK_LENGTHS; a length of 0 is a fully masked sample: uniform weights, xbar = 0).
q_scale = 4 makes a peaked case: one position carries much of a sample's mass, so that a (da - sum a da) cancels in the backward."""
import functools

import numpy as np
import torch

from robo_vln_amd import train

TM, CM = train.TOKEN_MAJOR, train.CHANNEL_MAJOR
PEAKED_Q_SCALE = 4.0
# the issue's table: one position; RGB; the five depth shapes (82 x 25 floats leave odd samples off a 16-byte boundary, 57 is no multiple of
# four); text with lengths 200, 150, 1 and 0; a short masked text; the trainer's L = 80; one position past a wave; the largest I
CASES = [
    (CM, 1, 4, 0, 1, False, False, 1.0),
    (CM, 3, 2048, 64, 16, False, False, 1.0),
    (CM, 2, 128, 64, 16, False, True, 1.0),
    (CM, 2, 512, 64, 4, False, False, 1.0),
    (CM, 3, 228, 64, 9, False, False, 1.0),
    (CM, 3, 82, 64, 25, False, False, 1.0),
    (CM, 2, 57, 64, 36, False, False, 1.0),
    (TM, 4, 512, 0, 200, True, False, 1.0),
    (TM, 3, 256, 0, 9, True, True, 1.0),
    (TM, 2, 512, 0, 80, False, False, 1.0),
    (TM, 2, 512, 0, 65, True, False, 1.0),
    (TM, 1, 256, 0, 256, False, False, 1.0),
]
PEAKED_CASES = [(CM, 3, 2048, 64, 16, False, False, PEAKED_Q_SCALE), (TM, 4, 512, 0, 200, True, False, PEAKED_Q_SCALE)]
# beyond the table, the forms it leaves out: dword access on token-major rows, with a tail and a mask; a channel-major sample with more than 64
# dword positions (several sweeps of a wave) and d_x; 16-byte token-major rows with a tail; a channel-major mask
EXTRA_CASES = [
    (TM, 3, 30, 8, 5, True, True, 1.0),
    (CM, 2, 6, 4, 130, False, True, 1.0),
    (TM, 2, 1028, 64, 7, False, False, 1.0),
    (CM, 3, 12, 0, 8, True, False, 1.0),
]
ALL_CASES = CASES + PEAKED_CASES + EXTRA_CASES
MASK_LENGTHS = {4: (None, 150, 1, 0), 3: (None, 4, 0), 2: (None, 0)}       # per B; None = the whole sample stays
NAMES = ("d_qt", "d_x", "d_e")


def positions(x, layout):
    """x as (B, I, C0) whatever its layout (a view)"""
    return x if layout == TM else x.transpose(1, 2)


def make_inputs(layout, B, C0, Ce, I, mask_zero, want_dx, q_scale, seed=0):
    """(qt, x, e or None, cotangent), float32 on the CPU.  In a masked case with a tail, the tail rows behind the longest kept length are zeroed
    too: a position is masked only when ALL its channels are zero."""
    g = torch.Generator().manual_seed(seed)

    def u(*shape):
        return torch.rand(*shape, generator=g) * 2 - 1

    qt = u(B, C0 + Ce) * q_scale
    x = u(B, I, C0) if layout == TM else u(B, C0, I)
    e = u(I, Ce) if Ce else None
    cot = u(B, C0 + Ce)
    if mask_zero:
        lengths = [I if n is None else min(n, I) for n in MASK_LENGTHS[B]]
        for b, n in enumerate(lengths):
            positions(x, layout)[b, n:] = 0
        if e is not None:
            e[max(1, I - 2):] = 0
    return qt, x, e, cot


@functools.lru_cache(maxsize=None)
def case(layout, B, C0, Ce, I, mask_zero, want_dx, q_scale):
    """Inputs, cotangent, and in float64 the output, the weights and the gradients (d_x always: want_dx only says whether the device computes it)"""
    qt, x, e, cot = make_inputs(layout, B, C0, Ce, I, mask_zero, want_dx, q_scale)
    leaves = [t.double().requires_grad_() for t in (qt, x, e) if t is not None]
    taps = {}
    out64 = train.attn1q_ref(leaves[0], leaves[1], leaves[2] if e is not None else None, mask_zero, 1.0 / 16.0, layout, _taps=taps)
    g64 = torch.autograd.grad(out64, leaves, cot.double())
    ref = dict(zip(NAMES, g64))
    return dict(qt=qt, x=x, e=e, cot=cot, scale=1.0 / 16.0, out64=out64.detach(), a64=taps["a"].detach(), ref=ref)


def mean_peak(c):
    """the mean over samples of the largest weight of a case, in float64"""
    return c["a64"].max(1).values.mean().item()


def module_batch(obs, h0, masks, conv=lambda t: t):
    """train.CMANet's batch (observations with features, state, prev_actions, masks) from numpy observations; conv moves or casts each tensor"""
    o = {k: conv(torch.from_numpy(np.asarray(obs[k]))) for k in ("rgb_features", "depth_features")}
    o["instruction"] = conv(torch.from_numpy(np.asarray(obs["instruction"])))
    return o, conv(h0.clone()), None, conv(torch.from_numpy(masks).reshape(-1, 1))
