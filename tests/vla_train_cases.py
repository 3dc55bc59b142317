"""Shared cases of the differentiable cross-modal layer (robo_vln_amd.train.vla_layer): inputs from a seeded generator and the float64
CPU-autograd reference through train.vla_layer_ref, computed once per case and never modified.

Inputs: q, I, kv and the cotangent uniform in +-1, weights and biases uniform in +-0.1, LayerNorm weights in 1 +- 0.5, LayerNorm biases in +-0.5;
keep masks `rand >= p` from the same generator (None when p = 0).

The ReLU kink is the one place where a float32 result may differ from float64 by more than round-off: a pre-activation whose sign flips changes a
whole gradient term.  So `case` asserts, in float64, that every fc1 pre-activation has magnitude >= KINK (2e-5; float32 torch deviates from
float64 by at most 3.2e-6 on these pre-activations), and SEEDS holds a seed per case for which it does.  That is a condition on the inputs, not
a tolerance: no element is excluded from any comparison.  `peaked_case` builds the PEAKED_CASES the same way with q times 16 (one key carries
most of a row's mass), under seeds of their own."""
import functools

import torch

from robo_vln_amd import train

D = 256
KINK = 2e-5
# (B, L, Lk, d_ff, p): one row and one key; a few rows; one row past the inference kernel's 80-row block (two row blocks of the training kernel);
# ragged rows with keys past 32; full d_ff with the most keys; whole row blocks without dropout; d_ff 512 with 36 keys (384-pixel depth frames).
# Then the launch forms those leave out (the attention backward is instantiated per KB = ceil(Lk / 16) key blocks): KB 2 at its lower edge; KB 2
# at its upper edge with three d_ff chunks; either side of the KB 3 / 4 edge; KB 1 with an idle key lane and three d_ff chunks; and 130 rows --
# three row blocks with a ragged last one, three 64-row chunks of the attention forward, three LayerNorm partials -- behind a KB 2 backward
CASES = [(1, 1, 1, 256, 0.0), (2, 5, 16, 256, 0.25), (1, 81, 16, 256, 0.25), (3, 17, 33, 256, 0.25), (1, 7, 64, 1024, 0.25), (2, 80, 16, 256, 0.0),
         (1, 33, 36, 512, 0.1),
         (2, 9, 17, 256, 0.25), (1, 5, 32, 768, 0.1), (1, 6, 48, 256, 0.0), (1, 6, 49, 512, 0.25), (2, 3, 15, 768, 0.0), (1, 130, 31, 256, 0.25)]
SEEDS = {(1, 1, 1, 256, 0.0): 0, (2, 5, 16, 256, 0.25): 0, (1, 81, 16, 256, 0.25): 10, (3, 17, 33, 256, 0.25): 1, (1, 7, 64, 1024, 0.25): 0,
         (2, 80, 16, 256, 0.0): 4, (1, 33, 36, 512, 0.1): 1}          # the first seed per case whose smallest |pre-activation| is >= 1e-4
SEEDS.update({(2, 9, 17, 256, 0.25): 1, (1, 5, 32, 768, 0.1): 0, (1, 6, 48, 256, 0.0): 0, (1, 6, 49, 512, 0.25): 0, (2, 3, 15, 768, 0.0): 0,
              (1, 130, 31, 256, 0.25): 0})     # first_seed() of each: the first from 0 that meets the kink condition (>= KINK; all six are >= 1e-4 too)
# Peaked attention: the first three of the new cases with q times PEAKED_Q_SCALE.  The listed inputs keep |score| / 8 below one, a softmax close to
# uniform; times 16 the largest probability of a row is about 0.8 in the mean, so that P (dP - sum P dP) cancels in the backward.
PEAKED_Q_SCALE = 16.0
PEAKED_CASES = [(2, 9, 17, 256, 0.25), (1, 5, 32, 768, 0.1), (1, 6, 48, 256, 0.0)]
PEAKED_SEEDS = {(2, 9, 17, 256, 0.25): 0, (1, 5, 32, 768, 0.1): 0, (1, 6, 48, 256, 0.0): 0}     # first_seed(..., q_scale=PEAKED_Q_SCALE)
NAMES = ("d_q", "d_I", "d_kv", "d_wo", "d_bo", "d_w1", "d_b1", "d_w2", "d_b2", "d_g1", "d_be1", "d_g2", "d_be2")


def make_inputs(B, L, Lk, d_ff, p, seed, q_scale=1.0):
    """(the thirteen float32 CPU tensors in vla_layer's order, keep masks or None, cotangent); q_scale multiplies q behind the draws, so that
    every other tensor of a seed is the same with and without it"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, scale=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale

    q, I, kv = u(B, L, D), u(B, L, D), u(B, Lk, 2 * D)
    wo, bo = u(D, D, scale=0.1), u(D, scale=0.1)
    w1, b1 = u(d_ff, D, scale=0.1), u(d_ff, scale=0.1)
    w2, b2 = u(D, d_ff, scale=0.1), u(D, scale=0.1)
    g1, be1, g2, be2 = 1 + u(D, scale=0.5), u(D, scale=0.5), 1 + u(D, scale=0.5), u(D, scale=0.5)
    keep = None
    if p > 0:
        keep = tuple((torch.rand(B * L, n, generator=g) >= p).to(torch.uint8) for n in (D, d_ff, D))
    cot = u(B, L, D)
    if q_scale != 1.0:
        q = q * q_scale
    return (q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2), keep, cot


def min_preactivation(args64, keep, p):
    """min |x1 W1^T + b1| of a case in float64"""
    q, I, kv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2 = args64
    x1 = train.vla_attention_ref(q, I, kv, wo, bo, g1, be1, keep[0] if keep is not None else None, p)
    return torch.nn.functional.linear(x1, w1, b1).abs().min().item()


def first_seed(B, L, Lk, d_ff, p, q_scale=1.0):
    """the first seed from 0 whose smallest |pre-activation| is >= KINK"""
    seed = 0
    while True:
        args, keep, _ = make_inputs(B, L, Lk, d_ff, p, seed, q_scale)
        if min_preactivation([t.double() for t in args], keep, p) >= KINK:
            return seed
        seed += 1


def _case(B, L, Lk, d_ff, p, seed, q_scale):
    args, keep, cot = make_inputs(B, L, Lk, d_ff, p, seed, q_scale)
    leaves = [t.double().requires_grad_() for t in args]
    kink = min_preactivation([t.detach() for t in leaves], keep, p)
    assert kink >= KINK, f"case {(B, L, Lk, d_ff, p)}: an fc1 pre-activation of magnitude {kink:.3e} sits on the ReLU kink; choose another seed"
    out64 = train.vla_layer_ref(*leaves, keep=keep, p=p)
    g64 = torch.autograd.grad(out64, leaves, cot.double())
    return dict(args=args, keep=keep, cot=cot, p=p, out64=out64.detach(), ref=dict(zip(NAMES, g64)), kink=kink)


@functools.lru_cache(maxsize=None)
def case(B, L, Lk, d_ff, p):
    """Inputs (float32, CPU), keep masks, cotangent, the float64 output and the thirteen float64 gradients of one listed case"""
    return _case(B, L, Lk, d_ff, p, SEEDS[(B, L, Lk, d_ff, p)], 1.0)


@functools.lru_cache(maxsize=None)
def peaked_case(B, L, Lk, d_ff, p):
    """`case` with q times PEAKED_Q_SCALE and the seed of PEAKED_SEEDS"""
    return _case(B, L, Lk, d_ff, p, PEAKED_SEEDS[(B, L, Lk, d_ff, p)], PEAKED_Q_SCALE)


def mean_peak(c):
    """the mean over rows and heads of the largest attention probability of a case, in float64"""
    q, kv = c["args"][0].double(), c["args"][2].double()
    B, L, _ = q.shape
    d_k = D // train.VLA_HEADS
    qh = q.reshape(B, L, train.VLA_HEADS, d_k).permute(0, 2, 1, 3)
    kh = kv[..., :D].reshape(B, kv.shape[1], train.VLA_HEADS, d_k).permute(0, 2, 3, 1)
    return torch.softmax(torch.matmul(qh, kh) / d_k ** 0.5, -1).max(-1).values.mean().item()


def rel(g, g64, what):
    """max|g - g64| / max|g64|, or exactly zero where the reference is identically zero (the rule of tests/test_state_scan_train_gpu.py)"""
    scale = g64.abs().max().item()
    if scale == 0:
        worst = g.abs().max().item()
        print(f"{what}: reference identically zero, result max {worst:.3e}")
        assert worst == 0, what
        return 0.0
    e = (g.double() - g64).abs().max().item() / scale
    print(f"{what}: {e:.3e}")
    return e
