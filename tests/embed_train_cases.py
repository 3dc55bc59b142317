"""Shared cases of the differentiable prologue half (robo_vln_amd.train.embed_ln): inputs from a seeded generator and the float64 CPU-autograd
reference through train.embed_ln_ref, computed once per case and never modified.

Inputs: x and the cotangent uniform in +-1, W and b uniform in +-0.1, gamma in 1 +- 0.5, beta in +-0.5; the keep mask `rand >= p` from the same
generator (None when p = 0); post = sinusoid_table(period, 256) (None when period = 0).

The ReLU kink, as in tests/vla_train_cases.py: `case` asserts, in float64, that every pre-activation x W^T + b has magnitude >= KINK (2e-5; a
float32 k-ordered chain over K <= 1024 products of magnitude <= 0.1 deviates from float64 by a few 1e-6 at most), and SEEDS holds, per case, the
first seed from 0 for which it does.  That is a condition on the inputs, not a tolerance: no element is excluded from any comparison."""
import functools

import torch

from robo_vln_amd import train
from tests.vla_train_cases import rel  # noqa: F401  (the project's bound rule, shared)

D = 256
KINK = 2e-5
# (rows, K, period or 0, p, want_dx): one row, smallest K; a few rows with a table; one short of the 64-row block; one row past it at BERT's width
# without d_x; two blocks and a ragged tail with K in three slices; whole blocks at the largest K without dropout or table.
# Then K past one 256 slice without being a multiple of it (a full slice, then a ragged one of 64 or 192 with zero fill behind it; in the backward
# a last d_x panel of 2 or 6 tiles at a non-zero offset into the packed weight): one full slice + 64; 192 behind one full slice with two row blocks
# and a table whose period does not divide the block; two full slices + 64; three full + 192 on exactly one row block; a single 192 slice; and
# three row blocks with three full slices + 64 without d_x; and, to complete the tails behind a full slice, one full slice + 128 (a 4-tile d_x panel
# at a non-zero offset)
CASES = [(1, 64, 0, 0.0, True), (5, 256, 5, 0.25, True), (63, 128, 0, 0.25, True), (65, 768, 13, 0.25, False), (130, 768, 65, 0.1, True),
         (128, 1024, 0, 0.0, True),
         (3, 320, 0, 0.25, True), (66, 448, 7, 0.1, True), (5, 576, 0, 0.0, True), (64, 960, 0, 0.25, True), (2, 192, 2, 0.0, True),
         (129, 832, 0, 0.25, False), (4, 384, 3, 0.1, True)]
SEEDS = {(1, 64, 0, 0.0, True): 0, (5, 256, 5, 0.25, True): 0, (63, 128, 0, 0.25, True): 2, (65, 768, 13, 0.25, False): 1,
         (130, 768, 65, 0.1, True): 1, (128, 1024, 0, 0.0, True): 0,
         (3, 320, 0, 0.25, True): 0, (66, 448, 7, 0.1, True): 0, (5, 576, 0, 0.0, True): 0, (64, 960, 0, 0.25, True): 2, (2, 192, 2, 0.0, True): 0,
         (129, 832, 0, 0.25, False): 1, (4, 384, 3, 0.1, True): 0}          # first_seed() of each case
NAMES = ("d_x", "d_w", "d_b", "d_gamma", "d_beta")


def make_inputs(rows, K, period, p, seed):
    """((x, w, b, gamma, beta) float32 on the CPU, keep mask or None, post or None, cotangent)"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, scale=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale

    x, w, b = u(rows, K), u(D, K, scale=0.1), u(D, scale=0.1)
    gamma, beta = 1 + u(D, scale=0.5), u(D, scale=0.5)
    keep = (torch.rand(rows, D, generator=g) >= p).to(torch.uint8) if p > 0 else None
    cot = u(rows, D)
    post = train.sinusoid_table(period, D) if period else None
    return (x, w, b, gamma, beta), keep, post, cot


def min_preactivation(x, w, b):
    return torch.nn.functional.linear(x.double(), w.double(), b.double()).abs().min().item()


def first_seed(rows, K, period, p):
    """the first seed from 0 whose smallest |pre-activation| is >= KINK"""
    seed = 0
    while min_preactivation(*make_inputs(rows, K, period, p, seed)[0][:3]) < KINK:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def case(rows, K, period, p, want_dx):
    """Inputs (float32, CPU), keep mask, table, cotangent, and in float64: y, xhat, rstd, the gate and the five gradients of one listed case"""
    args, keep, post, cot = make_inputs(rows, K, period, p, SEEDS[(rows, K, period, p, want_dx)])
    leaves = [t.double().requires_grad_() for t in args]
    x, w, b, gamma, beta = leaves
    pre = torch.nn.functional.linear(x, w, b).detach()
    kink = pre.abs().min().item()
    assert kink >= KINK, f"case {(rows, K, period, p, want_dx)}: a pre-activation of magnitude {kink:.3e} sits on the ReLU kink; choose another seed"
    y64 = train.embed_ln_ref(*leaves, keep=keep, p=p, post=post)
    g64 = torch.autograd.grad(y64, leaves, cot.double())
    r = train.mask_dropout(torch.relu(pre), keep, p)
    rstd64 = 1 / torch.sqrt(r.var(1, unbiased=False) + 1e-5)
    xhat64 = (r - r.mean(1, keepdim=True)) * rstd64[:, None]
    gate = (pre > 0) & (keep.bool() if keep is not None else torch.ones_like(pre, dtype=torch.bool))
    return dict(args=args, keep=keep, post=post, cot=cot, p=p, y64=y64.detach(), xhat64=xhat64, rstd64=rstd64, gate=gate.to(torch.uint8),
                ref=dict(zip(NAMES, g64)), kink=kink)
