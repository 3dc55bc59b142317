"""Shared cases of the flat trainer's fused heads and criterion (robo_vln_amd.train.flat_heads_loss): inputs from a seeded generator, the float64
CPU-autograd reference through train.flat_heads_loss_ref, computed once per case and never modified, the same criterion written with torch's
criterion classes (`torch_criteria`), and the launch rules of csrc/flat_heads_train.hip restated for the coverage test.

Inputs: x ~ N(0, 1); weights ~ N(0, 1/512), so that every head output is ~ N(0, 1) and the tanh of the monitor sits in its middle range; biases
~ N(0, 0.01); corrected_actions ~ N(0, 1) and oracle_stop in {0, 1} with the label edges at fixed rows (`labels`); progress uniform in [0, 1];
the cotangent of the three losses is (0.7, 1.3, 0.9).  Test infrastructure only."""
import functools
import math

import numpy as np
import torch
from torch import nn

from robo_vln_amd import synth, train
from robo_vln_amd.config import CMAConfig, S2SConfig

H = 512
COT = (0.7, 1.3, 0.9)
# (rows, num_actions, monitor, d_x).  Rows: one below, at and one above the forward's 4 rows per workgroup; the backward's half block (16) and row
# block (32), the second block's edges (63, 64, 65) and the criterion's 256-thread stride; 300 rows end in a ragged block of 12 (one half idle),
# 600 rows are more than two per criterion thread.  num_actions 1, 2, 4, the monitor and d_x each on and off at small and at large sizes.
CASES = [(1, 2, True, True), (2, 2, False, True), (3, 1, True, False), (4, 4, True, True), (5, 2, True, True),
         (15, 2, False, False), (16, 1, True, True), (17, 2, True, True),
         (31, 4, False, True), (32, 2, True, True), (33, 2, True, False),
         (63, 1, False, True), (64, 2, True, True), (65, 4, True, True),
         (255, 2, False, True), (256, 2, True, True), (257, 1, True, False),
         (300, 2, True, True), (600, 2, True, True), (600, 4, False, False)]
NAMES = ("d_x", "d_w_lin", "d_b_lin", "d_w_stop", "d_b_stop", "d_w_pm", "d_b_pm")
# A bias gradient is ONE number per head, a sum over the rows that can cancel, and a single row's output can be a cancelling dot product: relative
# to itself such a number is as badly conditioned as the draw makes it.  So each case takes the first seed from 0 for which the float32
# restatement on the CPU stays within SEED_BOUND of its float64 run in every tensor (first_seed; a fifth of the half bound that
# test_float32_restatement_stays_within_half_the_bound asserts).  A condition on the inputs, not a tolerance: no tensor is left out of a comparison.
SEED_BOUND = 1e-6
SEEDS = {(1, 2, True, True): 1}          # every other case: seed 0


# ---- the launch rules of csrc/flat_heads_train.hip, restated: a change there must change these, and the cases with them
def fwd_workgroups(rows):
    """the heads launch: a wave per row, 4 rows per workgroup"""
    return math.ceil(rows / train.FLAT_HEADS_FWD_ROWS)


def bwd_blocks(rows):
    """the backward's main launch: a workgroup per block of 32 rows; (blocks, rows of the last block, rows of its first and second half)"""
    n = math.ceil(rows / train.FLAT_HEADS_BWD_ROWS)
    last = rows - (n - 1) * train.FLAT_HEADS_BWD_ROWS
    return n, last, min(last, train.FLAT_HEADS_BWD_HALF), max(0, last - train.FLAT_HEADS_BWD_HALF)


def criterion_rows_per_thread(rows):
    """flat_val_loss_kernel: one workgroup of 256 threads, thread t adds the rows t, t + 256, ...: the most rows any thread adds"""
    return math.ceil(rows / train.FLAT_LOSS_THREADS)


def labels(rows, A, g):
    """(corrected (rows, A), oracle_stop (rows, 1), progress (rows,)): row r is padded (corrected 0, stop -1) where r % 7 == 4; a valid row has an
    exact 0 in column 0 where r % 5 == 1 (it leaves the aux selection and stays in the stop loss) and in its last column alone where r % 6 == 3
    and A > 1 (it stays in both)"""
    corrected = torch.randn(rows, A, generator=g)
    stop = (torch.rand(rows, 1, generator=g) < 0.5).float()
    for r in range(rows):
        if r % 7 == 4:
            corrected[r], stop[r] = 0.0, -1.0
        elif r % 5 == 1:
            corrected[r, 0] = 0.0
        elif r % 6 == 3 and A > 1:
            corrected[r, A - 1] = 0.0
    return corrected, stop, torch.rand(rows, generator=g)


def make_inputs(rows, A, monitor, seed=0):
    """float32 CPU tensors in flat_heads_loss's argument order (w_pm, b_pm, progress None without the monitor)"""
    g = torch.Generator().manual_seed(1000 * rows + 10 * A + seed)
    x = torch.randn(rows, H, generator=g)
    w = [torch.randn(n, H, generator=g) / math.sqrt(H) for n in (A, 1, 1)]
    b = [torch.randn(n, generator=g) * 0.1 for n in (A, 1, 1)]
    corrected, stop, progress = labels(rows, A, g)
    pm = (w[2], b[2], progress) if monitor else (None, None, None)
    return (x, w[0], b[0], w[1], b[1], pm[0], pm[1], corrected, stop, pm[2])


def cotangent(dtype=torch.float32, device="cpu"):
    return torch.tensor(COT + (0.0,) * 5, dtype=dtype, device=device)


def leaves_of(args, dx, conv):
    """`args` through conv, the differentiable ones made leaves: ([all ten], {name: leaf})"""
    out, named = [], {}
    for i, t in enumerate(args):
        if t is None:
            out.append(None)
            continue
        t = conv(t)
        if i < 7 and (i > 0 or dx):
            t = t.requires_grad_()
            named[NAMES[i]] = t
        out.append(t)
    return out, named


def run(fn, args, dx, conv):
    """fn (flat_heads_loss or its restatement) on the case's inputs through conv -> (result, out, stop, progress_hat, {name: gradient})"""
    a, named = leaves_of(args, dx, conv)
    result, out, stop, progress_hat = fn(*a)
    grads = torch.autograd.grad(result, list(named.values()), cotangent(result.dtype, result.device))
    return result.detach(), out.detach(), stop.detach(), None if progress_hat is None else progress_hat.detach(), dict(zip(named, grads))


def conditioning(rows, A, monitor, dx, seed):
    """the largest per-tensor max|t32 - t64| / max|t64| of the float32 restatement against its float64 run: the three losses, out, stop,
    progress_hat and every gradient"""
    args = make_inputs(rows, A, monitor, seed=seed)
    r64 = run(train.flat_heads_loss_ref, args, dx, lambda t: t.double())
    r32 = run(train.flat_heads_loss_ref, args, dx, lambda t: t)
    pairs = [(r32[0][:3], r64[0][:3])] + [(a, b) for a, b in zip(r32[1:4], r64[1:4]) if b is not None] + [(r32[4][n], r64[4][n]) for n in r64[4]]
    return max(((a.double() - b).abs().max() / b.abs().max()).item() for a, b in pairs)


def first_seed(rows, A, monitor, dx):
    seed = 0
    while conditioning(rows, A, monitor, dx, seed) > SEED_BOUND:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def case(rows, A, monitor, dx):
    """Inputs (float32, CPU) and the float64 reference of one case: dict(args, result64, out64, stop64, progress_hat64, ref={name: gradient})"""
    args = make_inputs(rows, A, monitor, seed=SEEDS.get((rows, A, monitor, dx), 0))
    result, out, stop, progress_hat, grads = run(train.flat_heads_loss_ref, args, dx, lambda t: t.double())
    return dict(args=args, result64=result, out64=out, stop64=stop, progress_hat64=progress_hat, ref=grads)


def torch_criteria(x, w_lin, b_lin, w_stop, b_stop, w_pm, b_pm, corrected, oracle_stop, progress):
    """tests/flat_val_ref.criteria in the inputs' dtype and with the graph kept: the heads by F.linear / tanh, then torch's criterion classes
    statement by statement as robo_vln_trainer.py:521-533 -> (action loss, stop loss, aux loss (0.0 without the monitor), stop rows, aux rows)"""
    F = nn.functional
    out, stop = F.linear(x, w_lin, b_lin), F.linear(x, w_stop, b_stop)
    corrected = corrected.to(x.dtype).reshape(out.shape)
    oracle_stop = oracle_stop.to(x.dtype).reshape(-1, 1)
    action_mask = corrected == 0
    action = nn.MSELoss()(out.clone().masked_fill_(action_mask, 0), corrected)
    keep = oracle_stop != -1
    stop_loss = nn.BCEWithLogitsLoss()(torch.masked_select(stop, keep), torch.masked_select(oracle_stop, keep))
    aux, n_aux = 0.0, 0
    if w_pm is not None:
        p = torch.tanh(F.linear(x, w_pm, b_pm))
        aux_mask = ~action_mask[:, 0]
        aux = 1.0 * torch.masked_select(F.mse_loss(p.squeeze(1), progress.to(x.dtype).reshape(-1), reduction="none"), aux_mask).mean()
        n_aux = int(aux_mask.sum())
    return action, stop_loss, aux, int(keep.sum()), n_aux


def module_case(kind, monitor, T=3, N=2):
    """(config, train.Seq2SeqNet ("s2s") or train.CMANet ("cma") with seeded reference weights, the batch (observations with random post-ReLU
    features of the trunks' shapes, h0, prev_actions, masks (rows, 2)), corrected_actions, oracle_stop), float32 on the CPU: GRU state encoders,
    LSTM instruction encoder, one instruction per environment tiled over the steps, one environment reset at step 1"""
    if kind == "s2s":
        cfg = S2SConfig(rgb_hw=128, depth_hw=128, instr_len=12, rnn_type="GRU", progress_monitor=monitor).validate()
        sd, net = synth.make_s2s_weights(cfg, 5), train.Seq2SeqNet(cfg)
        ids = synth.make_s2s_observations(cfg, N, seed=5)["instruction"]
        rgb_shape = (2048, 1, 1)
    else:
        cfg = CMAConfig(rgb_hw=128, depth_hw=128, instr_len=12, rnn_type="GRU").validate()
        sd, net = synth.make_cma_weights(cfg, 5), train.CMANet(cfg, progress_monitor=monitor)
        ids = synth.make_cma_observations(cfg, N, seed=5)["instruction"]
        rgb_shape = (2048, 4, 4)
    net.load_reference_state_dict(sd)
    rows = T * N
    g = torch.Generator().manual_seed(29)
    fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
    obs = {"rgb_features": torch.relu(torch.rand(rows, *rgb_shape, generator=g) * 2 - 0.5),
           "depth_features": torch.relu(torch.rand(rows, cc, fs, fs, generator=g) * 2 - 0.5),
           "instruction": torch.from_numpy(np.tile(ids, (T, 1)))}
    if monitor:
        obs["progress"] = torch.rand(rows, generator=g)
    corrected, stop, _ = labels(rows, cfg.num_actions, g)
    masks = torch.ones(rows, 2)
    masks[:N] = 0
    if T > 1:
        masks[N + 1] = 0
    h0 = torch.rand(cfg.num_recurrent_layers, N, cfg.hidden, generator=g) - 0.5
    return cfg, net, (obs, h0, torch.zeros(rows, 2), masks), corrected, stop


def convert_batch(batch, conv):
    """a module_case batch with every floating tensor through conv and the token ids moved only (conv's device)"""
    obs, h0, prev, masks = batch
    probe = conv(h0)
    return ({k: v.to(probe.device) if k == "instruction" else conv(v) for k, v in obs.items()}, probe, conv(prev), conv(masks))
