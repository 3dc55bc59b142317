"""Shared cases of the hierarchical trainer's fused sub-task head and cross-entropy (robo_vln_amd.train.subtask_ce): inputs from a seeded
generator, the float64 CPU-autograd reference through train.subtask_ce_ref, computed once per case and never modified, the same criterion written
with nn.CrossEntropyLoss as the trainer writes it (`torch_criterion`), the launch rules of csrc/subtask_ce_train.hip restated for the coverage
test, and the module cases of train.HighLevel / train.LowLevel.

Inputs: x ~ N(0, 1); weights ~ N(0, 1/512), so that every logit is ~ N(0, 1); biases ~ N(0, 0.01); the labels are scripted (`labels`); the
cotangent of the loss is 0.7.  Test infrastructure only."""
import functools
import math

import torch
from torch import nn

from robo_vln_amd import synth, train
from robo_vln_amd.config import HCMConfig

H = 512
COT = 0.7
BAD_ROW, BAD_LABEL = 2, 9
# (rows, A, num_sub_tasks, d_x, out-of-range label at row BAD_ROW).  Rows: one below, at and one above the forward's 4 rows per workgroup; the
# backward's half block (16) and row block (32), the second block's edges (63, 64, 65) and the criterion's 256-thread stride; 300 rows end in a
# ragged block of 12 (one half idle), 600 rows are more than two per criterion thread.  A 1, 2, 4, 6 with num_sub_tasks == A and below it, d_x and
# the out-of-range label each on and off at small and at large sizes.
CASES = [(1, 4, 4, True, False), (2, 2, 2, False, False), (3, 1, 1, True, True), (4, 6, 6, True, False), (5, 4, 4, True, True),
         (15, 2, 1, False, False), (16, 4, 4, True, False), (17, 6, 4, True, True),
         (31, 4, 3, False, False), (32, 2, 2, True, True), (33, 4, 4, False, False),
         (63, 1, 1, False, False), (64, 6, 6, True, True), (65, 4, 4, True, False),
         (255, 2, 2, True, False), (256, 4, 4, True, True), (257, 6, 5, False, False),
         (300, 4, 4, True, True), (600, 6, 6, True, False), (600, 4, 4, False, True)]
NAMES = ("d_x", "d_w", "d_b")
# A bias gradient is ONE number per class, a sum over the rows that can cancel, and a single row's logit can be a cancelling dot product:
# relative to itself such a number is as badly conditioned as the draw makes it.  So each case takes the first seed from 0 for which the float32
# restatement on the CPU stays within SEED_BOUND of its float64 run in every tensor and has its counts (first_seed; a fifth of the half bound that
# test_float32_restatement_stays_within_half_the_bound asserts).  A condition on the inputs, not a tolerance: no tensor is left out of a comparison.
SEED_BOUND = 1e-6
SEEDS = {(33, 4, 4, False, False): 1}          # every other case: seed 0


# ---- the launch rules of csrc/subtask_ce_train.hip, restated: a change there must change these, and the cases with them
def fwd_workgroups(rows):
    """the head launch: a wave per row, 4 rows per workgroup"""
    return math.ceil(rows / train.SUBTASK_CE_FWD_ROWS)


def bwd_blocks(rows):
    """the backward's main launch: a workgroup per block of 32 rows; (blocks, rows of the last block, rows of its first and second half)"""
    n = math.ceil(rows / train.SUBTASK_CE_BWD_ROWS)
    last = rows - (n - 1) * train.SUBTASK_CE_BWD_ROWS
    return n, last, min(last, train.SUBTASK_CE_BWD_HALF), max(0, last - train.SUBTASK_CE_BWD_HALF)


def criterion_rows_per_thread(rows):
    """the criterion launch: one workgroup of 256 threads, thread t adds the rows t, t + 256, ...: the most rows any thread adds"""
    return math.ceil(rows / train.SUBTASK_CE_LOSS_THREADS)


def labels(rows, nst, bad):
    """oracle_subtask (rows, 1) float32, as the collate function carries it: row r is padded (0) where r % 7 == 4; the valid rows walk the classes
    1..nst in turn, so every class occurs as soon as the rows allow; with `bad` row BAD_ROW (row 0 of fewer rows) holds BAD_LABEL, outside
    [0, num_sub_tasks]"""
    o = torch.zeros(rows, 1)
    k = 0
    for r in range(rows):
        if r % 7 != 4:
            o[r, 0] = 1 + k % nst
            k += 1
    if bad:
        o[min(BAD_ROW, rows - 1), 0] = BAD_LABEL
    return o


def make_inputs(rows, A, nst, bad, seed=0):
    """float32 CPU tensors (x, w, b, oracle_subtask) in subtask_ce's argument order"""
    g = torch.Generator().manual_seed(1000 * rows + 10 * A + seed)
    x = torch.randn(rows, H, generator=g)
    w = torch.randn(A, H, generator=g) / math.sqrt(H)
    b = torch.randn(A, generator=g) * 0.1
    return x, w, b, labels(rows, nst, bad)


def cotangent(dtype=torch.float32, device="cpu"):
    return torch.tensor((COT,) + (0.0,) * 7, dtype=dtype, device=device)


def leaves_of(args, dx, conv):
    """(x, w, b) through conv, the differentiable ones made leaves, the labels moved only: ([all four], {name: leaf})"""
    out, named = [], {}
    for i, t in enumerate(args[:3]):
        t = conv(t)
        if i > 0 or dx:
            t = t.requires_grad_()
            named[NAMES[i]] = t
        out.append(t)
    out.append(args[3].to(out[0].device))
    return out, named


def run(fn, args, nst, dx, conv):
    """fn (subtask_ce or its restatement) on the case's inputs through conv -> (result, logits, {name: gradient})"""
    a, named = leaves_of(args, dx, conv)
    result, logits = fn(*a, nst)
    grads = torch.autograd.grad(result, list(named.values()), cotangent(result.dtype, result.device))
    return result.detach(), logits.detach(), dict(zip(named, grads))


def _rel(a, b):
    """max|a - b| / max|b|; a reference of exact zeros (one row, an out-of-range label: every gradient) is met exactly or not at all"""
    scale = b.abs().max().item()
    err = (a.double() - b).abs().max().item()
    return err / scale if scale > 0 else (0.0 if err == 0 else math.inf)


def conditioning(rows, A, nst, dx, bad, seed):
    """the largest per-tensor max|t32 - t64| / max|t64| of the float32 restatement against its float64 run -- the loss, the logits and every
    gradient -- and infinity when a count differs (an argmax that float32 and float64 see differently)"""
    args = make_inputs(rows, A, nst, bad, seed=seed)
    r64 = run(train.subtask_ce_ref, args, nst, dx, lambda t: t.double())
    r32 = run(train.subtask_ce_ref, args, nst, dx, lambda t: t)
    if r32[0][1:].tolist() != r64[0][1:].tolist():
        return math.inf
    pairs = [(r32[1], r64[1])] + [(r32[2][n], r64[2][n]) for n in r64[2]]
    if r64[0][4] > 0:
        pairs.append((r32[0][:1], r64[0][:1]))
    return max(_rel(a, b) for a, b in pairs)


def first_seed(rows, A, nst, dx, bad):
    seed = 0
    while conditioning(rows, A, nst, dx, bad, seed) > SEED_BOUND:
        seed += 1
    return seed


@functools.lru_cache(maxsize=None)
def case(rows, A, nst, dx, bad):
    """Inputs (float32, CPU) and the float64 reference of one case: dict(args, result64, logits64, ref={name: gradient})"""
    args = make_inputs(rows, A, nst, bad, seed=SEEDS.get((rows, A, nst, dx, bad), 0))
    result, logits, grads = run(train.subtask_ce_ref, args, nst, dx, lambda t: t.double())
    return dict(args=args, result64=result, logits64=logits, ref=grads)


def torch_criterion(x, w, b, oracle, nst):
    """hierarchical_trainer.py:498, :506-511 with nn.CrossEntropyLoss as the trainer writes it, in the inputs' dtype and with the graph kept; the
    out-of-range labels made padded first, as tests/val_ref.criteria does -> (loss, correct, total, out-of-range rows)"""
    high_level_criterion = nn.CrossEntropyLoss(ignore_index=-1, reduction="mean")
    output = nn.functional.linear(x, w, b)
    raw = output.detach().clone()
    sensor = oracle.clone()
    bad = (sensor < 0) | (sensor > nst)
    sensor = sensor.masked_fill(bad, 0)
    high_level_action_mask = sensor == 0
    output = output.masked_fill_(high_level_action_mask, 0)
    sensor = sensor.squeeze(1).to(dtype=torch.int64)
    loss = high_level_criterion(output, (sensor - 1))
    valid = sensor != 0
    correct = int((torch.argmax(raw, 1)[valid] == (sensor - 1)[valid]).sum())
    return loss, correct, int(valid.sum()), int(bad.sum())


# ---- the two models
L_INS = 12


def module_cfg(**kw):
    return HCMConfig(**dict(dict(rgb_hw=128, depth_hw=128, instr_len=L_INS, rnn_type="GRU", bert_layers=2), **kw)).validate()


def module_case(T=3, N=2, seed=5, **kw):
    """(config, train.HighLevel, train.LowLevel with seeded reference weights and dropout off, observations -- random post-ReLU features as the
    (high, low) pairs HCMEngine.encode_features returns, a random instruction stream of one instruction per environment tiled over the steps, the
    oracle sub-task (rows, 1) float with a padded and an out-of-range row -- h0 of both models, prev_actions, masks (rows, 2) with one
    environment reset at step 1, corrected_actions, oracle_stop), float32 on the CPU"""
    cfg = module_cfg(**kw)
    hi_sd, lo_sd = (synth.materialize(synth.high_level_spec(cfg), "hi", seed), synth.materialize(synth.low_level_spec(cfg), "lo", seed))
    high, low = train.HighLevel(cfg, dropout=0.0), train.LowLevel(cfg)
    high.load_reference_state_dict(hi_sd)
    low.load_reference_state_dict(lo_sd)
    rows = T * N
    g = torch.Generator().manual_seed(31)
    fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()

    def feat(*shape):
        return torch.relu(torch.rand(rows, *shape, generator=g) * 2 - 0.5)

    obs = {"rgb_features": (feat(2048, 4, 4), feat(2048, 1, 1)), "depth_features": (feat(cc, fs, fs), feat(cc, fs, fs)),
           "instruction_features": torch.randn(N, L_INS, cfg.ins_in, generator=g).repeat(T, 1, 1)}
    oracle = torch.tensor([1.0, 2, 3, 2, 0, 4, 1, 3]).repeat(math.ceil(rows / 8))[:rows].reshape(rows, 1)
    if rows > 3:
        oracle[3, 0] = 9.0                                                     # out of range; the classes 1..4 all stay among the first six rows
    obs["vln_oracle_action_sensor"] = oracle
    corrected = torch.randn(rows, cfg.lo_actions, generator=g)
    stop = (torch.rand(rows, 1, generator=g) < 0.5).float()
    pad = oracle[:, 0] == 0
    corrected[pad], stop[pad] = 0.0, -1.0
    masks = torch.ones(rows, 2)
    masks[:N] = 0
    if T > 1:
        masks[N + 1] = 0
    R = cfg.num_recurrent_layers
    h_hi, h_lo = (torch.rand(R, N, cfg.hidden, generator=g) - 0.5 for _ in range(2))
    return cfg, high, low, obs, h_hi, h_lo, torch.zeros(rows, 2), masks, corrected, stop


def convert_obs(obs, conv):
    """module_case observations with every tensor (the pairs' entries too) through conv"""
    return {k: tuple(conv(t) for t in v) if isinstance(v, tuple) else conv(v) for k, v in obs.items()}
