"""Teacher-forced validation step: the case table shared by tools/gen_val_golden.py and the tests, the scripted label sets, and a torch-CPU
restatement of `HierarchicalTrainer._update_agent_val` (hierarchical_trainer.py:562-631) -- the two model restatements of
oracle/hcm_oracle.py followed by torch's own criterion classes.  Test infrastructure only."""
import numpy as np
import torch
from torch import nn

from oracle import cases, hcm_oracle
from robo_vln_amd import synth
from robo_vln_amd.config import HCMConfig

SEED = cases.SEED
_S = dict(rgb_hw=128, depth_hw=128, instr_len=20, bert_layers=2)

# name -> (HCMConfig kwargs, T, N); frames, instruction, masks and initial hidden state are those of oracle/cases.py's SEQ_CASES
VAL_CASES = {
    "val_T4_N2_gru": (dict(_S, rnn_type="GRU"), 4, 2),
    "val_T4_N2_lstm": (dict(_S), 4, 2),
}
# the reference's in-tree seq_forward raises for LSTM (oracle/cases.py:96-100): only the GRU case has a golden from the imported models
VAL_GOLDEN = ("val_T4_N2_gru",)
# every valid row's two largest logits must be further apart than this in the fp32 restatement (twice the 16-bit output tolerance of
# tests/test_parity_gpu.py), so that the accuracy count is the same number in every precision mode
LOGIT_GAP = 2 * 1e-2


def case(name):
    kw, T, N = VAL_CASES[name]
    return HCMConfig(**kw).validate(), T, N


def weights(cfg):
    return (synth.materialize(synth.high_level_spec(cfg), "hi", SEED), synth.materialize(synth.low_level_spec(cfg), "lo", SEED))


def h0(cfg, N):
    g = torch.Generator().manual_seed(3)
    return torch.rand(cfg.num_recurrent_layers, N, cfg.hidden, generator=g) - 0.5


def labels(T, N, kind="mixed"):
    """Scripted labels for T*N rows, in the dtypes and shapes the trainer's collate_fn carries them (hierarchical_trainer.py:135-154):
    oracle (T*N,1) f32, corrected (T*N,2) f32, oracle_stop (T*N,1) f32.
      mixed   row 4 is padded (oracle 0, stop -1, corrected 0 0); row 1 is valid with an exact 0 in corrected[:, 0]; sub-tasks 1..4 and both
              stop labels all occur
      padded  every row padded: the NaN contract
      bad     as mixed with row 2's sub-task set to 9 (outside [0, num_sub_tasks])"""
    rows = T * N
    oracle = np.resize(np.array([1, 2, 3, 2, 0, 4, 1, 3], np.float32), rows)
    stop = np.resize(np.array([0, 1, 0, 0, -1, 1, 0, 1], np.float32), rows)
    corrected = np.random.RandomState(11).uniform(-1.0, 1.0, (rows, 2)).astype(np.float32)
    corrected[oracle == 0] = 0
    corrected[1, 0] = 0
    if kind == "padded":
        oracle[:] = 0
        stop[:] = -1
        corrected[:] = 0
    elif kind == "bad":
        oracle[2] = 9
    elif kind != "mixed":
        raise ValueError(kind)
    return oracle.reshape(rows, 1), corrected, stop.reshape(rows, 1)


def criteria(logits, vel, stop, oracle, corrected, oracle_stop, num_sub_tasks=4):
    """The eight numbers of hcm_val_step (include/hcm.h) from the models' outputs, with torch's criterion classes, in fp32 on the CPU."""
    logits, vel, stop = (torch.as_tensor(t).detach().float().cpu().clone() for t in (logits, vel, stop))
    oracle = torch.as_tensor(oracle).detach().cpu().reshape(-1).to(torch.int64)
    corrected = torch.as_tensor(corrected).detach().float().cpu().reshape(-1, vel.shape[1])
    oracle_stop = torch.as_tensor(oracle_stop).detach().float().cpu().reshape(-1, 1)
    bad = (oracle < 0) | (oracle > num_sub_tasks)
    oracle = oracle.masked_fill(bad, 0)                       # counted, then treated as padded
    padded = oracle == 0
    target = oracle - 1                                       # -1 on the padded rows: ignore_index
    high = nn.CrossEntropyLoss(ignore_index=-1, reduction="mean")(logits.masked_fill(padded.view(-1, 1), 0), target)
    pred = torch.argmax(logits, dim=1)
    correct = int((pred[~padded] == target[~padded]).sum())
    total = int((~padded).sum())
    action = nn.MSELoss()(vel.masked_fill(corrected == 0, 0), corrected)
    keep = oracle_stop != -1
    stop_loss = nn.BCEWithLogitsLoss()(stop[keep], oracle_stop[keep])
    return torch.tensor([float(high), float(action), float(stop_loss), correct, total, int(keep.sum()), int(bad.sum()), 0.0], dtype=torch.float32)


def remap(oracle, num_sub_tasks=4):
    """The low-level model's sub-task: oracle - 1, and num_sub_tasks on the padded (and out-of-range) rows."""
    o = torch.as_tensor(oracle).reshape(-1).to(torch.int64)
    return torch.where((o >= 1) & (o <= num_sub_tasks), o - 1, torch.full_like(o, num_sub_tasks))


class ValOracle:
    """val_step on the CPU: same signature and return value as HCMEngine.val_step, so that it can stand in for the engine under
    robo_vln_amd.validate.HCMValidator."""
    device = "cpu"

    def __init__(self, cfg, hi_sd, lo_sd):
        self.cfg = cfg
        self.num_recurrent_layers = cfg.num_recurrent_layers
        self.hi = hcm_oracle.HighLevelOracle(cfg, hi_sd)
        self.lo = hcm_oracle.LowLevelOracle(cfg, lo_sd)
        self.calls = []

    @torch.no_grad()
    def val_step(self, observations, corrected_actions, oracle_stop, hi_hidden, lo_hidden, masks, result=None, return_outputs=False):
        obs = {k: np.asarray(v) for k, v in observations.items()}
        rows = obs["rgb"].shape[0]
        if obs["instruction"].shape[0] == 1:
            obs["instruction"] = np.repeat(obs["instruction"], rows, 0)
        oracle = obs.pop("vln_oracle_action_sensor")
        m = np.asarray(masks, np.float32).reshape(rows, -1)[:, 0]
        hh = torch.as_tensor(hi_hidden).float().clone()
        lh = torch.as_tensor(lo_hidden).float().clone()
        self.calls.append(dict(rows=rows, hi_hidden=hh.clone(), lo_hidden=lh.clone()))
        logits, hh2 = self.hi.forward(obs, hh, m)
        vel, stop, lh2 = self.lo.forward(obs, lh, m, remap(oracle, self.cfg.num_sub_tasks))
        res = criteria(logits, vel, stop, oracle, corrected_actions, oracle_stop, self.cfg.num_sub_tasks)
        if result is not None:
            result.copy_(res)
            res = result
        if return_outputs:
            return res, hh2, lh2, (logits, vel, stop)
        return res, hh2, lh2

    @staticmethod
    def check_val_result(result):
        from robo_vln_amd.policy import HCMEngine
        return HCMEngine.check_val_result(result)


def observations(cfg, T, N, kind="mixed"):
    """(obs dict with the oracle sub-task inside, corrected, oracle_stop, masks) for one call."""
    obs = cases.seq_observations(cfg, T, N)
    oracle, corrected, stop = labels(T, N, kind)
    obs["vln_oracle_action_sensor"] = oracle
    return obs, corrected, stop, cases.seq_masks(T, N)
