"""The flat trainer's validation step (hcm_flat_val_step): the case table shared by tools/gen_flat_val_golden.py and the tests, the seeded
label sets, torch's own criteria as `_update_agent_val` applies them (robo_vln_trainer.py:544-575), and a torch-CPU stand-in for
CMAEngine.val_step / S2SEngine.val_step over the two model restatements (oracle.hcm_oracle.CMAOracle, tests/s2s_ref.S2SOracle).
Test infrastructure only."""
import numpy as np
import torch
from torch import nn

from oracle import cases, hcm_oracle
from robo_vln_amd import synth
from robo_vln_amd.config import S2SConfig
from tests import cma_seq_cases, s2s_ref, val_ref

SEED = cases.SEED
_S = dict(rgb_hw=128, depth_hw=128, instr_len=12)

# name -> (kind, config, T, N).  Frames, instructions, masks and initial state are those of the kind's sequence-forward cases
# (tests/cma_seq_cases.py, tests/s2s_ref.py); the progress-monitor cases use Seq2SeqNet's inputs with their own config.
FLAT_VAL_CASES = {
    "flatval_cma_T4_N2": ("cma", lambda: cma_seq_cases.seq_case("cma_seq_T4_N2_L12")[0], 4, 2),
    "flatval_s2s_T4_N2_gru": ("s2s", lambda: s2s_ref.seq_case("s2s_seq_T4_N2_gru")[0], 4, 2),
    "flatval_s2s_pm_T3_N2_gru": ("s2s", lambda: S2SConfig(**_S, rnn_type="GRU", progress_monitor=True).validate(), 3, 2),
    "flatval_cma_T4_N3_lstm": ("cma", lambda: cma_seq_cases.seq_case("cma_seq_T4_N3_lstm")[0], 4, 3),
    "flatval_s2s_pm_T2_N2_lstm": ("s2s", lambda: S2SConfig(**_S, progress_monitor=True).validate(), 2, 2),
}
# the reference's in-tree seq_forward raises for LSTM state encoders (oracle/cases.py): those cases are checked against the restatement only
FLAT_VAL_GOLDEN = ("flatval_cma_T4_N2", "flatval_s2s_T4_N2_gru", "flatval_s2s_pm_T3_N2_gru")


def case(name):
    kind, cfg, T, N = FLAT_VAL_CASES[name]
    return kind, cfg(), T, N


def weights(kind, cfg):
    return synth.make_cma_weights(cfg, SEED) if kind == "cma" else synth.make_s2s_weights(cfg, SEED)


def h0(kind, cfg, N):
    return cma_seq_cases.seq_h0(cfg, N) if kind == "cma" else s2s_ref.seq_h0(cfg, N)


def masks(kind, T, N):
    return cma_seq_cases.seq_masks(T, N) if kind == "cma" else cases.seq_masks(T, N)


def progress_targets(rows):
    """observations["progress"] (rows,): a seeded uniform [0, 1] draw."""
    return np.random.RandomState(13).uniform(0.0, 1.0, rows).astype(np.float32)


def labels(T, N, kind="mixed"):
    """(corrected (T*N,2), oracle_stop (T*N,1)) of tests/val_ref.labels: `mixed` has a valid row with an exact 0 in corrected[:, 0] (row 1) and,
    from 5 rows up, a padded row (row 4: corrected 0 0, stop -1); `padded` pads every row."""
    _, corrected, stop = val_ref.labels(T, N, kind)
    return corrected, stop


def observations(kind, cfg, T, N):
    obs = cma_seq_cases.seq_observations(cfg, T, N) if kind == "cma" else s2s_ref.seq_observations(cfg, T, N)
    if getattr(cfg, "progress_monitor", False):
        obs["progress"] = progress_targets(T * N)
    return obs


def masked_mean(loss, mask):
    """`torch.masked_select(loss, mask).mean()` of AuxLosses.reduce (common/aux_losses.py:27-33); NaN over an empty selection."""
    return torch.masked_select(loss, mask).mean()


def criteria(out, stop, progress_hat, corrected, oracle_stop, progress):
    """The eight numbers of hcm_flat_val_step (include/hcm.h) from the model's outputs with torch's criterion classes, in fp32 on the CPU,
    statement by statement as robo_vln_trainer.py:557-570.  progress_hat / progress None = no progress monitor: nothing registered."""
    out, stop = (torch.as_tensor(t).detach().float().cpu().clone() for t in (out, stop))
    corrected = torch.as_tensor(corrected).detach().float().cpu().reshape(out.shape)
    oracle_stop = torch.as_tensor(oracle_stop).detach().float().cpu().reshape(-1, 1)
    stop = stop.reshape(-1, 1)
    action_mask = corrected == 0
    action = nn.MSELoss()(out.masked_fill_(action_mask, 0), corrected)
    keep = oracle_stop != -1
    stop_loss = nn.BCEWithLogitsLoss()(torch.masked_select(stop, keep), torch.masked_select(oracle_stop, keep))
    aux, n_aux = 0.0, 0
    if progress_hat is not None:
        p = torch.as_tensor(progress_hat).detach().float().cpu().reshape(-1)
        y = torch.as_tensor(progress).detach().float().cpu().reshape(-1)
        aux_mask = ~action_mask[:, 0]
        # register_loss receives PROGRESS_MONITOR.alpha in its `masks` slot (seq2seq.py:181-185): the weight is the default 1.0
        aux = float(1.0 * masked_mean(nn.functional.mse_loss(p, y, reduction="none"), aux_mask))
        n_aux = int(aux_mask.sum())
    return torch.tensor([float(action), float(stop_loss), aux, int(keep.sum()), n_aux, 0.0, 0.0, 0.0], dtype=torch.float32)


class FlatValOracle:
    """val_step on the CPU: same signature and return value as CMAEngine.val_step / S2SEngine.val_step, so that it can stand in for either
    under robo_vln_amd.validate.FlatValidator."""
    device = "cpu"

    def __init__(self, kind, cfg, sd):
        self.kind, self.cfg = kind, cfg
        self.num_recurrent_layers = cfg.num_recurrent_layers
        self.model = hcm_oracle.CMAOracle(cfg, sd) if kind == "cma" else s2s_ref.S2SOracle(cfg, sd)
        self.calls = []

    @torch.no_grad()
    def val_step(self, observations, corrected_actions, oracle_stop, hidden, masks, result=None, return_outputs=False):
        obs = {k: np.asarray(v) for k, v in observations.items()}
        rows = obs["rgb"].shape[0]
        if obs["instruction"].shape[0] == 1 and self.kind == "cma":
            obs["instruction"] = np.repeat(obs["instruction"], rows, 0)
        progress = obs.pop("progress", None)
        m = np.asarray(masks, np.float32).reshape(rows, -1)[:, 0]
        h = torch.as_tensor(hidden).float().clone()
        self.calls.append(dict(rows=rows, hidden=h.clone()))
        if self.kind == "cma":
            out, stop, h2 = self.model.forward(obs, h, m)
            prog = None
        else:
            out, stop, prog, h2 = self.model.forward(obs, h, m)
        res = criteria(out, stop, prog, corrected_actions, oracle_stop, progress if prog is not None else None)
        if result is not None:
            result.copy_(res)
            res = result
        if return_outputs:
            return res, h2, (out, stop, prog)
        return res, h2


def oracle(name):
    kind, cfg, T, N = case(name)
    return FlatValOracle(kind, cfg, weights(kind, cfg))


def inputs(name, label_kind="mixed"):
    """(kind, cfg, T, N, observations, corrected, oracle_stop, masks (T*N,), h0) of one call, numpy / CPU torch."""
    kind, cfg, T, N = case(name)
    corrected, stop = labels(T, N, label_kind)
    return kind, cfg, T, N, observations(kind, cfg, T, N), corrected, stop, masks(kind, T, N), h0(kind, cfg, N)


def epoch_batches(name, n_batches, T_total):
    """Batches as the flat trainer's collate_fn returns them: T_total*N rows, masks / prev_actions (rows, 2), one instruction per trajectory,
    `progress` among the observations when the model has the monitor."""
    kind, cfg, _, N = case(name)
    make = synth.make_cma_observations if kind == "cma" else synth.make_s2s_observations
    out = []
    for b in range(n_batches):
        rows = T_total * N
        obs = make(cfg, rows, step=20 + b, seed=SEED)
        obs["instruction"] = make(cfg, N, step=b, seed=SEED)["instruction"]
        if getattr(cfg, "progress_monitor", False):
            obs["progress"] = np.roll(progress_targets(rows), b)
        corrected, stop = labels(T_total, N)
        corrected, stop = np.roll(corrected, b, 0), np.roll(stop, b, 0)
        m = np.ones((rows, 2), np.float32)
        m[:N] = 0
        out.append(({k: torch.from_numpy(np.asarray(v)) for k, v in obs.items()}, torch.zeros(rows, 2), torch.from_numpy(m),
                    torch.from_numpy(corrected.copy()), torch.from_numpy(stop.copy())))
    return out
