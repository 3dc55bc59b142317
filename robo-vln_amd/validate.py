"""The validation epoch of the reference's trainer on top of `HCMEngine.val_step`: `HierarchicalTrainer.val_epoch`
(robo_vln_baselines/hierarchical_trainer.py:747-831) driving `_update_agent_val` (:562-631).

One library call per truncated-BPTT chunk, every chunk's eight numbers written into its own row of a device-side table, ONE
device-to-host read at the end of the epoch.  torch is used for buffers and slicing only.

`FlatValidator` is the same epoch for the two flat baselines, CMANet and Seq2SeqNet: the other trainer's `val_epoch`
(robo_vln_baselines/robo_vln_trainer.py:726-813) driving its `_update_agent_val` (:544-575) through `CMAEngine.val_step` / `S2SEngine.val_step`.
"""
import torch


def split_rows(t, steps):
    """`tensor.split(tbptt_steps, dim=0)` of common/utils.py:128-134: consecutive chunks of `steps` rows, the last one shorter."""
    return t.split(steps, dim=0)


class HCMValidator:
    """val_epoch over batches shaped as the trainer's `collate_fn` (hierarchical_trainer.py:66-154) returns them:

        (observations, prev_actions, not_done_masks, corrected_actions, oracle_stop)

    observations: dict of tensors with T*N rows (`rgb`, `depth`, `vln_oracle_action_sensor`, ...) and `instruction`; the other four have
    T*N rows as well.  For every batch the hidden states start at zero (:770-781); every tensor except the instruction is cut into
    consecutive chunks of `tbptt_steps` rows (common/utils.py:120-142); the hidden states are carried from chunk to chunk; each chunk is one
    `engine.val_step` call.  `batch_size` is N, the trainer's DAGGER.BATCH_SIZE: the width of the hidden states.

    The instruction is passed whole to every chunk, as the reference does: (1, L), or one row per chunk row; an (N, L) instruction
    (one per trajectory) is repeated for every time step of the chunk.

    `engine` needs `val_step`, `num_recurrent_layers`, `cfg.hidden`, `device` and `check_val_result` -- HCMEngine, or a stand-in in tests.
    """

    def __init__(self, engine, tbptt_steps, batch_size):
        if tbptt_steps < 1 or batch_size < 1:
            raise ValueError("tbptt_steps and batch_size must be >= 1")
        self.engine = engine
        self.tbptt_steps = int(tbptt_steps)
        self.batch_size = int(batch_size)

    def _instruction(self, ids, rows):
        N = self.batch_size
        if ids.shape[0] in (1, rows) or ids.shape[0] != N:
            return ids                                     # (anything else is refused by the engine with its own message)
        return ids.repeat(rows // N, 1)                    # row t*N + n -> the instruction of trajectory n

    def run(self, batches):
        """Returns a dict:
            high_loss   mean over chunks of the high-level (sub-task cross-entropy) loss
            low_loss    mean over chunks of action loss + stop loss
            accuracy    100 * sum(correct) / sum(total)   (:827)
            table       (chunks, 8) CPU tensor, one val_step result per chunk in call order
            chunks      number of chunks
        The reference logs the two epoch means under each other's names -- `val_low_losses.append(loss[0])`, the high-level loss, and
        `val_high_losses.append(loss[1]+loss[2])` (:824-829); here each is returned under its own name.
        Raises ValueError if any chunk reported sub-task labels outside [0, num_sub_tasks], or if a chunk's row count is not a multiple
        of batch_size."""
        eng, N, S = self.engine, self.batch_size, self.tbptt_steps
        R, H, dev = eng.num_recurrent_layers, eng.cfg.hidden, eng.device
        tables = []
        for batch in batches:
            observations, _prev_actions, not_done_masks, corrected_actions, oracle_stop = batch
            rows_total = corrected_actions.shape[0]
            per_key = {k: (None if k == "instruction" else split_rows(torch.as_tensor(v), S)) for k, v in observations.items()}
            m_split = split_rows(torch.as_tensor(not_done_masks), S)
            c_split = split_rows(torch.as_tensor(corrected_actions), S)
            s_split = split_rows(torch.as_tensor(oracle_stop), S)
            n_chunks = len(c_split)
            for i, c in enumerate(c_split):
                if c.shape[0] % N:
                    raise ValueError(f"chunk {i} of a batch of {rows_total} rows has {c.shape[0]} rows, not a multiple of batch_size {N} "
                                     f"(tbptt_steps {S}): the reference fails on it at models/decoder/state_encoder.py:96, "
                                     "`x = x.view(t, n, x.size(1))`")
            table = torch.zeros(n_chunks, 8, device=dev, dtype=torch.float32)
            hh = torch.zeros(R, N, H, device=dev)          # :770-781
            lh = torch.zeros(R, N, H, device=dev)
            ids = torch.as_tensor(observations["instruction"])
            for i in range(n_chunks):
                rows = c_split[i].shape[0]
                obs = {k: v[i] for k, v in per_key.items() if v is not None}
                obs["instruction"] = self._instruction(ids, rows)
                _, hh, lh = eng.val_step(obs, c_split[i], s_split[i], hh, lh, m_split[i], result=table[i])
            tables.append(table)
        if not tables:
            raise ValueError("no batches")
        table = eng.check_val_result(torch.cat(tables, 0))  # the one device-to-host read; raises on out-of-range labels
        total = float(table[:, 4].sum())
        return {
            "high_loss": float(table[:, 0].double().mean()),
            "low_loss": float((table[:, 1].double() + table[:, 2].double()).mean()),
            "accuracy": 100.0 * float(table[:, 3].sum()) / total if total else float("nan"),
            "table": table,
            "chunks": table.shape[0],
        }


class FlatValidator:
    """val_epoch of the flat trainer (robo_vln_trainer.py:726-813) over batches shaped as its `collate_fn` returns them:

        (observations, prev_actions, not_done_masks, corrected_actions, oracle_stop)

    observations: dict of tensors with T*N rows (`rgb`, `depth`, `progress` when the model has a progress monitor, ...) and `instruction`; the
    other four have T*N rows as well.  For every batch the hidden state starts as zeros(num_recurrent_layers, batch_size, hidden); every tensor
    except the instruction -- `progress` included -- is cut into consecutive chunks of `tbptt_steps` rows (common/utils.py:120-142); the state
    is carried from chunk to chunk; each chunk is one `engine.val_step` call writing its own row of a device-side table.  `batch_size` is N,
    the trainer's DAGGER.BATCH_SIZE: the width of the hidden state.

    The instruction is handled as by HCMValidator: passed whole to every chunk -- (1, L), or one row per chunk row -- and an (N, L)
    instruction (one per trajectory) is repeated for every time step of the chunk.

    `engine` needs `val_step`, `num_recurrent_layers`, `cfg.hidden` and `device` -- CMAEngine, S2SEngine, or a stand-in in tests.
    """

    def __init__(self, engine, tbptt_steps, batch_size):
        if tbptt_steps < 1 or batch_size < 1:
            raise ValueError("tbptt_steps and batch_size must be >= 1")
        self.engine = engine
        self.tbptt_steps = int(tbptt_steps)
        self.batch_size = int(batch_size)

    def _instruction(self, ids, rows):
        N = self.batch_size
        if ids.shape[0] in (1, rows) or ids.shape[0] != N:
            return ids                                     # (anything else is refused by the engine with its own message)
        return ids.repeat(rows // N, 1)                    # row t*N + n -> the instruction of trajectory n

    def run(self, batches):
        """Returns a dict:
            action_loss, stop_loss, aux_loss   means over chunks of the three terms the reference logs per chunk
            val_loss    mean over chunks of the per-chunk sum action + stop + aux: the reference's "Val Loss Epoch"
            table       (chunks, 8) CPU tensor, one val_step result per chunk in call order
            chunks      number of chunks
        Raises ValueError if a chunk's row count is not a multiple of batch_size."""
        eng, N, S = self.engine, self.batch_size, self.tbptt_steps
        R, H, dev = eng.num_recurrent_layers, eng.cfg.hidden, eng.device
        tables = []
        for batch in batches:
            observations, _prev_actions, not_done_masks, corrected_actions, oracle_stop = batch
            rows_total = corrected_actions.shape[0]
            per_key = {k: (None if k == "instruction" else split_rows(torch.as_tensor(v), S)) for k, v in observations.items()}
            m_split = split_rows(torch.as_tensor(not_done_masks), S)
            c_split = split_rows(torch.as_tensor(corrected_actions), S)
            s_split = split_rows(torch.as_tensor(oracle_stop), S)
            n_chunks = len(c_split)
            for i, c in enumerate(c_split):
                if c.shape[0] % N:
                    raise ValueError(f"chunk {i} of a batch of {rows_total} rows has {c.shape[0]} rows, not a multiple of batch_size {N} "
                                     f"(tbptt_steps {S}): the reference fails on it at models/decoder/state_encoder.py:96, "
                                     "`x = x.view(t, n, x.size(1))`")
            table = torch.zeros(n_chunks, 8, device=dev, dtype=torch.float32)
            h = torch.zeros(R, N, H, device=dev)
            ids = torch.as_tensor(observations["instruction"])
            for i in range(n_chunks):
                rows = c_split[i].shape[0]
                obs = {k: v[i] for k, v in per_key.items() if v is not None}
                obs["instruction"] = self._instruction(ids, rows)
                _, h = eng.val_step(obs, c_split[i], s_split[i], h, m_split[i], result=table[i])
            tables.append(table)
        if not tables:
            raise ValueError("no batches")
        table = torch.cat(tables, 0).detach().to("cpu", torch.float32)      # the one device-to-host read
        t = table[:, :3].double()
        return {
            "action_loss": float(t[:, 0].mean()),
            "stop_loss": float(t[:, 1].mean()),
            "aux_loss": float(t[:, 2].mean()),
            "val_loss": float(t.sum(1).mean()),
            "table": table,
            "chunks": table.shape[0],
        }
