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


def _map_feats(feats, fn):
    """fn over the tensors of an encode_features() dict (a value is one tensor, or a (high, low) pair with None where an encoder takes none)"""
    return {k: (tuple(None if t is None else fn(t) for t in v) if isinstance(v, (tuple, list)) else fn(v)) for k, v in feats.items()}


class _FeatureCache:
    """cache_features=True for the two validators.  Both trunks are frozen in the reference (resnet_encoders.py:35-36, :146-149) and val_epoch
    walks the same recorded frames every epoch, so every epoch after the first recomputes the same trunk outputs.  With the cache the first run()
    over a list of batches encodes each chunk once (engine.encode_features) and keeps the result per (batch, chunk); that run and every later one
    hand the chunk to val_step under the reference's feature keys (`rgb_features`, `depth_features`) with no `rgb` / `depth` -- the same bits as
    from the frames.  cache_device "cuda" keeps the features on the engine's device, "cpu" in pinned host memory.  A later run() must bring the
    same batches: the same number of chunks with the same row counts (ValueError otherwise); clear_cache() forgets them."""

    def _init_cache(self, cache_features, cache_device):
        if cache_device not in ("cuda", "cpu"):
            raise ValueError('cache_device must be "cuda" or "cpu"')
        self.cache_features = bool(cache_features)
        self.cache_device = cache_device
        self.clear_cache()

    def clear_cache(self):
        self._cache = {}
        self._cache_full = False        # a run() has completed: the set of (batch, chunk) keys is closed

    def _keep(self, t):
        if self.cache_device == "cuda":
            return t
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=torch.cuda.is_available())
        host.copy_(t)
        return host

    def _chunk_obs(self, batch_idx, chunk_idx, obs, rows):
        """the chunk's observations as val_step gets them: unchanged without the cache, else the feature keys in place of the frames"""
        if not self.cache_features:
            return obs
        key = (batch_idx, chunk_idx)
        hit = self._cache.get(key)
        if hit is None:
            if self._cache_full:
                raise ValueError(f"cache_features: batch {batch_idx} chunk {chunk_idx} was not part of the cached run (clear_cache() first)")
            feats = self.engine.encode_features(obs)
            hit = self._cache[key] = (rows, _map_feats(feats, self._keep))
        elif hit[0] != rows:
            raise ValueError(f"cache_features: batch {batch_idx} chunk {chunk_idx} has {rows} rows, the cached features {hit[0]} "
                             "(clear_cache() before validating other batches)")
        out = {k: v for k, v in obs.items() if k not in ("rgb", "depth")}
        out.update(hit[1])
        return out

    def _close_cache(self, n_keys):
        if not self.cache_features:
            return
        if self._cache_full and n_keys != len(self._cache):
            raise ValueError(f"cache_features: this run had {n_keys} chunks, the cached one {len(self._cache)} (clear_cache() first)")
        self._cache_full = True


class HCMValidator(_FeatureCache):
    """val_epoch over batches shaped as the trainer's `collate_fn` (hierarchical_trainer.py:66-154) returns them:

        (observations, prev_actions, not_done_masks, corrected_actions, oracle_stop)

    observations: dict of tensors with T*N rows (`rgb`, `depth`, `vln_oracle_action_sensor`, ...) and `instruction`; the other four have
    T*N rows as well.  For every batch the hidden states start at zero (:770-781); every tensor except the instruction is cut into
    consecutive chunks of `tbptt_steps` rows (common/utils.py:120-142); the hidden states are carried from chunk to chunk; each chunk is one
    `engine.val_step` call.  `batch_size` is N, the trainer's DAGGER.BATCH_SIZE: the width of the hidden states.

    The instruction is passed whole to every chunk, as the reference does: (1, L), or one row per chunk row; an (N, L) instruction
    (one per trajectory) is repeated for every time step of the chunk.

    `engine` needs `val_step`, `num_recurrent_layers`, `cfg.hidden`, `device` and `check_val_result` -- HCMEngine, or a stand-in in tests.
    cache_features / cache_device: see _FeatureCache (off by default; the engine then needs `encode_features` too).
    cache_instruction (off by default; the engine then needs `encode_instruction`; independent of cache_features): BERT is frozen and runs
    under no_grad in the reference (seq2seq_highlevel_cma.py:192-195), and the collate repeats an episode's instruction at every step, so only
    N of a chunk's T*N instruction rows are distinct.  The first run() encodes each chunk's first N rows (time step 0) once and keeps the
    (N, L, bert_hidden) stream per (batch, chunk) -- on cache_device, under _FeatureCache's rules: a later run() must bring the same chunks,
    clear_cache() forgets the streams too.  That run and every later one hand the chunk to val_step as `instruction_features` with no
    `instruction`: BERT runs on N rows once instead of on T*N rows every epoch.  `instruction_lengths` passes through (the first N entries go
    to the encoder).  check_instruction=True verifies the precondition on the encoding run, `instruction.view(T, N, L) == instruction[:N]`, one
    device-to-host read per chunk, and raises ValueError when an instruction changes along T.
    """

    def __init__(self, engine, tbptt_steps, batch_size, cache_features=False, cache_device="cuda", cache_instruction=False, check_instruction=True):
        if tbptt_steps < 1 or batch_size < 1:
            raise ValueError("tbptt_steps and batch_size must be >= 1")
        self.engine = engine
        self.tbptt_steps = int(tbptt_steps)
        self.batch_size = int(batch_size)
        self.cache_instruction = bool(cache_instruction)
        self.check_instruction = bool(check_instruction)
        self._init_cache(cache_features, cache_device)

    def clear_cache(self):
        super().clear_cache()
        self._streams = {}
        self._streams_full = False      # as _cache_full, for the instruction streams

    def _instruction(self, ids, rows):
        N = self.batch_size
        if ids.shape[0] in (1, rows) or ids.shape[0] != N:
            return ids                                     # (anything else is refused by the engine with its own message)
        return ids.repeat(rows // N, 1)                    # row t*N + n -> the instruction of trajectory n

    def _chunk_stream(self, batch_idx, chunk_idx, obs, rows):
        """cache_instruction: the chunk's observations with the cached BERT stream under `instruction_features` in place of `instruction`"""
        if not self.cache_instruction:
            return obs
        key = (batch_idx, chunk_idx)
        hit = self._streams.get(key)
        if hit is None:
            if self._streams_full:
                raise ValueError(f"cache_instruction: batch {batch_idx} chunk {chunk_idx} was not part of the cached run (clear_cache() first)")
            ids = torch.as_tensor(obs["instruction"])
            N, lens = self.batch_size, obs.get("instruction_lengths")
            if ids.shape[0] != 1:                          # (1, L): one instruction for every row, nothing to compare
                if ids.dim() != 2 or ids.shape[0] != rows:
                    raise ValueError(f"cache_instruction: instruction must be (1, L), ({N}, L) or ({rows}, L), got {tuple(ids.shape)}")
                if self.check_instruction and not bool((ids.view(rows // N, N, ids.shape[1]) == ids[:N]).all()):
                    raise ValueError(f"cache_instruction: batch {batch_idx} chunk {chunk_idx}: an instruction changes along the chunk's time steps -- "
                                     "the collate repeats an episode's instruction at every step (hierarchical_trainer.py:66-154), and one stream "
                                     "per trajectory stands for all of them")
                ids = ids[:N]
                if lens is not None:
                    lens = torch.as_tensor(lens).reshape(-1)[:N]
            elif lens is not None:
                raise ValueError("cache_instruction: a (1, L) instruction with per-row instruction_lengths has no single stream")
            hit = self._streams[key] = (rows, self._keep(self.engine.encode_instruction(ids, lens)))
        elif hit[0] != rows:
            raise ValueError(f"cache_instruction: batch {batch_idx} chunk {chunk_idx} has {rows} rows, the cached stream was made for {hit[0]} "
                             "(clear_cache() before validating other batches)")
        out = {k: v for k, v in obs.items() if k != "instruction"}
        out["instruction_features"] = hit[1].to(self.engine.device, non_blocking=True)
        return out

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
        n_keys = 0
        for bi, batch in enumerate(batches):
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
                obs = self._chunk_obs(bi, i, obs, rows)
                obs = self._chunk_stream(bi, i, obs, rows)
                n_keys += 1
                _, hh, lh = eng.val_step(obs, c_split[i], s_split[i], hh, lh, m_split[i], result=table[i])
            tables.append(table)
        if not tables:
            raise ValueError("no batches")
        self._close_cache(n_keys)
        if self.cache_instruction:
            if self._streams_full and n_keys != len(self._streams):
                raise ValueError(f"cache_instruction: this run had {n_keys} chunks, the cached one {len(self._streams)} (clear_cache() first)")
            self._streams_full = True
        table = eng.check_val_result(torch.cat(tables, 0))  # the one device-to-host read; raises on out-of-range labels
        total = float(table[:, 4].sum())
        return {
            "high_loss": float(table[:, 0].double().mean()),
            "low_loss": float((table[:, 1].double() + table[:, 2].double()).mean()),
            "accuracy": 100.0 * float(table[:, 3].sum()) / total if total else float("nan"),
            "table": table,
            "chunks": table.shape[0],
        }


class FlatValidator(_FeatureCache):
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
    cache_features / cache_device: see _FeatureCache (off by default; the engine then needs `encode_features` too).
    """

    def __init__(self, engine, tbptt_steps, batch_size, cache_features=False, cache_device="cuda"):
        if tbptt_steps < 1 or batch_size < 1:
            raise ValueError("tbptt_steps and batch_size must be >= 1")
        self.engine = engine
        self.tbptt_steps = int(tbptt_steps)
        self.batch_size = int(batch_size)
        self._init_cache(cache_features, cache_device)

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
        n_keys = 0
        for bi, batch in enumerate(batches):
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
                obs = self._chunk_obs(bi, i, obs, rows)
                n_keys += 1
                _, h = eng.val_step(obs, c_split[i], s_split[i], h, m_split[i], result=table[i])
            tables.append(table)
        if not tables:
            raise ValueError("no batches")
        self._close_cache(n_keys)
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
