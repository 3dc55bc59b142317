"""The four trainable models, from cached trunk features, and the trainers' update steps around them.

`CMANet`: the reference's flat baseline (models/cma.py) around `attn1q`, `InstructionEncoder` and two `RNNStateEncoder`s.  `Seq2SeqNet`: the second
flat baseline (models/seq2seq.py).  Both have `update_loss`, the model with its heads and the masked criteria on `flat_heads_loss`, and
`flat_update` is the flat trainer's `_update_agent` (robo_vln_trainer.py:505-542) around it.

`HighLevel` (models/seq2seq_highlevel_cma.py, the frozen BERT's output entering as a tensor, its criterion on `subtask_ce`) and `LowLevel`
(models/seq2seq_lowlevel.py, its heads on `flat_heads_loss`) are the hierarchical pair, and `hier_update` is the hierarchical trainer's
`_update_agent` (hierarchical_trainer.py:492-560) around them.

What the models share stands once, above them: loading a reference state dict without its frozen parts (`_FromReference`), the refusals of a
missing or misshapen trunk feature (`_check_feature`), the flat front end of Seq2SeqNet and LowLevel (`_flat_visual`), the two-operand visual FC
of CMANet and HighLevel (`_visual_fc`), the SimpleCNN refusal and the progress monitor's initialisation.  The four `_encode`s are four
different models and stay apart."""
import torch
from torch import nn

from .modules import InstructionEncoder, RNNStateEncoder, SimpleDepthCNN, SimpleRGBCNN, Visual_Ling_Attn
from .ops import CHANNEL_MAJOR, TOKEN_MAJOR, _zero_grads, _ZeroGrad, attn1q, attn1q_ref, flat_heads_loss, subtask_ce

CMA_TRUNK_PREFIXES = ("rgb_encoder.cnn.", "depth_encoder.visual_encoder.")
S2S_TRUNK_PREFIXES = CMA_TRUNK_PREFIXES
HCM_HIGH_FROZEN_PREFIXES = ("rgb_encoder.cnn.", "depth_encoder.visual_encoder.", "embedding_layer.")
HCM_LOW_FROZEN_PREFIXES = CMA_TRUNK_PREFIXES


class _FromReference(nn.Module):
    """Base of the four models: FROZEN_PREFIXES names the parts of the reference's model that are frozen and kept outside this one"""

    FROZEN_PREFIXES = ()

    def load_reference_state_dict(self, sd):
        """Load the reference model's state dict (tensors or arrays): the keys of its frozen parts -- the two trunks, and BERT for the high-level
        model -- are dropped, everything else is strict: a missing, unexpected or misshapen key raises"""
        kept = {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(self.FROZEN_PREFIXES)}
        return self.load_state_dict(kept, strict=True)


def _refuse_simple_cnn(cls, cfg):
    """The SimpleCNN encoders are trunks that train with the model: there is nothing to cache, and they are refused"""
    if cfg.rgb_encoder != "TorchVisionResNet50" or cfg.depth_encoder != "VlnResnetDepthEncoder":
        raise ValueError(f"train.{cls} trains from cached features of the two frozen ResNet trunks; SimpleRGBCNN / SimpleDepthCNN are trainable "
                         f"trunks with nothing to cache (got rgb_encoder {cfg.rgb_encoder!r}, depth_encoder {cfg.depth_encoder!r})")


def _simple_trunks(cls, cfg, trainable_trunks):
    """(rgb is a SimpleRGBCNN, depth is a SimpleDepthCNN) for a model built with trainable_trunks=True; without the keyword the SimpleCNN
    encoders are refused, as they always were"""
    if not trainable_trunks:
        _refuse_simple_cnn(cls, cfg)
        return False, False
    return cfg.rgb_encoder == "SimpleRGBCNN", cfg.depth_encoder == "SimpleDepthCNN"


def _frozen_prefixes(simple_rgb, simple_depth):
    """the trunk prefixes load_reference_state_dict drops: those of the ResNet modalities; a SimpleCNN's keys are the model's own"""
    return tuple(p for p, simple in zip(CMA_TRUNK_PREFIXES, (simple_rgb, simple_depth)) if not simple)


def _simple_visual(model, enc, observations, ablated, rows, like):
    """One modality's embedding from a trainable SimpleCNN encoder (rows, out): the encoder on its frames; ablated: the encoder runs and its
    output is multiplied by 0 (seq2seq.py:158-161, seq2seq_lowlevel.py:132-135), so its parameters get zero gradients; ablated without the
    frames key: exact zeros, and zero gradients through _zero_grads"""
    if ablated and enc.KEY not in observations:
        return _zero_grads(like.new_zeros(rows, enc.output_size), *enc.parameters())
    y = enc(observations)
    if y.shape[0] != rows:
        raise ValueError(f"{model} takes one {enc.KEY} frame per row: {rows} rows, observations['{enc.KEY}'] {tuple(observations[enc.KEY].shape)}")
    return y * 0 if ablated else y


def _init_monitor(progress_monitor):
    """the reference's _init_layers (seq2seq.py:136-138, seq2seq_highlevel_cma.py:166-168, seq2seq_lowlevel.py:112-114)"""
    nn.init.kaiming_normal_(progress_monitor.weight, nonlinearity="tanh")
    nn.init.constant_(progress_monitor.bias, 0)


def _model_slot(feat, slot):
    """one model's entry of a feature HCMEngine.encode_features returned for both: (high, low) pairs -> entry `slot`; a tensor is taken as it is"""
    return feat[slot] if isinstance(feat, (tuple, list)) else feat


def _check_feature(model, engine, name, feat, rows, shape):
    """A cached trunk feature must be there and be (rows, *shape), shape = (C, s, s), as the engine's encode_features returns it"""
    if feat is None:
        raise ValueError(f"{model} trains from cached trunk features: observations['{name}_features'] is missing; {engine}.encode_features "
                         "returns it from the frames")
    if tuple(feat.shape) != (rows, *shape):
        raise ValueError(f"{model} takes {name}_features {(rows, *shape)} as {engine}.encode_features returns them, got {tuple(feat.shape)}")


def _flat_visual(model, engine, name, feat, fc, ablated, rows, shape, like):
    """One modality's embedding in the flat front end of Seq2SeqNet and LowLevel: relu(fc(flatten(feature))) (rows, out) from the trunk feature;
    ablated: times 0 (seq2seq.py:158-161, seq2seq_lowlevel.py:132-135), and exact zeros without the key"""
    if feat is None and ablated:
        return _zero_grads(like.new_zeros(rows, fc.out_features), fc.weight, fc.bias)
    _check_feature(model, engine, name, feat, rows, shape)
    y = torch.relu(fc(feat.flatten(1)))                                       # Flatten in NCHW order
    return y * 0 if ablated else y


def _visual_fc(fc, x, cm, pooled):
    """The visual FC of CMANet and HighLevel, relu(fc([feature | spatial embedding])) (rows, out), with the feature x (rows, C0, I) and the
    embedding cm (64, I) of enc.tail() as two operands, so no (rows, C0 + 64, I) tensor exists: rgb_linear pools over the positions first
    (AdaptiveAvgPool1d(1)), depth_linear flattens in NCHW order"""
    C0, I = x.shape[1], x.shape[2]
    if pooled:
        x_in = torch.addmm(torch.nn.functional.linear(cm.mean(1), fc.weight[:, C0:], fc.bias), x.mean(2), fc.weight[:, :C0].t())
    else:
        x_in = torch.addmm(torch.nn.functional.linear(cm.reshape(-1), fc.weight[:, C0 * I:], fc.bias), x.flatten(1), fc.weight[:, :C0 * I].t())
    return torch.relu(x_in)


def _progress_target(observations, monitor):
    """observations["progress"] when the model has the monitor (a missing key raises, as S2SEngine.val_step does), None otherwise"""
    if not monitor:
        return None
    if "progress" not in observations:
        raise ValueError("observations['progress'] is missing: the model was built with the progress monitor")
    return observations["progress"]


def _heads_loss(model, x, corrected_actions, oracle_stop, progress):
    """model._flat_heads (flat_heads_loss; tools/bench_flat_update.py swaps in the restatement) over a model's heads; the labels are brought to
    x's device and dtype"""
    rows = x.shape[0]
    labels = [t.to(device=x.device, dtype=x.dtype) for t in (corrected_actions, oracle_stop)]
    if labels[0].numel() != rows * model.linear.out_features or labels[1].numel() != rows:
        raise ValueError(f"update_loss takes corrected_actions ({rows}, {model.linear.out_features}) and oracle_stop ({rows}, 1), got "
                         f"{tuple(corrected_actions.shape)}, {tuple(oracle_stop.shape)}")
    pm_w = pm_b = None
    if progress is not None:
        progress = progress.to(device=x.device, dtype=x.dtype)
        if tuple(progress.shape) not in ((rows,), (rows, 1)):
            raise ValueError(f"observations['progress'] must be ({rows},) or ({rows}, 1), got {tuple(progress.shape)}")
        pm_w, pm_b = model.progress_monitor.weight, model.progress_monitor.bias
    return model._flat_heads(x, model.linear.weight, model.linear.bias, model.stop_linear.weight, model.stop_linear.bias, pm_w, pm_b,
                             labels[0], labels[1], progress)[0]


class _SpatialEncoder(nn.Module):
    """What a spatial encoder of the reference keeps outside its frozen trunk: the (positions, 64) table under `spatial_embeddings.weight`"""

    def __init__(self, positions):
        super().__init__()
        self.spatial_embeddings = nn.Embedding(positions, 64)

    def tail(self):
        """(channels-major (64, I), kernel operand (I, 64)): the reference appends the table as `.view(1, -1, h, w)` (resnet_encoders.py:91-104,
        :218-231) -- a raw reinterpretation of the (I, 64) storage as 64 channels of I positions, not a transpose -- so channel c of position i
        is element c * I + i of the table"""
        w = self.spatial_embeddings.weight
        cm = w.view(64, w.shape[0])
        return cm, cm.t().contiguous()


class CMANet(_FromReference):
    """The reference's CMANet (models/cma.py:28-333) as a trainable model from cached trunk features: the reference's parameters, buffer, state-dict
    keys and shapes outside the two frozen trunks (robo_vln_amd.synth.cma_spec lists them), and its forward signature.  Takes a
    robo_vln_amd.config.CMAConfig; `embeddings=` goes to InstructionEncoder.

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (output, stop_out, rnn_hidden_states) as cma.py:211-333, with
    observations["rgb_features"] (rows, 2048, 4, 4) and ["depth_features"] (rows, C, s, s) -- what CMAEngine.encode_features returns; an ablated
    modality needs no key -- and ["instruction"] (rows, L) or (1, L).  The returned state is a new tensor (the reference writes into its argument).

    The three attention stages are attn1q on the device and attn1q_ref on the CPU: text attention with qt = state_q(state) W_text_k over the
    instruction encoder's (rows, L, D) output, token-major and masked; RGB and depth attention with qt = text_q(text) W_k over the trunk feature,
    channel-major, with the spatial embedding as the shared tail, and the value projection xbar W_v^T + b_v behind it.  The instruction encoder is
    train.InstructionEncoder and both state encoders train.RNNStateEncoder; the linear layers around them are torch.  rgb_linear and depth_linear
    take the feature and the embedding as two operands, so no (rows, C + 64, I) tensor exists.  The key biases -- text_k.bias and the first
    hidden/2 entries of rgb_kv.bias and depth_kv.bias -- cancel and receive exact zero gradients.  `_scale` is kept as the reference's buffer; the
    stages use its constructor value 1 / sqrt(hidden / 2) as a host number, so nothing is read back from the device.

    update_loss(batch, corrected_actions, oracle_stop) is the model and the criterion of the trainer's update step; progress_monitor=True adds the
    auxiliary progress loss to it (CMAConfig.validate keeps refusing its own flag: that is the engine's configuration).  forward is the same
    either way, and without the keyword progress_monitor.* takes part in nothing."""

    FROZEN_PREFIXES = CMA_TRUNK_PREFIXES
    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg, embeddings=None, progress_monitor=False):
        super().__init__()
        cfg.validate()
        self.cfg = cfg
        self.monitor = bool(progress_monitor)
        hh, fs, cc = cfg.hidden // 2, cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.hh, self.depth_shape = hh, (cc, fs * fs)
        self.instruction_encoder = InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden,
                                                      rnn_type=cfg.instr_rnn, bidirectional=cfg.bidirectional, final_state_only=False,
                                                      fine_tune_embeddings=True, embeddings=embeddings)
        self.depth_encoder = _SpatialEncoder(fs * fs)
        self.rgb_encoder = _SpatialEncoder(16)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2048 + 64, cfg.rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear((cc + 64) * fs * fs, cfg.depth_out), nn.ReLU(True))
        self.state_encoder = RNNStateEncoder(cfg.rgb_out + cfg.depth_out, cfg.hidden, 1, cfg.rnn_type)
        self.rgb_kv = nn.Conv1d(2048 + 64, hh + cfg.rgb_out, 1)
        self.depth_kv = nn.Conv1d(cc + 64, hh + cfg.depth_out, 1)
        self.state_q = nn.Linear(cfg.hidden, hh)
        self.text_k = nn.Conv1d(cfg.instr_out, hh, 1)
        self.text_q = nn.Linear(cfg.instr_out, hh)
        self.scale = 1.0 / (hh ** 0.5)
        self.register_buffer("_scale", torch.tensor(self.scale))
        self.second_state_compress = nn.Sequential(nn.Linear(cfg.hidden + cfg.rgb_out + cfg.depth_out + cfg.instr_out, cfg.hidden), nn.ReLU(True))
        self.second_state_encoder = RNNStateEncoder(cfg.hidden, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)      # read by update_loss with progress_monitor=True; parameters only otherwise
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        self.stop_linear = nn.Linear(cfg.hidden, 1)

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers + self.second_state_encoder.num_recurrent_layers

    def _attend(self, q, w_k, x, e, mask_zero, layout, kernel=True):
        fn = attn1q if kernel and x.is_cuda else attn1q_ref
        return fn(q @ w_k, x, e, mask_zero, self.scale, layout)

    def _visual(self, name, feat, enc, fc, pooled, ablated, rows, C0, I, like):
        """One modality's operands: (x (rows, C0, I), e (I, 64), input of the first state encoder (rows, out) by _visual_fc) from the trunk
        feature.  Ablated: zeros for the whole embedding, the spatial tail included (cma.py:238-241)."""
        if ablated:
            return (like.new_zeros(rows, C0, I), like.new_zeros(I, 64),
                    _zero_grads(torch.relu(fc.bias).expand(rows, -1), fc.weight, enc.spatial_embeddings.weight))
        s = int(round(I ** 0.5))
        _check_feature("CMANet", "CMAEngine", name, feat, rows, (C0, s, s))
        x = feat.flatten(2)
        cm, e = enc.tail()
        return x, e, _visual_fc(fc, x, cm, pooled)

    def forward(self, batch, taps=None):
        x, hidden = self._encode(batch, taps)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of `_update_agent` (robo_vln_trainer.py:515-533): the model up to the second state encoder, then
        flat_heads_loss.  -> (result (8,), rnn_hidden_states); result[0] + result[1] + result[2] is the trainer's loss.  With progress_monitor=True
        the auxiliary loss Seq2SeqNet registers (seq2seq.py:176-185) is formed on CMANet's progress_monitor against observations["progress"]."""
        progress = _progress_target(batch[0], self.monitor)
        x, hidden = self._encode(batch, None)
        return _heads_loss(self, x, corrected_actions, oracle_stop, progress), hidden

    def _encode(self, batch, taps):
        """forward up to the second state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg, hh = self.cfg, self.hh
        masks = masks.reshape(masks.shape[0], -1)[:, 0]
        rows = masks.shape[0]
        R = self.state_encoder.num_recurrent_layers
        instruction = observations["instruction"].long()
        instruction = instruction.expand(rows, instruction.shape[1])
        ins = self.instruction_encoder(instruction).permute(0, 2, 1)            # (rows, L, D): the encoder's own storage order
        if cfg.ablate_instruction:
            ins = ins * 0                                                       # every position masked: uniform weights, text = exact zeros
        cc, I_d = self.depth_shape
        rgb_x, rgb_e, rgb_in = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder, self.rgb_linear[2], True, cfg.ablate_rgb,
                                            rows, 2048, 16, ins)
        dep_x, dep_e, dep_in = self._visual("depth", observations.get("depth_features"), self.depth_encoder, self.depth_linear[1], False,
                                            cfg.ablate_depth, rows, cc, I_d, ins)
        state, h1 = self.state_encoder(torch.cat([rgb_in, dep_in], 1), rnn_hidden_states[:R], masks)

        text = self._attend(self.state_q(state), self.text_k.weight[:, :, 0], ins, None, True, TOKEN_MAJOR)
        text = _ZeroGrad.apply(text, self.text_k.bias)
        text_q = self.text_q(text)
        att = []
        for x, e, kv, ablated in ((rgb_x, rgb_e, self.rgb_kv, cfg.ablate_rgb), (dep_x, dep_e, self.depth_kv, cfg.ablate_depth)):
            xbar = self._attend(text_q, kv.weight[:hh, :, 0], x, e, False, CHANNEL_MAJOR, kernel=not ablated)
            att.append(torch.nn.functional.linear(xbar, kv.weight[hh:, :, 0], kv.bias[hh:]))

        x = self.second_state_compress(torch.cat([state, text, att[0], att[1]], 1))
        x, h2 = self.second_state_encoder(x, rnn_hidden_states[R:], masks)
        if taps is not None:
            taps.update(state=state, text=text, rgb_att=att[0], depth_att=att[1], rnn2_out=x)
        return x, torch.cat([h1, h2], 0)


class _FlatRgbEncoder(nn.Module):
    """What TorchVisionResNet50 in flat mode keeps outside its frozen trunk (resnet_encoders.py:189-237): `fc`, 2048 -> output_size, ReLU behind it"""

    def __init__(self, out):
        super().__init__()
        self.fc = nn.Linear(2048, out)


class _FlatDepthEncoder(nn.Module):
    """What VlnResnetDepthEncoder in flat mode keeps outside its frozen trunk (resnet_encoders.py:56-62): visual_fc = Flatten, Linear, ReLU"""

    def __init__(self, in_features, out):
        super().__init__()
        self.visual_fc = nn.Sequential(nn.Flatten(), nn.Linear(in_features, out), nn.ReLU(True))


class Seq2SeqNet(_FromReference):
    """The reference's Seq2SeqNet (models/seq2seq.py:21-189) as a trainable model from cached trunk features: the reference's parameters, state-dict
    keys and shapes outside the two frozen trunks (robo_vln_amd.synth.seq2seq_spec lists them), and its forward signature.  Takes a
    robo_vln_amd.config.S2SConfig; `embeddings=` goes to InstructionEncoder.  The progress monitor is on when cfg.progress_monitor is set.

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (output, stop_out, rnn_hidden_states) as seq2seq.py:140-189, with
    observations["rgb_features"] (rows, 2048, 1, 1) and ["depth_features"] (rows, C, s, s) -- what S2SEngine.encode_features returns; an ablated
    modality needs no key -- and ["instruction"] (rows, L) or (1, L): one instruction is encoded once and expanded (seq2seq.py:163).  The
    instruction encoder is train.InstructionEncoder with final_state_only, the state encoder train.RNNStateEncoder; rgb_encoder.fc and
    depth_encoder.visual_fc.1 with their ReLUs are torch; the cat is the reference's [instruction | depth | rgb].  sub_goal_linear holds
    parameters only, as in the reference.  update_loss(batch, corrected_actions, oracle_stop) is the model and the criterion of the trainer's
    update step, with the auxiliary progress loss against observations["progress"] when the monitor is on.

    The SimpleCNN encoders are trunks that train with the model: there is nothing to cache, and without a keyword they are refused.  With
    trainable_trunks=True a modality whose encoder is a SimpleCNN gets train.SimpleRGBCNN / train.SimpleDepthCNN under the reference's keys
    (rgb_encoder.cnn.*, depth_encoder.cnn.*), reads observations["rgb"] / ["depth"] -- the frames -- in place of the cached feature, and is
    loaded by load_reference_state_dict with everything else; a ResNet modality of the same model still trains from its cached feature."""

    FROZEN_PREFIXES = S2S_TRUNK_PREFIXES
    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg, embeddings=None, trainable_trunks=False):
        super().__init__()
        cfg.validate()
        self.simple_rgb, self.simple_depth = _simple_trunks("Seq2SeqNet", cfg, trainable_trunks)
        self.FROZEN_PREFIXES = _frozen_prefixes(self.simple_rgb, self.simple_depth)
        self.cfg = cfg
        self.monitor = bool(cfg.progress_monitor)
        fs, cc = (0, 0) if self.simple_depth else (cfg.depth_final_spatial(), cfg.depth_compress_channels())
        self.depth_shape = (cc, fs)
        self.instruction_encoder = InstructionEncoder(vocab_size=cfg.vocab_size, embedding_size=cfg.embedding_size, hidden_size=cfg.instr_hidden,
                                                      rnn_type=cfg.instr_rnn, bidirectional=False, final_state_only=True,
                                                      fine_tune_embeddings=True, embeddings=embeddings)
        self.depth_encoder = SimpleDepthCNN(cfg.depth_shape, cfg.depth_out) if self.simple_depth else _FlatDepthEncoder(cc * fs * fs, cfg.depth_out)
        self.rgb_encoder = SimpleRGBCNN(cfg.rgb_shape, cfg.rgb_out) if self.simple_rgb else _FlatRgbEncoder(cfg.rgb_out)
        self.state_encoder = RNNStateEncoder(cfg.rnn_input_size, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        self.sub_goal_linear = nn.Linear(cfg.hidden, cfg.num_sub_tasks)      # parameters only (seq2seq.py:108): no forward reads it
        self.stop_linear = nn.Linear(cfg.hidden, 1)
        _init_monitor(self.progress_monitor)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def _encode(self, batch):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                       # :172
        rows = masks.shape[0]
        instruction = observations["instruction"].long()
        if instruction.dim() != 2 or instruction.shape[0] not in (1, rows):
            raise ValueError(f"Seq2SeqNet takes instruction ({rows} or 1, L), got {tuple(instruction.shape)}")
        ins = self.instruction_encoder(instruction)                           # :153
        cc, fs = self.depth_shape
        if self.simple_depth:
            depth = _simple_visual("Seq2SeqNet", self.depth_encoder, observations, cfg.ablate_depth, rows, ins)
        else:
            depth = _flat_visual("Seq2SeqNet", "S2SEngine", "depth", observations.get("depth_features"), self.depth_encoder.visual_fc[1],
                                 cfg.ablate_depth, rows, (cc, fs, fs), ins)
        if self.simple_rgb:
            rgb = _simple_visual("Seq2SeqNet", self.rgb_encoder, observations, cfg.ablate_rgb, rows, ins)
        else:
            rgb = _flat_visual("Seq2SeqNet", "S2SEngine", "rgb", observations.get("rgb_features"), self.rgb_encoder.fc, cfg.ablate_rgb, rows,
                               (2048, 1, 1), ins)
        if cfg.ablate_instruction:
            ins = ins * 0                                                     # :156-157
        ins = ins.expand(rows, ins.shape[1])                                  # :163
        x = torch.cat([ins, depth, rgb], 1)                                   # :164
        return self.state_encoder(x, rnn_hidden_states, masks)                # :174

    def forward(self, batch):
        x, hidden = self._encode(batch)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of `_update_agent` (robo_vln_trainer.py:515-533): the model up to the state encoder, then flat_heads_loss.
        -> (result (8,), rnn_hidden_states); result[0] + result[1] + result[2] is the trainer's loss."""
        progress = _progress_target(batch[0], self.monitor)
        x, hidden = self._encode(batch)
        return _heads_loss(self, x, corrected_actions, oracle_stop, progress), hidden


def flat_update(model, optimizer, observations, prev_actions, not_done_masks, corrected_actions, oracle_stop, rnn_hidden_states):
    """The reference's `_update_agent` (robo_vln_trainer.py:505-542) for train.CMANet / train.Seq2SeqNet: zero_grad, detach the carried state
    (repackage_hidden), model.update_loss, loss = result[0] + result[1] + result[2], backward, optimizer.step().  Returns (result, rnn_hidden_states)
    with `result` the detached (8,) tensor on the model's device -- [action loss, stop loss, aux loss, stop rows, aux rows, 0, 0, 0] -- where the
    reference returns three host numbers: nothing is read back and nothing synchronises, so a caller keeps the results of an epoch and reads once,
    as FlatValidator does."""
    optimizer.zero_grad()
    rnn_hidden_states = rnn_hidden_states.detach()
    result, rnn_hidden_states = model.update_loss((observations, rnn_hidden_states, prev_actions, not_done_masks), corrected_actions, oracle_stop)
    loss = result[0] + result[1] + result[2]
    loss.backward()
    optimizer.step()
    return result.detach(), rnn_hidden_states


class HighLevel(_FromReference):
    """The reference's Seq2Seq_HighLevel_CMA (models/seq2seq_highlevel_cma.py:29-233) as a trainable model from cached trunk features and a cached
    instruction stream: the reference's parameters, state-dict keys and shapes outside its three frozen parts -- the two trunks and BERT
    (robo_vln_amd.synth.high_level_spec lists them all) -- and its forward signature.  Takes a robo_vln_amd.config.HCMConfig; `dropout` is
    VISUAL_LING_ATTN.dropout (config/default.py:164); `embedder`, optional, maps token ids (B, L) to BERT's last hidden state (B, L, ins_in).

    forward((observations, rnn_hidden_states, prev_actions, masks)) -> (logits, rnn_hidden_states) as :170-233, with
    observations["rgb_features"] (rows, 2048, 4, 4) and ["depth_features"] (rows, C, s, s) -- the high entries of HCMEngine.encode_features' pairs;
    a pair is accepted and its entry 0 taken; an ablated modality needs no key -- and ["instruction_features"] (rows or 1 or N | rows, L, ins_in): BERT is
    frozen and runs under no_grad in the reference (:192-195), so its output enters as a tensor.  Without that key the stream is
    embedder(observations["instruction"]) under no_grad; with neither a ValueError names the key.

    rgb_kv / depth_kv are 1x1 convolutions of [feature | spatial embedding]: the tokens are x^T W[:, :C0]^T plus a row-independent (I, vis_in)
    tail from the spatial table and the bias, computed once per call -- no (rows, C0 + 64, I) tensor is formed -- and rgb_linear / depth_linear
    take the two operands as train.CMANet's do.  Then the two Visual_Ling_Attn calls on the one image_cm_encoder, the token mean over all L
    positions (cross_pooler), the cat [rgb_in | depth_in | ins_rgb | ins_depth], train.RNNStateEncoder and `linear`.  ablate_rgb / ablate_depth zero
    the whole embedding, the spatial tail included (:185-188); ablate_instruction and use_prev_action are branches the reference cannot run and
    HCMConfig.validate refuses them.  ins_fc and progress_monitor hold parameters only: no forward of the reference reads the first, the
    monitor's branch reads an undefined name (:221-224) and the trainer adds no aux loss.

    update_loss(batch, oracle_subtask) -> (result (8,), rnn_hidden_states) is the model and the criterion of the trainer's high-level step through
    subtask_ce; result[0] is the loss."""

    FROZEN_PREFIXES = HCM_HIGH_FROZEN_PREFIXES
    _subtask_ce = staticmethod(subtask_ce)

    def __init__(self, cfg, embedder=None, dropout=0.25):
        super().__init__()
        cfg.validate()
        _refuse_simple_cnn("HighLevel", cfg)
        self.cfg = cfg
        object.__setattr__(self, "embedder", embedder)        # frozen and the caller's: not a submodule, so no key of it enters the state dict
        fs, cc = cfg.depth_final_spatial(), cfg.depth_compress_channels()
        self.depth_shape = (cc, fs * fs)
        self.ins_fc = nn.Linear(768, 256)                     # TRANSFORMER_INSTRUCTION_ENCODER d_in / d_model (:46): parameters only
        self.depth_encoder = _SpatialEncoder(fs * fs)
        self.rgb_encoder = _SpatialEncoder(16)
        self.rgb_linear = nn.Sequential(nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(2048 + 64, cfg.rgb_out), nn.ReLU(True))
        self.depth_linear = nn.Sequential(nn.Flatten(), nn.Linear((cc + 64) * fs * fs, cfg.depth_out), nn.ReLU(True))
        self.rgb_kv = nn.Conv1d(2048 + 64, cfg.vis_in, 1)
        self.depth_kv = nn.Conv1d(cc + 64, cfg.vis_in, 1)
        self.image_cm_encoder = Visual_Ling_Attn(N=cfg.vla_layers, vis_in_features=cfg.vis_in, ins_in_features=cfg.ins_in, d_model=cfg.d_model,
                                                 h=cfg.vla_heads, d_ff=cfg.d_ff, dropout=dropout)
        self.state_encoder = RNNStateEncoder(cfg.cm_d_model * 2 + cfg.depth_out + cfg.rgb_out, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        self.linear = nn.Linear(cfg.hidden, cfg.num_actions)
        _init_monitor(self.progress_monitor)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def _instruction_stream(self, observations, rows):
        stream = observations.get("instruction_features")
        if stream is None:
            if self.embedder is None or "instruction" not in observations:
                raise ValueError("HighLevel trains from the frozen BERT's output: observations['instruction_features'] (rows or 1, L, "
                                 f"{self.cfg.ins_in}) is missing, and there is no embedder with observations['instruction'] to compute it from")
            with torch.no_grad():                                              # :192-195
                stream = self.embedder(observations["instruction"].long())
        if stream.dim() != 3 or stream.shape[0] < 1 or rows % stream.shape[0] or stream.shape[2] != self.cfg.ins_in:
            raise ValueError(f"HighLevel takes instruction_features ({rows} or 1, L, {self.cfg.ins_in}) -- or (N, L, {self.cfg.ins_in}) with N dividing "
                             f"the {rows} time-major rows, one stream per trajectory -- got {tuple(stream.shape)}")
        if stream.shape[0] not in (1, rows):
            # one stream per trajectory (HCMEngine.encode_instruction of the N instructions): row t*N + n takes trajectory n's, as the collate repeats the ids
            return stream.detach().repeat(rows // stream.shape[0], 1, 1)
        return stream.detach().expand(rows, stream.shape[1], stream.shape[2])  # :190

    def _visual(self, name, feat, enc, fc, kv, pooled, ablated, rows, C0, I, like):
        """One modality: (tokens (rows, I, vis_in) = the 1x1 convolution of [feature | spatial embedding], transposed as the cross-modal encoder
        takes it; input of the state encoder (rows, out) by _visual_fc).  Ablated: zeros for the whole embedding, so the tokens are the bias alone."""
        if ablated:
            return (_zero_grads(kv.bias.expand(rows, I, -1), kv.weight),
                    _zero_grads(torch.relu(fc.bias).expand(rows, -1), fc.weight, enc.spatial_embeddings.weight))
        feat = _model_slot(feat, 0)
        s = int(round(I ** 0.5))
        _check_feature("HighLevel", "HCMEngine", name, feat, rows, (C0, s, s))
        x = feat.flatten(2)
        cm, e = enc.tail()
        w = kv.weight[:, :, 0]
        tail = torch.addmm(kv.bias, e, w[:, C0:].t())                          # (I, vis_in): the same for every row
        tokens = torch.matmul(x.transpose(1, 2), w[:, :C0].t()) + tail
        return tokens, _visual_fc(fc, x, cm, pooled)

    def _encode(self, batch, taps=None):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                        # :208
        rows = masks.shape[0]
        embedded = self._instruction_stream(observations, rows)
        cc, I_d = self.depth_shape
        rgb_tok, rgb_in = self._visual("rgb", observations.get("rgb_features"), self.rgb_encoder, self.rgb_linear[2], self.rgb_kv, True,
                                       cfg.ablate_rgb, rows, 2048, 16, embedded)
        dep_tok, dep_in = self._visual("depth", observations.get("depth_features"), self.depth_encoder, self.depth_linear[1], self.depth_kv, False,
                                       cfg.ablate_depth, rows, cc, I_d, embedded)
        ins_rgb = self.image_cm_encoder(embedded, rgb_tok, None, None).mean(1)      # :200, :209
        ins_dep = self.image_cm_encoder(embedded, dep_tok, None, None).mean(1)      # :201, :210
        x = torch.cat((rgb_in, dep_in, ins_rgb, ins_dep), 1)                   # :215
        if taps is not None:
            taps.update(rgb_kv=rgb_tok, depth_kv=dep_tok, rnn_in=x)
        return self.state_encoder(x, rnn_hidden_states, masks)                 # :219

    def forward(self, batch, taps=None):
        x, hidden = self._encode(batch, taps)
        return self.linear(x), hidden

    def update_loss(self, batch, oracle_subtask):
        """The forward and the criterion of the high-level half of `_update_agent` (hierarchical_trainer.py:505-511): the model up to the state
        encoder, then subtask_ce with oracle_subtask as the collate function carries it ((rows, 1) float, converted on the device).
        -> (result (8,), rnn_hidden_states); result[0] is the trainer's high-level loss."""
        x, hidden = self._encode(batch)
        if oracle_subtask.numel() != x.shape[0]:
            raise ValueError(f"update_loss takes oracle_subtask ({x.shape[0]}, 1), got {tuple(oracle_subtask.shape)}")
        return self._subtask_ce(x, self.linear.weight, self.linear.bias, oracle_subtask.to(x.device), self.cfg.num_sub_tasks)[0], hidden


class LowLevel(_FromReference):
    """The reference's Seq2Seq_LowLevel (models/seq2seq_lowlevel.py:21-162) as a trainable model from cached trunk features: the reference's
    parameters, state-dict keys and shapes outside the two frozen trunks (robo_vln_amd.synth.low_level_spec lists them), and its forward signature.
    Takes a robo_vln_amd.config.HCMConfig.

    forward((observations, rnn_hidden_states, prev_actions, masks, discrete_actions)) -> (output, stop_out, rnn_hidden_states) as :116-162, with
    observations["rgb_features"] (rows, 2048, 1, 1) and ["depth_features"] (rows, C, s, s) -- the low entries of HCMEngine.encode_features' pairs;
    a pair is accepted and its entry 1 taken; an ablated modality needs no key -- and discrete_actions (rows,) the sub-task of every row,
    num_sub_tasks on the padded ones.  rgb_encoder.fc and depth_encoder.visual_fc.1 with their ReLUs are torch, as in train.Seq2SeqNet;
    sub_task_embedding has padding_idx = num_sub_tasks (the reference writes 4, its num_sub_tasks): that row is zero at construction and gets
    no gradient; the cat is the reference's [depth | rgb | sub_task]; the state encoder is train.RNNStateEncoder.  progress_monitor holds
    parameters only (the trainer clears AuxLosses and adds no aux loss).

    update_loss(batch, corrected_actions, oracle_stop) -> (result (8,), rnn_hidden_states) is the model and the criterion of the trainer's
    low-level step through flat_heads_loss without the monitor; result[0] + result[1] is the loss.

    The SimpleCNN encoders are trunks that train with the model: there is nothing to cache, and without a keyword they are refused.  With
    trainable_trunks=True a modality whose encoder is a SimpleCNN gets train.SimpleRGBCNN / train.SimpleDepthCNN under the reference's keys
    (rgb_encoder.cnn.*, depth_encoder.cnn.*), reads observations["rgb"] / ["depth"] -- the frames -- in place of the cached feature, and is
    loaded by load_reference_state_dict with everything else; a ResNet modality of the same model still trains from its cached feature.  The
    state dict of such a model is what HCMEngine loads as its low-level weights."""

    FROZEN_PREFIXES = HCM_LOW_FROZEN_PREFIXES
    _flat_heads = staticmethod(flat_heads_loss)

    def __init__(self, cfg, trainable_trunks=False):
        super().__init__()
        cfg.validate()
        self.simple_rgb, self.simple_depth = _simple_trunks("LowLevel", cfg, trainable_trunks)
        self.FROZEN_PREFIXES = _frozen_prefixes(self.simple_rgb, self.simple_depth)
        self.cfg = cfg
        fs, cc = (0, 0) if self.simple_depth else (cfg.depth_final_spatial(), cfg.depth_compress_channels())
        self.depth_shape = (cc, fs)
        self.depth_encoder = SimpleDepthCNN(cfg.depth_shape, cfg.depth_out) if self.simple_depth else _FlatDepthEncoder(cc * fs * fs, cfg.depth_out)
        self.rgb_encoder = SimpleRGBCNN(cfg.rgb_shape, cfg.rgb_out) if self.simple_rgb else _FlatRgbEncoder(cfg.rgb_out)
        self.sub_task_embedding = nn.Embedding(cfg.num_sub_tasks + 1, 32, padding_idx=cfg.num_sub_tasks)
        self.state_encoder = RNNStateEncoder(cfg.depth_out + cfg.rgb_out + 32, cfg.hidden, 1, cfg.rnn_type)
        self.progress_monitor = nn.Linear(cfg.hidden, 1)
        _init_monitor(self.progress_monitor)                 # before `linear` is drawn, as the reference's __init__ has it
        self.linear = nn.Linear(cfg.hidden, cfg.lo_actions)
        self.stop_linear = nn.Linear(cfg.hidden, 1)

    @property
    def output_size(self):
        return self.cfg.hidden

    @property
    def num_recurrent_layers(self):
        return self.state_encoder.num_recurrent_layers

    def _encode(self, batch):
        """forward up to the state encoder: (its output (rows, hidden), the new packed state)"""
        observations, rnn_hidden_states, prev_actions, masks, discrete_actions = batch
        cfg = self.cfg
        masks = masks.reshape(masks.shape[0], -1)[:, 0]                        # :145
        rows = masks.shape[0]
        if discrete_actions.numel() != rows or discrete_actions.dtype.is_floating_point:
            raise ValueError(f"LowLevel takes discrete_actions ({rows},) as an integer tensor, got {discrete_actions.dtype} {tuple(discrete_actions.shape)}")
        cc, fs = self.depth_shape
        if self.simple_depth:
            depth = _simple_visual("LowLevel", self.depth_encoder, observations, cfg.ablate_depth, rows, rnn_hidden_states)
        else:
            depth = _flat_visual("LowLevel", "HCMEngine", "depth", _model_slot(observations.get("depth_features"), 1),
                                 self.depth_encoder.visual_fc[1], cfg.ablate_depth, rows, (cc, fs, fs), rnn_hidden_states)
        if self.simple_rgb:
            rgb = _simple_visual("LowLevel", self.rgb_encoder, observations, cfg.ablate_rgb, rows, rnn_hidden_states)
        else:
            rgb = _flat_visual("LowLevel", "HCMEngine", "rgb", _model_slot(observations.get("rgb_features"), 1), self.rgb_encoder.fc, cfg.ablate_rgb,
                               rows, (2048, 1, 1), rnn_hidden_states)
        sub_task = self.sub_task_embedding(discrete_actions.reshape(-1).long())    # :141
        x = torch.cat([depth, rgb, sub_task], 1)                               # :143
        return self.state_encoder(x, rnn_hidden_states, masks)                 # :147

    def forward(self, batch):
        x, hidden = self._encode(batch)
        return self.linear(x), self.stop_linear(x), hidden

    def update_loss(self, batch, corrected_actions, oracle_stop):
        """The forward and the criterion of the low-level half of `_update_agent` (hierarchical_trainer.py:539-553): the model up to the state
        encoder, then flat_heads_loss without the monitor.  -> (result (8,), rnn_hidden_states); result[0] + result[1] is the trainer's loss."""
        x, hidden = self._encode(batch)
        return _heads_loss(self, x, corrected_actions, oracle_stop, None), hidden


def hier_update(high, low, opt_high, opt_low, observations, prev_actions, not_done_masks, corrected_actions, oracle_stop, hi_hidden, lo_hidden):
    """The reference's `_update_agent` (hierarchical_trainer.py:492-560) for train.HighLevel / train.LowLevel, in its order: zero both optimizers,
    detach both carried states (repackage_hidden), the high-level loss with its backward and step, then the low-level model teacher-forced with
    oracle - 1 -- num_sub_tasks where the label is 0 or out of range, formed by torch.where on the device -- with loss = result[0] + result[1],
    backward and step.  observations["vln_oracle_action_sensor"] is the label tensor as the collate function carries it, (rows, 1) float; it is
    converted on the device and `observations` is left as it was (the reference deletes keys from it).  Both models run on one device (the
    reference moves the low-level model's inputs to a second one).

    Returns (result_high, result_low, hi_hidden, lo_hidden), all detached and on the device: result_high (8,) as subtask_ce writes it, result_low
    (8,) as flat_heads_loss does, where the reference returns four host numbers: nothing is read back and nothing synchronises."""
    opt_high.zero_grad()
    opt_low.zero_grad()
    hi_hidden, lo_hidden = hi_hidden.detach(), lo_hidden.detach()
    if "vln_oracle_action_sensor" not in observations:
        raise ValueError("observations['vln_oracle_action_sensor'] is missing: the oracle sub-task of every row, (rows, 1)")
    oracle = observations["vln_oracle_action_sensor"]
    result_high, hi_hidden = high.update_loss((observations, hi_hidden, prev_actions, not_done_masks), oracle)
    result_high[0].backward()
    opt_high.step()

    n = low.cfg.num_sub_tasks
    o = oracle.to(lo_hidden.device).reshape(-1).to(torch.int64)
    discrete_actions = torch.where((o >= 1) & (o <= n), o - 1, torch.full_like(o, n))      # :522-524
    result_low, lo_hidden = low.update_loss((observations, lo_hidden, prev_actions, not_done_masks, discrete_actions), corrected_actions, oracle_stop)
    (result_low[0] + result_low[1]).backward()
    opt_low.step()
    return result_high.detach(), result_low.detach(), hi_hidden.detach(), lo_hidden.detach()
