"""The training side: the differentiable ops over the HIP training kernels (train/ops.py), the reference's modules as drop-ins around them
(train/modules.py), and the four trainable models with the trainers' update steps (train/models.py).  Every name is importable from here, so
`from robo_vln_amd import train; train.X` reads the same whichever of the three X lives in."""
from .models import (CMA_TRUNK_PREFIXES, HCM_HIGH_FROZEN_PREFIXES, HCM_LOW_FROZEN_PREFIXES, S2S_TRUNK_PREFIXES, CMANet, HighLevel, LowLevel, Seq2SeqNet,
                     _FlatDepthEncoder, _FlatRgbEncoder, _heads_loss, _model_slot, _progress_target, _refuse_simple_cnn, _SpatialEncoder, flat_update,
                     hier_update)
from .modules import (InstructionEncoder, InterModuleAttnLayer, RNNStateEncoder, SimpleDepthCNN, SimpleRGBCNN, Visual_Ling_Attn, _MultiHeadAttention, _PositionWiseFeedForward,
                      _ScaledDotProductAttention)
from .ops import (ATTN1Q_MAX_C, ATTN1Q_MAX_I, CHANNEL_MAJOR, EMBED_K_STEP, EMBED_MAX_K, FLAT_HEADS_BWD_HALF, FLAT_HEADS_BWD_ROWS, FLAT_HEADS_FWD_ROWS,
                  FLAT_HEADS_HIDDEN, FLAT_HEADS_MAX_ACTIONS, FLAT_LOSS_THREADS, INSTR_HIDDEN, SCAN_HIDDEN, SUBTASK_CE_BWD_HALF, SUBTASK_CE_BWD_ROWS,
                  SUBTASK_CE_FWD_ROWS, SUBTASK_CE_HIDDEN, SUBTASK_CE_LOSS_THREADS, SUBTASK_CE_MAX_CLASSES, TOKEN_MAJOR, VLA_D_MODEL, VLA_HEADS,
                  VLA_MAX_D_FF, VLA_MAX_KEYS, _Attn1q, _EmbedLn, _f32c, _FlatHeadsLoss, _InstrScan, _instr_params, _ptr, _StateScan, _stream, _SubtaskCe,
                  _subtask_labels, _VlaLayer, _zero_grads, _ZeroGrad, attn1q, attn1q_access, attn1q_ref, cell_loop, embed_k_ok, embed_ln, embed_ln_ref,
                  flat_heads_loss, flat_heads_loss_ref, flat_heads_ok, instr_encoder_ref, instr_scan, mask_dropout, sinusoid_table, state_scan,
                  simple_cnn, simple_cnn_out_hw, simple_cnn_ref, subtask_ce, subtask_ce_ok, subtask_ce_ref, vla_attention_ref, vla_layer, vla_layer_ref,
                  SIMPLE_CNN_CHANNELS, SIMPLE_CNN_MIN_HW, _SimpleCnn)
