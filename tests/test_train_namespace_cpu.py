"""robo_vln_amd.train is a package of three modules; every name the single module train.py defined at module level before the split (its functions,
classes and assignments, read off its syntax tree) is still an attribute of the package."""
import importlib

from robo_vln_amd import train

NAMES = [
    "SCAN_HIDDEN", "INSTR_HIDDEN", "VLA_D_MODEL", "VLA_HEADS", "VLA_MAX_KEYS", "VLA_MAX_D_FF", "EMBED_K_STEP", "EMBED_MAX_K", "_ptr", "_stream", "_f32c",
    "_StateScan", "state_scan", "cell_loop", "RNNStateEncoder", "mask_dropout", "vla_attention_ref", "vla_layer_ref", "_VlaLayer", "vla_layer",
    "_ScaledDotProductAttention", "_MultiHeadAttention", "_PositionWiseFeedForward", "InterModuleAttnLayer", "sinusoid_table", "embed_ln_ref",
    "embed_k_ok", "_EmbedLn", "embed_ln", "Visual_Ling_Attn", "_instr_params", "instr_encoder_ref", "_InstrScan", "instr_scan", "InstructionEncoder",
    "TOKEN_MAJOR", "CHANNEL_MAJOR", "ATTN1Q_MAX_I", "ATTN1Q_MAX_C", "attn1q_access", "attn1q_ref", "_Attn1q", "attn1q", "FLAT_HEADS_HIDDEN",
    "FLAT_HEADS_MAX_ACTIONS", "FLAT_HEADS_FWD_ROWS", "FLAT_HEADS_BWD_ROWS", "FLAT_HEADS_BWD_HALF", "FLAT_LOSS_THREADS", "flat_heads_ok",
    "flat_heads_loss_ref", "_FlatHeadsLoss", "flat_heads_loss", "_progress_target", "_heads_loss", "_ZeroGrad", "_zero_grads", "_SpatialEncoder",
    "CMA_TRUNK_PREFIXES", "CMANet", "S2S_TRUNK_PREFIXES", "_FlatRgbEncoder", "_FlatDepthEncoder", "Seq2SeqNet", "flat_update", "SUBTASK_CE_HIDDEN",
    "SUBTASK_CE_MAX_CLASSES", "SUBTASK_CE_FWD_ROWS", "SUBTASK_CE_BWD_ROWS", "SUBTASK_CE_BWD_HALF", "SUBTASK_CE_LOSS_THREADS", "subtask_ce_ok",
    "_subtask_labels", "subtask_ce_ref", "_SubtaskCe", "subtask_ce", "_model_slot", "HCM_HIGH_FROZEN_PREFIXES", "HCM_LOW_FROZEN_PREFIXES",
    "_refuse_simple_cnn", "HighLevel", "LowLevel", "hier_update",
]


def test_every_name_of_the_single_module_is_an_attribute_of_the_package():
    assert len(set(NAMES)) == len(NAMES) == 83
    assert [n for n in NAMES if not hasattr(train, n)] == []


def test_the_three_modules_import():
    for name in ("ops", "modules", "models"):
        assert importlib.import_module(f"robo_vln_amd.train.{name}").__name__ == f"robo_vln_amd.train.{name}"
