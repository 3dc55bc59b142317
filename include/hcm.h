/*
 * libhcm -- MI355X-native per-step policy forward of robo-vln's Hierarchical Cross-Modal agent.
 *
 * Plain C ABI (no torch types): pointers, sizes, an opaque handle.  Every entry point returns an
 * int status (0 = ok, negative = hcm_status) and records a message readable by hcm_last_error().
 * All I/O buffers of the forward calls are caller-owned DEVICE pointers; weights passed to
 * hcm_load_tensor are HOST pointers.  All work of a forward call is enqueued on the passed
 * hipStream_t (as void*); no host synchronisation happens inside a forward call.  A handle is not
 * thread-safe: one handle per device per thread.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/robo_vln_baselines/).  The reference is pure Python with no FFI; the ctypes
 * binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef HCM_H
#define HCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hcm_ctx* hcm_handle;

enum hcm_status {
    HCM_OK = 0,
    HCM_ERR_ARG = -1,          /* null / out-of-range argument                         (Python: ValueError)  */
    HCM_ERR_STATE = -2,        /* call order violated (e.g. forward before finalize)   (RuntimeError)        */
    HCM_ERR_KEY = -3,          /* unknown or missing state_dict key                    (KeyError)            */
    HCM_ERR_SHAPE = -4,        /* tensor shape does not match the configured model     (ValueError)          */
    HCM_ERR_HIP = -5,          /* HIP runtime error                                    (RuntimeError)        */
    HCM_ERR_UNSUPPORTED = -6,  /* configuration the reference itself cannot run        (ValueError)          */
    HCM_ERR_NOMEM = -7
};

enum hcm_dtype { HCM_F32 = 0, HCM_BF16 = 1, HCM_I32 = 2, HCM_I64 = 3, HCM_U8 = 4, HCM_F16 = 5,
                 HCM_FEATURES = 6 /* as `rgb_dtype` only: the `rgb` argument is a host `const hcm_features*` (below) */,
                 HCM_INSTR_FEATURES = 7 /* as `ids_dtype` only: the `ids` argument is a host `const hcm_instr_features*` (below) */ };
enum hcm_model { HCM_HIGH = 0, HCM_LOW = 1, HCM_CMA = 2 /* CMANet flat baseline: hcm_cma_create handles only */,
                 HCM_S2S = 3 /* Seq2SeqNet flat baseline: hcm_s2s_create handles only */ };
enum hcm_encoder { HCM_ENC_RESNET = 0, HCM_ENC_SIMPLECNN = 1 };
enum hcm_rnn { HCM_LSTM = 0, HCM_GRU = 1 };

/* hcm_query() selectors: properties the reference's callers read from the models
 * (state_encoder.num_recurrent_layers hierarchical_trainer.py:1053,:1059; MODEL.STATE_ENCODER.hidden_size). */
enum hcm_query_what {
    HCM_NUM_RECURRENT_LAYERS = 0,  /* 2 for LSTM (cat[h,c]), 1 for GRU: models/decoder/state_encoder.py:41-45 */
    HCM_HIDDEN_SIZE = 1,
    HCM_NUM_ACTIONS = 2,           /* high-level sub-task logits (4) */
    HCM_RECORD_WIDTH = 3,          /* 7 = 4 logits + (v, w) + stop logit */
    HCM_WORKSPACE_BYTES = 4,
    HCM_WEIGHT_BYTES = 5,
    HCM_MAX_BATCH = 6,
    HCM_GRAPH_LAUNCHES = 7,        /* hcm_act calls served by a captured hipGraph replay */
    HCM_EAGER_LAUNCHES = 8,
    HCM_FP16_FALLBACK = 9,         /* bit 0: BERT, bit 1: the depth trunks, bit 2: the RGB trunks, bit 3: the cross-modal block were re-built on bf16 tiles after a range calibration */
    HCM_CALIB_MAX_BERT = 10,       /* max |x| (rounded down) over the GEMM outputs of BERT / the depth trunks in the last calibration forward */
    HCM_CALIB_MAX_DEPTH = 11,
    HCM_CALIB_NONFINITE = 12,      /* non-finite values seen in the last calibration forward */
    HCM_CALIB_MAX_RGB = 13,        /* as HCM_CALIB_MAX_BERT, over the conv outputs of the RGB trunks */
    HCM_CALIB_MAX_VLA = 14,        /* ... over the cross-modal block (its GEMM outputs and the fused layer's LDS-only intermediates) */
    HCM_STEP_NONFINITE = 15,       /* overflow guard: (sample, recurrent step) pairs since hcm_finalize whose gate pre-activations were not all
                                      finite -- an fp16 overflow or a NaN anywhere upstream of the state encoder lands there, and the squashing
                                      cell would otherwise turn it into finite garbage.  0 on a healthy engine.  Synchronises the device. */
    HCM_GATHER_JOINED = 17,        /* 1 when the handle's LAST hcm_act_gather / hcm_gather_poison call enqueued its ncclAllGather, 0 when it returned in
                                      front of the collective (argument error, no communicator): a caller whose peers are about to enter the step's
                                      all-gather must then join it itself (hcm_gather_poison) -- robo-vln_amd/policy.py act(gather=True) */
    /* hcm_features: f32 elements PER ROW of the feature tensor a (model, modality) takes; 0 = it takes none (SimpleCNN encoder, ablated modality,
       model not held).  HI = the high-level model, or the one model of a CMANet / Seq2SeqNet handle; LO = the low-level model */
    HCM_FEAT_RGB_HI = 18, HCM_FEAT_RGB_LO = 19, HCM_FEAT_DEPTH_HI = 20, HCM_FEAT_DEPTH_LO = 21,
    HCM_FEAT_SHARED = 22,          /* bit 0: the two models' RGB trunks are one (bit-identical weights, hcm_config.reserved[5] clear), bit 1: the depth trunks */
    HCM_RANGE_FOLD = 16            /* bit 1: a power-of-two scale was folded into convs of the GroupNorm depth trunks, bit 2: into the RGB trunks
                                      (the exact alternative to a bf16 fall-back where the network is scale-invariant; hcm_calibrate below) */
};

/* Model hyper-parameters: the values the reference reads from MODEL.* (config/default.py:131,:156-164,
 * :180-199).  Zero-initialise, set struct_size = sizeof(hcm_config), fill. */
typedef struct hcm_config {
    int32_t struct_size;
    int32_t precision;        /* HCM_F16: fp16 storage + fp16 MFMA tiles behind the range calibration below (the measured 16-bit mode);
                                 HCM_BF16: bf16 storage + bf16 MFMA tiles in BERT (f32 residual stream) and the cross-modal block -- the sub-networks that
                                 are not scale-invariant (no range limit there); both trunk kinds stay on range-folded fp16 tiles (GroupNorm's
                                 subtraction amplifies bf16's rounding 8x: 1.9e-2 on the record from the depth trunk alone; the RGB trunks' 50
                                 bf16-rounded layers were 6e-3 of a 1e-2 tolerance -- and the exact power-of-two folds make fp16 range-safe in
                                 both by construction; round 6);
                                 HCM_F32: fp32 MFMA.  fp32 accumulation and fp32 recurrent cells / heads in every mode */
    int32_t max_batch;        /* workspace is sized for this many environments per call */
    int32_t rgb_h, rgb_w;     /* frames are NHWC; any H x W >= 32 with HCM_ENC_RESNET (adaptive pools, resnet_encoders.py:211-236), >= 36 with HCM_ENC_SIMPLECNN (simple_cnns.py:63-73) */
    int32_t depth_h, depth_w; /* HCM_ENC_RESNET: square, a multiple of 64, <= 1024 (habitat sizes the encoder from the frame height); HCM_ENC_SIMPLECNN: any H x W >= 36 */
    int32_t instr_len;        /* MAXIMUM instruction length: sizes the workspace (and the positional tables); every forward call
                                 passes its own L <= instr_len (the reference model accepts any (B or 1, L) per call and its
                                 eval loop feeds unpadded ids, common/utils.py:18-20); <= bert_max_pos (512) */
    int32_t rgb_encoder;      /* hcm_encoder; SIMPLECNN is valid for the low-level model only */
    int32_t depth_encoder;
    int32_t rgb_out, depth_out, depth_baseplanes;
    int32_t vla_layers, d_model, vla_heads, d_ff, vis_in, ins_in;
    int32_t hidden, rnn_type, num_actions, num_sub_tasks, lo_actions;
    int32_t bert_layers, bert_hidden, bert_heads, bert_inter, bert_vocab, bert_max_pos;
    int32_t build_high, build_low;      /* which of the two models this handle holds */
    int32_t use_prev_action;            /* must be 0: broken branch in the reference (seq2seq_highlevel_cma.py:203-207) */
    int32_t ablate_instruction;         /* must be 0: broken branch (:183-184) */
    int32_t progress_monitor;           /* must be 0 in forward (:221-225 references an undefined name) */
    int32_t ablate_depth;               /* working flags of both models: the encoder output is multiplied by 0 */
    int32_t ablate_rgb;                 /* (seq2seq_highlevel_cma.py:185-188, seq2seq_lowlevel.py:132-135, config/default.py:92-93) */
    int32_t reserved[8];                /* [0..3]: storage-type override (hcm_dtype + 1, 0 = default) for the depth trunk /
                                           BERT / cross-modal block / RGB trunk; see DESIGN.md section 5.
                                           [4]: keep the f32 host copies of the weights after hcm_finalize so that hcm_calibrate can
                                           re-build a sub-network (release them with hcm_release_host_weights)
                                           [5]: 1 = do not share a trunk between the two models when their trunk weights are bit-identical
                                           (the default runs it once per step and feeds both heads: same values, half the work) */
} hcm_config;

/* Precomputed trunk features: the `rgb_features` / `depth_features` observation keys of the reference's ResNet encoders.
 * VlnResnetDepthEncoder.forward takes observations["depth_features"] instead of running visual_encoder (models/encoders/resnet_encoders.py:83-86),
 * TorchVisionResNet50.forward takes observations["rgb_features"] instead of running the hooked cnn (:207-214); both trunks are frozen
 * (:35-36, :146-149), so a caller that walks the same recorded frames again (val_epoch) can compute them once.
 * Every entry point that takes `rgb, rgb_dtype, depth` accepts rgb_dtype == HCM_FEATURES: `rgb` is then a HOST pointer to this struct and `depth`
 * must be NULL.  The members are DEVICE pointers; the struct itself is consumed during the call.
 *   rgb / rgb_dtype / depth   the frames, as the entry point documents them, for every (model, modality) whose feature pointer is NULL;
 *                             may be NULL when no trunk of the call needs them
 *   rgb_feat[m], depth_feat[m]  m = 0: the high-level model, or the one model of a CMANet / Seq2SeqNet handle; m = 1: the low-level model.
 *                             Non-NULL replaces that model's trunk; given together with a frame the feature wins, as in the reference.
 * Layouts (the reference's, f32, contiguous; element counts per row from hcm_query(HCM_FEAT_*)):
 *   rgb_feat of a spatial encoder (high-level model, CMANet)   (rows, 2048, 4, 4): the hooked avgpool output behind adaptive_avg_pool2d((4,4)) (:225-230)
 *   rgb_feat of a flat encoder (low-level model, Seq2SeqNet)   (rows, 2048, 1, 1)  (:234-236)
 *   depth_feat                                                 (rows, C, s, s), C = round(2048 / s^2), s = depth_h / 64: the ResNetEncoder output (:87-88)
 * The values are the reference's: a range fold of the RGB trunk (HCM_RANGE_FOLD) is multiplied in on the way in and divided out by
 * hcm_encode_features, both exactly.  Non-finite values propagate and end up in the overflow guard (HCM_STEP_NONFINITE) like a broken frame's.
 * Refused with a message, never a GPU fault: a feature for a SimpleCNN encoder (simple_cnns.py has no such key) or an ablated modality
 * (HCM_ERR_UNSUPPORTED); a feature in a slot the handle has no model for, HCM_ACT_HOST_FRAMES together with HCM_FEATURES, hcm_calibrate with
 * HCM_FEATURES (calibration needs the trunks to run), a NULL frame that some trunk of the call still needs (HCM_ERR_ARG).
 * A captured hcm_act graph is keyed by the four feature pointers like by every other argument. */
typedef struct hcm_features {
    const void*  rgb;  int32_t rgb_dtype;
    const float* depth;
    const float* rgb_feat[2];
    const float* depth_feat[2];
} hcm_features;

/* Precomputed instruction stream: the output of the high-level model's BERT, the counterpart of hcm_features for the text side.
 * Seq2Seq_HighLevel_CMA.forward runs BERT under torch.no_grad() (models/seq2seq_highlevel_cma.py:192-195) on ids that are fixed for an episode
 * (:189-190), so its last hidden state is a function of the episode's instruction alone: a rollout can compute it once per episode, a validation
 * epoch once per trajectory (the trainer's collate repeats one instruction over the T steps of a chunk), a trainer once per episode
 * (robo-vln_amd/train.py reads it as observations["instruction_features"]).
 * Every HCM entry point that takes `ids, ids_dtype` and runs the high-level model -- hcm_high_forward, hcm_high_forward_seq, hcm_act, hcm_act_ex,
 * hcm_act_gather, hcm_val_step -- accepts ids_dtype == HCM_INSTR_FEATURES: `ids` is then a HOST pointer to this struct, consumed during the call.
 *   stream    DEVICE pointer, f32 (rows, L, bert_hidden) contiguous: BERT's last hidden state, as hcm_encode_instruction writes it
 *   rows      divides the call's row count (B; T*N for the sequence / validation calls): row r of the call reads stream row r % rows.  rows = B: one
 *             stream per row; 1: one instruction for every row (:189-190); N in a time-major T*N call: row t*N + n takes environment n's stream
 *   reserved  must be 0
 * L and `lengths` stay arguments of the call.  The call runs one conversion launch in place of BERT, on the stream that would have carried the
 * BERT chain, into the buffer BERT fills (the `hi.bert` tap shows it); the instruction side of Visual_Ling_Attn and everything behind it run
 * unchanged.  With `lengths`, the positions behind a row's length are filled with zeros and the stream is not read there: whatever a cache holds
 * behind a length (NaN included) cannot reach the result.  A length below 1 zero-fills the whole row.
 * Bits: a call fed hcm_encode_instruction's output returns the bits of the same call fed the ids, in every precision mode -- the stream holds the
 * values of BERT's storage type (fp16 / bf16 / f32 per mode), which f32 carries exactly.  ONE condition: BERT's GEMM launches are chosen by the
 * row count (tile form and staging depend on rows * L, csrc/igemm.hip; the folded-LayerNorm form of big engines is the exception, it is fixed per
 * engine), and two launch forms agree to round-off only.  The promise therefore holds for a stream ENCODED AT THE CALL'S OWN ROW COUNT AND L
 * (encode B rows for a B-row call, T*N for a sequence call; its first row / first N rows are then the rows = 1 / rows = N forms); a stream
 * encoded at another row count is BERT's output just as well, and reproduces the call to the precision mode's round-off.
 * A stream computed elsewhere (the reference's own BERT) is rounded once to BERT's storage type on the way in.
 * Refused with a message, never a GPU fault.  HCM_ERR_UNSUPPORTED: a CMANet / Seq2SeqNet handle (their instruction encoders are recurrent, not
 * BERT), a handle without a high-level model, an ablated instruction.  HCM_ERR_ARG: rows < 1 or not a divisor of the call's rows, reserved != 0,
 * a NULL stream, HCM_ACT_REUSE_INSTRUCTION beside it (the flag's cache and a handed-over stream contradict each other), hcm_refresh_instruction,
 * hcm_calibrate (calibration measures BERT's ranges and needs it to run).  The handle stays usable after a refusal.
 * A captured hcm_act graph is keyed by `stream` and `rows` like by every other argument. */
typedef struct hcm_instr_features { const float* stream; int32_t rows; int32_t reserved; } hcm_instr_features;

/* Replaces model construction, hierarchical_trainer.py:315-328 (Seq2Seq_HighLevel_CMA.__init__
 * models/seq2seq_highlevel_cma.py:33-141, Seq2Seq_LowLevel.__init__ models/seq2seq_lowlevel.py:32-98).
 * Rejects the flags whose branches crash in the reference. */
int hcm_create(const hcm_config* cfg, hcm_handle* out);

/* Replaces `load_state_dict(ckpt["high_level_state_dict"])` / `["low_level_state_dict"]`
 * (hierarchical_trainer.py:343-345): call once per state_dict entry with the reference's own key.
 * `data` is a HOST pointer to a contiguous tensor of `dtype` (HCM_F32 or HCM_I64); it is copied.
 * Unknown keys fail with HCM_ERR_KEY, wrong shapes with HCM_ERR_SHAPE (strict=True semantics). */
int hcm_load_tensor(hcm_handle h, int model, const char* key, const void* data, int dtype,
                    const int64_t* shape, int ndim);

/* After the last hcm_load_tensor: checks that every required key arrived, folds eval-mode BatchNorm into
 * the convolutions, re-lays weights out for NHWC implicit GEMM, converts to the compute precision,
 * uploads, and allocates the per-handle workspace for max_batch.  (The reference does the equivalent
 * implicitly in `.to(device)` + `.eval()`, hierarchical_trainer.py:339-340,:1080-1081.) */
int hcm_finalize(hcm_handle h);

/* Replaces `logits, hidden' = high_level((observations, hidden, prev_actions, masks))`
 * (hierarchical_trainer.py:1096-1097 -> models/seq2seq_highlevel_cma.py:170-233).
 *   rgb    (B,H,W,3)  rgb_dtype HCM_F32 (values 0..255, the batch_obs contract common/utils.py:78-83) or HCM_U8
 *   depth  (B,H,W,1)  f32
 *   ids    (B,L)      ids_dtype HCM_I32 / HCM_I64 / HCM_F32 (the reference carries ids as f32 and casts .long());
 *                     L is per call, 1 <= L <= cfg.instr_len: BERT runs without an attention mask and the poolers average over
 *                     all L positions (:209-210), so a padded instruction gives a different result than the unpadded one --
 *                     pass the ids exactly as the reference caller does
 *   lengths (B,) int32 device pointer or NULL.  NULL = the reference call: every row has L tokens.  The reference evaluates ONE
 *                     environment per call with its unpadded instruction; a batched rollout whose environments carry
 *                     instructions of different lengths pads the rows to a common L and passes each row's token count here:
 *                     environment b then attends over / pools over its first lengths[b] positions only and gets, bit for bit,
 *                     the result of its own unpadded (1, lengths[b]) call.  Values are clamped to [1, L].
 *   h_in   (R,B,hidden) f32, R = hcm_query(HCM_NUM_RECURRENT_LAYERS)
 *   mask   (B,) f32   -- column 0 of the reference's masks (masks[:,0], :208); 0 at episode start
 *   logits (B,num_actions) f32 out;  h_out (R,B,hidden) f32 out (may alias h_in)
 * prev_actions is ignored on the working path of the reference and is not part of this ABI. */
int hcm_high_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth,
                     const void* ids, int ids_dtype, const int32_t* lengths, int B, int L,
                     const float* h_in, const float* mask,
                     float* logits, float* h_out, void* stream);

/* Replaces `vel, stop, hidden' = low_level((observations, hidden, prev_actions, masks, subtask))`
 * (hierarchical_trainer.py:1099-1100 -> models/seq2seq_lowlevel.py:116-162).
 *   subtask (B,) int64 in [0, num_sub_tasks];  vel (B,2) f32;  stop (B,1) f32 (logit). */
int hcm_low_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int B,
                    const float* h_in, const float* mask, const int64_t* subtask,
                    float* vel, float* stop, float* h_out, void* stream);

/* Training / validation path: the models are called on T*N frames at once
 * (hierarchical_trainer.py:505-506,:539 and :575-576,:613) and RNNStateEncoder.forward takes the seq_forward branch
 * (models/decoder/state_encoder.py:83-133): encoders on all T*N frames, then a T-step masked recurrent scan.
 *   rgb/depth/ids/subtask: T*N rows, time-major (row t*N + n);  masks (T*N,) f32;  h_in/h_out (R,N,hidden);
 *   logits (T*N,num_actions) / vel (T*N,2) / stop (T*N,1).  T*N must not exceed max_batch.  Inference only (no autograd). */
int hcm_high_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
                         const int32_t* lengths /* (T*N,) or NULL */, int T, int N, int L, const float* h_in, const float* masks, float* logits, float* h_out, void* stream);
int hcm_low_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int T, int N,
                        const float* h_in, const float* masks, const int64_t* subtask,
                        float* vel, float* stop, float* h_out, void* stream);

/* The teacher-forced validation step, HierarchicalTrainer._update_agent_val (hierarchical_trainer.py:562-631, driven by val_epoch :747-831): both
 * models on the same T*N frames and the three criteria + the sub-task accuracy counts, in one call.  HCM handles that hold both models only
 * (a CMANet / Seq2SeqNet handle: HCM_ERR_STATE).  Rows, lengths, masks, hidden states and the T*N <= max_batch rule are those of
 * hcm_high_forward_seq / hcm_low_forward_seq.
 *   oracle_subtask    (T*N,)   int64  observations['vln_oracle_action_sensor'] (:578-580): 0 = padded row, k = sub-task k - 1
 *   corrected_actions (T*N,2)  f32    (:615-620)
 *   oracle_stop       (T*N,1)  f32    -1 = padded row (:623)
 * The high-level model gives logits (T*N, num_actions) (:575-576); the low-level model is TEACHER-FORCED with sub-task oracle_subtask - 1, and
 * num_sub_tasks (the embedding's extra row) where oracle_subtask == 0 (:597-599, :613), and gives vel (T*N,2), stop (T*N,1).  The two models have
 * no data dependence: five encoder chains are in flight together (the high-level RGB trunk on the caller's stream; the low-level RGB trunk, BERT, and
 * the two depth trunks one behind the other, on three side streams of the handle), then the low-level tail (sub-task embedding, masked T-step scan, heads) runs on a side
 * stream beside the cross-modal block and the high-level scan, and one criterion launch on the caller's stream follows the join.  Each model's trunks run with the launches of its own
 * sequence call (no shared or hi|lo-paired trunks: those agree with the single-model calls to round-off only) and no instruction stream is cached.
 *   result (8,) f32 device out:
 *     [0] high-level loss: CrossEntropyLoss(ignore_index=-1, reduction="mean") against oracle_subtask - 1 (:567, :581) = the mean over the rows
 *         with oracle_subtask != 0 of logsumexp(logits[r]) - logits[r, target]  (the masked_fill_ of the padded rows, :579, cannot reach the value)
 *     [1] low-level action loss: vel set to 0 wherever corrected_actions == 0, element by element, then MSELoss(): the mean over ALL 2*T*N
 *         elements (:617-621)
 *     [2] stop loss: BCEWithLogitsLoss() over the rows with oracle_stop != -1 (:623-626), as max(x,0) - x*y + log1p(exp(-|x|))
 *     [3] correct: rows with oracle_subtask != 0 whose argmax(logits[r]) (first maximal index; a NaN counts as the maximum, as in torch.argmax)
 *         is the target (:583-587);  [4] total (:588)
 *     [5] rows that entered the stop loss
 *     [6] rows whose oracle_subtask lies outside [0, num_sub_tasks]: such a row counts as padded for [0], [3], [4] and the low-level model gets
 *         the padded sub-task for it, so the call never reads outside the embedding; a caller should treat a non-zero count as an error
 *     [7] 0
 *   With no valid row the call gives what torch gives: 0/0 = NaN in [0] (respectively [2]) and counts of 0.  That NaN is a result, not a fault:
 *   it does not touch the overflow guard (HCM_STEP_NONFINITE).  NaN / inf in a valid row's model outputs propagate into the loss as in torch.
 *   hi_h_out / lo_h_out (R,N,hidden) out (may alias the inputs)
 *   logits / vel / stop: optional outputs (NULL = not wanted): the models' outputs BEFORE any masking, bit-identical -- as are both hidden
 *   states -- to what hcm_high_forward_seq and hcm_low_forward_seq (given the remapped sub-task) write for the same inputs.
 * All f32 arithmetic of the criteria is done in a fixed order by one workgroup: two calls on the same inputs give the same eight words.
 * No host synchronisation, no allocation, nothing read back: the call may be enqueued inside a stream capture (after one eager call at the
 * same shape, which performs the one-time kernel attribute setup).  The call itself is never replayed from a graph of the library's own. */
int hcm_val_step(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth,
                 const void* ids, int ids_dtype, const int32_t* lengths, int T, int N, int L,
                 const int64_t* oracle_subtask, const float* corrected_actions, const float* oracle_stop,
                 const float* hi_h_in, const float* lo_h_in, const float* masks,
                 float* result, float* hi_h_out, float* lo_h_out,
                 float* logits, float* vel, float* stop, void* stream);

/* The caller-side step of the eval loop, hierarchical_trainer.py:1095-1101: high -> argmax(dim=1) -> low.
 *   record (B,7) f32 out: [4 sub-task logits, lin_vel, ang_vel, stop logit].
 * When called repeatedly with the same pointers on a non-default stream, the step (all forked encoder streams
 * included) is captured into a hipGraph on the second call and replayed afterwards (HCM_GRAPH=0 disables). */
int hcm_act(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth,
            const void* ids, int ids_dtype, const int32_t* lengths, int B, int L,
            const float* hi_h_in, const float* lo_h_in, const float* mask,
            float* record, float* hi_h_out, float* lo_h_out, void* stream);

/* hcm_act with flags.  HCM_ACT_REUSE_INSTRUCTION: the instruction ids of every environment are the same as in the previous
 * hcm_act / hcm_act_ex call on this handle (same B and L): BERT and the instruction stream of Visual_Ling_Attn are not recomputed,
 * the tensors of the previous step are reused (the reference recomputes them every step although an instruction is fixed
 * for an episode, seq2seq_highlevel_cma.py:189-195).  NOT the measured configuration: bench.py and the parity tests run with
 * flags = 0; with the flag the step executes 13.8 GFLOP per environment less.  Returns HCM_ERR_STATE if there is no
 * previous hcm_act / hcm_act_ex step with this batch size and L, or if any other forward entry point ran on the handle in between
 * (they re-use the workspace region that holds the cached tensors). */
/* HCM_ACT_HOST_FRAMES: `rgb` and `depth` point to HOST memory (page-locked: hipHostMalloc / a pinned torch tensor; what a simulator process
 * hands over) instead of device memory.  The library copies each frame tensor host -> device at the head of the encoder chain that reads
 * it (the RGB frames on the RGB trunks' stream, the depth frames on the depth trunks' stream), so the copies run beside BERT and beside
 * each other's compute instead of in front of the whole step, and they are nodes of the captured hipGraph.  `ids`, the hidden states, the mask
 * and the outputs stay device pointers.  Results are bit-identical to copying the frames first and calling without the flag.  Measured at
 * B = 64 (29 MB of uint8 RGB + f32 depth per step, two boxes): 5.20-5.26 ms against 5.28-5.30 ms with the frames copied in front of the step
 * and 4.64 ms with resident frames -- on this runtime a graph's memcpy nodes overlap its kernels only marginally (eager launches with the
 * copy engine beside them reached 4.95-5.27 ms depending on the host). */
/* HCM_ACT_CHAIN_GRAPHS (round 4): replay the step as four LINEAR hipGraphs (BERT, depth trunks, RGB trunks, tail), one per chain on the chain's own
 * stream, stitched by events, instead of ONE graph captured across the forked streams.  hipGraphLaunch enqueues a forked graph node by node at ~2.1 us per
 * node (0.5-0.8 ms of host time for the step's ~240 nodes, in capture order: at B = 1 the last chain starts 0.3 ms late), a single-stream graph at ~0.1 us per
 * node.  With the flag the host cost of a step is ~0.18 ms and the synchronous latency of a B = 1 step drops by 7-25 % (box-dependent); the GPU runs the
 * linear graphs' nodes slightly slower than the forked graph's, so PIPELINED throughput is 2-4 % lower -- a latency option for single-environment loops
 * (hierarchical_trainer.py:1088-1107 calls the policy once per simulator step), not the measured configuration.  Results are bit-identical.  The side streams
 * are picked by a one-time timing probe so that the chains' streams do not share a hardware queue.  Together with HCM_ACT_HOST_FRAMES the replay enqueues the
 * two frame copies itself, outside the graphs, at the head of their chains' streams: they then run beside BERT (B = 64, PCIe-inclusive: 4.87 -> 4.40 ms per step;
 * a gain from ~4 MB per frame tensor up -- smaller pinned copies are carried out by the calling thread behind the stream's earlier work). */
enum hcm_act_flags { HCM_ACT_REUSE_INSTRUCTION = 1, HCM_ACT_HOST_FRAMES = 2, HCM_ACT_CHAIN_GRAPHS = 4 };
int hcm_act_ex(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
               const int32_t* lengths, int B, int L,
               const float* hi_h_in, const float* lo_h_in, const float* mask, float* record, float* hi_h_out, float* lo_h_out,
               int flags, void* stream);

/* Companion of HCM_ACT_REUSE_INSTRUCTION for batched rollouts in which a few environments start a new episode: recomputes
 * the cached instruction stream of the n listed environments (HOST array of indices into the batch) from ids (B,L) (device),
 * leaving the other environments' cached tensors untouched.  Needs a previous hcm_act / hcm_act_ex step at this batch size. */
int hcm_refresh_instruction(hcm_handle h, const void* ids, int ids_dtype, const int32_t* lengths, int B, int L,
                            const int32_t* env_indices, int n, void* stream);

/* ---- multi-GPU: environment-sharded replicas, ONE collective per step (no reference counterpart: the reference evaluates one
 * environment in one process, hierarchical_trainer.py:1088-1107).  One process per GPU, every rank a full weight replica stepping its own
 * B_local environments; the (B_local, 7) action records are all-gathered over RCCL / xGMI into the (world * B_local, 7) record of the whole batch,
 * rank-major = environment order.  The collective is enqueued by the library on the step's stream right behind the (hipGraph-replayed) step:
 * no Python call per step, no host synchronisation.  RCCL is resolved with dlopen when first asked for.
 *   hcm_comm_unique_id   rank 0: 128 bytes (ncclUniqueId) to hand to every rank through any side channel (torch.distributed broadcast, a file, MPI)
 *   hcm_comm_init        every rank, collectively: creates the handle's communicator (blocks until all `world` ranks have called)
 *   hcm_act_gather       hcm_act_ex + ncclAllGather(record -> gathered) on `stream`; B must be the same on every rank.  A rank whose own step
 *                        fails (bad argument, workspace, launch error) STILL takes part in the collective, with an all-NaN record, and returns
 *                        its error afterwards -- the private communicator has no watchdog, so a rank that simply returned would leave the
 *                        others blocked in ncclAllGather; they see NaN rows for that rank's environments instead
 *                        (an argument error that every rank shares -- B outside [1, max_batch], null buffers -- returns HCM_ERR_ARG
 *                        WITHOUT entering the collective: the element count must agree across ranks)
 *   hcm_gather_poison    this rank cannot even start its step (its caller failed in front of the library: a broken observation, an exception
 *                        in the host code) -- join THIS step's all-gather with an all-NaN (B, 7) block so that the peers, which are already
 *                        inside it, see NaN rows for this rank's environments and leave at the same step
 *   hcm_comm_abort       ncclCommAbort of the handle's communicator (a rank that is going to stop stepping: an exception outside the library,
 *                        shutdown after a peer's NaN record); the handle can create a new one with hcm_comm_init afterwards */
int hcm_comm_unique_id(void* out128);
int hcm_comm_init(hcm_handle h, const void* unique_id128, int rank, int world);
int hcm_comm_abort(hcm_handle h);
int hcm_gather_poison(hcm_handle h, int B, float* record, float* gathered, void* stream);
int hcm_act_gather(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, const int32_t* lengths,
                   int B, int L, const float* hi_h_in, const float* lo_h_in, const float* mask, float* record, float* hi_h_out, float* lo_h_out,
                   int flags, float* gathered, void* stream);

/* The trunks alone: runs, for any handle kind, each ResNet trunk and its pool on `rows` frames (rgb / rgb_dtype / depth as for the forward calls,
 * rows <= max_batch) and writes the hcm_features layouts above into the four pointers of `out` (device, f32; NULL = that feature is not wanted and its
 * trunk is not run; a frame may be NULL when no wanted trunk reads it).  Independent trunks run concurrently on the handle's side streams, as in
 * the step; two models whose trunk is one (HCM_FEAT_SHARED) get it run once.  Fed back through HCM_FEATURES the features reproduce the stored
 * bits of the frame call exactly, in every precision mode: the fold is a power of two and f32 holds every fp16 / bf16 value.
 * flags = 0: each model's trunk runs with the launches of its own forward / sequence call -- the bits of hcm_high_forward, hcm_low_forward, the
 * sequence calls, hcm_val_step and the flat handles' calls.  HCM_ENCODE_ACT: the launches of hcm_act, which runs two models' unequal trunks as
 * one channel-paired network (equal to the own-model launches to round-off only); the same as 0 where the handle shares or has one model.
 * No synchronisation, no allocation.  HCM_ERR_UNSUPPORTED: a wanted feature of a SimpleCNN encoder or an ablated modality. */
enum hcm_encode_flags { HCM_ENCODE_ACT = 1 };
int hcm_encode_features(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int rows, const hcm_features* out, void* stream);
int hcm_encode_features_ex(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int rows, const hcm_features* out, int flags, void* stream);

/* BERT alone: runs the high-level model's BERT (seq2seq_highlevel_cma.py:192-195) on `rows` <= max_batch instructions -- ids (rows, L) of
 * ids_dtype HCM_I32 / HCM_I64 / HCM_F32 and lengths (rows,) or NULL, as for hcm_high_forward -- and writes its last hidden state as f32
 * (rows, L, bert_hidden) to `out` (device), zeros behind each row's length: the tensor hcm_instr_features.stream takes.  The launches are those
 * of hcm_high_forward at the same (rows, L), the values those of BERT's storage type; in the "bf16" mode that is the bf16 operand the
 * instruction side of Visual_Ling_Attn reads, not the internal f32 residual stream.  See hcm_instr_features on row counts and bits.
 * On the caller's stream; no synchronisation, no allocation.  Uses the workspace like every other forward entry point: an
 * HCM_ACT_REUSE_INSTRUCTION cache is invalidated.  HCM_ERR_UNSUPPORTED: a CMANet / Seq2SeqNet handle, no high-level model;
 * HCM_ERR_ARG: rows outside [1, max_batch], L outside [1, instr_len], NULL ids or out, ids_dtype HCM_INSTR_FEATURES. */
int hcm_encode_instruction(hcm_handle h, const void* ids, int ids_dtype, const int32_t* lengths, int rows, int L, float* out, void* stream);

/* fp16 range safety (no reference counterpart: the reference is fp32).  Sub-networks that store fp16 (all four in HCM_F16 mode, the depth
 * trunks in HCM_BF16 mode) have a range that ends at 65504.  hcm_finalize runs one forward on a synthetic batch with range hooks on every GEMM
 * output of those sub-networks; hcm_calibrate does the same on the caller's own observations (device pointers as for hcm_act; zero recurrent
 * state; synchronises the stream).  When max |x| exceeds 2^14 or a non-finite value appears (needs the host copies of the weights:
 * hcm_config.reserved[4], else HCM_ERR_STATE):
 *   - GroupNorm depth trunks: the un-normalised output of a conv is the only tensor that can grow without bound, and GroupNorm is invariant to
 *     its scale: a power of two is folded into that conv's weights and the GroupNorm's eps is scaled to match -- exact, the trunk stays on
 *     fp16 (hcm_query(HCM_RANGE_FOLD) bit 1);
 *   - BatchNorm-folded RGB trunks: conv + bias + ReLU, pools and the residual additions are positively homogeneous, so ONE power of two is
 *     carried by every activation of the trunk (stem weights and all folded biases scaled by it) and divided out in the weights of the
 *     projections that consume the trunk features -- exact up to fp16's sub-normal floor, the trunk stays on fp16 (HCM_RANGE_FOLD bit 2);
 *   - BERT and the cross-modal block (GELU / softmax are not homogeneous), or a trunk whose overflow the fold cannot reach: re-built on bf16
 *     tiles, reported by hcm_query(HCM_FP16_FALLBACK).
 * The forward is repeated on the re-built engine, so that what sat downstream of the overflow is judged on clean inputs and the reported
 * ranges are those of the engine as it runs.  At run time NaN / inf are never washed out (ReLU, max-pool and the variance clamps propagate them
 * as torch's do) and the recurrent cells count what reaches them: hcm_query(HCM_STEP_NONFINITE). */
int hcm_calibrate(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int L, void* stream);
int hcm_release_host_weights(hcm_handle h);

int hcm_query(hcm_handle h, int what, int64_t* out);

/* The run-time overflow guard without a synchronisation (hcm_query(HCM_STEP_NONFINITE) waits for the device): enqueues a copy of the
 * guard word to a pinned host word behind `stream` and returns in *out the value of the last copy that has COMPLETED -- i.e. the
 * count as of an earlier poll.  Cheap enough to call every few steps from a rollout loop; a non-zero value means that some
 * environment's recurrent cell saw non-finite gate pre-activations (a broken frame, or a sub-network outside its fp16 range:
 * hcm_calibrate on real observations) and that its actions since then are not to be trusted. */
int hcm_guard_poll(hcm_handle h, void* stream, int64_t* out);

/* Message of the last failing call on this handle (or on creation when h is NULL). */
const char* hcm_last_error(hcm_handle h);

void hcm_destroy(hcm_handle h);

/* ---- CMANet flat baseline ----
 * `CMANet` (models/cma.py:19-333; constructed at robo_vln_trainer.py:326-331 with num_actions = 2) behind the same
 * handle type: hcm_cma_create -> hcm_load_tensor(h, HCM_CMA, key, ...) for every entry of the module's state_dict
 * (strict) -> hcm_finalize -> hcm_cma_forward ...; hcm_query / hcm_last_error / hcm_destroy work as for the HCM handles. */
typedef struct hcm_cma_config {
    int32_t struct_size;
    int32_t precision;            /* HCM_F16 / HCM_BF16 (16-bit trunks as in hcm_config.precision; fp32 text / recurrent / attention side) or HCM_F32 */
    int32_t max_batch;
    int32_t rgb_h, rgb_w, depth_h, depth_w;
    int32_t instr_len;            /* MAXIMUM padded token count per instruction (<= 256); every forward passes its own L <= instr_len */
    int32_t vocab_size, embedding_size, instr_hidden, bidirectional;   /* MODEL.INSTRUCTION_ENCODER.* (default.py:97-115) */
    int32_t rgb_out, depth_out, depth_baseplanes;
    int32_t hidden, rnn_type;     /* MODEL.STATE_ENCODER.* for both state encoders */
    int32_t num_actions;          /* 2 */
    int32_t use_prev_action;      /* must be 0 (MODEL.CMA.use_prev_action default) */
    int32_t rcm_state_encoder;    /* must be 0 (MODEL.CMA.rcm_state_encoder default) */
    int32_t progress_monitor;     /* must be 0: the auxiliary loss is a training-only branch (cma.py:320-329) */
    /* round 6 (carved out of the reserved words: zero = the defaults, struct size unchanged) */
    int32_t instr_rnn;            /* MODEL.INSTRUCTION_ENCODER.rnn_type: HCM_LSTM (0, default.py:111) or HCM_GRU (instruction_encoder.py:42) */
    int32_t ablate_instruction;   /* cma.py:236-241: `embedding * 0` behind the encoder -- the encoder is then not run, everything downstream sees the zeros */
    int32_t ablate_depth;         /*   (text attention over an all-zero instruction: every position masked, uniform weights, text = 0 exactly) */
    int32_t ablate_rgb;
    int32_t reserved[4];
} hcm_cma_config;

int hcm_cma_create(const hcm_cma_config* cfg, hcm_handle* out);

/* Replaces `output, stop_out, rnn_hidden_states = actor_critic((observations, rnn_hidden_states, prev_actions, masks))`
 * (robo_vln_trainer.py:1096 -> models/cma.py:211-333).
 *   rgb (B,H,W,3) HCM_F32 / HCM_U8; depth (B,H,W,1) f32; ids (B,L) HCM_I32 / HCM_I64 / HCM_F32, 0 = padding
 *   h_in (R,B,hidden) f32 with R = hcm_query(HCM_NUM_RECURRENT_LAYERS) = both state encoders (4 for LSTM, 2 for GRU)
 *   mask (B,) f32 (column 0 of the reference's masks, cma.py:219)
 *   out (B,num_actions), stop (B,1), h_out (R,B,hidden): f32 outputs.  The reference writes the new hidden state into
 *   the tensor it was given and returns it; here h_out may alias h_in to get the same effect. */
int hcm_cma_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int L,
                    const float* h_in, const float* mask, float* out, float* stop, float* h_out, void* stream);
/* Training / validation path of the flat trainer: `self.actor_critic(batch)` on a whole truncated-BPTT chunk (robo_vln_trainer.py:516-518 and
 * :553-555) -- T*N rows at once, time-major (row t*N + n), with an (R,N,hidden) state, so that RNNStateEncoder.forward takes seq_forward
 * (state_encoder.py:83-133) for BOTH state encoders (cma.py:262-270, :313-318).
 *   rgb (T*N,H,W,3), depth (T*N,H,W,1), ids (T*N,L) with 0 = padding (the trainer's collate repeats an episode's padded instruction at every step);
 *   masks (T*N,); h_in / h_out (R,N,hidden), first half state_encoder, second half second_state_encoder, h_out may alias h_in;
 *   out (T*N,num_actions), stop (T*N,1).
 * Order: the three encoder chains and the token-side projections on all T*N rows; the masked T-step scan of the first encoder; both attention
 * stages and second_state_compress on all rows; the scan of the second encoder; linear / stop_linear over all rows in one launch.  A scan is one
 * input-projection GEMM over all rows plus ONE launch per time step (csrc/state_scan.hip) for hidden = 512 and, for other sizes, the
 * per-step launches of the single-step call.  T = 1 is hcm_cma_forward (same bits).  No synchronisation, no allocation: capturable by the caller.
 * HCM_ERR_ARG: T < 1, N < 1, T*N > max_batch, L outside [1, instr_len], a null pointer; HCM_ERR_STATE: not a CMANet handle. */
int hcm_cma_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int T, int N, int L,
                        const float* h_in, const float* masks, float* out, float* stop, float* h_out, void* stream);

/* ---- Seq2SeqNet flat baseline (paper_configs/seq2seq_robo.yaml, seq2seq_robo_pm.yaml) ----
 * `Seq2SeqNet` (models/seq2seq.py:21-189; constructed at robo_vln_trainer.py:333-339 whenever MODEL.CMA.use is false) behind the same
 * handle type: hcm_s2s_create -> hcm_load_tensor(h, HCM_S2S, key, ...) for every entry of the module's state_dict (strict; `sub_goal_linear.*`
 * and `progress_monitor.*` are always part of it, seq2seq.py:104-109, and `sub_goal_linear` is never read by forward) -> hcm_finalize ->
 * hcm_s2s_forward ...; hcm_query / hcm_last_error / hcm_destroy and the tap hooks work as for the other handles (taps: `s2s.instruction`,
 * `s2s.depth_flat`, `s2s.rgb_flat`, `s2s.rnn_in`).  hcm_query(HCM_NUM_RECURRENT_LAYERS) = 2 for LSTM, 1 for GRU (seq2seq.py:132-134). */
typedef struct hcm_s2s_config {
    int32_t struct_size;
    int32_t precision;            /* as hcm_cma_config: 16-bit trunks behind the range calibration, fp32 text / recurrent side */
    int32_t max_batch;
    int32_t rgb_h, rgb_w, depth_h, depth_w;   /* frame sizes: the limits of hcm_config for the chosen encoder kinds */
    int32_t instr_len;            /* MAXIMUM padded token count per instruction (<= 256); every forward passes its own L <= instr_len */
    int32_t vocab_size, embedding_size, instr_hidden;    /* MODEL.INSTRUCTION_ENCODER.* (default.py:97-115); instr_hidden: a multiple of 64, <= 512 */
    int32_t instr_rnn;            /* INSTRUCTION_ENCODER.rnn_type: HCM_LSTM or HCM_GRU (instruction_encoder.py:42) */
    int32_t bidirectional;        /* must be 0: with final_state_only the encoder returns (2,B,H) (instruction_encoder.py:90) and seq2seq.py:163 raises */
    int32_t rgb_encoder, depth_encoder;       /* hcm_encoder: TorchVisionResNet50 / VlnResnetDepthEncoder in flat mode, or SimpleRGBCNN / SimpleDepthCNN (seq2seq.py:50-82) */
    int32_t rgb_out, depth_out, depth_baseplanes;
    int32_t hidden, rnn_type;     /* MODEL.STATE_ENCODER.* */
    int32_t num_actions;          /* 2 */
    int32_t num_sub_tasks;        /* rows of sub_goal_linear (seq2seq.py:108): part of the state_dict only */
    int32_t use_prev_action;      /* must be 0: SEQ2SEQ.use_prev_action (default.py:202 default False; seq2seq.py:167-171 raises at the cat) */
    int32_t is_bert;              /* must be 0: INSTRUCTION_ENCODER.is_bert selects LanguageEncoder (seq2seq.py:45-46), not built */
    int32_t progress_monitor;     /* PROGRESS_MONITOR.use (seq2seq_robo_pm.yaml): tanh(progress_monitor(x)) (seq2seq.py:177) becomes an extra OUTPUT */
    int32_t ablate_instruction;   /* seq2seq.py:156-161: `embedding * 0` behind an encoder -- the encoder is then not run, zeros go in */
    int32_t ablate_depth;
    int32_t ablate_rgb;
    int32_t reserved[6];
} hcm_s2s_config;

int hcm_s2s_create(const hcm_s2s_config* cfg, hcm_handle* out);

/* Replaces `output, stop_out, rnn_hidden_states = actor_critic((observations, rnn_hidden_states, prev_actions, masks))`
 * (robo_vln_trainer.py:1096 -> models/seq2seq.py:140-189).
 *   rgb (B,H,W,3) HCM_F32 / HCM_U8; depth (B,H,W,1) f32
 *   ids (B_instr,L) HCM_I32 / HCM_I64 / HCM_F32, 0 = padding; B_instr = B, or 1: ONE instruction for all B frames (the `.expand` of
 *       seq2seq.py:163) -- the encoder then runs for one sample.  The instruction vector is the encoder's hidden state at each sample's own
 *       last non-padding token (final_state_only, instruction_encoder.py:86-90).  A row that is all padding makes the reference raise
 *       (pack_padded_sequence); here it yields the zero vector, as such a row does on the CMANet path.
 *   h_in (R,B,hidden) f32, R = 2 (LSTM) / 1 (GRU);  mask (B,) f32 (column 0 of the reference's masks, seq2seq.py:172)
 *   out (B,num_actions), stop (B,1), h_out (R,B,hidden): f32 outputs; h_out may alias h_in
 *   progress (B,1) f32 out = tanh(progress_monitor(x)) when the config's progress_monitor is set; must be NULL when it is clear.  (The
 *       reference computes the value only while AuxLosses is active and keeps it inside the loss, seq2seq.py:176-185; the loss itself needs
 *       observations["progress"] and stays with the caller.)
 * Repeated calls with the same pointers on a non-default stream are captured into a hipGraph and replayed, as for the other handle kinds. */
int hcm_s2s_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int B_instr, int L,
                    const float* h_in, const float* mask, float* out, float* stop, float* progress, float* h_out, void* stream);
/* Training / validation path: T*N rows at once, time-major, then the masked T-step scan (RNNStateEncoder.seq_forward, state_encoder.py:83-133),
 * as hcm_low_forward_seq.  ids (B_instr,L) with B_instr = T*N or 1; masks (T*N,); h_in / h_out (R,N,hidden); out (T*N,num_actions), stop (T*N,1),
 * progress (T*N,1) or NULL.  T*N must not exceed max_batch. */
int hcm_s2s_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int T, int N, int B_instr,
                        int L, const float* h_in, const float* masks, float* out, float* stop, float* progress, float* h_out, void* stream);

/* The flat trainer's validation step, RoboVLNTrainer._update_agent_val (robo_vln_trainer.py:544-575, driven by val_epoch :726-813): the model on the
 * chunk's T*N time-major frames and the three criteria, in one call.  CMANet and Seq2SeqNet handles only (an HCM handle: HCM_ERR_STATE; the
 * hierarchical pair has hcm_val_step).  Rows, masks, h_in / h_out (R,N,hidden) with R = hcm_query(HCM_NUM_RECURRENT_LAYERS), aliasing, L and the
 * T*N <= max_batch rule are those of the handle kind's own sequence call, hcm_cma_forward_seq / hcm_s2s_forward_seq; T = 1 is legal.
 *   ids               (B_instr,L)  CMANet: B_instr must be T*N; Seq2SeqNet: T*N, or 1 = one instruction for every frame (seq2seq.py:163)
 *   corrected_actions (T*N,num_actions) f32  (:557-561)
 *   oracle_stop       (T*N,1)      f32    -1 = padded row (:563)
 *   progress          (T*N,)       f32    observations["progress"]: required on a Seq2SeqNet handle created with progress_monitor = 1 (the loss of
 *                                  seq2seq.py:176-185), and NULL -- as progress_hat -- on every other handle (HCM_ERR_ARG otherwise)
 * The forward is `output, stop_out, h' = actor_critic((obs, h, prev_actions, masks))` (:553-555) with the launches of the sequence call.
 *   result (8,) f32 device out:
 *     [0] action loss: output set to 0 wherever corrected_actions == 0, element by element, then MSELoss(): the mean over ALL num_actions*T*N
 *         elements (:557-561)
 *     [1] stop loss: BCEWithLogitsLoss() over the rows with oracle_stop != -1 (:563-566), as max(x,0) - x*y + log1p(exp(-|x|))
 *     [2] aux loss: AuxLosses.reduce(~action_mask[:,0]) (:569-570; common/aux_losses.py:27-33) = the mean over the rows with
 *         corrected_actions[r,0] != 0 of (tanh(progress_monitor(x))[r] - progress[r])^2, weight 1.0: the model hands PROGRESS_MONITOR.alpha to
 *         register_loss in the `masks` position (seq2seq.py:181-185 against aux_losses.py:15), so the configured alpha never arrives and the
 *         default of 1.0 applies -- reproduced.  Exactly 0 when the handle has no progress monitor (nothing registered: reduce returns 0.0)
 *     [3] rows that entered the stop loss;  [4] rows that entered the aux mean (0 without the monitor);  [5..7] 0
 *   Empty selections give what torch gives: 0/0 = NaN in [1], and in [2] with the monitor on.  That NaN is a result, not a fault: it does not
 *   touch the overflow guard (HCM_STEP_NONFINITE).  NaN / inf in a selected row's model outputs propagate into the loss as in torch.
 *   out (T*N,num_actions) / stop (T*N,1) / progress_hat (T*N,1): optional outputs (NULL = not wanted): the model's outputs BEFORE any masking,
 *   bit-identical -- as is h_out -- to what the sequence call writes for the same inputs.  With the monitor on the progress head runs
 *   whether or not progress_hat is wanted (into workspace otherwise).
 * All f32 arithmetic of the criteria is done in a fixed order by one workgroup: two calls on the same inputs give the same eight words.
 * No host synchronisation, no allocation, nothing read back: the call may be enqueued inside a stream capture (after one eager call at the
 * same shape, which performs the one-time kernel attribute setup).  The call itself is never replayed from a graph of the library's own.
 * The epoch on top (zero state per batch, chunks of tbptt_steps rows, the state carried, "Val Loss Epoch" = the mean over chunks of
 * [0] + [1] + [2]) is robo-vln_amd/validate.py FlatValidator. */
int hcm_flat_val_step(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
                      int T, int N, int B_instr, int L,
                      const float* corrected_actions, const float* oracle_stop, const float* progress,
                      const float* h_in, const float* masks, float* result, float* h_out,
                      float* out, float* stop, float* progress_hat, void* stream);

/* ---- test / profiling hooks (not part of the drop-in surface) ---- */

/* Enable capture of named intermediate activations during the next forward calls. */
int hcm_debug_enable_taps(hcm_handle h, int enable);
/* Copy a captured intermediate (as f32) to host; synchronises the device.  *n_out = element count;
 * shape_out receives up to 4 dims (0-padded). */
int hcm_debug_get_tap(hcm_handle h, const char* name, float* host_out, int64_t capacity,
                      int64_t* n_out, int64_t* shape_out);
/* Development aid: cycle totals of the implicit-GEMM K-loop phases, collected only when the process runs with
 * HCM_IGEMM_PROF=1 (which selects instrumented builds of the 8-wave bf16 kernels).  out8: prologue, DMA issue,
 * fragment reads + MFMA issue, DMA wait, barrier, epilogue (cycles summed over waves), waves, K iterations. */
int hcm_debug_igemm_prof(uint64_t* out8, int reset);
/* Development aid: phase cycle totals of the profiled builds of the 256 x 256 GEMM kernels (`make DEV=1` library,
 * hcm_op_linear_impl variants 13-15): out1024 = [16 workgroups][8 waves][8 counters], see csrc/gemm256.hip. */
int hcm_debug_gemm256_prof(uint64_t* out1024, int reset);
/* Development aid (`make DEV=1` library created under HCM_MARKS=1; otherwise returns 0): wall-clock stamps (100 MHz ticks) that one-lane marker
 * kernels wrote at named points of the last step's chains -- how the three encoder chains really interleave inside a hipGraph-replayed step, which
 * a kernel trace cannot show (rocprofv3 serialises the streams).  Returns the number of marks; names = '\n'-joined, in slot order. */
int hcm_debug_marks(hcm_handle h, uint64_t* out256, char* names, int names_cap);

/* Stand-alone operator entry points used by the kernel-level parity tests (device pointers, f32 or bf16
 * per `dtype`; layouts NHWC / row-major); implemented at the end of robo-vln_amd/csrc/api.cpp. */
int hcm_op_conv2d(const void* x, const void* w_ohwi, const float* bias, const void* residual, void* y,
                  int dtype, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                  int act, void* stream);
/* conv2d (no bias) + GroupNorm(groups) (+ residual) (+ ReLU) in one launch; the output map must have Ho*Wo | 64 pixels and
 * Cout / groups must be a multiple of 8 dividing 128 (the GN-ResNet layers at 8x8 and 4x4). */
int hcm_op_conv2d_gn(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* residual, void* y,
                     int dtype, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int groups, float eps,
                     int relu, void* stream);
/* Tail of a BatchNorm-folded ResNet bottleneck in ONE launch (16-bit dtypes, C1 = 64 or 128):
 *   y = relu(conv1x1(relu(conv3x3(x, w2, stride, pad 1) + b2), w3) + b3 + identity)
 * x (B,H,W,C1), w2 [C1][3][3][C1], w3 [4*C1][C1], identity and y (B,Ho,Wo,4*C1).  Bit-identical to hcm_op_conv2d applied
 * twice (reference: torchvision Bottleneck.forward conv2/bn2/relu/conv3/bn3/+identity/relu as used by
 * resnet_encoders.py:196-225 TorchVisionResNet50). */
int hcm_op_bottleneck_tail(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                           void* y, int dtype, int B, int H, int W, int C1, int stride, void* stream);
/* hcm_op_bottleneck_tail plus the NEXT block's 1x1 reduction from the output tile, still one launch:
 *   o1 = relu(conv1x1(y, w1) + b1),  w1 [CN][4*C1], CN = 64 or 128 with C1 = 64, 128 or 256 with C1 = 128, 256 with C1 = 256; o1 (B,Ho,Wo,CN).
 * Bit-identical to hcm_op_conv2d applied three times. */
int hcm_op_bottleneck_tail_next(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                                void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int C1, int stride,
                                int CN, void* stream);
/* A ResNet stage's FIRST bottleneck (C1 = 64 mid channels, 64-channel block input xd): as hcm_op_bottleneck_tail_next with CN = 64,
 * but the identity is the block's own 1x1 down-sample conv, folded into the expansion GEMM: w3ds [256][128] = [W3 | Wds],
 * b3ds = b3 + bds;  y = relu(conv1x1(t, W3) + conv1x1_stride(xd, Wds) + b3ds),  t = relu(conv3x3_stride(x, w2) + b2). */
int hcm_op_bottleneck_tail_ds(const void* x, const void* w2, const float* b2, const void* w3ds, const float* b3ds, const void* xd,
                              void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int stride,
                              void* stream);
/* The general form of the three operators above, with the hi|lo PAIR layout of the step: `groups` independent bottlenecks whose channels lie
 * side by side in every pixel -- x (B,H,W,groups*C1), identity and y (B,Ho,Wo,groups*4*C1), o1 (B,Ho,Wo,groups*CN), xd (B,H,W,groups*64*KD);
 * weights and biases [groups][...] as for one bottleneck.  Either `identity` (KD = 0, xd = NULL) or the folded down-sample operand xd with
 * w3 = [W3 | Wds] ([4*C1][C1 + 64*KD]) and b3 = b3 + bds.  (C1, CN, KD) as built: (64, 64|128, 0), (128, 128|256, 0), (256, 256, 0), (64, 64, 1), (128, 128, 4);
 * anything else is HCM_ERR_ARG.  The KD = 0 forms are bit-identical to hcm_op_conv2d applied three times per group. */
int hcm_op_bottleneck_stage(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                            const void* xd, void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int C1,
                            int stride, int CN, int KD, int groups, void* stream);
/* conv2d (no bias) + GroupNorm(groups) (+ residual) (+ ReLU) for LARGE maps (Ho*Wo a multiple of 64 and >= 256, 16-bit dtypes): the
 * conv's epilogue emits the GroupNorm partial sums from its f32 tile image, one more launch normalises in place (the GN-ResNet
 * layers at 64x64 .. 16x16; resnet_encoders.py:37-101 / habitat resnet.py GroupNorm(ngroups)). */
int hcm_op_conv2d_gn_large(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* residual, void* y,
                           int dtype, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int groups, float eps,
                           int relu, void* stream);
/* first-layer (Cin = 1 or 3) convolution gathering straight from the raw frame x (x_dtype HCM_F32 / HCM_U8 / dtype):
 * w is [Cout][Kp] with k = (kh*KW+kw)*C + ci (rowrun = 0) or k = kh*24 + kw*3 + ci (rowrun = 1, f32 RGB frames only). */
int hcm_op_stem_conv(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W, int C,
                     int Cout, int KH, int KW, int stride, int pad, int K, int Kp, int rowrun, float scale, int act, void* stream);
/* 7x7 stride-2 pad-3 RGB stem on a 16-bit trunk through the packed-frame path: x is the raw (B,H,W,3) frame (HCM_F32 or
 * HCM_U8, H and W even), w is [Cout][224] with k = kh*32 + kw*4 + ci, scratch holds hcm_op_stem_scratch_bytes(B,H,W). */
int hcm_op_stem_conv_packed(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                            int Cout, float scale, int act, void* scratch, void* stream);
/* The same stem followed by ReLU and MaxPool2d(3, 2, 1) (torchvision resnet50 conv1/bn1/relu/maxpool), with the horizontal half of
 * the pool fused into the conv's epilogue and a vertical-only pool kernel after it: y is (B, H/4, W/4, Cout), bit-identical to
 * hcm_op_stem_conv_packed(act = ReLU) + hcm_op_maxpool3x3s2.  W/2 must be a power of two <= 128, Cout a multiple of 64; half_map holds
 * B * (H/2) * (W/4) * Cout elements of `dtype`. */
int hcm_op_stem_conv_packed_pool(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                                 int Cout, float scale, void* scratch, void* half_map, void* stream);
/* Round 6: the same three modules as ONE launch behind the frame packing (csrc/stem.hip: weights in registers, the packed frame streamed through
 * an LDS ring, both pool halves in LDS).  W == 256, H % 4 == 0, Cout % 64 == 0, 16-bit dtypes; bit-identical to hcm_op_stem_conv_packed_pool. */
int hcm_op_stem_pool_fused(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                           int Cout, float scale, void* scratch, void* stream);
/* ... plus layer1 block 0's 1x1 reduction of the pooled map in the same launch: o1 (B, H/4, W/4, Cout) = ReLU(w1 x pooled + b1) per 64-channel group
 * (w1 [Cout][64], group g = rows 64 g .. over the group's own 64 channels); bit-identical to hcm_op_conv2d (1x1, ReLU) applied to each 64-channel group. */
int hcm_op_stem_pool_fused_red(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                               int Cout, float scale, void* scratch, const void* w1, const float* b1, void* o1, void* stream);
int64_t hcm_op_stem_scratch_bytes(int B, int H, int W);
/* SimpleDepthCNN's first layer, Conv2d(1, 32, 8, stride 4) (+ bias, activation) straight from a raw f32 depth frame (B,H,H,1) in one pass
 * (csrc/simplecnn.hip; H a multiple of 4, <= 1024); w is the OHWI weight [32][64] in `dtype` (16-bit), scratch holds B*H*H + 64 elements of
 * `dtype` (used by the convert + implicit-GEMM route only, HCM_NO_DEPTH_CONV0=1) (simple_cnns.py:76-84). */
int hcm_op_depth_conv8x8s4(const float* depth, const void* w, const float* bias, void* y, int dtype, int B, int H, int act, void* scratch,
                           void* stream);
/* SimpleDepthCNN's three convolutions (models/encoders/simple_cnns.py:76-100; depth branch :104-125) in ONE launch (csrc/simplecnn.hip): depth (B,H,H,1)
 * f32 -> y (B,h3,h3,32), the map the Linear reads; the 63 x 63 x 32 and 30 x 30 x 64 maps of a 256-pixel frame never leave the chip.  w0 (32,64) as
 * hcm_op_depth_conv8x8s4 takes it; w1_frag / w2_frag: the 4x4/2 and 3x3/1 weights as (64,512) / (32,576) rows with k = (kh*KW + kw)*Cin + ci (the OHWI
 * layout of hcm_op_conv2d), passed through hcm_op_pack_frag.  16-bit dtypes, H % 4 == 0, H <= 256.  Bit-identical to hcm_op_depth_conv8x8s4 +
 * hcm_op_conv2d (ReLU) + hcm_op_conv2d. */
int hcm_op_simplecnn3(const float* depth, const void* w0, const float* b0, const void* w1_frag, const float* b1, const void* w2_frag, const float* b2,
                      void* y, int dtype, int B, int H, void* stream);
int hcm_op_linear(const void* x, const void* w, const float* bias, const void* residual, void* y,
                  int dtype, int M, int N, int K, int act, int out_f32, void* stream);
/* One cross-modal layer after the projections for `streams` (1 or 2) visual streams in one launch (csrc/vla_fused.hip;
 * InterModuleAttnLayer.forward, models/transformer/transformer.py:209-221): [kv != NULL: softmax(q k^T / 8) v over Lk[s] <= 32 keys, kv[s] =
 * (B, Lk[s], 512) = fc_k | fc_v; else att[s] (B, L, 256) is the attention output] -> LayerNorm(I + . Wo^T + bo) -> LayerNorm(x1 + relu(x1 W1^T + b1)
 * W2^T + b2) -> out[s] (B, L, 256); pooled[s] (optional, L <= 80): mean over each environment's first lens[b] (or L) tokens -> pooled[s][b * ld_pool + c].
 * 16-bit dtypes; kv / att / out / pooled are HOST arrays of `streams` device pointers. */
int hcm_op_vla_layer(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out, float* const* pooled,
                     int ld_pool, const void* wo, const float* bo, const void* w1, const float* b1, const void* w2, const float* b2, const float* g1,
                     const float* be1, const float* g2, const float* be2, const int32_t* lens, int dtype, int B, int L, int d_ff, int streams,
                     void* stream);
/* The same layer with its three weight matrices in MFMA-fragment order (hcm_op_pack_frag of the (256, 256), (d_ff, 256) and (256, d_ff) K-contiguous
 * weights): every wave reads its operand fragments straight from L2 into registers, no weight staging in LDS and no barrier per K tile (round 6;
 * the form the engine's own step uses).  Bit-identical to hcm_op_vla_layer. */
int hcm_op_vla_layer_frag(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out,
                          float* const* pooled, int ld_pool, const void* wo_frag, const float* bo, const void* w1_frag, const float* b1,
                          const void* w2_frag, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                          const int32_t* lens, int dtype, int B, int L, int d_ff, int streams, void* stream);
/* hcm_op_linear with the kernel family chosen by the caller: impl 0 = the library's choice, 1 = the 128-wide implicit-GEMM kernels,
 * 2 = the 256 x 256-tile 8-phase kernel (csrc/gemm256.hip; HCM_ERR_ARG when the shape does not qualify), 3 = the few-row kernel (csrc/skinny.hip:
 * a wave per 16 x 16 output tile, operands straight into registers; any row count here, the library's own choice takes it up to 160 rows where its
 * cost model says so).  All three must agree bit for bit.
 * (impl values >= 16 select timing-experiment builds of the 256-wide kernel that exist in `make DEV=1` libraries only: HCM_ERR_HIP otherwise.) */
int hcm_op_linear_impl(const void* x, const void* w, const float* bias, const void* residual, void* y,
                       int dtype, int M, int N, int K, int act, int out_f32, int impl, void* stream);
int hcm_op_attention(const void* q, const void* k, const void* v, void* out, int dtype,
                     int B, int heads, int Lq, int Lk, int ldq, int ldk, int ldv, int ldo, void* stream);
int hcm_op_layernorm(const void* x, const void* residual, const float* gamma, const float* beta,
                     void* y, int dtype, int rows, int D, float eps, void* stream);
/* BERT attention block tail in ONE launch (csrc/bert_block.hip; BertSelfAttention + BertSelfOutput of the BertModel call,
 * seq2seq_highlevel_cma.py:192-195): y = LayerNorm(softmax(Q K^T / 8) V Wo^T + bo + residual) over B samples of L <= 96 rows, 12 heads of 64;
 * qkv (B*L, 2304) = Q | K | V, lengths (B,) int32 keys per sample or NULL; wo_frag = the (768, 768) weight in MFMA-fragment order as
 * hcm_op_pack_frag writes it (N % 16 == 0, K % 32 == 0: the 16-byte chunk W[ct*16 + fr][ks*32 + fg*8 ..] at chunk index (ks*(N/16) + ct)*64 + fg*16 + fr:
 * a wave's operand fragment is 1 KB contiguous -- hcm_finalize keeps this second copy of every BERT layer's output projection).  Bit-identical to hcm_op_attention + hcm_op_linear
 * (+ residual) + hcm_op_layernorm.  residual32 / y32 non-NULL: the residual stream and the sum stay f32 (the "bf16" mode's BERT), y is the 16-bit
 * operand copy of the LayerNorm output and y32 the stream; y may alias residual, y32 may alias residual32. */
int hcm_op_pack_frag(const void* w, void* out, int dtype, int N, int K, void* stream);
int hcm_op_bert_attn_block(const void* qkv, const void* wo_frag, const float* bo, const void* residual, const float* residual32, const float* gamma,
                           const float* beta, void* y, float* y32, int dtype, int B, int L, const int32_t* lengths, float eps, void* stream);
/* LayerNorm followed by the addition of a row table: y[r] = LN(x[r] (+ residual[r])) + post[r % post_rows]  (the positional
 * encoding of Visual_Ling_Attn, transformer.py:265-269) */
int hcm_op_layernorm_post(const void* x, const void* residual, const float* gamma, const float* beta, const float* post, int post_rows,
                          void* y, int dtype, int rows, int D, float eps, void* stream);
int hcm_op_groupnorm(void* x_inplace, const void* residual, const float* gamma, const float* beta,
                     int dtype, int B, int HW, int C, int groups, float eps, int relu, void* stream);
/* conv (bias-free, statistics from its epilogue) -> MaxPool2d(3, 2, 1) over relu(GroupNorm(conv)) with the normalisation applied on load by the pool
 * (the depth stem of the GroupNorm trunk as the step runs it since round 5; replaces habitat's ResNet stem conv1 = Sequential(conv, GroupNorm, ReLU) +
 * maxpool as used at resnet_encoders.py:27-33).  y is [B][Hp][Wp][Cout]; 16-bit types, the conv's map a multiple of 64 pixels per sample. */
int hcm_op_conv2d_gn_pool(const void* x, const void* w_ohwi, const float* gamma, const float* beta, void* y, int dtype, int B, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int groups, float eps, void* stream);
/* y = relu?(GN(conv1x1(x, w)) + round(GN2(conv1x1_stride2(x2, w2)))) normalised in ONE pass over both un-normalised maps: the end of a stage-first
 * bottleneck of the GroupNorm trunk, `out = relu(bn3(conv3(.)) + downsample(x))`; x is [B][H][W][Cin], x2 [B][H*stride2][W*stride2][Cin2]. */
int hcm_op_conv2d_gn_res2(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* x2, const void* w2_ohwi, const float* gamma2,
                          const float* beta2, void* y, int dtype, int B, int H, int W, int Cin, int Cin2, int stride2, int Cout, int groups, float eps,
                          int relu, void* stream);
int hcm_op_maxpool3x3s2(const void* x, void* y, int dtype, int B, int H, int W, int C, void* stream);
/* The criterion launch of hcm_val_step on its own (csrc/elementwise.hip, val_loss_kernel): logits (rows, A), vel (rows, 2), stop (rows, 1), the three
 * label tensors as hcm_val_step takes them, result (8,) as it writes them; any rows >= 1 (one workgroup, rows strided over its 256 threads). */
int hcm_op_val_loss(const float* logits, const float* vel, const float* stop, const int64_t* oracle_subtask, const float* corrected_actions,
                    const float* oracle_stop, float* result, int rows, int A, int num_sub_tasks, void* stream);
/* The criterion launch of hcm_flat_val_step on its own (csrc/elementwise.hip, flat_val_loss_kernel): out (rows, num_actions), stop (rows, 1),
 * progress_hat (rows, 1) and progress (rows,) -- both NULL = no progress monitor, result[2] = 0 -- corrected_actions (rows, num_actions),
 * oracle_stop (rows, 1), result (8,) as hcm_flat_val_step writes them; any rows >= 1 (one workgroup, rows strided over its 256 threads). */
int hcm_op_flat_val_loss(const float* out, const float* stop, const float* progress_hat, const float* corrected_actions, const float* oracle_stop,
                         const float* progress, float* result, int rows, int num_actions, void* stream);
/* The state-encoder scan of hcm_cma_forward_seq on its own (csrc/state_scan.hip): T masked steps of nn.LSTM (rnn_type HCM_LSTM, gates i,f,g,o) or
 * nn.GRU (HCM_GRU, gates r,z,n) from the input projection of every row, one launch per step.
 *   pre (T*N, G*hidden) = x W_ih^T + bias (LSTM: b_ih + b_hh, b_hh = NULL here; GRU: b_ih, and b_hh (3*hidden,) is added inside the step)
 *   w_hh (G*hidden, hidden) as torch stores it (re-laid out for the kernel by this call); h_in / h_out (R,N,hidden), R = 2 (h, c) / 1, may alias
 *   masks (T*N,): the state is multiplied by masks[t*N + n] in front of step t; seq_out (T*N,hidden) = h_t of every row.
 * hidden must be 512 (HCM_ERR_ARG otherwise); any T, N >= 1.  Synchronises the stream (it owns temporary buffers). */
int hcm_op_state_scan(const float* pre, const float* w_hh, const float* b_hh, const float* h_in, const float* masks, float* seq_out, float* h_out,
                      int T, int N, int hidden, int rnn_type, void* stream);
/* The training form of hcm_op_state_scan: the same arguments and, bit for bit, the same seq_out / h_out, plus what the reverse scan needs.
 *   gates (T*N, 4*hidden): the post-activation gates of every row -- LSTM i,f,g,o; GRU r,z,n and hn = W_hn h' + b_hn (h' = h_{t-1} * mask), the
 *   value r multiplies inside tanh.  c_seq (T*N, hidden): c_t of every row, LSTM only (must be NULL for GRU).
 *   work: 4*hidden*hidden floats owned by the caller; w_hh (torch layout, on the device) is packed into it by a device kernel on `stream`.
 * Allocates nothing, copies nothing to the host and does not synchronise the stream: weights change after every optimizer step. */
int hcm_op_state_scan_train(const float* pre, const float* w_hh, const float* b_hh, const float* h_in, const float* masks, float* seq_out, float* h_out,
                            float* gates, float* c_seq, float* work, int T, int N, int hidden, int rnn_type, void* stream);
/* Back-propagation through time for hcm_op_state_scan_train (csrc/state_scan_bwd.hip), one launch per step from T-1 down to 0.
 *   in:  d_seq (T*N, hidden) the cotangent of every h_t; gates, c_seq (LSTM; NULL for GRU), seq_out, h_in, masks, w_hh as the forward had them
 *   out: d_pre (T*N, G*hidden) the gradient with respect to `pre`; d_gh (T*N, 3*hidden), GRU only (NULL for LSTM): the h-side gate gradients
 *        [da_r, da_z, da_n * r] (for LSTM they are d_pre); d_h_in (R, N, hidden), the carry behind step 0 -- a buffer of its own
 *   work: 4*hidden*hidden + 4*N*hidden floats owned by the caller: w_hh in the reverse scan's order (packed on `stream`) and the two ping-pong
 *        pairs of the (h, c) carry that successive launches alternate between.  No output may overlap it (HCM_ERR_ARG).
 * No gradient enters through the final state (the reference detaches it, state_encoder.py:131).  With x the input rows and
 * h' = cat(h_in[0], seq_out[:-N]) * masks: dx = d_pre W_ih, dW_ih = d_pre^T x, db_ih = sum d_pre, dW_hh = d_gh^T h', db_hh = sum d_gh -- dense
 * GEMMs left to the caller.  Allocates nothing and does not synchronise the stream; fixed summation order, bitwise reproducible. */
int hcm_op_state_scan_bwd(const float* d_seq, const float* gates, const float* c_seq, const float* seq_out, const float* h_in, const float* masks,
                          const float* w_hh, float* work, float* d_pre, float* d_gh, float* d_h_in, int T, int N, int hidden, int rnn_type,
                          void* stream);

/* The cross-modal layer (InterModuleAttnLayer, transformer.py:209-221) after its three projections, in float32 and with what a backward pass needs
 * (csrc/vla_train.hip).  d_model 256, 4 heads of 64; B, L >= 1 with L <= 4194240 and rows = B*L <= 33554431; Lk 1..64; d_ff 256, 512, 768 or 1024; anything else HCM_ERR_ARG.
 *   a = softmax(q k^T / 8) v;  x1 = LN1(I + keep1 s (a Wo^T + bo));  h = keep2 s relu(x1 W1^T + b1);  out = LN2(x1 + keep3 s (h W2^T + b2))
 *   q, I (rows, 256); kv (B, Lk, 512) = fc_k | fc_v of the keys; wo (256, 256), w1 (d_ff, 256), w2 (256, d_ff) and the biases / LayerNorm
 *   parameters as torch stores them, on the device; LayerNorm eps 1e-5.
 *   keep1 (rows, 256), keep2 (rows, d_ff), keep3 (rows, 256): uint8 keep masks of the three dropouts, s = 1 / (1 - p), 0 <= p < 1.  A NULL mask
 *   means no dropout at that place (keep everything, no scaling): all three NULL and p = 0 is the eval-mode layer.
 * Written by the forward, read by the backward (all float32, owned by the caller):
 *   a (rows, 256), x1 (rows, 256), h (rows, d_ff; post-dropout): the left operands of the three weight gradients, which the caller reduces;
 *   x1hat, x2hat (rows, 256): the two LayerNorms' normalised rows (y - mean) * rstd; rstd (rows, 2): their reciprocal standard deviations.
 *   With the normalised rows saved the means are not needed.  The attention probabilities are not saved: the backward recomputes them.
 * work: hcm_op_vla_train_work_floats(B, L, Lk, d_ff) floats (0 for unsupported sizes) owned by the caller, serving either op: the three weights
 *   in the kernels' operand order (packed on `stream` in every call: nothing is cached, weights change at every optimizer step), the backward's
 *   (rows, 256) attention-output gradient and its LayerNorm partial sums.  No output may overlap it (HCM_ERR_ARG).  Row tensors, weights and
 *   work must be 16-byte aligned, keep masks 4-byte aligned.
 * Both ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
int64_t hcm_op_vla_train_work_floats(int B, int L, int Lk, int d_ff);
int hcm_op_vla_layer_train(const float* q, const float* I, const float* kv, const float* wo, const float* bo, const float* w1, const float* b1,
                           const float* w2, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                           const uint8_t* keep1, const uint8_t* keep2, const uint8_t* keep3, float p, float* out, float* a, float* x1, float* x1hat,
                           float* h, float* x2hat, float* rstd, float* work, int B, int L, int Lk, int d_ff, void* stream);
/* Backward of hcm_op_vla_layer_train from d_out (rows, 256) and what the forward saved; q, kv, the weights, masks and p as the forward had them.
 *   out: d_q, d_I (rows, 256); d_kv (B, Lk, 512), summed over a sample's L rows in a fixed order (one workgroup per (sample, head));
 *        d_u (rows, 256), d_hpre (rows, d_ff), d_z (rows, 256): the row-local gradients of u = a Wo^T + bo, of fc1's pre-activation and of
 *        z = h W2^T + b2, so that dWo = d_u^T a, dW1 = d_hpre^T x1, dW2 = d_z^T h, d_bo / d_b1 / d_b2 = their column sums -- dense reductions
 *        over all rows, left to the caller; d_ln (4, 256) = d_g1, d_be1, d_g2, d_be2, reduced here (per-workgroup partials in `work`, summed
 *        in workgroup order) because the normalised rows never leave the op otherwise.
 * Four launches on `stream`, no host synchronisation. */
int hcm_op_vla_layer_bwd(const float* d_out, const float* q, const float* kv, const float* wo, const float* w1, const float* w2, const float* g1,
                         const float* g2, const uint8_t* keep1, const uint8_t* keep2, const uint8_t* keep3, float p, const float* x1hat, const float* h,
                         const float* x2hat, const float* rstd, float* work, float* d_q, float* d_I, float* d_kv, float* d_u, float* d_hpre, float* d_z,
                         float* d_ln, int B, int L, int Lk, int d_ff, void* stream);

/* One half of Visual_Ling_Attn's prologue (transformer.py:262-274) in float32 and with what a backward pass needs (csrc/embed_train.hip): Linear, ReLU,
 * dropout, LayerNorm and an optional additive table, output width 256.  rows >= 0; K a multiple of 64 from 64 to 1024; 0 <= p < 1; period >= 1 when
 * post is given (rows need not be a multiple of it); anything else HCM_ERR_ARG.
 *   pre  = x W^T + b;   r = keep s relu(pre), s = 1 / (1 - p)   (keep NULL: no dropout at all, r = relu(pre), and the backward takes p = 0)
 *   xhat = (r - mean(r)) rstd, rstd = 1 / sqrt(var(r) + 1e-5) (biased variance);   y = xhat gamma + beta + post[row % period]   (post NULL: no table)
 *   x (rows, K); w (256, K), b, gamma, beta (256) as torch stores them; keep (rows, 256) uint8; post (period, 256), e.g. the sinusoid table with
 *   period = L; all on the device.
 * Written by the forward, read by the backward (owned by the caller): xhat (rows, 256) and rstd (rows) float32, and gate (rows, 256) uint8 =
 *   (pre > 0) && keep -- one byte per element instead of a saved r, written with or without dropout.  pre, relu(pre) and r never reach memory.
 * work: hcm_op_embed_ln_work_floats(rows, K) floats (0 for unsupported sizes) owned by the caller, serving either op: the weight in the kernels'
 *   operand order (float4 index (ntile * Kb/8 + kk) * 64 + lane holds B[k = 8 kk + 4 (lane >> 5) + j][n = 32 ntile + (lane & 31)], j = 0..3, with
 *   B = W^T (Kb = K) forward and B = W (Kb = 256) backward; packed on `stream` in every call, nothing is cached) and the backward's LayerNorm
 *   partial sums.  No output may overlap it (HCM_ERR_ARG).  Float tensors and work must be 16-byte aligned, keep and gate 4-byte aligned.
 * Both ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible.
 * rows = 0: HCM_OK; the backward writes zeros to d_ln; nothing else is touched and the row pointers may be NULL. */
int64_t hcm_op_embed_ln_work_floats(int rows, int K);
int hcm_op_embed_ln_train(const float* x, const float* w, const float* b, const float* gamma, const float* beta, const uint8_t* keep, float p,
                          const float* post, int period, float* y, float* xhat, float* rstd, uint8_t* gate, float* work, int rows, int K, void* stream);
/* Backward of hcm_op_embed_ln_train from d_y (rows, 256) and what the forward saved; w, gamma and p as the forward had them.
 *   dxh = d_y gamma;  d_r = rstd (dxh - mean(dxh) - xhat mean(dxh xhat));  d_pre = gate s d_r;  d_x = d_pre W
 *   out: d_pre (rows, 256), the row-local gradient of the pre-activation, so that dW = d_pre^T x and db = its column sum -- dense reductions over
 *        all rows, left to the caller; d_x (rows, K), or NULL: the product and the weight pack are skipped; d_ln (2, 256) = d_gamma = sum_rows
 *        d_y xhat and d_beta = sum_rows d_y, reduced here (per-workgroup partials in `work`, summed in workgroup order).
 * Up to three launches on `stream` (pack, row kernel, reduce), no host synchronisation. */
int hcm_op_embed_ln_bwd(const float* d_y, const float* w, const float* gamma, const float* xhat, const float* rstd, const uint8_t* gate, float p,
                        float* work, float* d_pre, float* d_x, float* d_ln, int rows, int K, void* stream);

/* The instruction encoder's packed scan (InstructionEncoder, models/encoders/instruction_encoder.py:70-92) in float32 with what a backward pass
 * needs, and its reverse-time scan (csrc/instr_scan.hip): nn.LSTM (HCM_LSTM, gates i,f,g,o) or nn.GRU (HCM_GRU, gates r,z,n), one layer,
 * dirs = 1 or 2 directions, hidden 256, any B, L >= 1.  Row b is active at tokens t < lengths[b] (clamped to [0, L]) as in a packed sequence: the
 * reverse direction starts at the row's own last token, and a row of length 0 yields zeros everywhere and contributes nothing.  With G = 4 / 3:
 *   pre (dirs, B*L, G*256) = emb W_ih^T + bias per direction (LSTM: b_ih + b_hh; GRU: b_ih + (b_hr, b_hz, 0)); b_hn (dirs, 256): GRU's b_hn, which
 *   stays inside r * (W_hn h + b_hn) (NULL for LSTM); w_hh (dirs, G*256, 256) as torch stores weight_hh_l0 [/ _reverse]; lengths (B,) int32; all
 *   on the device.
 * hcm_op_instr_scan_train, ONE scan launch behind a weight pack, writes (owned by the caller)
 *   out (B, L, dirs*256): h_t of every active token, zeros at inactive ones -- the per-token output, and the left operand of dW_hh;
 *   final (B, 256), may be NULL: the forward direction's h at each row's own last token (final_state_only);
 *   gates (dirs, B*L, 4*256): the post-activation gates of every active token -- LSTM i,f,g,o; GRU r,z,n and hn = W_hn h + b_hn;
 *   c_seq (dirs, B*L, 256): c_t of every active token, LSTM only (NULL for GRU).  gates and c_seq are not written at inactive tokens.
 *   With the same weights the results equal, bit for bit, those of the engines' one-launch scans (hcm_op_instr_scan_infer).
 * hcm_op_instr_scan_bwd, ONE scan launch behind a weight pack, takes the cotangents d_out (B, L, dirs*256) and / or d_final (B, 256) -- either
 *   may be NULL; d_final enters at t = lengths[b] - 1 of the forward direction; a cotangent at an inactive token is not read -- and gates, c_seq,
 *   out, w_hh, lengths as the forward had them, and writes d_pre (dirs, B*L, G*256), the gradient with respect to `pre`, and for GRU
 *   d_gh (dirs, B*L, 3*256) = [da_r, da_z, da_n * r], the h-side gate gradients (NULL for LSTM, where they are d_pre); exact zeros at inactive
 *   tokens.  With h'[b, t] = out[b, t - 1] in the forward and out[b, t + 1] in the reverse direction (zero at each end), per direction:
 *   dW_ih = d_pre^T emb, db_ih = sum d_pre, dW_hh = d_gh^T h', db_hh = sum d_gh, d_emb = d_pre W_ih -- dense reductions left to the caller.
 * work: hcm_op_instr_scan_work_floats(B, L, dirs, rnn_type) floats (0 for unsupported arguments) owned by the caller, serving either op: W_hh in
 *   the launch's order ([k][unit][4 gates] forward, [row quad][k][4 rows] reverse), packed on `stream` in every call -- nothing is cached, weights
 *   change at every optimizer step.  No output may overlap it.  Float tensors and work must be 16-byte aligned, lengths 4-byte aligned.
 * HCM_ERR_ARG with a message (hcm_last_error(NULL)), never a launch: hidden != 256, dirs outside {1, 2}, a NULL required pointer, an output
 *   overlapping work, a misaligned pointer.
 * The ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
int64_t hcm_op_instr_scan_work_floats(int B, int L, int dirs, int rnn_type);
int hcm_op_instr_scan_train(const float* pre, const float* w_hh, const float* b_hn, const int32_t* lengths, float* out, float* final, float* gates,
                            float* c_seq, float* work, int B, int L, int hidden, int dirs, int rnn_type, void* stream);
int hcm_op_instr_scan_bwd(const float* d_out, const float* d_final, const float* gates, const float* c_seq, const float* out, const float* w_hh,
                          const int32_t* lengths, float* work, float* d_pre, float* d_gh, int B, int L, int hidden, int dirs, int rnn_type,
                          void* stream);
/* A comparison hook for the tests, not an operator to build on (it checks sizes and NULLs, not alignment or overlap): the engines' existing
 * one-launch inference scans on their own (the forms of csrc/instr_scan.hip's kernel without the saved tensors), to hold hcm_op_instr_scan_train
 * against: pre, b_hn and lengths as above, wt (dirs, 256, 256, 4) = W_hh already in the forward order (what hcm_op_instr_scan_train leaves in
 * `work`).  final_only != 0: the final-state form, dirs = 1, out (B, 256); otherwise the per-token form, LSTM only, out (B, L, dirs*256). */
int hcm_op_instr_scan_infer(const float* pre, const float* wt, const float* b_hn, const int32_t* lengths, float* out, int B, int L, int hidden, int dirs,
                            int rnn_type, int final_only, void* stream);

/* CMANet's attention stage (models/cma.py:271-311) in float32 with a backward pass (csrc/cma_attn_train.hip).  Every _attn call there has one query
 * per sample and keys that are a 1x1 convolution of the raw tokens X, so with qt = q W_k (the caller's product; q.b_k is the same for every
 * position and cancels in the softmax) and X = [x | e], C = C0 + Ce channels and I positions:
 *   a = softmax_i(scale (x_i . qt - 1e8 mask_i)),   xbar = sum_i a_i x_i       (text: xbar is the output; RGB / depth: out = xbar W_v^T + b_v)
 *   qt (B, C); x (B, I, C0) with layout = HCM_ATTN_TOKEN_MAJOR (the instruction encoder's output as hcm_op_instr_scan_train stores it) or (B, C0, I)
 *   with HCM_ATTN_CHANNEL_MAJOR (the reference's NCHW trunk feature, flattened); e (I, Ce): Ce further channels shared by all samples (the spatial
 *   embedding, read where it lies -- no concatenated copy), or NULL with Ce = 0; all float32 on the device.
 *   mask_zero != 0: position i of sample b is masked exactly when all C channels compare == 0.0f (-0.0 counts, NaN does not; cma.py:273), derived
 *   in the pass that forms the logits; 1e8 is subtracted before the scale as the reference writes it, so a fully masked sample gets uniform
 *   weights and xbar = exact zeros.
 * hcm_op_attn1q_train, ONE launch, writes a (B, I) and xbar (B, C).  It needs no work buffer; `work` may be NULL.
 * hcm_op_attn1q_bwd takes d_xbar (B, C) and qt, x, e, a, layout, scale as the forward had them, and writes, with da_i = x_i . d_xbar and
 *   dlog_i = scale a_i (da_i - sum_j a_j da_j):   d_qt (B, C) = sum_i dlog_i x_i;   d_x[c, i] = d_xbar_c a_i + qt_c dlog_i in x's layout, or NULL:
 *   not computed (frozen features);   d_e (I, Ce) = the same expression over the tail channels summed over the samples -- required exactly when e
 *   is given; per-sample partials in `work`, summed in sample order by a second launch.
 * work: hcm_op_attn1q_work_floats(B, C0, Ce, I) floats (B I Ce; 0 for unsupported sizes) owned by the caller, required by the backward when e is
 *   given.  No output may overlap it.  The kernels move 16 bytes per lane where the shape keeps every access aligned (token-major: C0 % 4 == 0;
 *   channel-major: I % 4 == 0) and a dword otherwise, chosen per call; every sum runs in an order fixed by (layout, C0, Ce, I).
 * HCM_ERR_ARG with a message (hcm_last_error(NULL)), never a launch: a NULL required pointer, e and Ce disagreeing, I outside 1..256, C above
 *   4096, Ce % 4 != 0, an unknown layout, an output overlapping work, a float tensor that is not 16-byte aligned.
 * B = 0: HCM_OK; the backward writes zeros to d_e; nothing else is touched and the per-sample pointers may be NULL.
 * The ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
#define HCM_ATTN_TOKEN_MAJOR 0
#define HCM_ATTN_CHANNEL_MAJOR 1
int64_t hcm_op_attn1q_work_floats(int B, int C0, int Ce, int I);
int hcm_op_attn1q_train(const float* qt, const float* x, const float* e, int layout, int mask_zero, float scale, float* a, float* xbar, float* work,
                        int B, int C0, int Ce, int I, void* stream);
int hcm_op_attn1q_bwd(const float* d_xbar, const float* qt, const float* x, const float* e, const float* a, int layout, float scale, float* d_qt,
                      float* d_x, float* d_e, float* work, int B, int C0, int Ce, int I, void* stream);

/* The end of the flat trainer's update step, _update_agent (robo_vln_trainer.py:505-542), in float32 with a backward pass
 * (csrc/flat_heads_train.hip): the heads of CMANet / Seq2SeqNet over the state encoder's rows and the criterion of hcm_flat_val_step.
 *   out = x W_lin^T + b_lin (rows, num_actions);  stop = x W_stop^T + b_stop (rows, 1);  progress_hat = tanh(x W_pm^T + b_pm) (rows, 1)
 *   x (rows, hidden); w_lin (num_actions, hidden), b_lin (num_actions), w_stop (1, hidden), b_stop (1), w_pm (1, hidden), b_pm (1) as nn.Linear
 *   stores them; corrected_actions (rows, num_actions), oracle_stop (rows, 1), progress (rows,); all float32 on the device.
 *   w_pm, b_pm, progress and progress_hat all NULL = no progress monitor; given together otherwise.
 * hcm_op_flat_heads_loss_train, TWO launches: the heads (a wave per row, a fixed summation order over hidden, so a row's out / stop /
 *   progress_hat bits depend on that row and the weights alone -- not on rows, the row's position or the grid), then flat_val_loss_kernel on them:
 *   result (8,) has the bits of hcm_op_flat_val_loss fed this call's out, stop and progress_hat, and its meaning -- [0] the masked MSE, [1] the BCE
 *   over the rows with oracle_stop != -1, [2] the aux mean over the rows with corrected_actions[r, 0] != 0 with weight 1.0 (the `alpha` quirk; 0
 *   without the monitor), [3], [4] the two counts, [5..7] 0; NaN over an empty selection.  out and stop are the raw head outputs, as the model's
 *   forward returns them: the masked_fill_ of :522 is applied inside the criterion only.
 * hcm_op_flat_heads_loss_bwd, TWO launches, takes the cotangent d_result (8,) ON THE DEVICE ([0..2] = g0, g1, g2 are read; nothing is read back to
 *   the host), the counts n_stop = result[3] and n_aux = result[4], and x, the weights, out, stop, progress_hat and the labels as the forward had
 *   them.  Per row:  d_out[r, j] = g0 2 (out - c) / (rows num_actions), exactly 0 where c == 0;  d_stop[r] = g1 (sigmoid(stop) - y) / n_stop on the
 *   selected rows, exactly 0 elsewhere;  d_pre[r] = g2 2 (p - y) (1 - p^2) / n_aux on the selected rows, exactly 0 elsewhere -- whatever the count:
 *   with an empty selection the loss is NaN and that term's gradients are zeros, as torch's masked_select(...).mean() over nothing.  Then
 *   d_x (rows, hidden) = sum_k d_head[r, k] W_k, or NULL: not computed;  d_W_k = sum_r d_head[r, k] x[r, :];  d_b_k = sum_r d_head[r, k]
 *   into d_w_lin / d_b_lin / d_w_stop / d_b_stop / d_w_pm / d_b_pm (the last two NULL exactly when w_pm is).  A workgroup owns 32 rows and sums
 *   its share in row order; a second launch adds the workgroups' shares from `work` in workgroup order.
 * work: hcm_op_flat_heads_work_floats(rows, hidden, num_actions) floats (0 for unsupported sizes) owned by the caller, required by the backward.
 *   No output may overlap it.  x, d_x, the weights, their gradients and work must be 16-byte aligned.
 * hidden must be 512 and 1 <= num_actions <= 4; rows >= 0, and rows == 0 is HCM_OK, writes nothing and reads no pointer.  HCM_ERR_ARG with a message (hcm_last_error(NULL)), never
 *   a launch: any other size, a NULL required pointer, the monitor's pointers disagreeing, an output overlapping work, a misaligned pointer.
 * The ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
int64_t hcm_op_flat_heads_work_floats(int rows, int hidden, int num_actions);
int hcm_op_flat_heads_loss_train(const float* x, const float* w_lin, const float* b_lin, const float* w_stop, const float* b_stop, const float* w_pm,
                                 const float* b_pm, const float* corrected_actions, const float* oracle_stop, const float* progress, float* out,
                                 float* stop, float* progress_hat, float* result, int rows, int hidden, int num_actions, void* stream);
int hcm_op_flat_heads_loss_bwd(const float* d_result, const float* x, const float* w_lin, const float* w_stop, const float* w_pm, const float* out,
                               const float* stop, const float* progress_hat, const float* corrected_actions, const float* oracle_stop,
                               const float* progress, const float* result, float* d_x, float* d_w_lin, float* d_b_lin, float* d_w_stop,
                               float* d_b_stop, float* d_w_pm, float* d_b_pm, float* work, int rows, int hidden, int num_actions, void* stream);

/* The end of the hierarchical trainer's high-level update step, _update_agent (hierarchical_trainer.py:506-512), in float32 with a backward pass
 * (csrc/subtask_ce_train.hip): the head of Seq2Seq_HighLevel_CMA over the state encoder's rows and the cross-entropy of hcm_val_step.
 *   logits = x W^T + b (rows, A);  x (rows, hidden); w (A, hidden), b (A) as nn.Linear stores them; all float32 on the device.
 *   oracle_subtask (rows,) int64 on the device, as hcm_val_step takes it: 0 = padded row, 1..num_sub_tasks = the target class plus one; a value
 *   outside [0, num_sub_tasks] is counted in result[6] and treated as padded.
 * hcm_op_subtask_ce_train, TWO launches: the head (a wave per row, a fixed summation order over hidden, so a row's logits bits depend on that
 *   row and the weights alone -- not on rows, the row's position or the grid), then the criterion with val_loss_kernel's arithmetic, launch shape
 *   and order of summation (one workgroup of 256 threads, thread t adds rows t, t + 256, ..., a xor butterfly, then the waves in wave order).
 *   result (8,) uses the index positions of hcm_val_step: [0] CrossEntropyLoss(ignore_index = -1, mean) of logits against oracle_subtask - 1
 *   over the valid rows, [3] the valid rows whose argmax (first maximal index) is the target, [4] the valid rows, [6] the out-of-range rows,
 *   [1] = [2] = [5] = [7] = 0; words [0], [3], [4], [6] have the bits of hcm_op_val_loss fed this call's logits.  No valid row: NaN in [0] and
 *   counts of 0, as torch gives; a NaN in a valid row's logits propagates into [0].  logits is the raw head output, as the model's forward
 *   returns it: the masked_fill_ of :509 touches padded rows only, which the criterion ignores.
 * hcm_op_subtask_ce_bwd, TWO launches, takes the cotangent d_result (8,) ON THE DEVICE ([0] = g0 is read; nothing is read back to the host), the
 *   count total = result[4], and x, w, logits and the labels as the forward had them.  Per valid row, with the softmax recomputed around the row
 *   maximum from the saved logits:  d_logits[r, j] = g0 (softmax(logits[r])[j] - [j == target]) / total;  exactly 0 on padded and out-of-range
 *   rows, and on every row when total == 0 (the loss is NaN and the gradients are zeros, as torch's).  Then
 *   d_x (rows, hidden) = d_logits W, or NULL: not computed;  d_w (A, hidden) = d_logits^T x;  d_b (A) = sum_r d_logits[r].  A workgroup owns 32
 *   rows (two halves of 16) and sums its share in row order; a second launch adds the workgroups' shares from `work` in workgroup order.
 * work: hcm_op_subtask_ce_work_floats(rows, hidden, A) floats (0 for unsupported sizes) owned by the caller, required by the backward.  No
 *   output may overlap it.  x, w, d_x, d_w and work must be 16-byte aligned, the other float tensors 4-byte and oracle_subtask 8-byte aligned.
 * hidden must be 512 and 1 <= num_sub_tasks <= A <= 6; rows >= 0, and rows == 0 is HCM_OK, writes nothing and reads no pointer.  HCM_ERR_ARG
 *   with a message (hcm_last_error(NULL)), never a launch: any other size, a NULL required pointer, an output overlapping work, a misaligned
 *   pointer.
 * The ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
int64_t hcm_op_subtask_ce_work_floats(int rows, int hidden, int A);
int hcm_op_subtask_ce_train(const float* x, const float* w, const float* b, const int64_t* oracle_subtask, float* logits, float* result, int rows,
                            int hidden, int A, int num_sub_tasks, void* stream);
int hcm_op_subtask_ce_bwd(const float* d_result, const float* x, const float* w, const float* logits, const int64_t* oracle_subtask,
                          const float* result, float* d_x, float* d_w, float* d_b, float* work, int rows, int hidden, int A, int num_sub_tasks,
                          void* stream);

/* The convolutional part of the reference's SimpleAllCNN.cnn (models/encoders/simple_cnns.py:76-95) in float32 with a backward pass
 * (csrc/simplecnn_train.hip), the trainable form of what hcm_op_simplecnn3 runs for the engines:
 *   Conv2d(Cin, 32, 8, stride 4) + ReLU -> Conv2d(32, 64, 4, stride 2) + ReLU -> Conv2d(64, 32, 3, stride 1), no padding.
 *   x (B, H, W, Cin), the frames as the observations carry them: HCM_F32, or HCM_U8 with Cin = 3; every element is multiplied by `scale` (1/255
 *   for RGB bytes, 1 for depth) as it is read.  Cin is 1 or 3; H, W >= 36, any other size, non-square allowed.
 *   w1 (32, Cin, 8, 8), b1 (32), w2 (64, 32, 4, 4), b2 (64), w3 (32, 64, 3, 3), b3 (32): torch's OIHW parameters, float32 on the device.
 *   With h1 = (H - 8) / 4 + 1, h2 = (h1 - 4) / 2 + 1, h3 = h2 - 2 (and w likewise):  y (B, 32, h3, w3), contiguous and channel-major, so
 *   y viewed as (B, 32 h3 w3) is the reference's Flatten order in front of cnn.7.
 * hcm_op_simplecnn_train packs the three weights into `work` (one small launch each) and runs one launch per convolution on
 *   v_mfma_f32_32x32x2f32.  It writes y and leaves the two post-ReLU maps in `work` for the backward; their layout is the kernels' business.
 *   Every output element sums its window in the order (ci, ky, kx) ascending, so a row's bits depend on that row and the weights alone, not on
 *   B or the row's position.
 * hcm_op_simplecnn_bwd takes d_y (B, 32, h3, w3), the frames, scale, w2 and w3 as the forward had them and THE SAME `work` the forward filled,
 *   and writes d_w1, d_b1, d_w2, d_b2, d_w3, d_b3 in the parameters' shapes: per layer from the last, the weight gradient (a chunk of output
 *   pixels per workgroup, the chunks' shares added in chunk order by a second launch), the bias sum (a fixed tree), and for conv3 and conv2 the
 *   gradient of the layer's input gated by `stored value > 0`, torch's in-place ReLU.  A pixel of map 1 or map 2 that no window of the next
 *   convolution covers receives an exact zero.  There is no frame gradient.  The backward leaves the maps intact, so it may run twice.
 * work: hcm_op_simplecnn_work_floats(B, H, W, Cin) floats (0 for unsupported arguments) owned by the caller: packed weights, the two maps,
 *   the two gated gradients, the chunk shares.  No output may overlap it.  The float tensors must be 4-byte aligned.
 * HCM_ERR_ARG with a message (hcm_last_error(NULL)), never a launch: Cin outside {1, 3}, a frame under 36 pixels, HCM_U8 with Cin = 1 or any
 *   other dtype, B < 0, a call so large that an element offset leaves 31 bits, a NULL required pointer, an output overlapping work, a
 *   misaligned pointer.  No pointer may be NULL, except that with B = 0 the forward is HCM_OK and touches nothing, and the backward writes
 *   zeros to the six gradients and reads no other pointer.
 * The ops allocate nothing, copy nothing to the host, do not synchronise, run on `stream`, use no atomics and are bitwise reproducible. */
int64_t hcm_op_simplecnn_work_floats(int B, int H, int W, int Cin);
int hcm_op_simplecnn_train(const void* x, int x_dtype, float scale, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, const float* b3, float* y, float* work, int B, int H, int W, int Cin, void* stream);
int hcm_op_simplecnn_bwd(const float* d_y, const void* x, int x_dtype, float scale, const float* w2, const float* w3, float* work, float* d_w1,
                         float* d_b1, float* d_w2, float* d_b2, float* d_w3, float* d_b3, int B, int H, int W, int Cin, void* stream);

/* csrc/features.hip alone: x (rows, C, S) f32 contiguous (the reference's NCHW feature) <-> columns [0, C) of y [rows][S][ld] in the storage
 * type `dtype`, times `scale` (a power of two at every call site).  Any rows in [1, 65535], C, S >= 1, ld >= C. */
int hcm_op_feat_ingest(const float* x, void* y, int dtype, int rows, int C, int S, int ld, float scale, void* stream);
int hcm_op_feat_export(const void* y, int dtype, float* x, int rows, int C, int S, int ld, float scale, void* stream);
/* csrc/features.hip alone, the two kernels of hcm_instr_features: x f32 (src_rows, L, D) -> y (B, L, D) contiguous in the storage type `dtype`
 * (HCM_F32 / HCM_F16 / HCM_BF16), output row r from source row r % src_rows; and y (rows, L, D) -> x f32 (rows, L, D).  lens: device (B,) /
 * (rows,) int32 or NULL; positions l >= lens[r] (clamped to [0, L]) are written as exact +0.0 and never read.  One round-to-nearest-even into
 * `dtype` on the way in, exact on the way out.  16-byte accesses on both sides when D is a multiple of 8 and both pointers are 16-byte aligned,
 * scalar ones otherwise.  HCM_ERR_ARG: B / rows, src_rows, L or D < 1, B % src_rows != 0, a NULL x or y, an unknown dtype. */
int hcm_op_instr_feat_ingest(const float* x, void* y, int dtype, const int32_t* lens, int B, int src_rows, int L, int D, void* stream);
int hcm_op_instr_feat_export(const void* y, int dtype, float* x, const int32_t* lens, int rows, int L, int D, void* stream);

/* The depth trunk's run kernels alone: `nblocks` identity bottlenecks (conv1x1 -> GroupNorm(16) -> ReLU -> conv3x3 pad 1 -> GroupNorm -> ReLU ->
 * conv1x1 -> GroupNorm -> + block input -> ReLU; habitat's GroupNorm ResNet-50 as used at resnet_encoders.py:27-62) in ONE launch, a workgroup per
 * (sample, trunk).  side 32: 128 / 32 channels, side 16: 256 / 64 (csrc/depth_blk.hip, 1..4 blocks); side 8: 512 / 128 (csrc/igemm.hip
 * depth_l3_kernel, 1..6 blocks); any other side is HCM_ERR_ARG.  x, y [B][side*side][ld] in `dtype` (HCM_F16 / HCM_BF16), trunk g at channels
 * [g*C, +C), ld a multiple of 8 and >= groups*C; columns beyond groups*C are neither read nor written.
 *   w    host array of 3*nblocks device pointers, w1 w2 w3 per block: [groups][CM][C], [groups][CM][9*CM] (k = tap*CM + ci), [groups][C][CM]
 *   gn   host array of 6*nblocks device pointers, gamma1 beta1 gamma2 beta2 gamma3 beta3 per block: [groups*channels] floats
 *   eps  host array of 3*nblocks floats
 * x == y: sides 32 / 16 with one block only (a run reads block 0's input from x and every later one from y: refused otherwise); side 8 with any
 * block count (a workgroup reads its whole slice of x before it writes one element of y).  Every refusal is HCM_ERR_ARG without a launch. */
int hcm_op_depth_run(const void* x, void* y, const void* const* w, const float* const* gn, const float* eps, int dtype, int B, int side,
                     int groups, int nblocks, int ld, void* stream);

/* ---- The step's small kernels alone (csrc/elementwise.hip), one entry per kernel family.  None allocates, copies to the host or synchronises;
 * all run on `stream`.  Every refusal is HCM_ERR_ARG without a launch.  `ld*` are row strides in ELEMENTS; columns between the logical width and
 * the stride are neither read nor written unless stated.
 *
 * hcm_op_heads: the small linear heads on a hidden state h (hidden,) f32, a wave per output row, lanes strided by 64 over hidden:
 *   out0[b*ld0 + r] = w0[r] . h + b0[r]  (r < r0),  out1 likewise,  out2[b*ld2 + r] = tanh(w2[r] . h + b2[r]);  w* are [r*][hidden] f32.
 *   A head with r* == 0 is absent.  pred (optional, hcm_op_rnn_cell only): pred[b] = torch.argmax(out0 row) -- the first maximal index, a NaN
 *   counts as the maximum and the first NaN wins -- and emb_out[b*emb_ld + j] = emb[min(pred[b], emb_rows - 1)*emb_dim + j], j < emb_dim.
 *   pred needs 1 <= r0 <= 64 (the kernel keeps the logits in 64 words of LDS), out0, emb, emb_out and emb_rows >= 1. */
typedef struct hcm_op_heads {
    const float* w0; const float* b0; float* out0; int32_t r0, ld0;
    const float* w1; const float* b1; float* out1; int32_t r1, ld1;
    const float* w2; const float* b2; float* out2; int32_t r2, ld2;
    int64_t* pred; const float* emb; float* emb_out; int32_t emb_rows, emb_dim, emb_ld;
} hcm_op_heads;

/* One recurrent step behind the gate products (RNNStateEncoder.single_forward, state_encoder.py:72-81), as the engines' rnn_finish launches it:
 *   xh (optional): xh[b*ld_xh + col0 + j] = h_in[0][b][j] * mask[b]  (the masked state the recurrent product reads), written first;
 *   HCM_LSTM: gates [B][4*hidden] (i,f,g,o) = x W_ih^T + b_ih + (h*mask) W_hh^T + b_hh, gh NULL; c = h_in[1]*mask;
 *             c' = sig(f) c + sig(i) tanh(g), h' = sig(o) tanh(c'); h_out (2,B,hidden) = (h', c').  h_in[0] is not read.
 *   HCM_GRU:  gates = gi, gh [B][3*hidden] (r,z,n) with their biases; h = h_in[0]*mask; r = sig(gi_r + gh_r), z = sig(gi_z + gh_z),
 *             n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h; h_out (1,B,hidden).
 *   mask [B] is multiplied in, whatever its value; h_out may alias h_in.  heads (optional) act on h'.
 *   bad (optional): *bad += 1 per SAMPLE whose gate pre-activations are not all finite. */
int hcm_op_rnn_cell(const float* gates, const float* gh, const float* h_in, const float* mask, float* h_out, float* xh, int ld_xh, int col0,
                    const hcm_op_heads* heads, unsigned* bad, int B, int hidden, int rnn_type, void* stream);
/* The heads over `rows` hidden states hs [rows][hidden]: bit-identical to hcm_op_rnn_cell's head outputs for the same h'.  A `pred` is refused. */
int hcm_op_heads_rows(const float* hs, const hcm_op_heads* heads, int rows, int hidden, void* stream);
/* One time step t of the packed instruction encoder (nn.LSTM / nn.GRU over pack_padded_sequence): sample b is active iff t < lengths[b].
 *   pre [B*L][G*hidden] = x_t W_ih^T + biases of the input side (LSTM: b_ih + b_hh), gh [B][G*hidden] = h W_hh^T (GRU: + b_hh); h, c [B][hidden]
 *   are updated in place (c NULL for GRU); out[(b*L + t)*ld_out + col0 + j] = h' where active.  An inactive sample keeps h and c and emits
 *   exact zeros. */
int hcm_op_instr_cell(const float* pre, const float* gh, float* h, float* c, const int32_t* lengths, float* out, int t, int B, int L, int hidden,
                      int ld_out, int col0, int rnn_type, void* stream);
/* CMANet._attn (cma.py:201-209), the inference kernel: one query per sample over S positions, f32.
 *   logits[s] = q[b] . k[b][s] (D terms); minus 1e8 where s >= lengths[b] (lengths NULL: nothing masked); p = softmax(logits * scale);
 *   out[b*ldo + c] = sum_s p[s] v[(b*S + s)*ldv + c], c < Dv.  q [B][ldq], k [B][S][ldk], v [B][S][ldv]; k and v may interleave in one
 *   buffer (ldk = ldv = D + Dv, v = k + D).  1 <= S <= 8192; lengths[b] >= 1 is the caller's contract (the reference cannot pack an empty row). */
int hcm_op_attn1q(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* lengths, float* out, int ldo, int B,
                  int S, int D, int Dv, float scale, void* stream);
/* F.adaptive_avg_pool2d over NHWC x [B][H][W][ldx] -> y [B][OH][OW][ldy], channels [0, C): window [floor(i*H/OH), ceil((i+1)*H/OH)), the sum in
 * row-major window order times 1 / count.  C, ldx, ldy multiples of the 16-byte chunk (4 f32 / 8 16-bit) and x, y aligned to it: a channel
 * offset base pointer picks one half of a hi|lo pair (ldx = 2C). */
int hcm_op_adaptive_avgpool(const void* x, void* y, int dtype, int B, int H, int W, int C, int OH, int OW, int ldx, int ldy, void* stream);
/* AdaptiveAvgPool1d(1) over tokens: y[b*ldy + c] = mean over the first n_b rows of x [B][S][ldx], c < C; n_b = S, or with lens (device, [B])
 * clamp(lens[b], 1, S): a length below 1 averages one row, one beyond S all S.  y is f32 when out_f32, else `dtype`. */
int hcm_op_mean_rows(const void* x, void* y, int dtype, int B, int S, int C, int ldx, int ldy, int out_f32, const int32_t* lens, void* stream);
/* F.avg_pool2d(x, 2) of the f32 depth frame x [B][H][W] -> y [B][H/2][W/2] in `dtype`: ((a + b) + (c + d)) * 0.25.  padded: the 16-bit types
 * only, y [B][H/2 + 6][W/2 + 8] with a zero border of 3 left / top, 5 right, 3 bottom and the same interior bits.  W even (padded: W % 4 == 0). */
int hcm_op_avgpool2(const float* x, void* y, int dtype, int B, int H, int W, int padded, void* stream);
/* BertEmbeddings: y[b][l] = LayerNorm(word[id] + pos[l] + type0) * gamma + beta, tables f32, y [B*L][D] in `dtype`; ids (B, L) as HCM_I64,
 * HCM_I32 or HCM_F32 (truncated) -- the same bits for the same values.  An id below 0 reads row 0, one >= vocab row vocab - 1.
 * D a multiple of 64, at most 1024. */
int hcm_op_bert_embed(const void* ids, int ids_dtype, const float* word, const float* pos, const float* type0, const float* gamma,
                      const float* beta, void* y, int dtype, int B, int L, int D, int vocab, float eps, void* stream);
/* InstructionEncoder's front end (instruction_encoder.py:70-92): x[(b*L + t)*ldx + j] = table[id][j] for j < E and exact 0 for E <= j < ldx
 * (ALL ldx columns are written); lengths[b] = the count of non-zero ids of row b (a zero in the middle is not counted, nothing else is
 * skipped).  ids as for hcm_op_bert_embed, the same clamp to [0, vocab - 1] for the lookup. */
int hcm_op_instr_embed(const void* ids, int ids_dtype, const float* table, float* x, int32_t* lengths, int B, int L, int E, int ldx, int vocab,
                       void* stream);
/* LayerNorm of f32 rows x [rows][D] (two-pass variance), D = 256 / 512 / 768, `dtype` HCM_F16 / HCM_BF16: y16 [rows][D] and EXACTLY ONE of
 * y32 [rows][D] (the same value unrounded) and stats [rows][2] = (mean, rstd).  Both or neither is refused. */
int hcm_op_layernorm_f32in(const float* x, const float* gamma, const float* beta, void* y16, float* y32, float* stats, int dtype, int rows,
                           int D, float eps, void* stream);
/* The calibration range check over x [rows][ld] in `dtype`, columns [0, cols): slot[0] = max(slot[0], bits of the largest finite |x|),
 * slot[1] += the count of NaN / +-inf elements.  The slot only grows. */
int hcm_op_absmax(const void* x, int dtype, int rows, int cols, int ld, unsigned* slot, void* stream);
/* pred[b] = torch.argmax(logits[b*ld .. + n)): first maximal index; a NaN counts as the maximum and the first NaN wins. */
int hcm_op_argmax(const float* logits, int64_t* pred, int B, int n, int ld, void* stream);
/* y[b*ld + col0 + j] = emb[clamp(idx[b], 0, nrows - 1)*D + j], j < D. */
int hcm_op_embed_rows(const float* emb, const int64_t* idx, float* y, int B, int D, int ld, int col0, int nrows, void* stream);
/* subtask[r] = oracle[r] - 1 for 1 <= oracle[r] <= num_sub_tasks, else num_sub_tasks (hierarchical_trainer.py:597-599). */
int hcm_op_val_subtask(const int64_t* oracle, int64_t* subtask, int rows, int num_sub_tasks, void* stream);
/* y[(b*S + s)*ldy + c] = tab[s*C + c] rounded to `dtype`, c < C. */
int hcm_op_fill_cols(const float* tab, void* y, int dtype, int B, int S, int C, int ldy, void* stream);
/* dst[r*ld_dst + j] = src[(n_src == 1 ? 0 : r)*ld_src + j], r < rows, j < cols; n_src == 1 or n_src >= rows. */
int hcm_op_copy_rows(const float* src, int ld_src, int n_src, float* dst, int ld_dst, int rows, int cols, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HCM_H */
