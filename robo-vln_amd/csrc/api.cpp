// C ABI of libhcm (include/hcm.h).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "model.h"

using namespace hcm;

static thread_local std::string g_create_err;

static int fail(hcm_ctx* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

#define REQUIRE(cond, code, msg) do { if (!(cond)) return fail(h, code, msg); } while (0)

static int check_fwd(hcm_ctx* h, int B);
static int check_len(hcm_ctx* h, int L);
static FwdCall frames(const void* rgb, int rgb_dt, const float* depth, const void* ids, int ids_dt, int rows, int L, void* stream);
static void drop_instruction_cache(hcm_ctx* h);
static bool rgb_dt_ok(int d);
static bool ids_dt_ok(int d);
static int check_obs(hcm_ctx* h, const FwdCall& c, const float* depth_arg, int rgb_dtype_arg);

static void destroy_entry(hcm_ctx::GraphEntry& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    for (auto& op : g.prog) if (op.exec) (void)hipGraphExecDestroy(op.exec);
    g.exec = nullptr;
    g.prog.clear();
}

// replay of a segmented entry: the step's top-level fork / chain launches / join, in the order the capture pass recorded them
static hipError_t replay_segments(hcm_ctx* h, const hcm_ctx::GraphEntry& g, hipStream_t stream) {
    hipError_t e = hipSuccess;
    unsigned used = 0;                                   // aux streams that received a launch since the fork
    for (const auto& op : g.prog) {
        if (op.kind == 0) {
            if ((e = hipEventRecord(h->ev_fork, stream)) != hipSuccess) return e;
            for (int i = 0; i < op.n; ++i) if ((e = hipStreamWaitEvent(g.aux[i], h->ev_fork, 0)) != hipSuccess) return e;
            used = 0;
        } else if (op.kind == 1 || op.kind == 3) {
            if (op.kind == 1) e = hipGraphLaunch(op.exec, op.st);
            else e = hipMemcpyAsync(op.dst, op.src, op.bytes, hipMemcpyHostToDevice, op.st);
            if (e != hipSuccess) return e;
            for (int i = 0; i < 4; ++i) if (op.st == g.aux[i] && op.st != stream) used |= 1u << i;
        } else {
            for (int i = 0; i < op.n; ++i) {
                if (!(used & (1u << i))) continue;       // nothing ran there: the fork's wait alone orders nothing anybody needs
                if ((e = hipEventRecord(h->ev_join[i], g.aux[i])) != hipSuccess) return e;
                if ((e = hipStreamWaitEvent(stream, h->ev_join[i], 0)) != hipSuccess) return e;
            }
        }
    }
    return e;
}

// Pick the side streams of the step's chains so that aux[1] (depth), aux[2] (BERT) and the caller's stream overlap pairwise (model.h).  The probe: two 150 us
// one-wave spin kernels, one per stream -- side by side they take 150 us, on a shared hardware queue 300.
static void pick_chain_streams(hcm_ctx* h, hipStream_t stream) {
    for (auto st : h->probed_for) if (st == stream) return;                    // (a caller that alternates between streams is probed once per stream)
    if (h->probed_for.size() >= 8) return;
    h->probed_for.push_back(stream);
    if (dev_env("HCM_NO_STREAM_PROBE")) return;
    constexpr double kSpinUs = 150.0;
    auto now = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto overlap = [&](hipStream_t x, hipStream_t y) {
        double best = 1e30;
        for (int r = 0; r < 2; ++r) {
            (void)hipStreamSynchronize(x); (void)hipStreamSynchronize(y);
            const double t0 = now();
            (void)launch_spin((unsigned long long)(kSpinUs * 100.0), x);
            (void)launch_spin((unsigned long long)(kSpinUs * 100.0), y);
            (void)hipStreamSynchronize(x); (void)hipStreamSynchronize(y);
            const double dt = now() - t0;
            if (dt < best) best = dt;
        }
        return best < 1.6 * kSpinUs;
    };
    std::vector<hipStream_t> cand;
    for (int i = 0; i < 4; ++i) if (h->aux[i]) cand.push_back(h->aux[i]);
    for (auto p : h->pool) if (p) cand.push_back(p);
    (void)launch_spin(1, stream); (void)hipStreamSynchronize(stream);      // (code object loaded before anything is timed)
    std::vector<hipStream_t> chosen;
    for (auto c : cand) {
        if (chosen.size() >= 2) break;
        bool ok = overlap(stream, c);
        for (auto k : chosen) ok = ok && overlap(k, c);
        if (ok) chosen.push_back(c);
    }
    if (dev_env("HCM_PROBE_LOG")) fprintf(stderr, "[hcm] stream probe: %zu of %zu candidate streams overlap with the caller's stream and each other\n", chosen.size(), cand.size());
    if (chosen.size() < 2) return;                                               // (a single hardware queue, or a probe disturbed by other work: keep what we have)
    // aux[1] <- chosen[0], aux[2] <- chosen[1]; the displaced streams take the chosen ones' old places
    auto place = [&](int slot, hipStream_t st) {
        if (h->aux[slot] == st) return;
        for (int i = 0; i < 4; ++i) if (h->aux[i] == st) { std::swap(h->aux[i], h->aux[slot]); return; }
        for (auto& p : h->pool) if (p == st) { std::swap(p, h->aux[slot]); return; }
    };
    place(1, chosen[0]);
    place(2, chosen[1]);
}

// graph-cache key of a call: every pointer and every scalar of its descriptor (stream and flags too), so that a field nobody thought of
// cannot make two different calls share a captured graph
static std::vector<uint64_t> call_key(const FwdCall& c, bool segmented) {
    auto p = [](const void* q) { return (uint64_t)(uintptr_t)q; };
    return {(uint64_t)c.do_hi | (uint64_t)c.do_lo << 1 | (uint64_t)c.reuse_instruction << 2 | (uint64_t)c.host_frames << 3 | (uint64_t)segmented << 4,
            (uint64_t)c.val, (uint64_t)c.rgb_dt, (uint64_t)c.ids_dt, (uint64_t)c.rows, (uint64_t)c.T, (uint64_t)c.Bi, (uint64_t)c.L,
            (uint64_t)c.ld_logits, (uint64_t)c.ld_vel, (uint64_t)c.ld_stop, p(c.stream), p(c.rgb), p(c.depth), p(c.ids), p(c.lens),
            p(c.hi_h_in), p(c.lo_h_in), p(c.hi_h_out), p(c.lo_h_out), p(c.mask), p(c.subtask), p(c.logits), p(c.vel), p(c.stop), p(c.progress),
            p(c.oracle), p(c.corrected), p(c.oracle_stop), p(c.progress_label), p(c.result),
            p(c.rgb_feat[0]), p(c.rgb_feat[1]), p(c.depth_feat[0]), p(c.depth_feat[1]), p(c.instr_feat), (uint64_t)c.instr_rows};
}

// hipGraph cache shared by the fused entry points, keyed by call_key().  A key is run eagerly the first time it is seen (that also
// performs the one-time kernel attribute setup) and captured -- forked side streams included -- the second time; later
// calls replay the instantiated graph.
// segmented = HCM_ACT_CHAIN_GRAPHS: one linear graph per chain, captured by the step itself at its chain boundaries (model.h, SegOp).
static int run_graphed(hcm_ctx* h, const FwdCall& call, bool segmented = false) {
    const hipStream_t stream = call.stream;
    auto run = [&]() { run_forward(h, call); };
    auto eager = [&]() -> int {
        try { run(); } catch (const std::exception& e) { return fail(h, HCM_ERR_HIP, e.what()); }
        ++h->eager_launches;
        return HCM_OK;
    };
    if (segmented && stream != nullptr && !h->taps_on) pick_chain_streams(h, stream);      // (once per caller stream; eager steps fork onto the same side streams)
    // the legacy default stream cannot be captured; taps allocate and synchronise
    if (!h->use_graph || h->taps_on || stream == nullptr) return eager();
    const std::vector<uint64_t> key = call_key(call, segmented);
    for (auto& g : h->graphs)
        if (g.key == key) {
            if (!g.prog.empty()) {
                if (replay_segments(h, g, stream) != hipSuccess) return fail(h, HCM_ERR_HIP, "replay of the step's chain graphs failed");
            } else
            if (hipGraphLaunch(g.exec, stream) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipGraphLaunch failed");
            ++h->graph_launches;
            return HCM_OK;
        }
    bool seen = false;
    for (auto& k : h->seen_keys) seen = seen || k == key;
    if (!seen) {
        if (h->seen_keys.size() >= 16) h->seen_keys.erase(h->seen_keys.begin());
        h->seen_keys.push_back(key);
        return eager();
    }
    if (segmented) {
        // one linear graph per chain (model.h, SegOp): the capture calls are made by the step itself at its chain boundaries
        h->seg_mode = true;
        h->seg_open = false;
        h->seg_prog.clear();
        std::string err;
        try { run(); } catch (const std::exception& e) { err = e.what(); }
        h->seg_mode = false;
        if (h->seg_open) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(h->seg_stream, &g); if (g) (void)hipGraphDestroy(g); h->seg_open = false; }
        hcm_ctx::GraphEntry ge;
        ge.key = key;
        ge.prog.swap(h->seg_prog);
        for (int i = 0; i < 4; ++i) ge.aux[i] = h->aux[i];
        bool any = false;
        for (auto& op : ge.prog) any = any || op.kind == 1;
        if (!err.empty() || !any) {
            destroy_entry(ge);
            (void)hipGetLastError();
            h->use_graph = false;
            if (!err.empty()) return fail(h, HCM_ERR_HIP, "graph capture failed: " + err);
            return eager();
        }
        if (h->graphs.size() >= 8) { destroy_entry(h->graphs.front()); h->graphs.erase(h->graphs.begin()); }
        h->graphs.push_back(ge);
        if (replay_segments(h, h->graphs.back(), stream) != hipSuccess) return fail(h, HCM_ERR_HIP, "replay of the step's chain graphs failed");
        ++h->graph_launches;
        return HCM_OK;
    }
    if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return eager(); }
    std::string cap_err;
    try { run(); } catch (const std::exception& e) { cap_err = e.what(); }
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamEndCapture(stream, &graph);
    if (!cap_err.empty() || ce != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        h->use_graph = false;                      // do not retry on this handle
        if (!cap_err.empty()) return fail(h, HCM_ERR_HIP, "graph capture failed: " + cap_err);
        return eager();
    }
    hcm_ctx::GraphEntry ge;
    ge.key = key;
    ce = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ce != hipSuccess) { (void)hipGetLastError(); h->use_graph = false; return eager(); }
    if (h->graphs.size() >= 8) { destroy_entry(h->graphs.front()); h->graphs.erase(h->graphs.begin()); }
    h->graphs.push_back(ge);
    if (hipGraphLaunch(ge.exec, stream) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipGraphLaunch failed");
    ++h->graph_launches;
    return HCM_OK;
}

extern "C" {

int hcm_create(const hcm_config* cfg, hcm_handle* out) {
    hcm_ctx* h = nullptr;
    REQUIRE(cfg && out, HCM_ERR_ARG, "hcm_create: null argument");
    REQUIRE(cfg->struct_size == (int32_t)sizeof(hcm_config), HCM_ERR_ARG, "hcm_create: struct_size mismatch");
    REQUIRE(cfg->precision == HCM_F32 || cfg->precision == HCM_BF16 || cfg->precision == HCM_F16, HCM_ERR_ARG, "precision must be HCM_F32, HCM_F16 or HCM_BF16");
    REQUIRE(cfg->max_batch >= 1, HCM_ERR_ARG, "max_batch must be >= 1");
    // flags whose branches crash in the reference are rejected, not emulated
    REQUIRE(!cfg->use_prev_action, HCM_ERR_UNSUPPORTED,
            "SEQ2SEQ.use_prev_action=True is a broken branch in the reference (seq2seq_highlevel_cma.py:203-207)");
    REQUIRE(!cfg->ablate_instruction, HCM_ERR_UNSUPPORTED,
            "ablate_instruction=True is a broken branch in the reference (seq2seq_highlevel_cma.py:183-184)");
    REQUIRE(!cfg->progress_monitor, HCM_ERR_UNSUPPORTED,
            "PROGRESS_MONITOR.use in forward references an undefined name (seq2seq_highlevel_cma.py:221-225)");
    REQUIRE(cfg->rnn_type == HCM_LSTM || cfg->rnn_type == HCM_GRU, HCM_ERR_ARG, "STATE_ENCODER.rnn_type must be LSTM or GRU");
    REQUIRE(cfg->build_high || cfg->build_low, HCM_ERR_ARG, "nothing to build");
    if (cfg->build_high) {
        REQUIRE(cfg->rgb_encoder == HCM_ENC_RESNET && cfg->depth_encoder == HCM_ENC_RESNET, HCM_ERR_UNSUPPORTED,
                "Seq2Seq_HighLevel_CMA needs TorchVisionResNet50 + VlnResnetDepthEncoder: SimpleCNN encoders have no "
                "output_shape (seq2seq_highlevel_cma.py:87,:96)");
        REQUIRE(cfg->d_model == 256 && cfg->vis_in % 32 == 0 && cfg->ins_in == cfg->bert_hidden, HCM_ERR_UNSUPPORTED,
                "VISUAL_LING_ATTN: d_model must be 256 and ins_in_features must equal the BERT width");
        REQUIRE(cfg->d_model / cfg->vla_heads == 64 && cfg->bert_hidden / cfg->bert_heads == 64, HCM_ERR_UNSUPPORTED,
                "attention head dim must be 64");
        REQUIRE(cfg->bert_hidden == 768 && cfg->instr_len >= 1 && cfg->instr_len <= 512 && cfg->instr_len <= cfg->bert_max_pos,
                HCM_ERR_UNSUPPORTED, "BERT width must be 768 and 1 <= instr_len (the maximum L of a call) <= min(512, bert_max_pos)");
        REQUIRE(cfg->vla_layers >= 1 && cfg->bert_layers >= 1, HCM_ERR_ARG, "layer counts must be >= 1");
    }
    REQUIRE(cfg->hidden == 512 || cfg->hidden % 64 == 0, HCM_ERR_UNSUPPORTED, "hidden size must be a multiple of 64");
    // depth: habitat's ResNet encoder sizes itself from the frame HEIGHT and assumes a square final map (resnet_encoders.py:37-62); RGB: the
    // torchvision trunk ends in adaptive pools and takes any H x W (resnet_encoders.py:211-236), SimpleRGBCNN sizes its FC from the two
    // dimensions on their own (simple_cnns.py:63-73, >= 36 pixels each for a 1 x 1 final map)
    REQUIRE(cfg->depth_h == cfg->depth_w || cfg->depth_encoder == HCM_ENC_SIMPLECNN, HCM_ERR_UNSUPPORTED,
            "depth frames must be square with the ResNet depth encoder");
    if (cfg->rgb_encoder == HCM_ENC_SIMPLECNN)
        REQUIRE(cfg->rgb_h >= 36 && cfg->rgb_w >= 36, HCM_ERR_UNSUPPORTED, "SimpleRGBCNN: rgb frame too small");
    if (cfg->depth_encoder == HCM_ENC_SIMPLECNN)
        REQUIRE(cfg->depth_h >= 36 && cfg->depth_w >= 36, HCM_ERR_UNSUPPORTED, "SimpleDepthCNN: depth frame too small");
    if (cfg->depth_encoder == HCM_ENC_RESNET)
        REQUIRE(cfg->depth_h >= 64 && cfg->depth_h % 64 == 0 && cfg->depth_h <= 1024, HCM_ERR_UNSUPPORTED,
                "depth frame size must be a multiple of 64 (habitat's ResNetEncoder: final map (H/2)/32, resnet_encoders.py:37-62)");
    if (cfg->rgb_encoder == HCM_ENC_RESNET)
        REQUIRE(cfg->rgb_h >= 32 && cfg->rgb_w >= 32, HCM_ERR_UNSUPPORTED, "rgb frame too small");
    REQUIRE(cfg->depth_baseplanes == 32, HCM_ERR_UNSUPPORTED, "resnet_baseplanes is 32 in the reference (resnet_encoders.py:19)");
    REQUIRE(cfg->rgb_out % 4 == 0 && cfg->depth_out % 4 == 0, HCM_ERR_UNSUPPORTED, "encoder output sizes must be multiples of 4");
    h = new hcm_ctx();
    (void)hipGetDevice(&h->device);
    h->cfg = *cfg;
    h->dt = cfg->precision == HCM_BF16 ? DT_BF16 : cfg->precision == HCM_F16 ? DT_F16 : DT_F32;
    // per-sub-network storage type; reserved[0..3] = (dtype + 1) overrides for depth / bert / vla / rgb, 0 = default.
    //   HCM_F16:  all four store fp16 behind the range calibration (same MFMA rate as bf16, three more mantissa bits: DESIGN.md section 5);
    //   HCM_BF16: BERT and the cross-modal block store bf16 -- the two sub-networks that are NOT scale-invariant, i.e. where a trained model's
    //             range can genuinely ask for it (bert-base's outlier channels); BOTH trunk kinds stay on fp16 tiles, which their exact power-of-two
    //             range folds make safe by construction (GroupNorm depth trunk on bf16: 1.9e-2 of the 1e-2 record tolerance from that trunk alone;
    //             round 6: the BatchNorm-folded RGB trunks too -- their 50 bf16-rounded layers were 6e-3 of the mode's 9.7e-3, which left the
    //             1e-2 gate to the luck of the rounding draw: forcing FMA contraction in one LayerNorm (R5.12) or pinning -ffp-contract moved a case
    //             across it.  With the trunks on fp16 the mode's error is BERT's 6.9e-3 and the cross-modal block's 3.3e-3 in quadrature.)
    h->dt_rgb = h->dt_bert = h->dt_vla = h->dt_depth = h->dt;
    if (h->dt == DT_BF16) h->dt_depth = h->dt_rgb = DT_F16;
    {
        int* slots[4] = {&h->dt_depth, &h->dt_bert, &h->dt_vla, &h->dt_rgb};
        for (int i = 0; i < 4; ++i) {
            const int ov = cfg->reserved[i];
            if (ov == 0) continue;
            const int d = ov - 1;
            if (d != HCM_F32 && d != HCM_BF16 && d != HCM_F16) { delete h; h = nullptr; return fail(nullptr, HCM_ERR_ARG, "bad sub-network precision override"); }
            *slots[i] = d == HCM_F32 ? DT_F32 : d == HCM_BF16 ? DT_BF16 : DT_F16;
        }
    }
    try {
        if (cfg->build_high) build_spec_high(h);
        if (cfg->build_low) build_spec_low(h);
    } catch (const std::exception& e) {
        std::string m = e.what();
        delete h;
        h = nullptr;
        return fail(nullptr, HCM_ERR_ARG, m);
    }
    *out = h;
    return HCM_OK;
}

int hcm_cma_create(const hcm_cma_config* cfg, hcm_handle* out) {
    hcm_ctx* h = nullptr;
    REQUIRE(cfg && out, HCM_ERR_ARG, "hcm_cma_create: null argument");
    REQUIRE(cfg->struct_size == (int32_t)sizeof(hcm_cma_config), HCM_ERR_ARG, "hcm_cma_create: struct_size mismatch");
    REQUIRE(cfg->precision == HCM_F32 || cfg->precision == HCM_BF16 || cfg->precision == HCM_F16, HCM_ERR_ARG, "precision must be HCM_F32, HCM_F16 or HCM_BF16");
    REQUIRE(cfg->max_batch >= 1, HCM_ERR_ARG, "max_batch must be >= 1");
    REQUIRE(!cfg->use_prev_action && !cfg->rcm_state_encoder, HCM_ERR_UNSUPPORTED,
            "CMA.use_prev_action / CMA.rcm_state_encoder (default.py:211-212 default False) are not built");
    REQUIRE(!cfg->progress_monitor, HCM_ERR_UNSUPPORTED, "the progress monitor is a training-only auxiliary loss (cma.py:320-329)");
    REQUIRE(cfg->rnn_type == HCM_LSTM || cfg->rnn_type == HCM_GRU, HCM_ERR_ARG, "STATE_ENCODER.rnn_type must be LSTM or GRU");
    REQUIRE(cfg->instr_rnn == HCM_LSTM || cfg->instr_rnn == HCM_GRU, HCM_ERR_ARG, "INSTRUCTION_ENCODER.rnn_type must be LSTM or GRU (instruction_encoder.py:42)");
    REQUIRE(cfg->hidden >= 64 && cfg->hidden % 64 == 0, HCM_ERR_UNSUPPORTED, "hidden size must be a multiple of 64");
    REQUIRE(cfg->rgb_out <= cfg->hidden / 2 && cfg->depth_out <= cfg->hidden / 2, HCM_ERR_UNSUPPORTED,
            "CMANet: encoder output sizes must not exceed hidden / 2 (models/cma.py:281-286 unpacks torch.split(kv, hidden // 2) into two pieces)");
    REQUIRE(cfg->instr_hidden >= 4 && cfg->instr_hidden % 4 == 0 && cfg->embedding_size >= 1 && cfg->vocab_size >= 2, HCM_ERR_ARG,
            "bad INSTRUCTION_ENCODER sizes");
    REQUIRE(cfg->instr_len >= 1 && cfg->instr_len <= 256, HCM_ERR_UNSUPPORTED, "1 <= instr_len <= 256");
    REQUIRE(cfg->depth_h == cfg->depth_w, HCM_ERR_UNSUPPORTED, "depth frames must be square");
    REQUIRE(cfg->depth_h >= 64 && cfg->depth_h % 64 == 0 && cfg->depth_h <= 1024, HCM_ERR_UNSUPPORTED, "depth frame size must be a multiple of 64");
    REQUIRE(cfg->rgb_h >= 32 && cfg->rgb_w >= 32, HCM_ERR_UNSUPPORTED, "rgb frame too small");
    REQUIRE(cfg->depth_baseplanes == 32, HCM_ERR_UNSUPPORTED, "resnet_baseplanes is 32 in the reference (resnet_encoders.py:19)");
    REQUIRE(cfg->rgb_out % 4 == 0 && cfg->depth_out % 4 == 0 && cfg->num_actions >= 1, HCM_ERR_UNSUPPORTED, "bad output sizes");
    h = new hcm_ctx();
    (void)hipGetDevice(&h->device);
    h->kind = 1;
    h->cma_cfg = *cfg;
    std::memset(&h->cfg, 0, sizeof(h->cfg));
    hcm_config& c = h->cfg;                      // the fields the shared trunk / recurrent code reads
    c.struct_size = (int32_t)sizeof(hcm_config);
    c.precision = cfg->precision; c.max_batch = cfg->max_batch;
    c.rgb_h = cfg->rgb_h; c.rgb_w = cfg->rgb_w; c.depth_h = cfg->depth_h; c.depth_w = cfg->depth_w; c.instr_len = cfg->instr_len;
    c.rgb_encoder = c.depth_encoder = HCM_ENC_RESNET;
    c.rgb_out = cfg->rgb_out; c.depth_out = cfg->depth_out; c.depth_baseplanes = cfg->depth_baseplanes;
    c.hidden = cfg->hidden; c.rnn_type = cfg->rnn_type; c.num_actions = cfg->num_actions;
    h->dt = cfg->precision == HCM_BF16 ? DT_BF16 : cfg->precision == HCM_F16 ? DT_F16 : DT_F32;
    h->dt_rgb = h->dt_bert = h->dt_vla = h->dt_depth = h->dt;
    // trunks as in the HCM handle: HCM_F16 both on range-calibrated fp16 tiles, HCM_BF16 the RGB trunk on bf16; the token-side
    // projections (dt_vla) follow the RGB trunk's type
    if (h->dt == DT_BF16) h->dt_depth = DT_F16;
    try {
        build_spec_cma(h);
    } catch (const std::exception& e) {
        std::string m = e.what();
        delete h;
        h = nullptr;
        return fail(nullptr, HCM_ERR_ARG, m);
    }
    *out = h;
    return HCM_OK;
}

int hcm_s2s_create(const hcm_s2s_config* cfg, hcm_handle* out) {
    hcm_ctx* h = nullptr;
    REQUIRE(cfg && out, HCM_ERR_ARG, "hcm_s2s_create: null argument");
    REQUIRE(cfg->struct_size == (int32_t)sizeof(hcm_s2s_config), HCM_ERR_ARG, "hcm_s2s_create: struct_size mismatch");
    REQUIRE(cfg->precision == HCM_F32 || cfg->precision == HCM_BF16 || cfg->precision == HCM_F16, HCM_ERR_ARG, "precision must be HCM_F32, HCM_F16 or HCM_BF16");
    REQUIRE(cfg->max_batch >= 1, HCM_ERR_ARG, "max_batch must be >= 1");
    // settings the reference's Seq2SeqNet cannot run, or that select a module that is not built
    REQUIRE(!cfg->bidirectional, HCM_ERR_UNSUPPORTED,
            "INSTRUCTION_ENCODER.bidirectional with final_state_only returns a (2,B,H) state (instruction_encoder.py:90) and Seq2SeqNet raises at seq2seq.py:163");
    REQUIRE(!cfg->use_prev_action, HCM_ERR_UNSUPPORTED,
            "SEQ2SEQ.use_prev_action (config/default.py:202 default False) is not built: the reference raises at the cat of seq2seq.py:167-171");
    REQUIRE(!cfg->is_bert, HCM_ERR_UNSUPPORTED, "INSTRUCTION_ENCODER.is_bert selects LanguageEncoder (seq2seq.py:45-46), which is not built");
    REQUIRE(cfg->rnn_type == HCM_LSTM || cfg->rnn_type == HCM_GRU, HCM_ERR_ARG, "STATE_ENCODER.rnn_type must be LSTM or GRU");
    REQUIRE(cfg->instr_rnn == HCM_LSTM || cfg->instr_rnn == HCM_GRU, HCM_ERR_ARG, "INSTRUCTION_ENCODER.rnn_type must be LSTM or GRU (instruction_encoder.py:42)");
    REQUIRE(cfg->rgb_encoder == HCM_ENC_RESNET || cfg->rgb_encoder == HCM_ENC_SIMPLECNN, HCM_ERR_ARG, "RGB_ENCODER.cnn_type must be SimpleRGBCNN or TorchVisionResNet50 (seq2seq.py:67-70)");
    REQUIRE(cfg->depth_encoder == HCM_ENC_RESNET || cfg->depth_encoder == HCM_ENC_SIMPLECNN, HCM_ERR_ARG, "DEPTH_ENCODER.cnn_type must be SimpleDepthCNN or VlnResnetDepthEncoder (seq2seq.py:50-53)");
    REQUIRE(cfg->hidden >= 64 && cfg->hidden % 64 == 0, HCM_ERR_UNSUPPORTED, "hidden size must be a multiple of 64");
    REQUIRE(cfg->instr_hidden >= 64 && cfg->instr_hidden % 64 == 0 && cfg->instr_hidden <= 512, HCM_ERR_UNSUPPORTED,
            "INSTRUCTION_ENCODER.hidden_size must be a multiple of 64 up to 512");
    REQUIRE(cfg->embedding_size >= 1 && cfg->vocab_size >= 2 && cfg->num_sub_tasks >= 1 && cfg->num_actions >= 1, HCM_ERR_ARG, "bad INSTRUCTION_ENCODER / head sizes");
    REQUIRE(cfg->instr_len >= 1 && cfg->instr_len <= 256, HCM_ERR_UNSUPPORTED, "1 <= instr_len <= 256");
    REQUIRE(cfg->depth_h == cfg->depth_w || cfg->depth_encoder == HCM_ENC_SIMPLECNN, HCM_ERR_UNSUPPORTED, "depth frames must be square with the ResNet depth encoder");
    if (cfg->rgb_encoder == HCM_ENC_SIMPLECNN) REQUIRE(cfg->rgb_h >= 36 && cfg->rgb_w >= 36, HCM_ERR_UNSUPPORTED, "SimpleRGBCNN: rgb frame too small");
    else REQUIRE(cfg->rgb_h >= 32 && cfg->rgb_w >= 32, HCM_ERR_UNSUPPORTED, "rgb frame too small");
    if (cfg->depth_encoder == HCM_ENC_SIMPLECNN) REQUIRE(cfg->depth_h >= 36 && cfg->depth_w >= 36, HCM_ERR_UNSUPPORTED, "SimpleDepthCNN: depth frame too small");
    else REQUIRE(cfg->depth_h >= 64 && cfg->depth_h % 64 == 0 && cfg->depth_h <= 1024, HCM_ERR_UNSUPPORTED,
                 "depth frame size must be a multiple of 64 (habitat's ResNetEncoder: final map (H/2)/32, resnet_encoders.py:37-62)");
    REQUIRE(cfg->depth_baseplanes == 32, HCM_ERR_UNSUPPORTED, "resnet_baseplanes is 32 in the reference (resnet_encoders.py:19)");
    REQUIRE(cfg->rgb_out % 4 == 0 && cfg->depth_out % 4 == 0 && cfg->rgb_out >= 4 && cfg->depth_out >= 4, HCM_ERR_UNSUPPORTED, "encoder output sizes must be multiples of 4");
    h = new hcm_ctx();
    (void)hipGetDevice(&h->device);
    h->kind = 2;
    h->s2s_cfg = *cfg;
    std::memset(&h->cfg, 0, sizeof(h->cfg));
    hcm_config& c = h->cfg;                      // the fields the shared trunk / recurrent code reads
    c.struct_size = (int32_t)sizeof(hcm_config);
    c.precision = cfg->precision; c.max_batch = cfg->max_batch;
    c.rgb_h = cfg->rgb_h; c.rgb_w = cfg->rgb_w; c.depth_h = cfg->depth_h; c.depth_w = cfg->depth_w; c.instr_len = cfg->instr_len;
    c.rgb_encoder = cfg->rgb_encoder; c.depth_encoder = cfg->depth_encoder;
    c.rgb_out = cfg->rgb_out; c.depth_out = cfg->depth_out; c.depth_baseplanes = cfg->depth_baseplanes;
    c.hidden = cfg->hidden; c.rnn_type = cfg->rnn_type; c.num_actions = cfg->num_actions; c.lo_actions = cfg->num_actions; c.num_sub_tasks = cfg->num_sub_tasks;
    h->dt = cfg->precision == HCM_BF16 ? DT_BF16 : cfg->precision == HCM_F16 ? DT_F16 : DT_F32;
    h->dt_rgb = h->dt_bert = h->dt_vla = h->dt_depth = h->dt;
    if (h->dt == DT_BF16) h->dt_depth = h->dt_rgb = DT_F16;          // both trunk kinds on range-folded fp16 tiles, as in the HCM handle's bf16 mode
    try {
        build_spec_s2s(h);
    } catch (const std::exception& e) {
        std::string m = e.what();
        delete h;
        h = nullptr;
        return fail(nullptr, HCM_ERR_ARG, m);
    }
    *out = h;
    return HCM_OK;
}

int hcm_load_tensor(hcm_handle h, int model, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(!h->finalized, HCM_ERR_STATE, "hcm_load_tensor after hcm_finalize");
    if (h->kind == 1) REQUIRE(model == HCM_CMA, HCM_ERR_ARG, "a CMANet handle takes model = HCM_CMA");
    else if (h->kind == 2) REQUIRE(model == HCM_S2S, HCM_ERR_ARG, "a Seq2SeqNet handle takes model = HCM_S2S");
    else REQUIRE(model == HCM_HIGH || model == HCM_LOW, HCM_ERR_ARG, "model must be HCM_HIGH or HCM_LOW");
    REQUIRE(key && data && (shape || ndim == 0), HCM_ERR_ARG, "null argument");
    auto& sd = h->sd[model];
    auto it = sd.find(key);
    REQUIRE(it != sd.end(), HCM_ERR_KEY, std::string("Unexpected key in state_dict: ") + key);
    HostTensor& t = it->second;
    bool same = (int)t.shape.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = t.shape[i] == shape[i];
    if (!same) {
        std::string m = std::string("size mismatch for ") + key + ": expected (";
        for (auto d : t.shape) m += std::to_string(d) + ",";
        m += ") got (";
        for (int i = 0; i < ndim; ++i) m += std::to_string(shape[i]) + ",";
        return fail(h, HCM_ERR_SHAPE, m + ")");
    }
    size_t n = 1;
    for (auto d : t.shape) n *= (size_t)d;
    t.f.resize(n);
    if (dtype == HCM_F32) std::memcpy(t.f.data(), data, n * 4);
    else if (dtype == HCM_I64) for (size_t i = 0; i < n; ++i) t.f[i] = (float)((const int64_t*)data)[i];
    else return fail(h, HCM_ERR_ARG, "hcm_load_tensor: dtype must be HCM_F32 or HCM_I64");
    t.loaded = true;
    return HCM_OK;
}

// Workspace sizing: the forward code is run in "dry" mode (allocations only) for every entry shape and the arena gets the largest
// peak: the single step at max_batch, the sequence path at T = 2 and 3 (its scan keeps ping-pong state buffers on top of the
// per-step scratch; larger T only shrink N = max_batch / T), each model alone (hcm_high_forward / hcm_low_forward take un-paired
// trunk paths), all at the maximum instruction length (every allocation is monotone in L).
static void dry_run(hcm_ctx* h, int B) {
    h->arena.dry = true;
    h->arena.peak = 0;
    FwdCall c;                                             // every pointer null: allocations only
    c.L = h->cfg.instr_len;
    // Every shape is sized in its frame form and in its hcm_features form (a stand-in address, never read in a dry pass, in every slot a ResNet
    // trunk can take a feature for: the ingest buffers instead of the trunks').  hcm_encode_features: below, once at B rows.
    const float* const stand_in = (const float*)0x1000;
    auto run = [&](int rows, int T, FwdCall::Val val = FwdCall::kNoVal) {
        c.rows = c.Bi = rows; c.T = T; c.val = val;
        for (const float* f : {(const float*)nullptr, stand_in}) {
            c.rgb_feat[0] = c.rgb_feat[1] = c.depth_feat[0] = c.depth_feat[1] = f;
            run_forward(h, c);
        }
        c.rgb_feat[0] = c.rgb_feat[1] = c.depth_feat[0] = c.depth_feat[1] = nullptr;
    };
    {
        FwdCall e;
        e.encode = true; e.rows = B;
        for (bool act : {false, true}) { e.enc_act = act; run_forward(h, e); }
    }
    if (h->kind == 0 && h->cfg.build_high) {               // hcm_encode_instruction: BERT alone at B rows (a subset of the step's buffers; sized all the same)
        FwdCall e;
        e.encode_instr = true; e.rows = B; e.L = h->cfg.instr_len;
        run_forward(h, e);
    }
    if (h->kind == 1) {
        run(B, 1);
        // hcm_cma_forward_seq: the scans' buffers on top of the step's.  What they hold grows with the rows (the projections, both sequence
        // buffers: T = B, N = 1 has all B rows whatever B's divisors) or with N (the per-step path's ping-pong state: largest at T = 2)
        for (int T : {2, 3, B})
            if (T >= 2 && T <= B) run(B / T * T, T);
        // hcm_flat_val_step: the same shapes with every optional output row (out, stop) in the workspace
        for (int T : {1, 2, 3, B})
            if (T <= B) run(B / T * T, T, FwdCall::kFlatVal);
        return;
    }
    if (h->kind == 2) {                                // the step with one instruction per row, and the sequence path at T = 2, 3 (as below)
        for (int T = 1; T <= 3 && T <= B; ++T) {
            run(B / T * T, T);
            // hcm_flat_val_step: out, stop and -- with the progress monitor, whose head runs whether or not its rows are wanted -- progress_hat in the workspace
            run(B / T * T, T, FwdCall::kFlatVal);
        }
        return;
    }
    const bool hi = h->cfg.build_high != 0, lo = h->cfg.build_low != 0;
    for (int T = 1; T <= 3 && T <= B; ++T) {
        const int rows = B / T * T;
        for (int which = 0; which < 3; ++which) {          // both (the fused step) / high alone / low alone
            c.do_hi = hi && which != 2; c.do_lo = lo && which != 1;
            if ((which == 0 && !(hi && lo)) || (which == 1 && !hi) || (which == 2 && !lo)) continue;
            // hcm_val_step runs both models on T*N rows; also at T = 1 (its trunks are never shared, and it keeps its own label / output rows)
            if (which == 0) run(rows, T, FwdCall::kVal);
            if (which == 0 && T > 1) continue;             // the fused step has no sequence form
            run(rows, T);
        }
    }
    // hcm_refresh_instruction of every environment at once: a second BERT / instruction-stream scratch set on top of the persistent
    // step tensors -- with small frames and a long instruction that is more than any step needs
    if (hi && lo) {
        const size_t peak = h->arena.peak;
        c.rows = B;
        run_refresh_instruction(h, c, nullptr, B);
        if (h->arena.peak < peak) h->arena.peak = peak;
    }
}

// ---- fp16 range calibration: BERT and the GroupNorm depth trunks store activations as fp16 (3 more mantissa
// bits than bf16 at the same MFMA rate, needed for the 1e-2 record tolerance), whose range ends at 65504.  One forward with the range
// hooks on measures max |x| over every GEMM output of those sub-networks; a sub-network whose maximum exceeds 2^14 (a factor 4 of
// head-room) or that produced a non-finite value is re-built on bf16 tiles (same range as fp32) and the fact is reported through
// hcm_query(HCM_FP16_FALLBACK).
static void free_device_weights(hcm_ctx* h) {
    for (void* p : h->dev_allocs) (void)hipFree(p);
    h->dev_allocs.clear();
    h->weight_bytes = 0;
    h->hi = hcm::HighW();
    h->lo = hcm::LowW();
    h->s2s = hcm::S2sW();
}
// calibrate_run / the tuning step of hcm_finalize: whatever the handle holds, once, on the B rows of `c` with scratch state and outputs
static FwdCall scratch_call(hcm_ctx* h, FwdCall c, float* hh, float* lh, float* hh2, float* lh2, float* mask, float* rec, const int64_t* subtask) {
    const hcm_config& g = h->cfg;
    c.mask = mask;
    if (h->kind != 0) { c.lo_h_in = hh; c.lo_h_out = hh2; c.vel = rec; c.stop = rec + 8 * (size_t)c.rows; return c; }
    c.do_hi = g.build_high != 0; c.do_lo = g.build_low != 0;
    if (c.do_hi) { c.hi_h_in = hh; c.hi_h_out = hh2; c.logits = rec; c.ld_logits = c.do_lo ? 7 : g.num_actions; }
    if (c.do_lo) { c.lo_h_in = lh; c.lo_h_out = lh2; c.vel = c.do_hi ? rec + 4 : rec; c.ld_vel = c.do_hi ? 7 : g.lo_actions; c.stop = c.do_hi ? rec + 6 : rec + 8; c.ld_stop = c.do_hi ? 7 : 1; }
    if (!c.do_hi) { c.ids = nullptr; c.ids_dt = DT_I64; c.subtask = subtask; }
    return c;
}
static int calibrate_run(hcm_ctx* h, const void* rgb, int rgb_dt, const float* depth, const void* ids, int ids_dt, int B, int L, hipStream_t stream,
                         int pass = 0) {
    const hcm_config& c = h->cfg;
    if (h->dt_bert != DT_F16 && h->dt_depth != DT_F16 && h->dt_rgb != DT_F16 && h->dt_vla != DT_F16) return HCM_OK;          // nothing stored as fp16
    const size_t R = (c.rnn_type == HCM_LSTM ? 2 : 1) * (h->kind == 1 ? 2 : 1);        // CMANet: two state encoders in one tensor
    const size_t n_hid = R * (size_t)B * c.hidden * 4;
    char* tmp = nullptr;
    const size_t total = 4 * n_hid + (size_t)B * 17 * 4 + 8 + (size_t)B * 8 + 4096;
    if (hipMalloc((void**)&tmp, total) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc of calibration scratch failed");
    (void)hipMemsetAsync(tmp, 0, total, stream);
    float* hh = (float*)tmp; float* lh = (float*)(tmp + n_hid); float* hh2 = (float*)(tmp + 2 * n_hid); float* lh2 = (float*)(tmp + 3 * n_hid);
    float* mask = (float*)(tmp + 4 * n_hid); float* rec = mask + B;
    int64_t* st = (int64_t*)(((uintptr_t)(rec + 16 * (size_t)B) + 7) & ~(uintptr_t)7);      // 8-byte aligned for every B
    (void)hipMemsetAsync(h->calib_buf, 0, 32, stream);
    (void)hipMemsetAsync(h->calib_buf + 16, 0, (hcm_ctx::kCalibWords - 16) * 4, stream);
    const bool conc = h->concurrent;
    h->concurrent = false;                       // one stream: the hooks are plain launches in program order
    h->calib = true;
    drop_instruction_cache(h);
    std::string err;
    try {
        run_forward(h, scratch_call(h, frames(rgb, rgb_dt, depth, ids, ids_dt, B, L, stream), hh, lh, hh2, lh2, mask, rec, st));
    } catch (const std::exception& e) { err = e.what(); }
    h->calib = false;
    h->concurrent = conc;
    unsigned out[hcm_ctx::kCalibWords];
    std::memset(out, 0, sizeof(out));
    const hipError_t se = hipStreamSynchronize(stream);
    if (se == hipSuccess) (void)hipMemcpy(out, h->calib_buf, sizeof(out), hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    if (!err.empty()) return fail(h, HCM_ERR_HIP, "calibration forward failed: " + err);
    if (se != hipSuccess) return fail(h, HCM_ERR_HIP, "calibration forward failed to complete");
    int rebuild = 0;
    for (int i = 0; i < 4; ++i) {
        std::memcpy(&h->calib_max[i], &out[2 * i], 4);
        h->calib_bad[i] = out[2 * i + 1];
        const bool is_f16 = (i == 0 ? h->dt_bert : i == 1 ? h->dt_depth : i == 2 ? h->dt_rgb : h->dt_vla) == DT_F16;
        if (is_f16 && (h->calib_bad[i] || h->calib_max[i] > 16384.0f)) rebuild |= 1 << i;
    }
    // NaN / inf travel downstream (ReLU, pools and the variance clamps propagate them, dev.h max_nan): non-finite values in the
    // cross-modal block while one of its three inputs was already non-finite say nothing about the block itself -- re-build the source
    // first; the forward below this re-build judges the block on clean inputs
    if ((rebuild & 8) && (rebuild & 7) && (h->calib_bad[0] || h->calib_bad[1] || h->calib_bad[2])) rebuild &= ~8;
    // Range folding, where the network is exactly scale-invariant, instead of giving up fp16 (include/hcm.h, hcm_calibrate):
    int refold = 0;                 // bit 1 / bit 2: the depth / RGB trunks are re-built with new folds, on the same storage type
    auto pow2_down = [](float v, float target) { int e = 0; while (v > target && e < 60) { v *= 0.5f; ++e; } return std::ldexp(1.0f, -e); };
    const bool has_gn_trunk = h->kind == 1 || h->cfg.depth_encoder == HCM_ENC_RESNET;
    const bool has_bn_trunk = h->kind == 1 || h->cfg.rgb_encoder == HCM_ENC_RESNET || (h->cfg.build_high != 0);
    if ((rebuild & 2) && has_gn_trunk) {
        // GroupNorm depth trunks: per conv position, the un-normalised conv output (the only tensor there that can grow without bound).
        // Finite overflows are folded down to <= 2^10 in one go; of the positions that went non-finite only the FIRST is touched (2^-16, re-centred
        // by a later pass): everything behind it saw its NaNs.  An overflow with no position to blame sits behind a GroupNorm (huge gamma)
        // or in the low-level model's SimpleCNN: bf16 as before.
        bool any = false;
        int first_bad = -1;
        for (int pos = 0; pos < hcm_ctx::kDepthPos; ++pos) {
            float mx; std::memcpy(&mx, &out[16 + 2 * pos], 4);
            const unsigned bad = out[16 + 2 * pos + 1];
            if (bad) { if (first_bad < 0) first_bad = pos; continue; }
            if (first_bad >= 0) continue;                                  // finite, but computed from non-finite inputs further up?  no: bad would be set
            if (mx > 16384.0f) { h->depth_fold[pos] *= pow2_down(mx, 1024.0f); any = true; }
        }
        if (first_bad >= 0 && h->depth_fold[first_bad] > 1e-12f) { h->depth_fold[first_bad] *= 1.0f / 65536.0f; any = true; }
        if (any) { refold |= 2; rebuild &= ~2; }
    }
    if (h->dt_depth == DT_F16 && !(rebuild & 2) && has_gn_trunk) {
        // re-centre a position whose (blind, 2^-16) fold left its values far below the range: back up to <= 2^10, never above the unfolded scale
        for (int pos = 0; pos < hcm_ctx::kDepthPos; ++pos) {
            float mx; std::memcpy(&mx, &out[16 + 2 * pos], 4);
            if (h->depth_fold[pos] >= 1.f || out[16 + 2 * pos + 1] || !(mx > 0.f) || mx >= 256.0f) continue;
            float f = h->depth_fold[pos];
            while (f < 1.f && mx * 2.f <= 1024.0f) { f *= 2.f; mx *= 2.f; }
            if (f != h->depth_fold[pos]) { h->depth_fold[pos] = f; refold |= 2; }
        }
    }
    if ((rebuild & 4) && has_bn_trunk && h->rgb_fold > 1e-7f) {
        // BatchNorm-folded RGB trunks: one power of two on every activation (target: the largest <= 2^12, so that the small early maps keep their
        // distance from fp16's sub-normal floor).  Non-finite: 2^-8 per pass.  Gives up (bf16) below 2^-23.
        h->rgb_fold *= h->calib_bad[2] ? 1.0f / 256.0f : pow2_down(h->calib_max[2], 4096.0f);
        refold |= 4; rebuild &= ~4;
        // the cross-modal block's verdict was formed on the unfolded features: judge it again behind the folded trunk
        if ((rebuild & 8) && !h->calib_bad[0] && !h->calib_bad[1]) rebuild &= ~8;
    }
    // A chain of range folds that has not converged after kFoldPasses passes (each pass repairs only the FIRST non-finite position of the depth
    // trunk; a fold can also bottom out) stops here: the trunk(s) still asking for a fold move to bf16 tiles -- always safe -- with their folds
    // cleared, and the passes that remain only measure.  Without this the last re-build was applied but never measured and the handle reported
    // success with stale ranges (round-3 advisor).
    constexpr int kFoldPasses = 12, kMaxPasses = 16;
    if (pass >= kFoldPasses && refold) {
        if (refold & 2) rebuild |= 2;
        if (refold & 4) rebuild |= 4;
        refold = 0;
    }
    if (!rebuild && !refold) return HCM_OK;
    if (pass >= kMaxPasses)
        return fail(h, HCM_ERR_STATE, "fp16 range calibration did not converge within " + std::to_string(kMaxPasses) + " passes (max |x| " +
                    std::to_string(h->calib_max[0]) + " BERT / " + std::to_string(h->calib_max[1]) + " depth / " + std::to_string(h->calib_max[2]) +
                    " RGB / " + std::to_string(h->calib_max[3]) + " cross-modal): create the engine with precision bf16");
    if (!h->host_weights)
        return fail(h, HCM_ERR_STATE, "fp16 range exceeded (max |x| " + std::to_string(h->calib_max[0]) + " BERT / " + std::to_string(h->calib_max[1]) +
                    " depth / " + std::to_string(h->calib_max[2]) + " RGB / " + std::to_string(h->calib_max[3]) + " cross-modal) but the host copies of the weights were released: create the engine with keep_host_weights or a bf16 sub-precision");
    // a trunk that leaves fp16 does not need (and no longer reports) a range fold -- cleared only now, behind the checks that can still fail the
    // call: on those error paths the device weights are still the folded ones and hcm_query(HCM_RANGE_FOLD) keeps saying so (round-4 advisor)
    if (rebuild & 2) { for (int pos = 0; pos < hcm_ctx::kDepthPos; ++pos) h->depth_fold[pos] = 1.f; h->range_fold &= ~2; }
    if (rebuild & 4) { h->rgb_fold = 1.f; h->range_fold &= ~4; }
    if (rebuild & 1) h->dt_bert = DT_BF16;
    if (rebuild & 2) h->dt_depth = DT_BF16;
    if (rebuild & 4) h->dt_rgb = DT_BF16;
    if (rebuild & 8) h->dt_vla = DT_BF16;
    h->range_fold |= refold;
    (void)hipMemset(h->calib_buf + hcm_ctx::kStepBadWord, 0, 4);          // the overflow this forward ran into is being repaired: the step guard starts again
    h->fp16_fallback |= rebuild;
    for (auto& g : h->graphs) destroy_entry(g);                                   // captured with the old weight pointers
    h->graphs.clear();
    h->seen_keys.clear();
    try {
        free_device_weights(h);
        if (h->kind == 1) prepare_cma(h);
        else if (h->kind == 2) prepare_s2s(h);
        else {
            if (c.build_high) prepare_high(h);
            if (c.build_low) prepare_low(h);
        }
        // sub-networks of different storage types hand their tensors over through conversion buffers that a uniform-type plan does not have:
        // size the workspace again for the new plan
        dry_run(h, c.max_batch);
        h->arena.dry = false;
        if (h->arena.peak + 4096 > h->arena.cap) {
            if (stream) (void)hipStreamSynchronize(stream); else (void)hipDeviceSynchronize();
            (void)hipFree(h->arena.base);
            h->arena.base = nullptr;
            h->arena.cap = 0;
            const size_t want = h->arena.peak + 4096;
            if (hipMalloc((void**)&h->arena.base, want) != hipSuccess) {
                h->arena.base = nullptr;
                h->unusable = true;                // no workspace: every forward entry point now answers HCM_ERR_STATE instead of writing through a null base
                return fail(h, HCM_ERR_NOMEM, "hipMalloc of the workspace failed (" + std::to_string(want) + " bytes); the handle is unusable");
            }
            h->arena.cap = want;
        }
    } catch (const std::exception& e) {
        h->arena.dry = false;
        return fail(h, HCM_ERR_HIP, std::string("re-building a sub-network on bf16 tiles failed: ") + e.what());
    }
    // once more on the re-built engine: what was downstream of the overflow is measured on clean inputs now (the reported ranges are
    // those of the engine as it runs).  A sub-network moves to bf16 at most once; folds converge in a pass or two per position (one blind step
    // and one re-centring for a position that went non-finite), the pass limit bounds a pathological chain of them.
    return calibrate_run(h, rgb, rgb_dt, depth, ids, ids_dt, B, L, stream, pass + 1);       // bounded by kMaxPasses above: the last pass only measures
}
// deterministic synthetic calibration batch for hcm_finalize: frames of mid-range noise, ids spread over the vocabulary
static int calibrate_synthetic(hcm_ctx* h) {
    const hcm_config& c = h->cfg;
    const int B = c.max_batch < 2 ? 1 : 2, L = c.instr_len < 32 ? c.instr_len : 32;
    const size_t n_rgb = (size_t)B * c.rgb_h * c.rgb_w * 3, n_dep = (size_t)B * c.depth_h * c.depth_w, n_ids = (size_t)B * L;
    std::vector<unsigned char> rgb(n_rgb);
    std::vector<float> dep(n_dep);
    std::vector<int64_t> ids(n_ids);
    uint32_t s = 0x9E3779B9u;
    auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    for (auto& v : rgb) v = (unsigned char)(next() >> 24);
    for (auto& v : dep) v = (float)(next() >> 8) * (1.0f / 16777216.0f);
    if (h->kind == 1 || h->kind == 2) {
        const int vocab = h->kind == 1 ? h->cma_cfg.vocab_size : h->s2s_cfg.vocab_size;
        for (auto& v : ids) v = 1 + (int64_t)(next() % (uint32_t)(vocab > 2 ? vocab - 1 : 1));      // the model's own vocabulary, no padding
    } else {
        for (auto& v : ids) v = 1000 + (int64_t)(next() % (uint32_t)(c.bert_vocab > 1001 ? c.bert_vocab - 1000 : 1));
        for (int b = 0; b < B; ++b) { ids[(size_t)b * L] = 101; ids[(size_t)b * L + L - 1] = 102; }
    }
    char* d = nullptr;
    if (hipMalloc((void**)&d, n_rgb + n_dep * 4 + n_ids * 8 + 64) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc of the calibration batch failed");
    char* d_dep = d + ((n_rgb + 15) & ~(size_t)15);
    char* d_ids = d_dep + n_dep * 4;
    (void)hipMemcpy(d, rgb.data(), n_rgb, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_dep, dep.data(), n_dep * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_ids, ids.data(), n_ids * 8, hipMemcpyHostToDevice);
    const int rc = calibrate_run(h, d, HCM_U8, (const float*)d_dep, d_ids, HCM_I64, B, L, nullptr);
    (void)hipDeviceSynchronize();
    (void)hipFree(d);
    return rc;
}

int hcm_finalize(hcm_handle h) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(!h->finalized, HCM_ERR_STATE, "hcm_finalize called twice");
    for (int m = 0; m < hcm_ctx::kModels; ++m)
        for (auto& kv : h->sd[m])
            if (!kv.second.loaded) return fail(h, HCM_ERR_KEY, std::string("Missing key in state_dict: ") + kv.first);
    try {
        if (h->kind == 1) {
            prepare_cma(h);
            if (hipMalloc((void**)&h->len_buf, (size_t)h->cfg.max_batch * sizeof(int)) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc failed");
        }
        if (h->kind == 2) {
            prepare_s2s(h);
            if (hipMalloc((void**)&h->len_buf, (size_t)h->cfg.max_batch * sizeof(int)) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc failed");
        }
        if (h->cfg.build_high) prepare_high(h);
        if (h->cfg.build_low) prepare_low(h);
        dry_run(h, h->cfg.max_batch);
        h->arena.cap = h->arena.peak + 4096;
        if (hipMalloc((void**)&h->arena.base, h->arena.cap) != hipSuccess)
            return fail(h, HCM_ERR_NOMEM, "hipMalloc of the workspace failed (" + std::to_string(h->arena.cap) + " bytes)");
        if (hipMalloc((void**)&h->pred_buf, (size_t)h->cfg.max_batch * sizeof(int64_t)) != hipSuccess)
            return fail(h, HCM_ERR_NOMEM, "hipMalloc failed");
        h->arena.dry = false;
        for (int i = 0; i < 4; ++i) {
            const hipError_t ce = hipStreamCreateWithFlags(&h->aux[i], hipStreamNonBlocking);
            if (ce != hipSuccess) return fail(h, HCM_ERR_HIP, "hipStreamCreate failed");
            if (hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipEventCreate failed");
        }
        for (auto& p : h->pool)
            if (hipStreamCreateWithFlags(&p, hipStreamNonBlocking) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipStreamCreate failed");
        if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipEventCreate failed");
        if (const char* e = getenv("HCM_SERIAL")) h->concurrent = atoi(e) == 0;
        if (const char* e = getenv("HCM_GRAPH")) h->use_graph = atoi(e) != 0;
        if (dev_env("HCM_MARKS")) {          // development build only: wall-clock stamps inside the step (hcm_debug_marks)
            if (hipMalloc((void**)&h->marks_dev, 256 * 8) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc failed");
            (void)hipMemset(h->marks_dev, 0, 256 * 8);
        }
        if (hipMalloc((void**)&h->calib_buf, hcm_ctx::kCalibWords * 4) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc failed");
        if (hipMemset(h->calib_buf, 0, hcm_ctx::kCalibWords * 4) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipMemset failed");       // words 0-7: calibration, 12: step guard, 16..: conv positions
        // fp16 range check on a synthetic batch; a real batch can follow through hcm_calibrate (reserved[4]: keep the host weights for it)
        if (!getenv("HCM_NO_CALIB")) {
            const int rc = calibrate_synthetic(h);
            if (rc != HCM_OK) return rc;
        }
        // one tuning step at max_batch on scratch inputs: every conv / linear shape of the plan picks its fastest
        // tile + staging variant (igemm.hip); steady-state calls then never synchronise the host
        // (opt-in: HCM_TUNE=1.  Isolated per-kernel timings rank variants differently from the concurrent multi-stream
        //  schedule, where the built-in heuristic measured faster end to end)
        const char* nt = dev_env("HCM_TUNE");
        if (nt && atoi(nt) && h->kind == 0) {
            const hcm_config& c = h->cfg;
            const size_t B = c.max_batch, R = c.rnn_type == HCM_LSTM ? 2 : 1;
            const size_t n_rgb = B * c.rgb_h * c.rgb_w * 3 * 4, n_dep = B * c.depth_h * c.depth_w * 4, n_ids = B * c.instr_len * 8;
            const size_t n_hid = R * B * c.hidden * 4, n_misc = B * 16 * 4;
            char* tmp = nullptr;
            const size_t total = n_rgb + n_dep + n_ids + 4 * n_hid + 2 * n_misc + 4096;
            if (hipMalloc((void**)&tmp, total) != hipSuccess) return fail(h, HCM_ERR_NOMEM, "hipMalloc of tuning scratch failed");
            (void)hipMemset(tmp, 0, total);
            (void)hipMemset(tmp, 0x3C, n_rgb + n_dep);                  // small positive f32 pattern for the frames
            char* p = tmp;
            void* rgb = p; p += n_rgb;
            float* dep = (float*)p; p += n_dep;
            void* ids = p; p += n_ids;
            float* hh = (float*)p; p += n_hid;
            float* lh = (float*)p; p += n_hid;
            float* hh2 = (float*)p; p += n_hid;
            float* lh2 = (float*)p; p += n_hid;
            float* mask = (float*)p; p += n_misc;
            float* rec = (float*)p;
            const bool conc = h->concurrent;
            h->concurrent = false;
            igemm_set_tuning(true);
            std::string terr;
            try {
                run_forward(h, scratch_call(h, frames(rgb, DT_F32, dep, ids, DT_I64, (int)B, c.instr_len, nullptr), hh, lh, hh2, lh2, mask, rec, (const int64_t*)ids));
            } catch (const std::exception& e) { terr = e.what(); }
            igemm_set_tuning(false);
            h->concurrent = conc;
            (void)hipDeviceSynchronize();
            (void)hipFree(tmp);
            if (!terr.empty()) return fail(h, HCM_ERR_HIP, "tuning step failed: " + terr);
        }
    } catch (const std::exception& e) {
        return fail(h, HCM_ERR_HIP, std::string("hcm_finalize: ") + e.what());
    }
    // host copies are no longer needed -- unless the caller wants to calibrate on its own observations (hcm_config.reserved[4])
    if (!h->cfg.reserved[4]) {
        for (int m = 0; m < hcm_ctx::kModels; ++m)
            for (auto& kv : h->sd[m]) { std::vector<float>().swap(kv.second.f); }
        h->host_weights = false;
    }
    h->finalized = true;
    return HCM_OK;
}

int hcm_calibrate(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int L, void* stream) {
    int rc = check_fwd(h, B);
    if (rc) return rc;
    const bool needs_ids = h->kind == 1 || h->kind == 2 || h->cfg.build_high;
    REQUIRE(rgb_dtype != HCM_FEATURES, HCM_ERR_ARG,
            "hcm_calibrate with HCM_FEATURES: the calibration measures the ranges inside the trunks and needs them to run -- pass the frames (the reference "
            "has no counterpart: resnet_encoders.py:83-86, :207-214 skip the trunk when the feature key is there)");
    REQUIRE(ids_dtype != HCM_INSTR_FEATURES, HCM_ERR_ARG,
            "hcm_calibrate with HCM_INSTR_FEATURES: the calibration measures the ranges inside BERT and needs it to run -- pass the token ids");
    REQUIRE(rgb && depth && (ids || !needs_ids), HCM_ERR_ARG, "null pointer");
    REQUIRE(rgb_dt_ok(rgb_dtype) && ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    if (needs_ids && (rc = check_len(h, L))) return rc;
    rc = calibrate_run(h, rgb, rgb_dtype, depth, ids, ids_dtype, B, needs_ids ? L : 1, (hipStream_t)stream);
    // The overflow guard's polled view starts again from what the device word holds NOW (a re-build zeroed it; a measuring pass may have added to it):
    // a value cached by an earlier hcm_guard_poll -- or still in flight to the host -- would otherwise come back as a new alarm for steps that were
    // already reported (round-4 advisor).  hcm_calibrate is a construction-time call; the synchronous read costs nothing that matters.
    if (h->guard_host) {
        if (h->guard_pending) (void)hipEventSynchronize(h->guard_ev);
        h->guard_pending = false;
        unsigned v = 0;
        if (hipStreamSynchronize((hipStream_t)stream) == hipSuccess &&
            hipMemcpy(&v, h->calib_buf + hcm_ctx::kStepBadWord, 4, hipMemcpyDeviceToHost) == hipSuccess) { h->guard_last = v; *h->guard_host = v; }
    }
    return rc;
}

int hcm_release_host_weights(hcm_handle h) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    for (int m = 0; m < hcm_ctx::kModels; ++m)
        for (auto& kv : h->sd[m]) { std::vector<float>().swap(kv.second.f); }
    h->host_weights = false;
    return HCM_OK;
}

// ---- the forward entry points: each makes its own checks, fills a descriptor (model.h, FwdCall) and runs it
static int check_fwd(hcm_ctx* h, int B) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(h->finalized, HCM_ERR_STATE, "forward before hcm_finalize");
    REQUIRE(!h->unusable, HCM_ERR_STATE, "the handle lost its workspace in a failed re-build (hcm_calibrate): destroy it");
    REQUIRE(B >= 1 && B <= h->cfg.max_batch, HCM_ERR_ARG, "batch must be in [1, max_batch]");
    return HCM_OK;
}
static int check_len(hcm_ctx* h, int L) {
    REQUIRE(L >= 1 && L <= h->cfg.instr_len, HCM_ERR_ARG,
            "instruction length " + std::to_string(L) + " outside [1, " + std::to_string(h->cfg.instr_len) + "] (hcm_config.instr_len is the maximum L)");
    return HCM_OK;
}
// shape of a sequence call; the product in 64 bits, so that no T * N can wrap its way past max_batch
static int check_seq(hcm_ctx* h, int T, int N) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(T >= 1 && N >= 1, HCM_ERR_ARG, "T and N must be >= 1");
    REQUIRE((int64_t)T * N <= h->cfg.max_batch, HCM_ERR_ARG, "T*N must not exceed max_batch");
    return HCM_OK;
}
// every entry point other than hcm_act_ex re-uses the workspace region that holds the cached instruction stream
static void drop_instruction_cache(hcm_ctx* h) { h->last_hi_batch = -1; h->last_hi_L = -1; }

static bool rgb_dt_ok(int d) { return d == HCM_F32 || d == HCM_U8; }
static bool ids_dt_ok(int d) { return d == HCM_F32 || d == HCM_I32 || d == HCM_I64; }

// the observation part of a descriptor
static FwdCall frames(const void* rgb, int rgb_dt, const float* depth, const void* ids, int ids_dt, int rows, int L, void* stream) {
    FwdCall c;
    if (rgb_dt == HCM_FEATURES && rgb) {                   // `rgb` is a host hcm_features: frames and features travel in it (check_obs judges them)
        const hcm_features* f = (const hcm_features*)rgb;
        c.rgb = f->rgb; c.rgb_dt = f->rgb_dtype; c.depth = f->depth;
        for (int m = 0; m < 2; ++m) { c.rgb_feat[m] = f->rgb_feat[m]; c.depth_feat[m] = f->depth_feat[m]; }
    } else { c.rgb = rgb; c.rgb_dt = rgb_dt; c.depth = depth; }
    c.ids = ids; c.ids_dt = ids_dt;
    if (ids_dt == HCM_INSTR_FEATURES && ids) {             // `ids` is a host hcm_instr_features (check_instr judges it): no token ids in this call
        const hcm_instr_features* f = (const hcm_instr_features*)ids;
        c.ids = nullptr; c.instr_feat = f->stream; c.instr_rows = f->rows; c.instr_reserved = f->reserved;
    }
    c.rows = c.Bi = rows; c.L = L; c.stream = (hipStream_t)stream;
    return c;
}
// HCM_INSTR_FEATURES and hcm_encode_instruction need a handle whose instruction encoder is BERT, and runs
static int instr_handle(hcm_ctx* h, const char* what) {
    REQUIRE(h->kind == 0, HCM_ERR_UNSUPPORTED,
            std::string(what) + ": the instruction encoder of a CMANet / Seq2SeqNet handle is a recurrent InstructionEncoder, not BERT (cma.py:50-52, "
            "seq2seq.py:45-48 with is_bert refused): there is no frozen BERT stream to take or to export");
    REQUIRE(h->cfg.build_high, HCM_ERR_UNSUPPORTED, std::string(what) + ": the handle holds no high-level model, and only that one reads the instruction");
    REQUIRE(!h->cfg.ablate_instruction, HCM_ERR_UNSUPPORTED, std::string(what) + ": the instruction is ablated and nothing would read the stream");
    return HCM_OK;
}
static bool ids_arg_ok(int d) { return ids_dt_ok(d) || d == HCM_INSTR_FEATURES; }
// The instruction part of a call, after frames() and after the call's flags are in the descriptor: a no-op for token ids
static int check_instr(hcm_ctx* h, const FwdCall& c, int ids_dtype_arg) {
    if (ids_dtype_arg != HCM_INSTR_FEATURES) return HCM_OK;
    if (const int rc = instr_handle(h, "HCM_INSTR_FEATURES")) return rc;
    REQUIRE(c.instr_feat, HCM_ERR_ARG, "HCM_INSTR_FEATURES: hcm_instr_features.stream is NULL");
    REQUIRE(c.instr_reserved == 0, HCM_ERR_ARG, "HCM_INSTR_FEATURES: hcm_instr_features.reserved must be 0");
    REQUIRE(c.instr_rows >= 1 && c.rows % c.instr_rows == 0, HCM_ERR_ARG,
            "HCM_INSTR_FEATURES: hcm_instr_features.rows = " + std::to_string(c.instr_rows) + " must be >= 1 and divide the call's " +
            std::to_string(c.rows) + " rows (B, or T*N of a sequence / validation call)");
    REQUIRE(!c.reuse_instruction, HCM_ERR_ARG,
            "HCM_INSTR_FEATURES together with HCM_ACT_REUSE_INSTRUCTION: the flag says `skip the instruction`, the dtype hands one over");
    return HCM_OK;
}
// Which (model, modality) pairs of this handle have a ResNet trunk that runs (no SimpleCNN, not ablated): [slot][0 rgb, 1 depth]; slot 0 = the
// high-level model or a flat handle's model, slot 1 = the low-level model.  `why` gets the reason a pair takes no feature.
static bool feat_slot(const hcm_ctx* h, int m, int mod, const char** why) {
    const char* none = "the handle holds no model for that slot";
    const char* simple = mod == 0 ? "that model's RGB encoder is a SimpleRGBCNN, which reads observations[\"rgb\"] only (models/encoders/simple_cnns.py:144-147; "
                                    "rgb_features is a key of TorchVisionResNet50, resnet_encoders.py:207-214)"
                                  : "that model's depth encoder is a SimpleDepthCNN, which reads observations[\"depth\"] only (models/encoders/simple_cnns.py:122-125; "
                                    "depth_features is a key of VlnResnetDepthEncoder, resnet_encoders.py:83-86)";
    const char* ablated = mod == 0 ? "the RGB modality is ablated: the encoder output is multiplied by 0 (seq2seq_highlevel_cma.py:187-188, seq2seq_lowlevel.py:134-135, "
                                     "cma.py:240-241, seq2seq.py:160-161) and nothing would read the feature"
                                   : "the depth modality is ablated: the encoder output is multiplied by 0 (seq2seq_highlevel_cma.py:185-186, seq2seq_lowlevel.py:132-133, "
                                     "cma.py:238-239, seq2seq.py:158-159) and nothing would read the feature";
    const char* dummy;
    if (!why) why = &dummy;
    if (h->kind == 1) {
        if (m != 0) { *why = none; return false; }
        if (mod == 0 ? h->cma_cfg.ablate_rgb : h->cma_cfg.ablate_depth) { *why = ablated; return false; }
        return true;
    }
    const bool lo = h->kind == 2 || m == 1;                // Seq2SeqNet runs the low-level model's encoder paths
    if (h->kind == 2 ? m != 0 : (m == 0 ? !h->cfg.build_high : !h->cfg.build_low)) { *why = none; return false; }
    if (lo && (mod == 0 ? h->lo.rgb_simple : h->lo.depth_simple)) { *why = simple; return false; }
    const bool abl = h->kind == 2 ? (mod == 0 ? h->s2s_cfg.ablate_rgb : h->s2s_cfg.ablate_depth) : (mod == 0 ? h->cfg.ablate_rgb : h->cfg.ablate_depth);
    if (abl) { *why = ablated; return false; }
    return true;
}
// f32 elements per row of the feature (slot m, modality mod) takes; 0 = none
static int64_t feat_elems(const hcm_ctx* h, int m, int mod) {
    if (!feat_slot(h, m, mod, nullptr)) return 0;
    if (mod == 0) return (h->kind == 2 || (h->kind == 0 && m == 1)) ? 2048 : 2048 * 16;
    const int fs = hcm::depth_final_spatial(h->cfg);
    return (int64_t)hcm::depth_compress_channels(h->cfg) * fs * fs;
}
// The observation part of a call, after frames(): features only where a ResNet trunk would run, and a frame for every trunk that still runs.
// depth_arg: the entry point's own `depth` argument -- NULL with HCM_FEATURES.  The models of the call: do_hi / do_lo on an HCM handle.
static int check_obs(hcm_ctx* h, const FwdCall& c, const float* depth_arg, int rgb_dtype_arg) {
    const bool feats = rgb_dtype_arg == HCM_FEATURES;
    if (feats) {
        REQUIRE(c.rgb || c.depth || c.rgb_feat[0] || c.rgb_feat[1] || c.depth_feat[0] || c.depth_feat[1], HCM_ERR_ARG,
                "HCM_FEATURES: `rgb` must point to an hcm_features holding at least one pointer");
        REQUIRE(!depth_arg, HCM_ERR_ARG, "HCM_FEATURES: `depth` must be NULL, the depth frames travel in hcm_features.depth");
        REQUIRE(!c.host_frames, HCM_ERR_ARG, "HCM_ACT_HOST_FRAMES together with HCM_FEATURES: the members of hcm_features are device pointers");
    }
    bool need[2] = {false, false};                         // a trunk of the call still reads the RGB / depth frames
    for (int m = 0; m < 2; ++m) {
        const bool runs = h->kind != 0 ? m == 0 : (m == 0 ? c.do_hi : c.do_lo);
        for (int mod = 0; mod < 2; ++mod) {
            const float* f = mod == 0 ? c.rgb_feat[m] : c.depth_feat[m];
            const char* why = "";
            const bool slot = feat_slot(h, m, mod, &why);
            if (f && !slot)
                return fail(h, h->kind != 0 && m == 1 ? HCM_ERR_ARG : HCM_ERR_UNSUPPORTED,
                            std::string(mod == 0 ? "rgb_feat[" : "depth_feat[") + std::to_string(m) + "] given, but " + why);
            if (!runs || f) continue;
            // no feature: the frame is read unless the modality is ablated (the encoder is then not run at all)
            const bool abl = h->kind == 1 ? (mod == 0 ? h->cma_cfg.ablate_rgb : h->cma_cfg.ablate_depth)
                           : h->kind == 2 ? (mod == 0 ? h->s2s_cfg.ablate_rgb : h->s2s_cfg.ablate_depth) : (mod == 0 ? h->cfg.ablate_rgb : h->cfg.ablate_depth);
            const bool held = h->kind != 0 || (m == 0 ? h->cfg.build_high : h->cfg.build_low);
            if (held && !(feats && abl)) need[mod] = true;
        }
    }
    REQUIRE(!need[0] || c.rgb, HCM_ERR_ARG, feats ? "hcm_features.rgb is NULL, but a model of this call has no rgb_feat and still runs its RGB encoder" : "null pointer");
    REQUIRE(!need[1] || c.depth, HCM_ERR_ARG, feats ? "hcm_features.depth is NULL, but a model of this call has no depth_feat and still runs its depth encoder" : "null pointer");
    REQUIRE(!c.rgb || rgb_dt_ok(c.rgb_dt), HCM_ERR_ARG, "unsupported rgb dtype");
    return HCM_OK;
}
// state, mask and outputs of a flat handle's one model
static void flat_io(hcm_ctx* h, FwdCall& c, const float* h_in, const float* mask, float* out, float* stop, float* progress, float* h_out) {
    c.lo_h_in = h_in; c.mask = mask; c.lo_h_out = h_out;
    c.vel = out; c.ld_vel = h->cfg.num_actions; c.stop = stop; c.ld_stop = 1; c.progress = progress;
}
static int run_eager(hcm_ctx* h, const FwdCall& c) {
    try { run_forward(h, c); } catch (const std::exception& e) { return fail(h, HCM_ERR_HIP, e.what()); }
    return HCM_OK;
}

// hcm_high_forward (T = 1) and hcm_high_forward_seq
static int high_forward(hcm_ctx* h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, const int32_t* lengths, int rows,
                        int T, int L, const float* h_in, const float* mask, float* logits, float* h_out, void* stream) {
    int rc = check_fwd(h, rows);
    if (rc) return rc;
    if ((rc = check_len(h, L))) return rc;
    drop_instruction_cache(h);
    if (ids_dtype == HCM_INSTR_FEATURES && (rc = instr_handle(h, "HCM_INSTR_FEATURES"))) return rc;
    REQUIRE(h->cfg.build_high, HCM_ERR_STATE, "handle holds no high-level model");
    REQUIRE(ids && h_in && mask && logits && h_out, HCM_ERR_ARG, "null pointer");
    REQUIRE(ids_arg_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, rows, L, stream);
    c.do_hi = true; c.T = T; c.lens = lengths;
    if ((rc = check_instr(h, c, ids_dtype))) return rc;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    c.hi_h_in = h_in; c.mask = mask; c.logits = logits; c.ld_logits = h->cfg.num_actions; c.hi_h_out = h_out;
    return run_eager(h, c);
}

int hcm_high_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
                     const int32_t* lengths, int B, int L, const float* h_in, const float* mask, float* logits, float* h_out, void* stream) {
    return high_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, lengths, B, 1, L, h_in, mask, logits, h_out, stream);
}

int hcm_high_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
                         const int32_t* lengths, int T, int N, int L, const float* h_in, const float* masks, float* logits, float* h_out, void* stream) {
    if (const int rc = check_seq(h, T, N)) return rc;
    return high_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, lengths, T * N, T, L, h_in, masks, logits, h_out, stream);
}

// hcm_low_forward (T = 1) and hcm_low_forward_seq
static int low_forward(hcm_ctx* h, const void* rgb, int rgb_dtype, const float* depth, int rows, int T, const float* h_in, const float* mask,
                       const int64_t* subtask, float* vel, float* stop, float* h_out, void* stream) {
    int rc = check_fwd(h, rows);
    if (rc) return rc;
    drop_instruction_cache(h);
    REQUIRE(h->cfg.build_low, HCM_ERR_STATE, "handle holds no low-level model");
    REQUIRE(h_in && mask && subtask && vel && stop && h_out, HCM_ERR_ARG, "null pointer");
    FwdCall c = frames(rgb, rgb_dtype, depth, nullptr, DT_I64, rows, 0, stream);
    c.do_lo = true; c.T = T;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    c.lo_h_in = h_in; c.mask = mask; c.subtask = subtask; c.lo_h_out = h_out;
    c.vel = vel; c.ld_vel = h->cfg.lo_actions; c.stop = stop; c.ld_stop = 1;
    return run_eager(h, c);
}

int hcm_low_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int B, const float* h_in,
                    const float* mask, const int64_t* subtask, float* vel, float* stop, float* h_out, void* stream) {
    return low_forward(h, rgb, rgb_dtype, depth, B, 1, h_in, mask, subtask, vel, stop, h_out, stream);
}

int hcm_low_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int T, int N, const float* h_in,
                        const float* masks, const int64_t* subtask, float* vel, float* stop, float* h_out, void* stream) {
    if (const int rc = check_seq(h, T, N)) return rc;
    return low_forward(h, rgb, rgb_dtype, depth, T * N, T, h_in, masks, subtask, vel, stop, h_out, stream);
}

// hcm_cma_forward (T = 1: through the graph cache) and hcm_cma_forward_seq at T > 1; the caller has checked the handle's kind, rows and L
static int cma_forward(hcm_ctx* h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int rows, int T, int L,
                       const float* h_in, const float* mask, float* out, float* stop, float* h_out, void* stream) {
    REQUIRE(ids && h_in && mask && out && stop && h_out, HCM_ERR_ARG, "null pointer");
    if (ids_dtype == HCM_INSTR_FEATURES) return instr_handle(h, "HCM_INSTR_FEATURES");
    REQUIRE(ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, rows, L, stream);
    c.T = T;
    if (const int rc = check_obs(h, c, depth, rgb_dtype)) return rc;
    flat_io(h, c, h_in, mask, out, stop, nullptr, h_out);
    return T == 1 ? run_graphed(h, c) : run_eager(h, c);
}

int hcm_cma_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int L,
                    const float* h_in, const float* mask, float* out, float* stop, float* h_out, void* stream) {
    int rc = check_fwd(h, B);
    if (rc) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(h->kind == 1, HCM_ERR_STATE, "not a CMANet handle (hcm_cma_create)");
    return cma_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, B, 1, L, h_in, mask, out, stop, h_out, stream);
}

int hcm_cma_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int T, int N, int L,
                        const float* h_in, const float* masks, float* out, float* stop, float* h_out, void* stream) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(h->kind == 1, HCM_ERR_STATE, "not a CMANet handle (hcm_cma_create)");
    int rc = check_seq(h, T, N);
    if (rc) return rc;
    if (T == 1) return hcm_cma_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, N, L, h_in, masks, out, stop, h_out, stream);
    if ((rc = check_fwd(h, T * N))) return rc;
    if ((rc = check_len(h, L))) return rc;
    return cma_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, T * N, T, L, h_in, masks, out, stop, h_out, stream);
}

// hcm_s2s_forward (through the graph cache) and hcm_s2s_forward_seq.  The argument checks that do not need a finalized handle come first, so
// that a caller's mistake is reported as such whatever state the handle is in
static int s2s_forward(hcm_ctx* h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int rows, int T, bool graphed,
                       int B_instr, int L, const float* h_in, const float* mask, float* out, float* stop, float* progress, float* h_out, void* stream) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(h->kind == 2, HCM_ERR_STATE, "not a Seq2SeqNet handle (hcm_s2s_create)");
    REQUIRE(B_instr == 1 || B_instr == rows, HCM_ERR_ARG, "B_instr must be 1 (one instruction for every frame, seq2seq.py:163) or the number of frames");
    REQUIRE(h->s2s_cfg.progress_monitor || !progress, HCM_ERR_ARG,
            "progress must be NULL: the handle was created without PROGRESS_MONITOR.use (hcm_s2s_config.progress_monitor)");
    int rc = check_fwd(h, rows);
    if (rc) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(ids && h_in && mask && out && stop && h_out, HCM_ERR_ARG, "null pointer");
    if (ids_dtype == HCM_INSTR_FEATURES) return instr_handle(h, "HCM_INSTR_FEATURES");
    REQUIRE(ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, rows, L, stream);
    c.T = T; c.Bi = B_instr;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    flat_io(h, c, h_in, mask, out, stop, progress, h_out);
    return graphed ? run_graphed(h, c) : run_eager(h, c);
}

int hcm_s2s_forward(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int B, int B_instr, int L,
                    const float* h_in, const float* mask, float* out, float* stop, float* progress, float* h_out, void* stream) {
    return s2s_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, B, 1, true, B_instr, L, h_in, mask, out, stop, progress, h_out, stream);
}

int hcm_s2s_forward_seq(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int T, int N, int B_instr,
                        int L, const float* h_in, const float* masks, float* out, float* stop, float* progress, float* h_out, void* stream) {
    if (const int rc = check_seq(h, T, N)) return rc;
    return s2s_forward(h, rgb, rgb_dtype, depth, ids, ids_dtype, T * N, T, false, B_instr, L, h_in, masks, out, stop, progress, h_out, stream);
}

int hcm_val_step(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, const int32_t* lengths, int T, int N,
                 int L, const int64_t* oracle_subtask, const float* corrected_actions, const float* oracle_stop, const float* hi_h_in,
                 const float* lo_h_in, const float* masks, float* result, float* hi_h_out, float* lo_h_out, float* logits, float* vel, float* stop,
                 void* stream) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    int rc = HCM_OK;
    if (ids_dtype == HCM_INSTR_FEATURES && (rc = instr_handle(h, "HCM_INSTR_FEATURES"))) return rc;
    REQUIRE(h->kind == 0, HCM_ERR_STATE, "hcm_val_step needs an HCM handle (hcm_create): the flat baselines have no high-level / low-level pair");
    if ((rc = check_seq(h, T, N))) return rc;
    REQUIRE(result, HCM_ERR_ARG, "null result");
    REQUIRE((rgb_dt_ok(rgb_dtype) || rgb_dtype == HCM_FEATURES) && ids_arg_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    if ((rc = check_fwd(h, T * N))) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(h->cfg.build_high && h->cfg.build_low, HCM_ERR_STATE, "hcm_val_step needs both models in the handle");
    REQUIRE(ids && oracle_subtask && corrected_actions && oracle_stop && hi_h_in && lo_h_in && masks && hi_h_out && lo_h_out,
            HCM_ERR_ARG, "null pointer");
    drop_instruction_cache(h);
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, T * N, L, stream);
    c.do_hi = c.do_lo = true; c.T = T; c.lens = lengths;
    if ((rc = check_instr(h, c, ids_dtype))) return rc;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    c.hi_h_in = hi_h_in; c.lo_h_in = lo_h_in; c.mask = masks; c.hi_h_out = hi_h_out; c.lo_h_out = lo_h_out;
    c.logits = logits; c.ld_logits = h->cfg.num_actions; c.vel = vel; c.ld_vel = h->cfg.lo_actions; c.stop = stop; c.ld_stop = 1;
    c.val = FwdCall::kVal; c.oracle = oracle_subtask; c.corrected = corrected_actions; c.oracle_stop = oracle_stop; c.result = result;
    return run_eager(h, c);
}

int hcm_flat_val_step(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, int T, int N, int B_instr, int L,
                      const float* corrected_actions, const float* oracle_stop, const float* progress, const float* h_in, const float* masks,
                      float* result, float* h_out, float* out, float* stop, float* progress_hat, void* stream) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    REQUIRE(h->kind == 1 || h->kind == 2, HCM_ERR_STATE,
            "hcm_flat_val_step needs a CMANet or Seq2SeqNet handle (hcm_cma_create / hcm_s2s_create): the hierarchical pair is validated by hcm_val_step");
    int rc = check_seq(h, T, N);
    if (rc) return rc;
    REQUIRE(result, HCM_ERR_ARG, "null result");
    if (ids_dtype == HCM_INSTR_FEATURES) return instr_handle(h, "HCM_INSTR_FEATURES");
    REQUIRE((rgb_dt_ok(rgb_dtype) || rgb_dtype == HCM_FEATURES) && ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    const bool monitor = h->kind == 2 && h->s2s_cfg.progress_monitor;
    if (h->kind == 1)
        REQUIRE(B_instr == T * N, HCM_ERR_ARG, "B_instr must be T*N on a CMANet handle: one instruction row per frame (hcm_cma_forward_seq)");
    else
        REQUIRE(B_instr == 1 || B_instr == T * N, HCM_ERR_ARG,
                "B_instr must be 1 (one instruction for every frame, seq2seq.py:163) or the number of frames");
    REQUIRE(monitor || (!progress && !progress_hat), HCM_ERR_ARG,
            "progress and progress_hat must be NULL: the handle has no progress monitor (hcm_s2s_config.progress_monitor)");
    REQUIRE(!monitor || progress, HCM_ERR_ARG,
            "null progress: the handle was created with PROGRESS_MONITOR.use, the auxiliary loss needs observations[\"progress\"]");
    if ((rc = check_fwd(h, T * N))) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(ids && corrected_actions && oracle_stop && h_in && masks && h_out, HCM_ERR_ARG, "null pointer");
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, T * N, L, stream);
    c.T = T; c.Bi = B_instr;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    flat_io(h, c, h_in, masks, out, stop, progress_hat, h_out);
    c.val = FwdCall::kFlatVal; c.corrected = corrected_actions; c.oracle_stop = oracle_stop; c.progress_label = progress; c.result = result;
    return run_eager(h, c);
}

int hcm_encode_features_ex(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int rows, const hcm_features* out, int flags, void* stream) {
    int rc = check_fwd(h, rows);
    if (rc) return rc;
    REQUIRE(out, HCM_ERR_ARG, "null `out`");
    REQUIRE(rgb_dtype != HCM_FEATURES, HCM_ERR_ARG, "hcm_encode_features reads frames: rgb_dtype must be HCM_F32 or HCM_U8");
    REQUIRE((flags & ~HCM_ENCODE_ACT) == 0, HCM_ERR_ARG, "unknown flag");
    drop_instruction_cache(h);
    FwdCall c = frames(rgb, rgb_dtype, depth, nullptr, DT_I64, rows, 0, stream);
    c.encode = true; c.enc_act = (flags & HCM_ENCODE_ACT) != 0;
    bool any = false, need[2] = {false, false};
    for (int m = 0; m < 2; ++m)
        for (int mod = 0; mod < 2; ++mod) {
            float* o = const_cast<float*>(mod == 0 ? out->rgb_feat[m] : out->depth_feat[m]);
            if (!o) continue;
            const char* why = "";
            if (!feat_slot(h, m, mod, &why))
                return fail(h, h->kind != 0 && m == 1 ? HCM_ERR_ARG : HCM_ERR_UNSUPPORTED,
                            std::string(mod == 0 ? "rgb_feat[" : "depth_feat[") + std::to_string(m) + "] wanted, but " + why);
            (mod == 0 ? c.enc_rgb[m] : c.enc_depth[m]) = o;
            any = need[mod] = true;
        }
    REQUIRE(any, HCM_ERR_ARG, "no feature wanted: every pointer of `out` is NULL");
    REQUIRE(!need[0] || (rgb && rgb_dt_ok(rgb_dtype)), HCM_ERR_ARG, "an RGB feature is wanted: `rgb` must be frames of dtype HCM_F32 or HCM_U8");
    REQUIRE(!need[1] || depth, HCM_ERR_ARG, "a depth feature is wanted: `depth` is NULL");
    return run_eager(h, c);
}
int hcm_encode_features(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, int rows, const hcm_features* out, void* stream) {
    return hcm_encode_features_ex(h, rgb, rgb_dtype, depth, rows, out, 0, stream);
}

int hcm_encode_instruction(hcm_handle h, const void* ids, int ids_dtype, const int32_t* lengths, int rows, int L, float* out, void* stream) {
    int rc = check_fwd(h, rows);
    if (rc) return rc;
    if ((rc = instr_handle(h, "hcm_encode_instruction"))) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(ids_dtype != HCM_INSTR_FEATURES, HCM_ERR_ARG, "hcm_encode_instruction reads token ids: ids_dtype must be HCM_I32, HCM_I64 or HCM_F32");
    REQUIRE(ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported ids dtype");
    REQUIRE(ids && out, HCM_ERR_ARG, "null pointer");
    drop_instruction_cache(h);
    FwdCall c = frames(nullptr, DT_F32, nullptr, ids, ids_dtype, rows, L, stream);
    c.lens = lengths; c.encode_instr = true; c.enc_instr = out;
    return run_eager(h, c);
}

int hcm_act_ex(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype,
               const int32_t* lengths, int B, int L, const float* hi_h_in, const float* lo_h_in, const float* mask, float* record, float* hi_h_out, float* lo_h_out,
               int flags, void* stream) {
    int rc = check_fwd(h, B);
    if (rc) return rc;
    if ((rc = check_len(h, L))) return rc;
    if (ids_dtype == HCM_INSTR_FEATURES && (rc = instr_handle(h, "HCM_INSTR_FEATURES"))) return rc;
    REQUIRE(h->cfg.build_high && h->cfg.build_low, HCM_ERR_STATE, "hcm_act needs both models in the handle");
    REQUIRE(ids && hi_h_in && lo_h_in && mask && record && hi_h_out && lo_h_out, HCM_ERR_ARG, "null pointer");
    REQUIRE(ids_arg_ok(ids_dtype), HCM_ERR_ARG, "unsupported rgb/ids dtype");
    REQUIRE(h->cfg.num_actions + h->cfg.lo_actions + 1 == 7, HCM_ERR_UNSUPPORTED, "record layout assumes 4 + 2 + 1 outputs");
    FwdCall c = frames(rgb, rgb_dtype, depth, ids, ids_dtype, B, L, stream);
    c.do_hi = c.do_lo = true; c.lens = lengths;
    c.reuse_instruction = (flags & HCM_ACT_REUSE_INSTRUCTION) != 0;
    if ((rc = check_instr(h, c, ids_dtype))) return rc;
    REQUIRE(!c.reuse_instruction || (h->last_hi_batch == B && h->last_hi_L == L), HCM_ERR_STATE,
            "HCM_ACT_REUSE_INSTRUCTION: the previous call on this handle was not an hcm_act step with this batch size and instruction length");
    c.host_frames = (flags & HCM_ACT_HOST_FRAMES) != 0;
    if ((rc = check_obs(h, c, depth, rgb_dtype))) return rc;
    if (c.host_frames && (!h->stage_rgb || !h->stage_depth)) {         // device staging for the largest call: f32 RGB frames + f32 depth frames
        const size_t n_rgb = (size_t)h->cfg.max_batch * h->cfg.rgb_h * h->cfg.rgb_w * 3 * 4, n_dep = (size_t)h->cfg.max_batch * h->cfg.depth_h * h->cfg.depth_w * 4;
        if (!h->stage_rgb && hipMalloc(&h->stage_rgb, n_rgb) != hipSuccess) { h->stage_rgb = nullptr; return fail(h, HCM_ERR_NOMEM, "hipMalloc of the RGB frame staging buffer failed"); }
        if (!h->stage_depth && hipMalloc((void**)&h->stage_depth, n_dep) != hipSuccess) { h->stage_depth = nullptr; return fail(h, HCM_ERR_NOMEM, "hipMalloc of the depth frame staging buffer failed"); }
    }
    c.hi_h_in = hi_h_in; c.lo_h_in = lo_h_in; c.mask = mask; c.hi_h_out = hi_h_out; c.lo_h_out = lo_h_out;
    c.logits = record; c.vel = record + 4; c.stop = record + 6; c.ld_logits = c.ld_vel = c.ld_stop = 7;      // the three column blocks of the record
    // HCM_ACT_CHAIN_GRAPHS: one linear graph per chain (the development build's HCM_RGB_SERIAL=0 keeps the single forked graph; HCM_SEG_GRAPH=1 / 0 of that
    // build forces the choice for A/B runs)
    static const bool seg_off = (dev_env("HCM_RGB_SERIAL") && atoi(dev_env("HCM_RGB_SERIAL")) == 0) || (dev_env("HCM_SEG_GRAPH") && atoi(dev_env("HCM_SEG_GRAPH")) == 0);
    static const bool seg_on = dev_env("HCM_SEG_GRAPH") && atoi(dev_env("HCM_SEG_GRAPH")) != 0;
    rc = run_graphed(h, c, !seg_off && (seg_on || (flags & HCM_ACT_CHAIN_GRAPHS) != 0));
    if (rc == HCM_OK) { h->last_hi_batch = B; h->last_hi_L = L; } else drop_instruction_cache(h);
    return rc;
}

int hcm_refresh_instruction(hcm_handle h, const void* ids, int ids_dtype, const int32_t* lengths, int B, int L, const int32_t* env_indices,
                            int n, void* stream) {
    int rc = check_fwd(h, B);
    if (rc) return rc;
    if ((rc = check_len(h, L))) return rc;
    REQUIRE(h->cfg.build_high, HCM_ERR_STATE, "handle holds no high-level model");
    REQUIRE(ids && (env_indices || n == 0) && n >= 0 && n <= B, HCM_ERR_ARG, "bad argument");
    REQUIRE(ids_dtype != HCM_INSTR_FEATURES, HCM_ERR_ARG,
            "hcm_refresh_instruction takes token ids: a stream for the listed environments is not built (pass it to hcm_act_ex without "
            "HCM_ACT_REUSE_INSTRUCTION instead)");
    REQUIRE(ids_dt_ok(ids_dtype), HCM_ERR_ARG, "unsupported ids dtype");
    REQUIRE(h->last_hi_batch == B && h->last_hi_L == L, HCM_ERR_STATE,
            "hcm_refresh_instruction: the previous call on this handle was not an hcm_act step with this batch size and instruction length");
    for (int i = 0; i < n; ++i) REQUIRE(env_indices[i] >= 0 && env_indices[i] < B, HCM_ERR_ARG, "environment index out of range");
    if (n == 0) return HCM_OK;
    FwdCall c = frames(nullptr, DT_F32, nullptr, ids, ids_dtype, B, L, stream);
    c.lens = lengths;
    try {
        run_refresh_instruction(h, c, env_indices, n);
    } catch (const std::exception& e) {
        return fail(h, HCM_ERR_HIP, e.what());
    }
    return HCM_OK;
}

int hcm_act(hcm_handle h, const void* rgb, int rgb_dtype, const float* depth, const void* ids, int ids_dtype, const int32_t* lengths,
            int B, int L, const float* hi_h_in, const float* lo_h_in, const float* mask, float* record, float* hi_h_out, float* lo_h_out,
            void* stream) {
    return hcm_act_ex(h, rgb, rgb_dtype, depth, ids, ids_dtype, lengths, B, L, hi_h_in, lo_h_in, mask, record, hi_h_out, lo_h_out, 0, stream);
}

int hcm_query(hcm_handle h, int what, int64_t* out) {
    REQUIRE(h && out, HCM_ERR_ARG, "null argument");
    switch (what) {
        case HCM_NUM_RECURRENT_LAYERS: *out = (h->cfg.rnn_type == HCM_LSTM ? 2 : 1) * (h->kind == 1 ? 2 : 1); break;   // cma.py:190-194
        case HCM_HIDDEN_SIZE: *out = h->cfg.hidden; break;
        case HCM_NUM_ACTIONS: *out = h->cfg.num_actions; break;
        case HCM_RECORD_WIDTH: *out = h->cfg.num_actions + h->cfg.lo_actions + 1; break;
        case HCM_WORKSPACE_BYTES: *out = (int64_t)h->arena.cap; break;
        case HCM_WEIGHT_BYTES: *out = (int64_t)h->weight_bytes; break;
        case HCM_MAX_BATCH: *out = h->cfg.max_batch; break;
        case HCM_GRAPH_LAUNCHES: *out = h->graph_launches; break;
        case HCM_EAGER_LAUNCHES: *out = h->eager_launches; break;
        case HCM_FP16_FALLBACK: *out = h->fp16_fallback; break;
        case HCM_RANGE_FOLD: *out = h->range_fold; break;
        case HCM_GATHER_JOINED: *out = h->gather_joined; break;
        case HCM_FEAT_RGB_HI: *out = feat_elems(h, 0, 0); break;
        case HCM_FEAT_RGB_LO: *out = feat_elems(h, 1, 0); break;
        case HCM_FEAT_DEPTH_HI: *out = feat_elems(h, 0, 1); break;
        case HCM_FEAT_DEPTH_LO: *out = feat_elems(h, 1, 1); break;
        case HCM_FEAT_SHARED:
            *out = h->kind == 0 && h->cfg.build_high && h->cfg.build_low
                       ? (int64_t)(h->hi.rgb_shared && !h->lo.rgb_simple) | (int64_t)(h->hi.depth_shared && !h->lo.depth_simple) << 1 : 0;
            break;
        case HCM_CALIB_MAX_BERT: *out = (int64_t)h->calib_max[0]; break;
        case HCM_CALIB_MAX_DEPTH: *out = (int64_t)h->calib_max[1]; break;
        case HCM_CALIB_NONFINITE: *out = (int64_t)h->calib_bad[0] + (int64_t)h->calib_bad[1] + (int64_t)h->calib_bad[2] + (int64_t)h->calib_bad[3]; break;
        case HCM_CALIB_MAX_VLA: *out = (int64_t)h->calib_max[3]; break;
        case HCM_CALIB_MAX_RGB: *out = (int64_t)h->calib_max[2]; break;
        case HCM_STEP_NONFINITE: {           // (synchronises the device: a diagnostic, not a per-step call)
            unsigned v = 0;
            if (!h->calib_buf) { *out = 0; break; }
            // wait for the steps in flight on the HANDLE's device, whatever device is current in the calling thread
            int cur = -1;
            (void)hipGetDevice(&cur);
            if (h->device >= 0 && cur != h->device) (void)hipSetDevice(h->device);
            const bool ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(&v, h->calib_buf + hcm_ctx::kStepBadWord, 4, hipMemcpyDeviceToHost) == hipSuccess;
            if (h->device >= 0 && cur >= 0 && cur != h->device) (void)hipSetDevice(cur);
            if (!ok) return fail(h, HCM_ERR_HIP, "hcm_query: reading the overflow guard failed");
            *out = (int64_t)v;
            break;
        }
        default: return fail(h, HCM_ERR_ARG, "hcm_query: unknown selector");
    }
    return HCM_OK;
}

int hcm_guard_poll(hcm_handle h, void* stream, int64_t* out) {
    REQUIRE(h && out, HCM_ERR_ARG, "null argument");
    REQUIRE(h->finalized && h->calib_buf, HCM_ERR_STATE, "hcm_guard_poll before hcm_finalize");
    if (!h->guard_host) {
        if (hipHostMalloc((void**)&h->guard_host, 8, hipHostMallocDefault) != hipSuccess) { h->guard_host = nullptr; return fail(h, HCM_ERR_NOMEM, "hipHostMalloc failed"); }
        *h->guard_host = 0u;
        if (hipEventCreateWithFlags(&h->guard_ev, hipEventDisableTiming) != hipSuccess) return fail(h, HCM_ERR_HIP, "hipEventCreate failed");
    }
    if (h->guard_pending && hipEventQuery(h->guard_ev) == hipSuccess) { h->guard_last = *h->guard_host; h->guard_pending = false; }
    if (!h->guard_pending) {
        if (hipMemcpyAsync(h->guard_host, h->calib_buf + hcm_ctx::kStepBadWord, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipEventRecord(h->guard_ev, (hipStream_t)stream) != hipSuccess)
            return fail(h, HCM_ERR_HIP, "hcm_guard_poll: enqueueing the read failed");
        h->guard_pending = true;
    }
    *out = (int64_t)h->guard_last;
    return HCM_OK;
}

const char* hcm_last_error(hcm_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

void hcm_destroy(hcm_handle h) {
    if (!h) return;
    comm_destroy(h);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    if (h->arena.base) (void)hipFree(h->arena.base);
    if (h->pred_buf) (void)hipFree(h->pred_buf);
    if (h->calib_buf) (void)hipFree(h->calib_buf);
    if (h->marks_dev) (void)hipFree(h->marks_dev);
    if (h->stage_rgb) (void)hipFree(h->stage_rgb);
    if (h->stage_depth) (void)hipFree(h->stage_depth);
    if (h->len_buf) (void)hipFree(h->len_buf);
    if (h->guard_ev) (void)hipEventDestroy(h->guard_ev);
    if (h->guard_host) (void)hipHostFree(h->guard_host);
    for (auto& kv : h->taps) if (kv.second.dev) (void)hipFree(kv.second.dev);
    for (auto& g : h->graphs) destroy_entry(g);
    for (int i = 0; i < 4; ++i) {
        if (h->aux[i]) (void)hipStreamDestroy(h->aux[i]);
        if (h->pool[i]) (void)hipStreamDestroy(h->pool[i]);
        if (h->pool[i + 4]) (void)hipStreamDestroy(h->pool[i + 4]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    delete h;
}

int hcm_debug_enable_taps(hcm_handle h, int enable) {
    REQUIRE(h, HCM_ERR_ARG, "null handle");
    h->taps_on = enable != 0;
    return HCM_OK;
}

int hcm_debug_igemm_prof(uint64_t* out8, int reset) {
    if (!out8) return HCM_ERR_ARG;
    unsigned long long v[8];
    if (hcm::igemm_prof_read(v, reset != 0) != hipSuccess) return HCM_ERR_HIP;
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return HCM_OK;
}

int hcm_debug_marks(hcm_handle h, uint64_t* out256, char* names, int names_cap) {
    REQUIRE(h && out256 && names && names_cap > 0, HCM_ERR_ARG, "null argument");
    names[0] = 0;
    if (!h->marks_dev) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return fail(h, HCM_ERR_HIP, "hipDeviceSynchronize failed");
    if (hipMemcpy(out256, h->marks_dev, 256 * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HCM_ERR_HIP, "marks copy failed");
    std::string all;
    for (const std::string& n : h->mark_names) { all += n; all += '\n'; }
    REQUIRE((int)all.size() < names_cap, HCM_ERR_ARG, "names buffer too small");
    std::memcpy(names, all.c_str(), all.size() + 1);
    return (int)h->mark_names.size();
}

int hcm_debug_gemm256_prof(uint64_t* out1024, int reset) {
    if (!out1024) return HCM_ERR_ARG;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    if (hcm::gemm256_prof_read(reinterpret_cast<unsigned long long*>(out1024), reset != 0) != hipSuccess) return HCM_ERR_HIP;
    return HCM_OK;
}

int hcm_debug_get_tap(hcm_handle h, const char* name, float* host_out, int64_t capacity, int64_t* n_out, int64_t* shape_out) {
    REQUIRE(h && name && n_out, HCM_ERR_ARG, "null argument");
    auto it = h->taps.find(name);
    REQUIRE(it != h->taps.end(), HCM_ERR_KEY, std::string("no such tap: ") + name);
    const Tap& t = it->second;
    *n_out = (int64_t)t.n;
    if (shape_out) for (int i = 0; i < 4; ++i) shape_out[i] = i < (int)t.shape.size() ? t.shape[i] : 0;
    if (host_out) {
        REQUIRE(capacity >= (int64_t)t.n, HCM_ERR_ARG, "tap buffer too small");
        if (hipDeviceSynchronize() != hipSuccess) return fail(h, HCM_ERR_HIP, "hipDeviceSynchronize failed");
        if (hipMemcpy(host_out, t.dev, t.n * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HCM_ERR_HIP, "tap copy failed");
    }
    return HCM_OK;
}

// ------------------------------------------------------------------ stand-alone operators (kernel-level parity tests)
static int op_rc(hipError_t e) {
    if (e == hipSuccess) return HCM_OK;
    g_create_err = std::string("op launch failed: ") + hipGetErrorString(e);
    return e == hipErrorInvalidValue ? HCM_ERR_ARG : HCM_ERR_HIP;
}
static int op_dt(int dtype) { return dtype == HCM_BF16 ? DT_BF16 : dtype == HCM_F16 ? DT_F16 : DT_F32; }

int hcm_op_conv2d(const void* x, const void* w_ohwi, const float* bias, const void* residual, void* y, int dtype, int B, int H,
                  int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int act, void* stream) {
    IGemm g;
    g.x = x; g.w = w_ohwi; g.bias = bias; g.res = residual; g.y = y;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.xC = Cin;
    g.Ho = (H + 2 * pad - KH) / stride + 1; g.Wo = (W + 2 * pad - KW) / stride + 1;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.M = B * g.Ho * g.Wo; g.N = Cout; g.K = KH * KW * Cin; g.Kp = g.K; g.ldy = Cout; g.ldr = Cout; g.act = act;
    return op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_bottleneck_tail(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                           void* y, int dtype, int B, int H, int W, int C1, int stride, void* stream) {
    Bneck23 b;
    b.x = x; b.w2 = w2; b.b2 = b2; b.w3 = w3; b.b3 = b3; b.res = identity; b.y = y;
    b.B = B; b.H = H; b.W = W; b.C1 = C1; b.stride = stride;
    return op_rc(launch_bneck23(b, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_bottleneck_tail_next(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                                void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int C1, int stride,
                                int CN, void* stream) {
    Bneck23 b;
    b.x = x; b.w2 = w2; b.b2 = b2; b.w3 = w3; b.b3 = b3; b.res = identity; b.y = y;
    b.B = B; b.H = H; b.W = W; b.C1 = C1; b.stride = stride;
    b.w1 = w1; b.b1 = b1; b.o1 = o1; b.CN = CN;
    if (!w1) return HCM_ERR_ARG;
    return op_rc(launch_bneck23(b, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_bottleneck_tail_ds(const void* x, const void* w2, const float* b2, const void* w3ds, const float* b3ds, const void* xd,
                              void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int stride,
                              void* stream) {
    if (!xd || !w1) return HCM_ERR_ARG;
    Bneck23 b;
    b.x = x; b.w2 = w2; b.b2 = b2; b.w3 = w3ds; b.b3 = b3ds; b.y = y;
    b.B = B; b.H = H; b.W = W; b.C1 = 64; b.stride = stride;
    b.w1 = w1; b.b1 = b1; b.o1 = o1; b.CN = 64;
    b.xd = xd; b.xdC = 64; b.KD = 1;
    return op_rc(launch_bneck23(b, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_bottleneck_stage(const void* x, const void* w2, const float* b2, const void* w3, const float* b3, const void* identity,
                            const void* xd, void* y, const void* w1, const float* b1, void* o1, int dtype, int B, int H, int W, int C1,
                            int stride, int CN, int KD, int groups, void* stream) {
    if (!w1 || groups < 1 || KD < 0 || (xd != nullptr) != (KD > 0) || (xd && identity)) return HCM_ERR_ARG;
    const int C3 = 4 * C1, K3 = C1 + 64 * KD;
    Bneck23 b;
    b.x = x; b.w2 = w2; b.b2 = b2; b.w3 = w3; b.b3 = b3; b.res = identity; b.y = y;
    b.B = B; b.H = H; b.W = W; b.C1 = C1; b.stride = stride; b.xC = groups * C1; b.ldy = b.ldr = groups * C3;
    b.w1 = w1; b.b1 = b1; b.o1 = o1; b.CN = CN; b.ldo = groups * CN;
    b.xd = xd; b.xdC = xd ? groups * 64 * KD : 0; b.KD = KD;
    if (groups > 1) {
        b.groups = groups; b.g_x = C1; b.g_w2 = (long long)C1 * 9 * C1; b.g_b2 = C1;
        b.g_w3 = (long long)C3 * K3; b.g_b3 = C3; b.g_y = C3;
        b.g_w1 = (long long)CN * C3; b.g_b1 = CN; b.g_o1 = CN; b.g_xd = 64 * KD;
    }
    return op_rc(launch_bneck23(b, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_conv2d_gn(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* residual, void* y,
                     int dtype, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int groups, float eps,
                     int relu, void* stream) {
    if (groups < 1 || Cout % groups) return HCM_ERR_ARG;
    IGemm g;
    g.x = x; g.w = w_ohwi; g.res = residual; g.y = y;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.xC = Cin;
    g.Ho = (H + 2 * pad - KH) / stride + 1; g.Wo = (W + 2 * pad - KW) / stride + 1;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.M = B * g.Ho * g.Wo; g.N = Cout; g.K = KH * KW * Cin; g.Kp = g.K; g.ldy = Cout; g.ldr = Cout; g.act = relu ? ACT_RELU : ACT_NONE;
    g.gn_gamma = gamma; g.gn_beta = beta; g.gn_cg = Cout / groups; g.gn_hw = g.Ho * g.Wo; g.gn_eps = eps;
    return op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_stem_conv(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W, int C, int Cout,
                     int KH, int KW, int stride, int pad, int K, int Kp, int rowrun, float scale, int act, void* stream) {
    IGemm g;
    g.x = x; g.w = w; g.bias = bias; g.y = y;
    g.B = B; g.H = H; g.W = W; g.Cin = C; g.xC = C;
    g.Ho = (H + 2 * pad - KH) / stride + 1; g.Wo = (W + 2 * pad - KW) / stride + 1;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.M = B * g.Ho * g.Wo; g.N = Cout; g.K = K; g.Kp = Kp; g.ldy = Cout; g.ldr = Cout; g.act = act;
    g.x_src_dt = x_dtype == HCM_U8 ? DT_U8 : x_dtype == HCM_F32 ? DT_F32 : op_dt(x_dtype);
    g.x_scale = scale; g.x_rowrun = rowrun;
    return op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
}
/* SimpleCNN's first layer on a depth frame (simple_cnns.py:76-84: Conv2d(1, 32, 8, stride 4) + ReLU) through the packed path of the model
 * code (forward.cpp: simple_cnn): the f32 frame is converted once to the storage type; a kernel row of an output pixel is then one
 * contiguous run of 8 elements, so the conv is an LDS-DMA implicit GEMM over "virtual pixels" of 4 real ones (KH = 8, KW = 1, Cin = 8,
 * pixel stride 4, K = 64).  w is the plain OHWI weight [32][8*8]; scratch holds B*H*H + 64 elements of `dtype`. */
int hcm_op_depth_conv8x8s4(const float* depth, const void* w, const float* bias, void* y, int dtype, int B, int H, int act, void* scratch,
                           void* stream) {
    const int dt = op_dt(dtype);
    if (!scratch || dt == DT_F32 || H % 4 || H < 8) return HCM_ERR_ARG;
    static const bool no_direct = dev_env("HCM_NO_DEPTH_CONV0") != nullptr;       // A/B aid: the convert + implicit-GEMM route
    if (!no_direct && depth_conv8x8s4_ok(dt, H, act)) return op_rc(launch_depth_conv8x8s4(depth, w, bias, y, dt, B, H, act, (hipStream_t)stream));
    int rc = op_rc(launch_convert_from_f32(depth, scratch, dt, (size_t)B * H * H, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    const int h1 = (H - 8) / 4 + 1;
    IGemm g;
    g.x = scratch; g.w = w; g.bias = bias; g.y = y;
    g.B = B; g.H = H; g.W = H / 4; g.Cin = 8; g.xC = 4;
    g.Ho = h1; g.Wo = h1; g.KH = 8; g.KW = 1; g.stride = 4; g.stride_w = 1; g.pad = 0;
    g.M = B * h1 * h1; g.N = 32; g.K = 64; g.Kp = 64; g.ldy = 32; g.ldr = 32; g.act = act;
    return op_rc(launch_igemm(g, dt, (hipStream_t)stream));
}
int64_t hcm_op_stem_scratch_bytes(int B, int H, int W) { return (int64_t)hcm::pack_frame_elems(B, H, W) * 2; }
int hcm_op_stem_conv_packed(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                            int Cout, float scale, int act, void* scratch, void* stream) {
    const int dt = op_dt(dtype);
    if (!scratch || (H & 1) || (W & 1)) return HCM_ERR_ARG;
    const int sdt = x_dtype == HCM_U8 ? DT_U8 : x_dtype == HCM_F32 ? DT_F32 : -1;
    if (sdt < 0) return HCM_ERR_ARG;
    int rc = op_rc(launch_pack_frame(x, sdt, scratch, dt, B, H, W, scale, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    IGemm g;
    g.x = scratch; g.w = w; g.bias = bias; g.y = y;
    g.B = B; g.H = H + 6; g.W = (W + 8) / 2; g.Cin = 32; g.xC = 8;
    g.Ho = H / 2; g.Wo = W / 2; g.KH = 7; g.KW = 1; g.stride = 2; g.stride_w = 1; g.pad = 0;
    g.M = B * g.Ho * g.Wo; g.N = Cout; g.K = 224; g.Kp = 224; g.ldy = Cout; g.ldr = Cout; g.act = act;
    return op_rc(launch_igemm(g, dt, (hipStream_t)stream));
}
int hcm_op_stem_conv_packed_pool(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                                 int Cout, float scale, void* scratch, void* half_map, void* stream) {
    const int dt = op_dt(dtype);
    if (!scratch || !half_map || (H & 1) || (W & 1)) return HCM_ERR_ARG;
    const int sdt = x_dtype == HCM_U8 ? DT_U8 : x_dtype == HCM_F32 ? DT_F32 : -1;
    if (sdt < 0) return HCM_ERR_ARG;
    int rc = op_rc(launch_pack_frame(x, sdt, scratch, dt, B, H, W, scale, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    IGemm g;
    g.x = scratch; g.w = w; g.bias = bias; g.y = half_map;
    g.B = B; g.H = H + 6; g.W = (W + 8) / 2; g.Cin = 32; g.xC = 8;
    g.Ho = H / 2; g.Wo = W / 2; g.KH = 7; g.KW = 1; g.stride = 2; g.stride_w = 1; g.pad = 0;
    g.M = B * g.Ho * g.Wo; g.N = Cout; g.K = 224; g.Kp = 224; g.ldy = Cout; g.ldr = Cout; g.act = ACT_RELU;
    g.hpool = 1;
    rc = op_rc(launch_igemm(g, dt, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    return op_rc(launch_vpool3s2(half_map, y, dt, B, g.Ho, g.Wo / 2, Cout, (hipStream_t)stream));
}
int hcm_op_stem_pool_fused(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                           int Cout, float scale, void* scratch, void* stream) {
    const int dt = op_dt(dtype);
    if (!scratch || !rgb_stem_pool_ok(dt, H, W, Cout, 224)) return HCM_ERR_ARG;
    const int sdt = x_dtype == HCM_U8 ? DT_U8 : x_dtype == HCM_F32 ? DT_F32 : -1;
    if (sdt < 0) return HCM_ERR_ARG;
    const int rc = op_rc(launch_pack_frame(x, sdt, scratch, dt, B, H, W, scale, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    return op_rc(launch_rgb_stem_pool(scratch, w, bias, y, dt, B, H, W, Cout, (hipStream_t)stream));
}
int hcm_op_stem_pool_fused_red(const void* x, int x_dtype, const void* w, const float* bias, void* y, int dtype, int B, int H, int W,
                               int Cout, float scale, void* scratch, const void* w1, const float* b1, void* o1, void* stream) {
    const int dt = op_dt(dtype);
    if (!scratch || !w1 || !b1 || !o1 || !rgb_stem_pool_ok(dt, H, W, Cout, 224)) return HCM_ERR_ARG;
    const int sdt = x_dtype == HCM_U8 ? DT_U8 : x_dtype == HCM_F32 ? DT_F32 : -1;
    if (sdt < 0) return HCM_ERR_ARG;
    const int rc = op_rc(launch_pack_frame(x, sdt, scratch, dt, B, H, W, scale, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    return op_rc(launch_rgb_stem_pool(scratch, w, bias, y, dt, B, H, W, Cout, (hipStream_t)stream, w1, b1, o1));
}
// scratch of the operator entry points that need a temporary (split-K partials, converted frames): grown on demand, test / probe use only
static void* op_scratch(size_t bytes) {
    static void* buf = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        if (buf) { (void)hipDeviceSynchronize(); (void)hipFree(buf); }
        if (hipMalloc(&buf, bytes) != hipSuccess) { buf = nullptr; cap = 0; return nullptr; }
        cap = bytes;
    }
    return buf;
}
int hcm_op_linear(const void* x, const void* w, const float* bias, const void* residual, void* y, int dtype, int M, int N, int K,
                  int act, int out_f32, void* stream) {
    // skinny long-K layers (M = batch rows behind a Flatten: SimpleCNN's 25088-wide FC) are split along K exactly as the model path does
    // (forward.cpp: Fwd::linear): grouped launch over K slices into f32 partials, fixed-order reduction with bias + activation
    {
        int S = splitk_slices(M, N, K, dtype == HCM_F32 ? 4 : 8, residual != nullptr);
        static const int force_s = dev_env("HCM_SPLITK_FORCE") ? atoi(dev_env("HCM_SPLITK_FORCE")) : 0;      // (development build: timing experiments)
        if (force_s > 0 && !residual && K % (force_s * 64) == 0) S = force_s;
        if (S > 1) {
            float* part = (float*)op_scratch((size_t)S * M * N * 4);
            if (!part) return HCM_ERR_NOMEM;
            const int Ks = K / S;
            IGemm g;
            g.x = x; g.w = w; g.y = part;
            g.B = M; g.Cin = Ks; g.xC = K; g.M = M; g.N = N; g.K = Ks; g.Kp = K; g.ldy = N; g.ldr = N; g.act = ACT_NONE; g.out_f32 = 1;
            g.groups = S; g.g_x = Ks; g.g_w = Ks; g.g_b = 0; g.g_y = (long long)M * N;
            int rc = op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
            if (rc != HCM_OK) return rc;
            return op_rc(launch_splitk_reduce(part, bias, y, op_dt(dtype), S, M, N, N, act, out_f32, (hipStream_t)stream));
        }
    }
    IGemm g;
    g.x = x; g.w = w; g.bias = bias; g.res = residual; g.y = y;
    g.B = M; g.Cin = K; g.xC = K; g.M = M; g.N = N; g.K = K; g.Kp = K; g.ldy = N; g.ldr = N; g.act = act; g.out_f32 = out_f32;
    return op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_linear_impl(const void* x, const void* w, const float* bias, const void* residual, void* y, int dtype, int M, int N, int K,
                       int act, int out_f32, int impl, void* stream) {
    IGemm g;
    g.x = x; g.w = w; g.bias = bias; g.res = residual; g.y = y;
    g.B = M; g.Cin = K; g.xC = K; g.M = M; g.N = N; g.K = K; g.Kp = K; g.ldy = N; g.ldr = N; g.act = act; g.out_f32 = out_f32;
    g.impl = impl;
    return op_rc(launch_igemm(g, op_dt(dtype), (hipStream_t)stream));
}
static int op_vla_layer(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out, float* const* pooled,
                        int ld_pool, const void* wo, const float* bo, const void* w1, const float* b1, const void* w2, const float* b2, const float* g1,
                        const float* be1, const float* g2, const float* be2, const int32_t* lens, int dtype, int B, int L, int d_ff, int streams,
                        void* stream, int wfrag);
int hcm_op_vla_layer(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out, float* const* pooled,
                     int ld_pool, const void* wo, const float* bo, const void* w1, const float* b1, const void* w2, const float* b2, const float* g1,
                     const float* be1, const float* g2, const float* be2, const int32_t* lens, int dtype, int B, int L, int d_ff, int streams,
                     void* stream) {
    return op_vla_layer(q, I, kv, Lk, att, out, pooled, ld_pool, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, lens, dtype, B, L, d_ff, streams, stream, 0);
}
int hcm_op_vla_layer_frag(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out,
                          float* const* pooled, int ld_pool, const void* wo_frag, const float* bo, const void* w1_frag, const float* b1,
                          const void* w2_frag, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                          const int32_t* lens, int dtype, int B, int L, int d_ff, int streams, void* stream) {
    return op_vla_layer(q, I, kv, Lk, att, out, pooled, ld_pool, wo_frag, bo, w1_frag, b1, w2_frag, b2, g1, be1, g2, be2, lens, dtype, B, L, d_ff, streams,
                        stream, 1);
}
static int op_vla_layer(const void* q, const void* I, const void* const* kv, const int* Lk, const void* const* att, void* const* out, float* const* pooled,
                        int ld_pool, const void* wo, const float* bo, const void* w1, const float* b1, const void* w2, const float* b2, const float* g1,
                        const float* be1, const float* g2, const float* be2, const int32_t* lens, int dtype, int B, int L, int d_ff, int streams,
                        void* stream, int wfrag) {
    if (!I || !out || !wo || !w1 || !w2 || !bo || !b1 || !b2 || !g1 || !be1 || !g2 || !be2 || streams < 1 || streams > 2) return HCM_ERR_ARG;
    if (!vla_post_ok(op_dt(dtype), 256, 4, d_ff)) return HCM_ERR_ARG;
    VlaPost p;
    p.q = q; p.I = I; p.B = B; p.L = L; p.d_ff = d_ff; p.lens = lens; p.streams = streams; p.ld_pool = ld_pool;
    p.wo = wo; p.bo = bo; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.g1 = g1; p.be1 = be1; p.g2 = g2; p.be2 = be2;
    p.wfrag = wfrag;
    p.fuse_att = kv != nullptr;
    if (p.fuse_att && (!q || !Lk)) return HCM_ERR_ARG;
    if (!p.fuse_att && !att) return HCM_ERR_ARG;
    for (int s = 0; s < streams; ++s) {
        if (p.fuse_att) { p.kv[s] = kv[s]; p.Lk[s] = Lk[s]; } else p.att[s] = att[s];
        p.out[s] = out[s];
        p.pooled[s] = pooled ? pooled[s] : nullptr;
    }
    return op_rc(launch_vla_post(p, op_dt(dtype), (hipStream_t)stream));
}
int hcm_op_attention(const void* q, const void* k, const void* v, void* out, int dtype, int B, int heads, int Lq, int Lk, int ldq,
                     int ldk, int ldv, int ldo, void* stream) {
    return op_rc(launch_attention(q, k, v, out, op_dt(dtype), B, heads, Lq, Lk, ldq, ldk, ldv, ldo, B, (hipStream_t)stream));
}
int hcm_op_layernorm(const void* x, const void* residual, const float* gamma, const float* beta, void* y, int dtype, int rows,
                     int D, float eps, void* stream) {
    return op_rc(launch_layernorm(x, residual, gamma, beta, nullptr, 0, y, op_dt(dtype), rows, D, eps, (hipStream_t)stream));
}
int hcm_op_simplecnn3(const float* depth, const void* w0, const float* b0, const void* w1_frag, const float* b1, const void* w2_frag, const float* b2,
                      void* y, int dtype, int B, int H, void* stream) {
    return op_rc(launch_simplecnn3(depth, w0, b0, w1_frag, b1, w2_frag, b2, y, op_dt(dtype), B, H, (hipStream_t)stream));
}
int hcm_op_pack_frag(const void* w, void* out, int dtype, int N, int K, void* stream) {
    return op_rc(launch_pack_frag(w, out, op_dt(dtype), N, K, (hipStream_t)stream));
}
int hcm_op_bert_attn_block(const void* qkv, const void* wo, const float* bo, const void* residual, const float* residual32, const float* gamma,
                           const float* beta, void* y, float* y32, int dtype, int B, int L, const int32_t* lengths, float eps, void* stream) {
    return op_rc(launch_bert_attn_block(qkv, 2304, wo, bo, residual, residual32, gamma, beta, y, y32, op_dt(dtype), B, L, lengths, eps, (hipStream_t)stream));
}
int hcm_op_layernorm_post(const void* x, const void* residual, const float* gamma, const float* beta, const float* post, int post_rows,
                          void* y, int dtype, int rows, int D, float eps, void* stream) {
    return op_rc(launch_layernorm(x, residual, gamma, beta, post, post_rows, y, op_dt(dtype), rows, D, eps, (hipStream_t)stream));
}
int hcm_op_groupnorm(void* x_inplace, const void* residual, const float* gamma, const float* beta, int dtype, int B, int HW, int C,
                     int groups, float eps, int relu, void* stream) {
    static float* scratch = nullptr;            // partial-sum scratch of the two-launch path, grown on demand (test entry point)
    static size_t scratch_floats = 0;
    const size_t need = gn_stats_floats(B, HW, groups);
    if (need > scratch_floats) {
        if (scratch) { (void)hipDeviceSynchronize(); (void)hipFree(scratch); }
        if (hipMalloc((void**)&scratch, need * 4) != hipSuccess) return HCM_ERR_NOMEM;
        scratch_floats = need;
    }
    return op_rc(launch_groupnorm(x_inplace, residual, gamma, beta, scratch, op_dt(dtype), B, HW, C, groups, eps, relu, (hipStream_t)stream));
}
int hcm_op_conv2d_gn_large(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* residual, void* y,
                           int dtype, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int groups, float eps,
                           int relu, void* stream) {
    if (groups < 1 || Cout % groups) return HCM_ERR_ARG;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1, hw = Ho * Wo, dt = op_dt(dtype);
    if (!groupnorm_apply_ok(dt, hw, Cout, groups)) return HCM_ERR_ARG;
    static float* scratch = nullptr;
    static size_t scratch_floats = 0;
    const size_t need = gn_stats_floats(B, hw, groups);
    if (need > scratch_floats) {
        if (scratch) { (void)hipDeviceSynchronize(); (void)hipFree(scratch); }
        if (hipMalloc((void**)&scratch, need * 4) != hipSuccess) return HCM_ERR_NOMEM;
        scratch_floats = need;
    }
    IGemm g;
    g.x = x; g.w = w_ohwi; g.y = y;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.xC = Cin; g.Ho = Ho; g.Wo = Wo;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.M = B * hw; g.N = Cout; g.K = KH * KW * Cin; g.Kp = g.K; g.ldy = Cout; g.ldr = Cout; g.act = ACT_NONE;
    g.cs_part = scratch; g.cs_cg = Cout / groups; g.cs_hw = hw; g.cs_G = groups;
    int rc = op_rc(launch_igemm(g, dt, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    return op_rc(launch_groupnorm_apply(y, residual, gamma, beta, scratch, hw / 64, dt, B, hw, Cout, groups, eps, relu, (hipStream_t)stream));
}
// conv (statistics from its epilogue) -> max-pool over relu(GroupNorm(.)) applied on load (maxpool_gn_kernel): the depth stem as forward.cpp runs it
int hcm_op_conv2d_gn_pool(const void* x, const void* w_ohwi, const float* gamma, const float* beta, void* y, int dtype, int B, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int groups, float eps, void* stream) {
    if (groups < 1 || Cout % groups) return HCM_ERR_ARG;
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1, hw = Ho * Wo, dt = op_dt(dtype);
    if (!groupnorm_apply_ok(dt, hw, Cout, groups) || !maxpool_gn_ok(dt, Cout, groups)) return HCM_ERR_ARG;
    const size_t stats_bytes = (gn_stats_floats(B, hw, groups) * 4 + 255) / 256 * 256, map_bytes = (size_t)B * hw * Cout * 2;
    char* sc = (char*)op_scratch(stats_bytes + map_bytes);
    if (!sc) return HCM_ERR_NOMEM;
    float* stats = (float*)sc;
    void* raw = sc + stats_bytes;
    IGemm g;
    g.x = x; g.w = w_ohwi; g.y = raw;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.xC = Cin; g.Ho = Ho; g.Wo = Wo;
    g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
    g.M = B * hw; g.N = Cout; g.K = KH * KW * Cin; g.Kp = g.K; g.ldy = Cout; g.ldr = Cout; g.act = ACT_NONE;
    g.cs_part = stats; g.cs_cg = Cout / groups; g.cs_hw = hw; g.cs_G = groups;
    int rc = op_rc(launch_igemm(g, dt, (hipStream_t)stream));
    if (rc != HCM_OK) return rc;
    const int Hp = (Ho + 2 - 3) / 2 + 1, Wp = (Wo + 2 - 3) / 2 + 1;
    return op_rc(launch_maxpool3x3s2_gn(raw, y, gamma, beta, stats, hw / 64, eps, groups, dt, B, Ho, Wo, Cout, Hp, Wp, (hipStream_t)stream));
}
// y = relu(GN(conv(x, w)) + round(GN2(conv(x2, w2)))) in ONE normalisation pass over both un-normalised maps (gn_apply2_kernel): the end of a stage-first
// bottleneck of the GroupNorm trunk (the second conv is the down-sample branch); both convs 1x1 / same output map
int hcm_op_conv2d_gn_res2(const void* x, const void* w_ohwi, const float* gamma, const float* beta, const void* x2, const void* w2_ohwi, const float* gamma2,
                          const float* beta2, void* y, int dtype, int B, int H, int W, int Cin, int Cin2, int stride2, int Cout, int groups, float eps,
                          int relu, void* stream) {
    if (groups < 1 || Cout % groups || stride2 < 1) return HCM_ERR_ARG;
    const int hw = H * W, dt = op_dt(dtype);
    if (!groupnorm_apply_ok(dt, hw, Cout, groups)) return HCM_ERR_ARG;
    const size_t stats_bytes = (gn_stats_floats(B, hw, groups) * 4 + 255) / 256 * 256, map_bytes = (size_t)B * hw * Cout * 2;
    char* sc = (char*)op_scratch(2 * stats_bytes + map_bytes);
    if (!sc) return HCM_ERR_NOMEM;
    float* st1 = (float*)sc;
    float* st2 = (float*)(sc + stats_bytes);
    void* raw2 = sc + 2 * stats_bytes;
    for (int which = 0; which < 2; ++which) {
        IGemm g;
        g.x = which ? x2 : x; g.w = which ? w2_ohwi : w_ohwi; g.y = which ? raw2 : y;
        const int st = which ? stride2 : 1, ci = which ? Cin2 : Cin;
        g.B = B; g.H = H * st; g.W = W * st; g.Cin = ci; g.xC = ci; g.Ho = H; g.Wo = W;
        g.KH = 1; g.KW = 1; g.stride = st; g.pad = 0;
        g.M = B * hw; g.N = Cout; g.K = ci; g.Kp = ci; g.ldy = Cout; g.ldr = Cout; g.act = ACT_NONE;
        g.cs_part = which ? st2 : st1; g.cs_cg = Cout / groups; g.cs_hw = hw; g.cs_G = groups;
        const int rc = op_rc(launch_igemm(g, dt, (hipStream_t)stream));
        if (rc != HCM_OK) return rc;
    }
    return op_rc(launch_groupnorm_apply2(y, raw2, gamma, beta, st1, gamma2, beta2, st2, hw / 64, dt, B, hw, Cout, groups, eps, eps, relu, (hipStream_t)stream));
}
int hcm_op_val_loss(const float* logits, const float* vel, const float* stop, const int64_t* oracle_subtask, const float* corrected_actions,
                    const float* oracle_stop, float* result, int rows, int A, int num_sub_tasks, void* stream) {
    if (!logits || !vel || !stop || !oracle_subtask || !corrected_actions || !oracle_stop || !result || rows < 1 || A < 1 || num_sub_tasks < 0)
        return HCM_ERR_ARG;
    return op_rc(launch_val_loss(logits, A, vel, 2, stop, 1, oracle_subtask, corrected_actions, oracle_stop, result, rows, A, num_sub_tasks, 2,
                                 (hipStream_t)stream));
}

int hcm_op_flat_val_loss(const float* out, const float* stop, const float* progress_hat, const float* corrected_actions, const float* oracle_stop,
                         const float* progress, float* result, int rows, int num_actions, void* stream) {
    if (!out || !stop || !corrected_actions || !oracle_stop || !result || rows < 1 || num_actions < 1 || (progress_hat == nullptr) != (progress == nullptr))
        return HCM_ERR_ARG;
    return op_rc(launch_flat_val_loss(out, num_actions, stop, 1, progress_hat, 1, corrected_actions, oracle_stop, progress, result, rows, num_actions,
                                      (hipStream_t)stream));
}

int hcm_op_state_scan(const float* pre, const float* w_hh, const float* b_hh, const float* h_in, const float* masks, float* seq_out, float* h_out,
                      int T, int N, int hidden, int rnn_type, void* stream) {
    if (!pre || !w_hh || !h_in || !masks || !seq_out || !h_out || T < 1 || N < 1 || !state_scan_ok(hidden)) return HCM_ERR_ARG;
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return HCM_ERR_ARG;
    const int G = rnn_type == HCM_LSTM ? 4 : 3;
    hipStream_t st = (hipStream_t)stream;
    const size_t wn = (size_t)hidden * hidden * 4;
    std::vector<float> w((size_t)G * hidden * hidden), packed(wn);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(w.data(), w_hh, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return HCM_ERR_HIP;
    state_scan_pack(w.data(), packed.data(), hidden, G);
    float* ws = nullptr;
    if (hipMalloc((void**)&ws, wn * 4) != hipSuccess) return HCM_ERR_NOMEM;
    hipError_t e = hipMemcpy(ws, packed.data(), wn * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_state_scan(pre, ws, b_hh, h_in, masks, seq_out, h_out, nullptr, nullptr, T, N, hidden, rnn_type == HCM_GRU ? 1 : 0, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(ws);
    return op_rc(e != hipSuccess ? e : e2);
}

int hcm_op_state_scan_train(const float* pre, const float* w_hh, const float* b_hh, const float* h_in, const float* masks, float* seq_out, float* h_out,
                            float* gates, float* c_seq, float* work, int T, int N, int hidden, int rnn_type, void* stream) {
    if (!pre || !w_hh || !h_in || !masks || !seq_out || !h_out || !gates || !work || T < 1 || N < 1 || !state_scan_ok(hidden)) return HCM_ERR_ARG;
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return HCM_ERR_ARG;
    if ((c_seq == nullptr) != (rnn_type == HCM_GRU)) return HCM_ERR_ARG;
    return op_rc(launch_state_scan_train(pre, w_hh, b_hh, h_in, masks, seq_out, h_out, gates, c_seq, work, T, N, hidden, rnn_type == HCM_GRU ? 1 : 0,
                                         (hipStream_t)stream));
}

int hcm_op_state_scan_bwd(const float* d_seq, const float* gates, const float* c_seq, const float* seq_out, const float* h_in, const float* masks,
                          const float* w_hh, float* work, float* d_pre, float* d_gh, float* d_h_in, int T, int N, int hidden, int rnn_type,
                          void* stream) {
    if (!d_seq || !gates || !seq_out || !h_in || !masks || !w_hh || !work || !d_pre || !d_h_in || T < 1 || N < 1 || !state_scan_ok(hidden))
        return HCM_ERR_ARG;
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return HCM_ERR_ARG;
    const bool gru = rnn_type == HCM_GRU;
    if ((c_seq == nullptr) != gru || (d_gh == nullptr) == gru) return HCM_ERR_ARG;
    // every workgroup of a step reads the packed weights and both carries in `work` while the outputs are stored: no output may lie inside it
    const size_t NH = (size_t)N * hidden, rows = (size_t)T * N * (gru ? 3 : 4) * hidden;
    const uintptr_t w0 = (uintptr_t)work, w1 = w0 + ((size_t)4 * hidden * hidden + 4 * NH) * sizeof(float);
    const auto in_work = [&](const float* p, size_t n) { return p && (uintptr_t)p < w1 && (uintptr_t)p + n * sizeof(float) > w0; };
    if (in_work(d_h_in, (gru ? 1 : 2) * NH) || in_work(d_pre, rows) || in_work(d_gh, rows)) return HCM_ERR_ARG;
    return op_rc(launch_state_scan_bwd(d_seq, gates, c_seq, seq_out, h_in, masks, w_hh, work, d_pre, d_gh, d_h_in, T, N, hidden, gru ? 1 : 0,
                                       (hipStream_t)stream));
}

int64_t hcm_op_vla_train_work_floats(int B, int L, int Lk, int d_ff) {
    return vla_train_ok(B, L, Lk, d_ff) ? (int64_t)vla_train_work_floats(B, L, Lk, d_ff) : 0;
}

// the kernels move 16 bytes per lane (4 for the keep masks); no output may lie inside the work buffer, which the launches read while they store
static bool vla_train_aligned(std::initializer_list<const void*> f32, std::initializer_list<const void*> u8) {
    for (const void* p : f32) if ((uintptr_t)p % 16) return false;
    for (const void* p : u8) if ((uintptr_t)p % 4) return false;
    return true;
}
static bool vla_train_in_work(const float* work, size_t work_floats, std::initializer_list<std::pair<const void*, size_t>> outs) {
    const uintptr_t w0 = (uintptr_t)work, w1 = w0 + work_floats * sizeof(float);
    for (const auto& o : outs)
        if (o.first && (uintptr_t)o.first < w1 && (uintptr_t)o.first + o.second * sizeof(float) > w0) return true;
    return false;
}

int hcm_op_vla_layer_train(const float* q, const float* I, const float* kv, const float* wo, const float* bo, const float* w1, const float* b1,
                           const float* w2, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                           const uint8_t* keep1, const uint8_t* keep2, const uint8_t* keep3, float p, float* out, float* a, float* x1, float* x1hat,
                           float* h, float* x2hat, float* rstd, float* work, int B, int L, int Lk, int d_ff, void* stream) {
    if (!q || !I || !kv || !wo || !bo || !w1 || !b1 || !w2 || !b2 || !g1 || !be1 || !g2 || !be2 || !out || !a || !x1 || !x1hat || !h || !x2hat || !rstd ||
        !work || !(p >= 0.f && p < 1.f) || !vla_train_ok(B, L, Lk, d_ff))
        return HCM_ERR_ARG;
    if (!vla_train_aligned({I, wo, w1, w2, g1, be1, g2, be2, out, a, x1, x1hat, x2hat, work}, {keep1, keep2, keep3})) return HCM_ERR_ARG;
    const size_t rows = (size_t)B * L;
    if (vla_train_in_work(work, vla_train_work_floats(B, L, Lk, d_ff),
                          {{out, rows * 256}, {a, rows * 256}, {x1, rows * 256}, {x1hat, rows * 256}, {h, rows * d_ff}, {x2hat, rows * 256}, {rstd, rows * 2}}))
        return HCM_ERR_ARG;
    VlaTrainArgs t;
    t.q = q; t.I = I; t.kv = kv; t.wo = wo; t.bo = bo; t.w1 = w1; t.b1 = b1; t.w2 = w2; t.b2 = b2; t.g1 = g1; t.be1 = be1; t.g2 = g2; t.be2 = be2;
    t.keep1 = keep1; t.keep2 = keep2; t.keep3 = keep3; t.p = p;
    t.out = out; t.a = a; t.x1 = x1; t.x1hat = x1hat; t.h = h; t.x2hat = x2hat; t.rstd = rstd; t.work = work;
    t.B = B; t.L = L; t.Lk = Lk; t.d_ff = d_ff;
    return op_rc(launch_vla_train_fwd(t, (hipStream_t)stream));
}

int hcm_op_vla_layer_bwd(const float* d_out, const float* q, const float* kv, const float* wo, const float* w1, const float* w2, const float* g1,
                         const float* g2, const uint8_t* keep1, const uint8_t* keep2, const uint8_t* keep3, float p, const float* x1hat, const float* h,
                         const float* x2hat, const float* rstd, float* work, float* d_q, float* d_I, float* d_kv, float* d_u, float* d_hpre, float* d_z,
                         float* d_ln, int B, int L, int Lk, int d_ff, void* stream) {
    if (!d_out || !q || !kv || !wo || !w1 || !w2 || !g1 || !g2 || !x1hat || !h || !x2hat || !rstd || !work || !d_q || !d_I || !d_kv || !d_u || !d_hpre ||
        !d_z || !d_ln || !(p >= 0.f && p < 1.f) || !vla_train_ok(B, L, Lk, d_ff))
        return HCM_ERR_ARG;
    if (!vla_train_aligned({d_out, wo, w1, w2, g1, g2, x1hat, x2hat, work, d_I, d_u, d_z}, {keep1, keep2, keep3})) return HCM_ERR_ARG;
    const size_t rows = (size_t)B * L;
    if (vla_train_in_work(work, vla_train_work_floats(B, L, Lk, d_ff),
                          {{d_q, rows * 256}, {d_I, rows * 256}, {d_kv, (size_t)B * Lk * 512}, {d_u, rows * 256}, {d_hpre, rows * d_ff}, {d_z, rows * 256}, {d_ln, 1024}}))
        return HCM_ERR_ARG;
    VlaTrainArgs t;
    t.d_out = d_out; t.q = q; t.kv = kv; t.wo = wo; t.w1 = w1; t.w2 = w2; t.g1 = g1; t.g2 = g2;
    t.keep1 = keep1; t.keep2 = keep2; t.keep3 = keep3; t.p = p;
    t.x1hat = const_cast<float*>(x1hat); t.h = const_cast<float*>(h); t.x2hat = const_cast<float*>(x2hat); t.rstd = const_cast<float*>(rstd); t.work = work;
    t.d_q = d_q; t.d_I = d_I; t.d_kv = d_kv; t.d_u = d_u; t.d_hpre = d_hpre; t.d_z = d_z; t.d_ln = d_ln;
    t.B = B; t.L = L; t.Lk = Lk; t.d_ff = d_ff;
    return op_rc(launch_vla_train_bwd(t, (hipStream_t)stream));
}

int64_t hcm_op_embed_ln_work_floats(int rows, int K) { return embed_train_ok(rows, K) ? (int64_t)embed_train_work_floats(rows, K) : 0; }

int hcm_op_embed_ln_train(const float* x, const float* w, const float* b, const float* gamma, const float* beta, const uint8_t* keep, float p,
                          const float* post, int period, float* y, float* xhat, float* rstd, uint8_t* gate, float* work, int rows, int K, void* stream) {
    if (!embed_train_ok(rows, K) || !(p >= 0.f && p < 1.f) || (post && period < 1)) return HCM_ERR_ARG;
    if (rows == 0) return HCM_OK;
    if (!x || !w || !b || !gamma || !beta || !y || !xhat || !rstd || !gate || !work) return HCM_ERR_ARG;
    if (!vla_train_aligned({x, w, gamma, beta, post, y, xhat, work}, {keep, gate})) return HCM_ERR_ARG;
    const size_t n = (size_t)rows * 256;
    if (vla_train_in_work(work, embed_train_work_floats(rows, K), {{y, n}, {xhat, n}, {rstd, (size_t)rows}, {gate, n / 4}})) return HCM_ERR_ARG;
    EmbedTrainArgs t;
    t.x = x; t.w = w; t.b = b; t.gamma = gamma; t.beta = beta; t.keep = keep; t.p = p; t.post = post; t.period = period;
    t.y = y; t.xhat = xhat; t.rstd = rstd; t.gate = gate; t.work = work; t.rows = rows; t.K = K;
    return op_rc(launch_embed_train_fwd(t, (hipStream_t)stream));
}

int hcm_op_embed_ln_bwd(const float* d_y, const float* w, const float* gamma, const float* xhat, const float* rstd, const uint8_t* gate, float p,
                        float* work, float* d_pre, float* d_x, float* d_ln, int rows, int K, void* stream) {
    if (!embed_train_ok(rows, K) || !(p >= 0.f && p < 1.f) || !d_ln || !work) return HCM_ERR_ARG;
    if (rows && (!d_y || !w || !gamma || !xhat || !rstd || !gate || !d_pre)) return HCM_ERR_ARG;
    if (!vla_train_aligned({d_y, w, gamma, xhat, work, d_pre, d_x}, {gate})) return HCM_ERR_ARG;
    const size_t n = (size_t)rows * 256;
    if (vla_train_in_work(work, embed_train_work_floats(rows, K), {{d_pre, n}, {d_x, (size_t)rows * K}, {d_ln, 512}})) return HCM_ERR_ARG;
    EmbedTrainArgs t;
    t.d_y = d_y; t.w = w; t.gamma = gamma; t.xhat = const_cast<float*>(xhat); t.rstd = const_cast<float*>(rstd); t.gate = const_cast<uint8_t*>(gate);
    t.p = p; t.work = work; t.d_pre = d_pre; t.d_x = d_x; t.d_ln = d_ln; t.rows = rows; t.K = K;
    return op_rc(launch_embed_train_bwd(t, (hipStream_t)stream));
}

int64_t hcm_op_instr_scan_work_floats(int B, int L, int dirs, int rnn_type) {
    if (!instr_scan_train_ok(B, L, 256, dirs) || (rnn_type != HCM_LSTM && rnn_type != HCM_GRU)) return 0;
    return (int64_t)instr_scan_work_floats(dirs);
}

static int instr_arg_err(const char* what) {
    g_create_err = std::string("instruction scan: ") + what;
    return HCM_ERR_ARG;
}
// hidden size, directions and cell kind of the three instruction-scan ops
static int instr_scan_dims(int B, int L, int hidden, int dirs, int rnn_type) {
    if (hidden != 256) return instr_arg_err("hidden size must be 256 (256 units x 4 partitions = 1024 threads)");
    if (dirs != 1 && dirs != 2) return instr_arg_err("dirs must be 1 or 2");
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return instr_arg_err("rnn_type must be HCM_LSTM or HCM_GRU");
    if (B < 1 || L < 1) return instr_arg_err("B and L must be at least 1");
    return HCM_OK;
}
// the forward scan's inputs from tensors stacked per direction: pre (dirs, B*L, G*256), wt (dirs, 256, 256, 4), b_hn (dirs, 256) or null
static InstrScanArgs instr_scan_args(const float* pre, const float* wt, const float* b_hn, const int32_t* lengths, int B, int L, int dirs, bool gru) {
    InstrScanArgs a;
    for (int d = 0; d < dirs; ++d) {
        a.pre[d] = pre + (size_t)d * B * L * (gru ? 3 : 4) * 256;
        a.wt[d] = wt + (size_t)d * 4 * 256 * 256;
        a.bhn[d] = b_hn ? b_hn + (size_t)d * 256 : nullptr;
    }
    a.lengths = lengths; a.B = B; a.L = L;
    return a;
}

int hcm_op_instr_scan_train(const float* pre, const float* w_hh, const float* b_hn, const int32_t* lengths, float* out, float* final, float* gates,
                            float* c_seq, float* work, int B, int L, int hidden, int dirs, int rnn_type, void* stream) {
    const int rc = instr_scan_dims(B, L, hidden, dirs, rnn_type);
    if (rc != HCM_OK) return rc;
    const bool gru = rnn_type == HCM_GRU;
    if (!pre || !w_hh || !lengths || !out || !gates || !work) return instr_arg_err("a required pointer is NULL");
    if (gru && !b_hn) return instr_arg_err("b_hn is required for GRU");
    if ((c_seq == nullptr) != gru) return instr_arg_err("c_seq is required for LSTM and must be NULL for GRU");
    if (!vla_train_aligned({pre, w_hh, b_hn, out, final, gates, c_seq, work}, {lengths})) return instr_arg_err("float tensors must be 16-byte aligned, lengths 4-byte");
    const size_t BL = (size_t)B * L, H = 256;
    if (vla_train_in_work(work, instr_scan_work_floats(dirs), {{out, BL * dirs * H}, {final, (size_t)B * H}, {gates, dirs * BL * 4 * H}, {c_seq, dirs * BL * H}}))
        return instr_arg_err("an output overlaps work");
    const hipError_t e = launch_instr_scan_pack_fwd(w_hh, work, dirs, gru ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return op_rc(e);
    InstrScanArgs a = instr_scan_args(pre, work, b_hn, lengths, B, L, dirs, gru);
    a.out = out; a.ld_out = dirs * hidden; a.fin = final; a.ld_fin = hidden; a.fin_rows = B; a.gates = gates; a.cseq = c_seq;
    return op_rc(launch_instr_scan(a, dirs, gru ? 1 : 0, (hipStream_t)stream));
}

int hcm_op_instr_scan_bwd(const float* d_out, const float* d_final, const float* gates, const float* c_seq, const float* out, const float* w_hh,
                          const int32_t* lengths, float* work, float* d_pre, float* d_gh, int B, int L, int hidden, int dirs, int rnn_type,
                          void* stream) {
    const int rc = instr_scan_dims(B, L, hidden, dirs, rnn_type);
    if (rc != HCM_OK) return rc;
    const bool gru = rnn_type == HCM_GRU;
    if (!gates || !out || !w_hh || !lengths || !work || !d_pre) return instr_arg_err("a required pointer is NULL");
    if ((c_seq == nullptr) != gru) return instr_arg_err("c_seq is required for LSTM and must be NULL for GRU");
    if ((d_gh == nullptr) == gru) return instr_arg_err("d_gh is required for GRU and must be NULL for LSTM");
    if (!vla_train_aligned({d_out, d_final, gates, c_seq, out, w_hh, work, d_pre, d_gh}, {lengths})) return instr_arg_err("float tensors must be 16-byte aligned, lengths 4-byte");
    const size_t n = (size_t)dirs * B * L * (gru ? 3 : 4) * 256;
    if (vla_train_in_work(work, instr_scan_work_floats(dirs), {{d_pre, n}, {d_gh, n}})) return instr_arg_err("an output overlaps work");
    return op_rc(launch_instr_scan_bwd(d_out, d_final, gates, c_seq, out, w_hh, lengths, work, d_pre, d_gh, B, L, hidden, dirs, gru ? 1 : 0,
                                       (hipStream_t)stream));
}

int hcm_op_instr_scan_infer(const float* pre, const float* wt, const float* b_hn, const int32_t* lengths, float* out, int B, int L, int hidden, int dirs,
                            int rnn_type, int final_only, void* stream) {
    const int rc = instr_scan_dims(B, L, hidden, dirs, rnn_type);
    if (rc != HCM_OK) return rc;
    const bool gru = rnn_type == HCM_GRU;
    if (!pre || !wt || !lengths || !out || (gru && !b_hn)) return instr_arg_err("a required pointer is NULL");
    if (final_only && dirs != 1) return instr_arg_err("the final-state scan has one direction");
    if (!final_only && gru) return instr_arg_err("the engines have no one-launch full-output GRU scan");
    InstrScanArgs a = instr_scan_args(pre, wt, b_hn, lengths, B, L, dirs, gru);
    if (final_only) a.fin = out, a.ld_fin = hidden, a.fin_rows = B;
    else a.out = out, a.ld_out = dirs * hidden;
    return op_rc(launch_instr_scan(a, dirs, gru ? 1 : 0, (hipStream_t)stream));
}

int64_t hcm_op_attn1q_work_floats(int B, int C0, int Ce, int I) {
    return attn1q_train_ok(B, C0, Ce, I) ? (int64_t)attn1q_train_work_floats(B, C0, Ce, I) : 0;
}

static int attn1q_arg_err(const char* what) {
    g_create_err = std::string("attn1q: ") + what;
    return HCM_ERR_ARG;
}
// layout, sizes and the tail of the two attn1q ops
static int attn1q_dims(const float* e, int layout, int B, int C0, int Ce, int I) {
    if (layout != HCM_ATTN_TOKEN_MAJOR && layout != HCM_ATTN_CHANNEL_MAJOR) return attn1q_arg_err("layout must be HCM_ATTN_TOKEN_MAJOR or HCM_ATTN_CHANNEL_MAJOR");
    if (B < 0 || C0 < 1 || Ce < 0) return attn1q_arg_err("B and Ce must be at least 0, C0 at least 1");
    if (I < 1 || I > 256) return attn1q_arg_err("I must be in 1..256");
    if ((int64_t)C0 + Ce > 4096) return attn1q_arg_err("C0 + Ce must be at most 4096");
    if (Ce % 4) return attn1q_arg_err("Ce must be a multiple of 4");
    if ((e != nullptr) != (Ce > 0)) return attn1q_arg_err("e is given exactly when Ce > 0");
    return HCM_OK;
}

int hcm_op_attn1q_train(const float* qt, const float* x, const float* e, int layout, int mask_zero, float scale, float* a, float* xbar, float* work,
                        int B, int C0, int Ce, int I, void* stream) {
    const int rc = attn1q_dims(e, layout, B, C0, Ce, I);
    if (rc != HCM_OK) return rc;
    if (B == 0) return HCM_OK;
    if (!qt || !x || !a || !xbar) return attn1q_arg_err("a required pointer is NULL");
    if (!vla_train_aligned({qt, x, e, a, xbar, work}, {})) return attn1q_arg_err("float tensors must be 16-byte aligned");
    if (work && vla_train_in_work(work, attn1q_train_work_floats(B, C0, Ce, I), {{a, (size_t)B * I}, {xbar, (size_t)B * (C0 + Ce)}}))
        return attn1q_arg_err("an output overlaps work");
    Attn1qTrainArgs t;
    t.qt = qt; t.x = x; t.e = e; t.layout = layout; t.mask_zero = mask_zero; t.scale = scale; t.a = a; t.xbar = xbar; t.work = work;
    t.B = B; t.C0 = C0; t.Ce = Ce; t.I = I;
    return op_rc(launch_attn1q_train_fwd(t, (hipStream_t)stream));
}

int hcm_op_attn1q_bwd(const float* d_xbar, const float* qt, const float* x, const float* e, const float* a, int layout, float scale, float* d_qt,
                      float* d_x, float* d_e, float* work, int B, int C0, int Ce, int I, void* stream) {
    const int rc = attn1q_dims(e, layout, B, C0, Ce, I);
    if (rc != HCM_OK) return rc;
    if ((d_e != nullptr) != (Ce > 0)) return attn1q_arg_err("d_e is required exactly when e is given");
    if (Ce && B && !work) return attn1q_arg_err("work is required when e is given");
    if (B && (!d_xbar || !qt || !x || !a || !d_qt)) return attn1q_arg_err("a required pointer is NULL");
    if (!vla_train_aligned({d_xbar, qt, x, e, a, d_qt, d_x, d_e, work}, {})) return attn1q_arg_err("float tensors must be 16-byte aligned");
    const size_t C = (size_t)C0 + Ce;
    if (work && vla_train_in_work(work, attn1q_train_work_floats(B, C0, Ce, I), {{d_qt, B * C}, {d_x, (size_t)B * C0 * I}, {d_e, (size_t)I * Ce}}))
        return attn1q_arg_err("an output overlaps work");
    Attn1qTrainArgs t;
    t.d_xbar = d_xbar; t.qt = qt; t.x = x; t.e = e; t.a = const_cast<float*>(a); t.layout = layout; t.scale = scale;
    t.d_qt = d_qt; t.d_x = d_x; t.d_e = d_e; t.work = work; t.B = B; t.C0 = C0; t.Ce = Ce; t.I = I;
    return op_rc(launch_attn1q_train_bwd(t, (hipStream_t)stream));
}

int64_t hcm_op_flat_heads_work_floats(int rows, int hidden, int num_actions) {
    return flat_heads_ok(rows, hidden, num_actions) ? (int64_t)flat_heads_work_floats(rows, num_actions) : 0;
}

static int flat_heads_arg_err(const char* what) {
    g_create_err = std::string("flat_heads: ") + what;
    return HCM_ERR_ARG;
}
static int flat_heads_dims(int rows, int hidden, int num_actions) {
    if (hidden != 512) return flat_heads_arg_err("hidden must be 512");
    if (num_actions < 1 || num_actions > 4) return flat_heads_arg_err("num_actions must be in 1..4");
    if (rows < 0) return flat_heads_arg_err("rows must be at least 0");
    return HCM_OK;
}

int hcm_op_flat_heads_loss_train(const float* x, const float* w_lin, const float* b_lin, const float* w_stop, const float* b_stop, const float* w_pm,
                                 const float* b_pm, const float* corrected_actions, const float* oracle_stop, const float* progress, float* out,
                                 float* stop, float* progress_hat, float* result, int rows, int hidden, int num_actions, void* stream) {
    const int rc = flat_heads_dims(rows, hidden, num_actions);
    if (rc != HCM_OK) return rc;
    if (rows == 0) return HCM_OK;
    if (!x || !w_lin || !b_lin || !w_stop || !b_stop || !corrected_actions || !oracle_stop || !out || !stop || !result)
        return flat_heads_arg_err("a required pointer is NULL");
    const bool monitor = w_pm != nullptr;
    if ((b_pm != nullptr) != monitor || (progress != nullptr) != monitor || (progress_hat != nullptr) != monitor)
        return flat_heads_arg_err("w_pm, b_pm, progress and progress_hat are given together or not at all");
    if (!vla_train_aligned({x, w_lin, w_stop, w_pm}, {})) return flat_heads_arg_err("x and the weights must be 16-byte aligned");
    FlatHeadsArgs t;
    t.x = x; t.w_lin = w_lin; t.b_lin = b_lin; t.w_stop = w_stop; t.b_stop = b_stop; t.w_pm = w_pm; t.b_pm = b_pm;
    t.corrected = corrected_actions; t.oracle_stop = oracle_stop; t.progress = progress;
    t.out = out; t.stop = stop; t.progress_hat = progress_hat; t.result = result; t.rows = rows; t.num_actions = num_actions;
    return op_rc(launch_flat_heads_fwd(t, (hipStream_t)stream));
}

int hcm_op_flat_heads_loss_bwd(const float* d_result, const float* x, const float* w_lin, const float* w_stop, const float* w_pm, const float* out,
                               const float* stop, const float* progress_hat, const float* corrected_actions, const float* oracle_stop,
                               const float* progress, const float* result, float* d_x, float* d_w_lin, float* d_b_lin, float* d_w_stop,
                               float* d_b_stop, float* d_w_pm, float* d_b_pm, float* work, int rows, int hidden, int num_actions, void* stream) {
    const int rc = flat_heads_dims(rows, hidden, num_actions);
    if (rc != HCM_OK) return rc;
    if (rows == 0) return HCM_OK;
    if (!d_result || !x || !w_lin || !w_stop || !out || !stop || !corrected_actions || !oracle_stop || !result || !d_w_lin || !d_b_lin || !d_w_stop ||
        !d_b_stop || !work)
        return flat_heads_arg_err("a required pointer is NULL");
    const bool monitor = w_pm != nullptr;
    if ((progress_hat != nullptr) != monitor || (progress != nullptr) != monitor || (d_w_pm != nullptr) != monitor || (d_b_pm != nullptr) != monitor)
        return flat_heads_arg_err("w_pm, progress_hat, progress, d_w_pm and d_b_pm are given together or not at all");
    if (!vla_train_aligned({x, w_lin, w_stop, w_pm, d_x, d_w_lin, d_w_stop, d_w_pm, work}, {}))
        return flat_heads_arg_err("x, d_x, the weights, their gradients and work must be 16-byte aligned");
    const size_t A = (size_t)num_actions;
    if (vla_train_in_work(work, flat_heads_work_floats(rows, num_actions),
                          {{d_x, (size_t)rows * 512}, {d_w_lin, A * 512}, {d_b_lin, A}, {d_w_stop, 512}, {d_b_stop, 1}, {d_w_pm, 512}, {d_b_pm, 1}}))
        return flat_heads_arg_err("an output overlaps work");
    FlatHeadsArgs t;
    t.d_result = d_result; t.x = x; t.w_lin = w_lin; t.w_stop = w_stop; t.w_pm = w_pm;
    t.out = const_cast<float*>(out); t.stop = const_cast<float*>(stop); t.progress_hat = const_cast<float*>(progress_hat);
    t.result = const_cast<float*>(result); t.corrected = corrected_actions; t.oracle_stop = oracle_stop; t.progress = progress;
    t.d_x = d_x; t.d_w_lin = d_w_lin; t.d_b_lin = d_b_lin; t.d_w_stop = d_w_stop; t.d_b_stop = d_b_stop; t.d_w_pm = d_w_pm; t.d_b_pm = d_b_pm;
    t.work = work; t.rows = rows; t.num_actions = num_actions;
    return op_rc(launch_flat_heads_bwd(t, (hipStream_t)stream));
}

int64_t hcm_op_subtask_ce_work_floats(int rows, int hidden, int A) {
    return subtask_ce_ok(rows, hidden, A, 1) ? (int64_t)subtask_ce_work_floats(rows, A) : 0;
}

static int subtask_ce_arg_err(const char* what) {
    g_create_err = std::string("subtask_ce: ") + what;
    return HCM_ERR_ARG;
}
static int subtask_ce_dims(int rows, int hidden, int A, int num_sub_tasks) {
    if (hidden != 512) return subtask_ce_arg_err("hidden must be 512");
    if (A < 1 || A > 6) return subtask_ce_arg_err("A must be in 1..6");
    if (num_sub_tasks < 1 || num_sub_tasks > A) return subtask_ce_arg_err("num_sub_tasks must be in 1..A");
    if (rows < 0) return subtask_ce_arg_err("rows must be at least 0");
    return HCM_OK;
}

int hcm_op_subtask_ce_train(const float* x, const float* w, const float* b, const int64_t* oracle_subtask, float* logits, float* result, int rows,
                            int hidden, int A, int num_sub_tasks, void* stream) {
    const int rc = subtask_ce_dims(rows, hidden, A, num_sub_tasks);
    if (rc != HCM_OK) return rc;
    if (rows == 0) return HCM_OK;
    if (!x || !w || !b || !oracle_subtask || !logits || !result) return subtask_ce_arg_err("a required pointer is NULL");
    if (!vla_train_aligned({x, w}, {b, logits, result}) || (uintptr_t)oracle_subtask % 8)
        return subtask_ce_arg_err("x and w must be 16-byte aligned, b, logits and result 4-byte, oracle_subtask 8-byte");
    SubtaskCeArgs t;
    t.x = x; t.w = w; t.b = b; t.oracle = oracle_subtask; t.logits = logits; t.result = result;
    t.rows = rows; t.A = A; t.num_sub_tasks = num_sub_tasks;
    return op_rc(launch_subtask_ce_fwd(t, (hipStream_t)stream));
}

int hcm_op_subtask_ce_bwd(const float* d_result, const float* x, const float* w, const float* logits, const int64_t* oracle_subtask,
                          const float* result, float* d_x, float* d_w, float* d_b, float* work, int rows, int hidden, int A, int num_sub_tasks,
                          void* stream) {
    const int rc = subtask_ce_dims(rows, hidden, A, num_sub_tasks);
    if (rc != HCM_OK) return rc;
    if (rows == 0) return HCM_OK;
    if (!d_result || !x || !w || !logits || !oracle_subtask || !result || !d_w || !d_b || !work) return subtask_ce_arg_err("a required pointer is NULL");
    if (!vla_train_aligned({x, w, d_x, d_w, work}, {d_result, logits, result, d_b}) || (uintptr_t)oracle_subtask % 8)
        return subtask_ce_arg_err("x, w, d_x, d_w and work must be 16-byte aligned, the other float tensors 4-byte, oracle_subtask 8-byte");
    if (vla_train_in_work(work, subtask_ce_work_floats(rows, A), {{d_x, (size_t)rows * 512}, {d_w, (size_t)A * 512}, {d_b, (size_t)A}}))
        return subtask_ce_arg_err("an output overlaps work");
    SubtaskCeArgs t;
    t.d_result = d_result; t.x = x; t.w = w; t.logits = const_cast<float*>(logits); t.oracle = oracle_subtask;
    t.result = const_cast<float*>(result); t.d_x = d_x; t.d_w = d_w; t.d_b = d_b; t.work = work;
    t.rows = rows; t.A = A; t.num_sub_tasks = num_sub_tasks;
    return op_rc(launch_subtask_ce_bwd(t, (hipStream_t)stream));
}

int64_t hcm_op_simplecnn_work_floats(int B, int H, int W, int Cin) {
    return simplecnn_train_ok(B, H, W, Cin) ? (int64_t)simplecnn_train_work_floats(B, H, W, Cin) : 0;
}

static int simplecnn_arg_err(const char* what) {
    g_create_err = std::string("simplecnn_train: ") + what;
    return HCM_ERR_ARG;
}
// the kernels move single floats: every float tensor on a 4-byte boundary
static bool simplecnn_aligned(std::initializer_list<const void*> f32) {
    for (const void* p : f32) if ((uintptr_t)p % 4) return false;
    return true;
}
static int simplecnn_dims(int x_dtype, int B, int H, int W, int Cin) {
    if (Cin != 1 && Cin != 3) return simplecnn_arg_err("Cin must be 1 or 3");
    if (x_dtype != HCM_F32 && !(x_dtype == HCM_U8 && Cin == 3)) return simplecnn_arg_err("frames are HCM_F32, or HCM_U8 with Cin = 3");
    if (B < 0) return simplecnn_arg_err("B must be at least 0");
    if (H < 36 || W < 36) return simplecnn_arg_err("frames must be at least 36 x 36");
    if (!simplecnn_train_ok(B, H, W, Cin)) return simplecnn_arg_err("the call is too large: an element offset would not fit 31 bits");
    return HCM_OK;
}
// the element counts of y (B, 32, h3, w3) and of the three weight tensors
static size_t simplecnn_y_floats(int B, int H, int W) {
    const int h1 = (H - 8) / 4 + 1, w1 = (W - 8) / 4 + 1, h2 = (h1 - 4) / 2 + 1, w2 = (w1 - 4) / 2 + 1;
    return (size_t)B * 32 * (h2 - 2) * (w2 - 2);
}

int hcm_op_simplecnn_train(const void* x, int x_dtype, float scale, const float* w1, const float* b1, const float* w2, const float* b2,
                           const float* w3, const float* b3, float* y, float* work, int B, int H, int W, int Cin, void* stream) {
    const int rc = simplecnn_dims(x_dtype, B, H, W, Cin);
    if (rc != HCM_OK) return rc;
    if (B == 0) return HCM_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !y || !work) return simplecnn_arg_err("a required pointer is NULL");
    if (!simplecnn_aligned({w1, b1, w2, b2, w3, b3, y, work, x_dtype == HCM_F32 ? x : nullptr}))
        return simplecnn_arg_err("the float tensors must be 4-byte aligned");
    if (vla_train_in_work(work, simplecnn_train_work_floats(B, H, W, Cin), {{y, simplecnn_y_floats(B, H, W)}}))
        return simplecnn_arg_err("an output overlaps work");
    SimpleCnnTrainArgs t;
    t.x = x; t.x_u8 = x_dtype == HCM_U8; t.scale = scale; t.w1 = w1; t.b1 = b1; t.w2 = w2; t.b2 = b2; t.w3 = w3; t.b3 = b3; t.y = y; t.work = work;
    t.B = B; t.H = H; t.W = W; t.Cin = Cin;
    return op_rc(launch_simplecnn_train_fwd(t, (hipStream_t)stream));
}

int hcm_op_simplecnn_bwd(const float* d_y, const void* x, int x_dtype, float scale, const float* w2, const float* w3, float* work, float* d_w1,
                         float* d_b1, float* d_w2, float* d_b2, float* d_w3, float* d_b3, int B, int H, int W, int Cin, void* stream) {
    const int rc = simplecnn_dims(x_dtype, B, H, W, Cin);
    if (rc != HCM_OK) return rc;
    if (!d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3) return simplecnn_arg_err("a required pointer is NULL");
    if (B > 0 && (!d_y || !x || !w2 || !w3 || !work)) return simplecnn_arg_err("a required pointer is NULL");
    if (!simplecnn_aligned({d_y, w2, w3, work, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, x_dtype == HCM_F32 ? x : nullptr}))
        return simplecnn_arg_err("the float tensors must be 4-byte aligned");
    if (B > 0 && vla_train_in_work(work, simplecnn_train_work_floats(B, H, W, Cin),
                                   {{d_w1, (size_t)32 * Cin * 64}, {d_b1, 32}, {d_w2, (size_t)64 * 512}, {d_b2, 64}, {d_w3, (size_t)32 * 576}, {d_b3, 32}}))
        return simplecnn_arg_err("an output overlaps work");
    SimpleCnnTrainArgs t;
    t.d_y = d_y; t.x = x; t.x_u8 = x_dtype == HCM_U8; t.scale = scale; t.w2 = w2; t.w3 = w3; t.work = work;
    t.d_w1 = d_w1; t.d_b1 = d_b1; t.d_w2 = d_w2; t.d_b2 = d_b2; t.d_w3 = d_w3; t.d_b3 = d_b3; t.B = B; t.H = H; t.W = W; t.Cin = Cin;
    return op_rc(launch_simplecnn_train_bwd(t, (hipStream_t)stream));
}

int hcm_op_feat_ingest(const float* x, void* y, int dtype, int rows, int C, int S, int ld, float scale, void* stream) {
    return op_rc(hcm::launch_feat_ingest(x, y, op_dt(dtype), rows, C, S, ld, scale, (hipStream_t)stream));
}
int hcm_op_feat_export(const void* y, int dtype, float* x, int rows, int C, int S, int ld, float scale, void* stream) {
    return op_rc(hcm::launch_feat_export(y, op_dt(dtype), x, rows, C, S, ld, scale, (hipStream_t)stream));
}
static bool op_feat_dt(int dtype) { return dtype == HCM_F32 || dtype == HCM_F16 || dtype == HCM_BF16; }
int hcm_op_instr_feat_ingest(const float* x, void* y, int dtype, const int32_t* lens, int B, int src_rows, int L, int D, void* stream) {
    if (!op_feat_dt(dtype)) return HCM_ERR_ARG;
    return op_rc(hcm::launch_instr_feat_ingest(x, y, op_dt(dtype), lens, B, src_rows, L, D, (hipStream_t)stream));
}
int hcm_op_instr_feat_export(const void* y, int dtype, float* x, const int32_t* lens, int rows, int L, int D, void* stream) {
    if (!op_feat_dt(dtype)) return HCM_ERR_ARG;
    return op_rc(hcm::launch_instr_feat_export(y, op_dt(dtype), x, lens, rows, L, D, (hipStream_t)stream));
}

int hcm_op_maxpool3x3s2(const void* x, void* y, int dtype, int B, int H, int W, int C, void* stream) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    return op_rc(launch_maxpool3x3s2(x, y, op_dt(dtype), B, H, W, C, Ho, Wo, (hipStream_t)stream));
}

int hcm_op_depth_run(const void* x, void* y, const void* const* w, const float* const* gn, const float* eps, int dtype, int B, int side,
                     int groups, int nblocks, int ld, void* stream) {
    if (!x || !y || !w || !gn || !eps || (dtype != HCM_F16 && dtype != HCM_BF16)) return HCM_ERR_ARG;
    // the run descriptor of either kernel from the pointer tables (its arrays hold `cap` blocks)
    auto fill = [&](auto& q, int cap) {
        if (nblocks < 1 || nblocks > cap) return false;
        q.x = x; q.y = y; q.ld = ld; q.B = B; q.groups = groups; q.nblocks = nblocks;
        for (int r = 0; r < nblocks; ++r) {
            for (int i = 0; i < 3; ++i) if (!w[3 * r + i]) return false;
            for (int i = 0; i < 6; ++i) if (!gn[6 * r + i]) return false;
            q.w1[r] = w[3 * r]; q.w2[r] = w[3 * r + 1]; q.w3[r] = w[3 * r + 2];
            q.g1[r] = gn[6 * r]; q.b1[r] = gn[6 * r + 1]; q.g2[r] = gn[6 * r + 2]; q.b2[r] = gn[6 * r + 3]; q.g3[r] = gn[6 * r + 4]; q.b3[r] = gn[6 * r + 5];
            q.eps1[r] = eps[3 * r]; q.eps2[r] = eps[3 * r + 1]; q.eps3[r] = eps[3 * r + 2];
        }
        return true;
    };
    if (side == 8) {
        DepthL3 q;
        if (!fill(q, 6)) return HCM_ERR_ARG;
        return op_rc(launch_depth_l3(q, op_dt(dtype), (hipStream_t)stream));
    }
    if (side != 32 && side != 16) return HCM_ERR_ARG;
    DepthBlk q;
    q.side = side; q.C = side == 32 ? 128 : 256; q.CM = q.C / 4;
    if (!fill(q, 4)) return HCM_ERR_ARG;
    return op_rc(launch_depth_blk(q, op_dt(dtype), (hipStream_t)stream));
}

// ------------------------------------------------------------------ the step's small kernels (csrc/elementwise.hip; include/hcm.h has the layouts)
static bool op_dt_known(int dtype) { return dtype == HCM_F32 || dtype == HCM_F16 || dtype == HCM_BF16; }
static bool op_ids_dt(int d, int* out) {
    *out = d == HCM_I64 ? DT_I64 : d == HCM_I32 ? DT_I32 : d == HCM_F32 ? DT_F32 : -1;
    return *out >= 0;
}
static bool op_aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }
// hcm_op_heads -> Heads; false on a head without its pointers, a stride below its rows, or a `pred` heads_eval cannot serve
static bool op_heads(const hcm_op_heads* in, bool allow_pred, Heads* hd) {
    if (!in) return true;
    if (in->r0 < 0 || in->r1 < 0 || in->r2 < 0) return false;
    if (in->r0 && (!in->w0 || !in->b0 || !in->out0 || in->ld0 < in->r0)) return false;
    if (in->r1 && (!in->w1 || !in->b1 || !in->out1 || in->ld1 < in->r1)) return false;
    if (in->r2 && (!in->w2 || !in->b2 || !in->out2 || in->ld2 < in->r2)) return false;
    if (in->pred) {
        if (!allow_pred || in->r0 < 1 || in->r0 > 64 || !in->emb || !in->emb_out || in->emb_rows < 1 || in->emb_dim < 0 || in->emb_ld < in->emb_dim)
            return false;
    }
    hd->w0 = in->w0; hd->b0 = in->b0; hd->out0 = in->out0; hd->r0 = in->r0; hd->ld0 = in->ld0;
    hd->w1 = in->w1; hd->b1 = in->b1; hd->out1 = in->out1; hd->r1 = in->r1; hd->ld1 = in->ld1;
    hd->w2 = in->w2; hd->b2 = in->b2; hd->out2 = in->out2; hd->r2 = in->r2; hd->ld2 = in->ld2;
    hd->pred = in->pred; hd->emb = in->emb; hd->emb_out = in->emb_out; hd->emb_rows = in->emb_rows; hd->emb_dim = in->emb_dim; hd->emb_ld = in->emb_ld;
    return true;
}
// the cells and heads_rows keep a hidden state in dynamic LDS
static bool op_hidden_ok(int hidden) { return hidden >= 1 && hidden <= 8192; }

int hcm_op_rnn_cell(const float* gates, const float* gh, const float* h_in, const float* mask, float* h_out, float* xh, int ld_xh, int col0,
                    const hcm_op_heads* heads, unsigned* bad, int B, int hidden, int rnn_type, void* stream) {
    if (!gates || !h_in || !mask || !h_out || B < 1 || !op_hidden_ok(hidden)) return HCM_ERR_ARG;
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return HCM_ERR_ARG;
    if ((gh != nullptr) != (rnn_type == HCM_GRU)) return HCM_ERR_ARG;
    if (xh && (col0 < 0 || ld_xh < col0 + hidden)) return HCM_ERR_ARG;
    Heads hd;
    if (!op_heads(heads, true, &hd)) return HCM_ERR_ARG;
    hd.bad = bad;
    if (xh) {
        const int rc = op_rc(launch_rnn_prep(h_in, mask, xh, B, hidden, ld_xh, col0, (hipStream_t)stream));
        if (rc != HCM_OK) return rc;
    }
    if (rnn_type == HCM_LSTM) return op_rc(launch_lstm_cell(gates, h_in, mask, h_out, B, hidden, hd, (hipStream_t)stream));
    return op_rc(launch_gru_cell(gates, gh, h_in, mask, h_out, B, hidden, hd, (hipStream_t)stream));
}

int hcm_op_heads_rows(const float* hs, const hcm_op_heads* heads, int rows, int hidden, void* stream) {
    Heads hd;
    if (!hs || !heads || rows < 1 || !op_hidden_ok(hidden) || !op_heads(heads, false, &hd)) return HCM_ERR_ARG;
    return op_rc(launch_heads_rows(hs, rows, hidden, hd, (hipStream_t)stream));
}

int hcm_op_instr_cell(const float* pre, const float* gh, float* h, float* c, const int32_t* lengths, float* out, int t, int B, int L, int hidden,
                      int ld_out, int col0, int rnn_type, void* stream) {
    if (!pre || !gh || !h || !lengths || !out || B < 1 || L < 1 || t < 0 || t >= L || hidden < 1 || col0 < 0 || ld_out < col0 + hidden)
        return HCM_ERR_ARG;
    if (rnn_type != HCM_LSTM && rnn_type != HCM_GRU) return HCM_ERR_ARG;
    if ((c == nullptr) != (rnn_type == HCM_GRU)) return HCM_ERR_ARG;
    if (rnn_type == HCM_GRU) return op_rc(launch_instr_gru_cell(pre, gh, h, lengths, out, t, B, L, hidden, ld_out, col0, (hipStream_t)stream));
    return op_rc(launch_instr_lstm_cell(pre, gh, h, c, lengths, out, t, B, L, hidden, ld_out, col0, (hipStream_t)stream));
}

int hcm_op_attn1q(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int32_t* lengths, float* out, int ldo, int B,
                  int S, int D, int Dv, float scale, void* stream) {
    if (!q || !k || !v || !out || B < 1 || S < 1 || S > 8192 || D < 1 || Dv < 1 || ldq < D || ldk < D || ldv < Dv || ldo < Dv) return HCM_ERR_ARG;
    return op_rc(launch_attn1q(q, ldq, k, ldk, v, ldv, lengths, out, ldo, B, S, D, Dv, scale, (hipStream_t)stream));
}

int hcm_op_adaptive_avgpool(const void* x, void* y, int dtype, int B, int H, int W, int C, int OH, int OW, int ldx, int ldy, void* stream) {
    if (!x || !y || !op_dt_known(dtype) || B < 1 || H < 1 || W < 1 || C < 1 || OH < 1 || OW < 1 || ldx < C || ldy < C) return HCM_ERR_ARG;
    if (!op_aligned(x, 16) || !op_aligned(y, 16)) return HCM_ERR_ARG;     // 16-byte chunks; C, ldx, ldy % chunk: the launcher's check
    return op_rc(launch_adaptive_avgpool(x, y, op_dt(dtype), B, H, W, C, OH, OW, ldy, (hipStream_t)stream, ldx));
}

int hcm_op_mean_rows(const void* x, void* y, int dtype, int B, int S, int C, int ldx, int ldy, int out_f32, const int32_t* lens, void* stream) {
    if (!x || !y || !op_dt_known(dtype) || B < 1 || S < 1 || C < 1 || ldx < C || ldy < C) return HCM_ERR_ARG;
    return op_rc(launch_mean_rows(x, y, op_dt(dtype), B, S, C, ldx, ldy, out_f32 ? 1 : 0, (hipStream_t)stream, lens));
}

int hcm_op_avgpool2(const float* x, void* y, int dtype, int B, int H, int W, int padded, void* stream) {
    if (!x || !y || !op_dt_known(dtype) || B < 1 || H < 2 || W < 2 || (W & 1) || !op_aligned(x, 8)) return HCM_ERR_ARG;     // float2 loads
    if (padded) return op_rc(launch_avgpool2_f32_padded(x, y, op_dt(dtype), B, H, W, (hipStream_t)stream));
    return op_rc(launch_avgpool2_f32(x, y, op_dt(dtype), B, H, W, (hipStream_t)stream));
}

int hcm_op_bert_embed(const void* ids, int ids_dtype, const float* word, const float* pos, const float* type0, const float* gamma,
                      const float* beta, void* y, int dtype, int B, int L, int D, int vocab, float eps, void* stream) {
    int idt;
    if (!ids || !word || !pos || !type0 || !gamma || !beta || !y || !op_dt_known(dtype) || !op_ids_dt(ids_dtype, &idt) || B < 1 || L < 1 || vocab < 1)
        return HCM_ERR_ARG;
    return op_rc(launch_bert_embed(ids, idt, word, pos, type0, gamma, beta, y, op_dt(dtype), B, L, D, vocab, eps, (hipStream_t)stream));
}

int hcm_op_instr_embed(const void* ids, int ids_dtype, const float* table, float* x, int32_t* lengths, int B, int L, int E, int ldx, int vocab,
                       void* stream) {
    int idt;
    if (!ids || !table || !x || !lengths || !op_ids_dt(ids_dtype, &idt) || B < 1 || L < 1 || E < 1 || ldx < E || vocab < 1) return HCM_ERR_ARG;
    return op_rc(launch_instr_embed(ids, idt, table, x, lengths, B, L, E, ldx, vocab, (hipStream_t)stream));
}

int hcm_op_layernorm_f32in(const float* x, const float* gamma, const float* beta, void* y16, float* y32, float* stats, int dtype, int rows,
                           int D, float eps, void* stream) {
    if (!x || !gamma || !beta || !y16 || rows < 1 || (y32 != nullptr) == (stats != nullptr)) return HCM_ERR_ARG;
    if (dtype != HCM_F16 && dtype != HCM_BF16) return HCM_ERR_ARG;
    if (!op_aligned(x, 16) || !op_aligned(gamma, 16) || !op_aligned(beta, 16) || !op_aligned(y16, 8) || !op_aligned(y32, 16) || !op_aligned(stats, 8))
        return HCM_ERR_ARG;
    return op_rc(launch_layernorm_f32in(x, gamma, beta, y16, y32, op_dt(dtype), rows, D, eps, (hipStream_t)stream, stats));
}

int hcm_op_absmax(const void* x, int dtype, int rows, int cols, int ld, unsigned* slot, void* stream) {
    if (!x || !slot || !op_dt_known(dtype) || rows < 1 || cols < 1 || ld < cols) return HCM_ERR_ARG;
    return op_rc(launch_absmax(x, op_dt(dtype), rows, cols, ld, slot, (hipStream_t)stream));
}

int hcm_op_argmax(const float* logits, int64_t* pred, int B, int n, int ld, void* stream) {
    if (!logits || !pred || B < 1 || n < 1 || ld < n) return HCM_ERR_ARG;
    return op_rc(launch_argmax(logits, pred, B, n, ld, (hipStream_t)stream));
}

int hcm_op_embed_rows(const float* emb, const int64_t* idx, float* y, int B, int D, int ld, int col0, int nrows, void* stream) {
    if (!emb || !idx || !y || B < 1 || D < 1 || col0 < 0 || ld < col0 + D || nrows < 1) return HCM_ERR_ARG;
    return op_rc(launch_embed_rows(emb, idx, y, B, D, ld, col0, nrows, (hipStream_t)stream));
}

int hcm_op_val_subtask(const int64_t* oracle, int64_t* subtask, int rows, int num_sub_tasks, void* stream) {
    if (!oracle || !subtask || rows < 1 || num_sub_tasks < 0) return HCM_ERR_ARG;
    return op_rc(launch_val_subtask(oracle, subtask, rows, num_sub_tasks, (hipStream_t)stream));
}

int hcm_op_fill_cols(const float* tab, void* y, int dtype, int B, int S, int C, int ldy, void* stream) {
    if (!tab || !y || !op_dt_known(dtype) || B < 1 || S < 1 || C < 1 || ldy < C) return HCM_ERR_ARG;
    return op_rc(launch_fill_cols(tab, y, op_dt(dtype), B, S, C, ldy, (hipStream_t)stream));
}

int hcm_op_copy_rows(const float* src, int ld_src, int n_src, float* dst, int ld_dst, int rows, int cols, void* stream) {
    if (!src || !dst || cols < 1 || ld_src < cols || ld_dst < cols) return HCM_ERR_ARG;
    return op_rc(launch_copy_rows(src, ld_src, n_src, dst, ld_dst, rows, cols, (hipStream_t)stream));
}

}  // extern "C"
