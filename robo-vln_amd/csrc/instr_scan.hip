// The instruction encoder's packed (bi)LSTM / GRU scan, for the engines and for training, and its reverse-time scan.  Hidden size 256, one layer, one
// or two directions, float32.  Each is ONE launch for the whole scan: a workgroup of 1024 threads owns SB samples of one direction for all of their
// steps, so the only synchronisation between steps is the workgroup barrier -- no grid barrier, no spinning, no atomics, plain vector stores, fixed
// summation order (bitwise reproducible).
//
// Packed-sequence semantics (pack_padded_sequence / pad_packed_sequence): row b is active at tokens t < length[b]; its state is the zero state in
// front of its first active token in scan order (token 0 forward, token length[b] - 1 in the reverse direction) and frozen behind its last one.
// A workgroup walks max(length) over its own samples steps, not L (the lengths are read on the device: nothing for the host to wait for, the
// launch is graph-capturable); tokens no sample of it reaches are filled in front of the loop.
//
// Forward (instr_scan_kernel<SB, GRU, FORM>): 1024 threads = 256 hidden units x 4 quarters of the k range.  Each thread streams a quarter of its
// unit's recurrent weights from L2 every step -- W_hh in the order [k][unit][4 gates], so the gate weights of (k, unit) are one 16-byte load,
// coalesced across the units (GRU: fourth slot zero, not accumulated); 4*H*H*4 bytes per step and workgroup -- for SB samples, several loads in
// flight.  h lives in LDS (double-buffered, broadcast reads), c in registers; the four partial sums per (gate, sample, unit) meet in LDS and are
// added as ((q0 + q1) + (q2 + q3)).  pre = x_t W_ih^T + bias for every token: LSTM bias b_ih + b_hh; GRU bias b_ih + (b_hr, b_hz, 0), b_hn stays
// inside the r * (.) product as in torch.  FORM says what is stored -- extra stores of values the epilogue has anyway: the sums, the cells and so
// every stored bit are the same in all three --
//   SEQ    h_t at every active token into out (ld_out floats per token, direction d at column d * 256), zero at inactive tokens: CMANet's
//          per-token encoder output (LSTM only: nothing runs it with a GRU, which is not instantiated);
//   FIN    no per-token store, only the forward direction's state behind each row's last token, straight into the caller's row (fin, ld_fin):
//          Seq2SeqNet's final_state_only encoder (instruction_encoder.py:86-90; both Seq2Seq paper configs).  B == 1 with fin_rows > 1: one
//          instruction for fin_rows frames (seq2seq.py:163 `.expand`) -- one sample is scanned, its result written to every row;
//   TRAIN  SEQ's output (also the left operand of dW_hh), FIN's final state where `fin` is given, and at every active token the post-activation
//          gates (LSTM i,f,g,o; GRU r,z,n and hn = W_hn h + b_hn) and c_t (LSTM): what the reverse scan reads.
// SB is chosen small (instr_scan_sb: 2 for B = 64 in both directions, 64 workgroups): per step a thread then does SB * 256 FMAs behind 64 16-byte
// loads, and the step is bounded by that weight stream (1 MB from L2) instead of by 8 samples' worth of FMAs and LDS broadcasts on 16 CUs (CMANet
// step at B = 64, L = 80: 3.15 -> 2.56 ms; the trunks alone take 2.4).
//
// Reverse (instr_scan_bwd_kernel<SB, GRU>): the same ownership, the direction's steps walked backwards.  Per step, with dH = d_out[b, t] + carry_h
// (+ d_fin[b] at t = length[b] - 1, forward direction), c' / h' the state in front of the step (zero at the direction's first token):
//   LSTM  tc = tanh(c_t); do = dH tc; dc = carry_c + dH o (1 - tc^2); da_i = dc g i(1-i); da_f = dc c' f(1-f); da_g = dc i (1-g^2);
//         da_o = do o(1-o); d_pre[b, t] = da; carry_c <- dc f; carry_h <- da . W_hh
//   GRU   da_n = dH (1-z)(1-n^2); da_r = da_n hn r(1-r); da_z = dH (h' - n) z(1-z); d_pre[b, t] = [da_r, da_z, da_n];
//         d_gh[b, t] = [da_r, da_z, da_n r]; carry_h <- d_gh[b, t] . W_hh + dH z
// (the formulas of state_scan_bwd.hip without masks).  Phase A: thread (sample, unit) computes the element-wise gradients from the saved values
// into LDS and stores d_pre / d_gh; carry_c stays in its registers; the saved values of the NEXT step are loaded behind it, so that their latency
// hides behind phase B.  Phase B: thread (k, quarter q) contracts a quarter of the G*256 gate rows, carry[k] = sum_row da[row] W_hh[row][k], from
// W_hh in the order [row quad][k][4 rows] (one 16-byte load per four rows, a wave's load 1 KB contiguous; packed on the stream by
// instr_scan_pack_bwd_kernel), the rows of a quad in order, the quads of a quarter in order, the quarters as ((q0 + q1) + (q2 + q3)).  carry_h is
// double-buffered in LDS.  Inactive tokens get exact zeros in d_pre / d_gh, and a cotangent at an inactive token is not read.
#include "dev.h"
#include "kernels.h"

#include <cstddef>

namespace hcm {

constexpr int kInstrH = 256;

enum { INSTR_SEQ = 0, INSTR_FIN = 1, INSTR_TRAIN = 2 };

template <int SB, bool GRU, int FORM>
__global__ __launch_bounds__(1024) void instr_scan_kernel(InstrScanArgs a) {
    constexpr int H = kInstrH, NG = GRU ? 3 : 4, KQ = H / 4;
    constexpr bool PER_TOKEN = FORM != INSTR_FIN, SAVE = FORM == INSTR_TRAIN;
    extern __shared__ float smf[];         // h [2][SB][H], partials [3][NG][SB][H]
    __shared__ int len_s[SB];
    float* hs = smf;
    float* ps = smf + 2 * SB * H;
    const int dir = blockIdx.y, b0 = blockIdx.x * SB;
    const int B = a.B, L = a.L, ldo = a.ld_out;
    const int j = threadIdx.x & 255, kq = threadIdx.x >> 8;
    const size_t BL = (size_t)B * L;
    const float* __restrict__ pre = dir ? a.pre[1] : a.pre[0];       // (selects: an indexed read is a second scalar load that waits for the first)
    const float* __restrict__ wq = (dir ? a.wt[1] : a.wt[0]) + ((size_t)kq * KQ * H + j) * 4;
    float* __restrict__ gates = SAVE ? a.gates + (size_t)dir * BL * 4 * H : nullptr;
    float* __restrict__ cseq = SAVE && !GRU ? a.cseq + (size_t)dir * BL * H : nullptr;
    float* __restrict__ out = a.out;
    if (threadIdx.x < SB) {
        const int b = b0 + threadIdx.x;
        int l = b < B ? a.lengths[b] : 0;              // samples past the batch never become active
        len_s[threadIdx.x] = l < 0 ? 0 : l > L ? L : l;
    }
    for (int i = threadIdx.x; i < 2 * SB * H; i += 1024) hs[i] = 0.f;
    __syncthreads();
    int tmax = 0;                                      // workgroup-uniform
#pragma unroll
    for (int s_ = 0; s_ < SB; ++s_) tmax = len_s[s_] > tmax ? len_s[s_] : tmax;
    // zeros at every inactive token of the samples this workgroup owns
    if (PER_TOKEN) {
        for (int s_ = 0; s_ < SB; ++s_) {
            if (b0 + s_ >= B) break;
            float* o = out + (size_t)(b0 + s_) * L * ldo + dir * H;
            for (int t = len_s[s_] + kq; t < L; t += 4) o[(size_t)t * ldo + j] = 0.f;
        }
    }
    float c[SB];
#pragma unroll
    for (int s_ = 0; s_ < SB; ++s_) c[s_] = 0.f;
    const float bn = GRU ? (dir ? a.bhn[1] : a.bhn[0])[j] : 0.f;
    int cur = 0;
    for (int n = 0; n < tmax; ++n) {
        const int t = dir ? tmax - 1 - n : n;
        float acc[NG][SB];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) acc[g][s_] = 0.f;
        const float* hc = hs + cur * SB * H + kq * KQ;
#pragma unroll 8
        for (int k = 0; k < KQ; ++k) {
            const float4 w4 = *reinterpret_cast<const float4*>(wq + (size_t)k * 4 * H);
            const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) {
                const float hk = hc[s_ * H + k];
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][s_] += wv[g] * hk;
            }
        }
        if (kq > 0) {
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int s_ = 0; s_ < SB; ++s_) ps[(((kq - 1) * NG + g) * SB + s_) * H + j] = acc[g][s_];
        }
        __syncthreads();
        float* hnext = hs + (cur ^ 1) * SB * H;
        if (kq == 0) {
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) {
                float hv = hs[cur * SB * H + s_ * H + j];
                if (t < len_s[s_]) {                   // (len_s > 0 only for b0 + s_ < B: every access below is in bounds)
                    const size_t row = (size_t)(b0 + s_) * L + t;
                    const float* p = pre + row * NG * H + j;
                    float* gp = SAVE ? gates + row * 4 * H + j : nullptr;
                    float rs[NG];
#pragma unroll
                    for (int g = 0; g < NG; ++g)
                        rs[g] = (acc[g][s_] + ps[((0 * NG + g) * SB + s_) * H + j]) + (ps[((1 * NG + g) * SB + s_) * H + j] + ps[((2 * NG + g) * SB + s_) * H + j]);
                    if (GRU) {
                        const float r = sigmoidf_(p[0] + rs[0]), z = sigmoidf_(p[H] + rs[1]);
                        const float ghn = rs[2] + bn;
                        const float nn = tanhf(p[2 * H] + r * ghn);
                        hv = (1.0f - z) * nn + z * hv;
                        if (SAVE) gp[0] = r, gp[H] = z, gp[2 * H] = nn, gp[3 * H] = ghn;
                    } else {
                        const float gi = sigmoidf_(p[0] + rs[0]), gf = sigmoidf_(p[H] + rs[1]), gg = tanhf(p[2 * H] + rs[2]), go = sigmoidf_(p[(NG - 1) * H] + rs[NG - 1]);
                        c[s_] = gf * c[s_] + gi * gg;
                        hv = go * tanhf(c[s_]);
                        if (SAVE) {
                            gp[0] = gi, gp[H] = gf, gp[2 * H] = gg, gp[3 * H] = go;
                            cseq[row * H + j] = c[s_];
                        }
                    }
                    if (PER_TOKEN) out[row * ldo + dir * H + j] = hv;
                }
                hnext[s_ * H + j] = hv;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    if (FORM != INSTR_SEQ && dir == 0 && a.fin) {
        const float* hf = hs + cur * SB * H;           // (length 0: the zero state)
        if (B == 1 && a.fin_rows > 1) {
            if (blockIdx.x == 0)
                for (int r = kq; r < a.fin_rows; r += 4) a.fin[(size_t)r * a.ld_fin + j] = hf[j];
        } else if (kq == 0) {
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_)
                if (b0 + s_ < B) a.fin[(size_t)(b0 + s_) * a.ld_fin + j] = hf[s_ * H + j];
        }
    }
}

struct InstrBwdArgs {
    const float* d_out;      // (B, L, dirs*H) or null
    const float* d_fin;      // (B, H) or null
    const float* gates;      // (dirs, B*L, 4H)
    const float* cseq;       // (dirs, B*L, H), LSTM
    const float* out;        // (B, L, dirs*H), GRU reads h' from it
    const float* wb;         // (dirs, NG*H/4 (row quad), H (k), 4 (row))
    const int* lengths;
    float* d_pre;            // (dirs, B*L, NG*H)
    float* d_gh;             // (dirs, B*L, 3H), GRU
    int B, L;
};

struct InstrSaved { float g0, g1, g2, g3, c, prev, dy; };

template <int SB, bool GRU>
__global__ __launch_bounds__(1024) void instr_scan_bwd_kernel(InstrBwdArgs a) {
    constexpr int H = kInstrH, NG = GRU ? 3 : 4, GH = NG * H, NRQ = GH / 16, NP = (SB * H + 1023) / 1024;
    extern __shared__ __attribute__((aligned(16))) float smb[];     // carry_h [2][SB][H], da [SB][GH], partials [3][SB][H], GRU: dH z [SB][H]
    __shared__ int len_s[SB];
    float* carry = smb;
    float* da = smb + 2 * SB * H;
    float* ps = da + SB * GH;
    float* dhz = ps + 3 * SB * H;
    const int dir = blockIdx.y, dirs = gridDim.y, b0 = blockIdx.x * SB;
    const int B = a.B, L = a.L, ldo = dirs * H;
    const int tid = threadIdx.x, k = tid & 255, q = tid >> 8;
    const size_t BL = (size_t)B * L;
    const float* __restrict__ gates = a.gates + (size_t)dir * BL * 4 * H;
    const float* __restrict__ cseq = GRU ? nullptr : a.cseq + (size_t)dir * BL * H;
    const float* __restrict__ wq = a.wb + (size_t)dir * GH * H + ((size_t)q * NRQ * H + k) * 4;
    float* __restrict__ d_pre = a.d_pre + (size_t)dir * BL * GH;
    float* __restrict__ d_gh = GRU ? a.d_gh + (size_t)dir * BL * GH : nullptr;
    if (tid < SB) {
        const int b = b0 + tid;
        int l = b < B ? a.lengths[b] : 0;
        len_s[tid] = l < 0 ? 0 : l > L ? L : l;
    }
    for (int i = tid; i < 2 * SB * H; i += 1024) carry[i] = 0.f;
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int s_ = 0; s_ < SB; ++s_) tmax = len_s[s_] > tmax ? len_s[s_] : tmax;
    // exact zeros at every inactive token of the samples this workgroup owns (16-byte stores: GH floats per token, 16-byte aligned)
    for (int s_ = 0; s_ < SB; ++s_) {
        if (b0 + s_ >= B) break;
        const size_t r0 = (size_t)(b0 + s_) * L + len_s[s_];
        const size_t n4 = (size_t)(L - len_s[s_]) * (GH / 4);
        float4* zp = reinterpret_cast<float4*>(d_pre + r0 * GH);
        float4* zg = GRU ? reinterpret_cast<float4*>(d_gh + r0 * GH) : nullptr;
        for (size_t i = tid; i < n4; i += 1024) {
            zp[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (GRU) zg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    // what phase A needs of token t for element (sample es, unit eu): loaded one step ahead
    auto load = [&](int t, int es, int eu) -> InstrSaved {
        InstrSaved v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int len = len_s[es];
        if (t < len) {                                 // (len > 0 only for b0 + es < B)
            const int b = b0 + es;
            const size_t row = (size_t)b * L + t;
            const float* gp = gates + row * 4 * H + eu;
            v.g0 = gp[0], v.g1 = gp[H], v.g2 = gp[2 * H], v.g3 = gp[3 * H];
            const bool has_prev = dir ? t + 1 < len : t > 0;
            const size_t prow = dir ? row + 1 : row - 1;
            if (GRU) {
                if (has_prev) v.prev = a.out[prow * ldo + dir * H + eu];
            } else {
                v.c = cseq[row * H + eu];
                if (has_prev) v.prev = cseq[prow * H + eu];
            }
            if (a.d_out) v.dy = a.d_out[row * ldo + dir * H + eu];
            if (dir == 0 && a.d_fin && t == len - 1) v.dy += a.d_fin[(size_t)b * H + eu];
        }
        return v;
    };

    float dc[NP];
    InstrSaved sv[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        dc[p] = 0.f;
        const int i = p * 1024 + tid;
        sv[p] = load(tmax > 0 ? (dir ? 0 : tmax - 1) : L, (i >> 8) % SB, i & 255);    // (tmax == 0: no token is active, nothing is read)
    }
    int cur = 0;
    for (int n = 0; n < tmax; ++n) {
        const int t = dir ? n : tmax - 1 - n;
        const int tn = dir ? t + 1 : t - 1;            // the next step's token
        // phase A
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = p * 1024 + tid;
            if (i < SB * H) {
                const int es = i >> 8, eu = i & 255;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, hz = 0.f;
                if (t < len_s[es]) {
                    const InstrSaved v = sv[p];
                    const size_t row = (size_t)(b0 + es) * L + t;
                    const float dH = v.dy + carry[cur * SB * H + i];
                    float* dp = d_pre + row * GH + eu;
                    if (GRU) {
                        const float r = v.g0, z = v.g1, nn = v.g2, ghn = v.g3;
                        const float dan = dH * (1.f - z) * (1.f - nn * nn);
                        g0 = dan * ghn * (r * (1.f - r));
                        g1 = dH * (v.prev - nn) * (z * (1.f - z));
                        g2 = dan * r;
                        hz = dH * z;
                        float* dg = d_gh + row * GH + eu;
                        dp[0] = g0, dp[H] = g1, dp[2 * H] = dan;
                        dg[0] = g0, dg[H] = g1, dg[2 * H] = g2;
                    } else {
                        const float gi = v.g0, gf = v.g1, gg = v.g2, go = v.g3;
                        const float tc = tanhf(v.c);
                        const float dO = dH * tc;
                        const float dcv = dc[p] + dH * go * (1.f - tc * tc);
                        g0 = dcv * gg * (gi * (1.f - gi));
                        g1 = dcv * v.prev * (gf * (1.f - gf));
                        g2 = dcv * gi * (1.f - gg * gg);
                        g3 = dO * (go * (1.f - go));
                        dp[0] = g0, dp[H] = g1, dp[2 * H] = g2, dp[3 * H] = g3;
                        dc[p] = dcv * gf;
                    }
                } else {
                    dc[p] = 0.f;
                }
                float* dq = da + es * GH + eu;
                dq[0] = g0, dq[H] = g1, dq[2 * H] = g2;
                if (!GRU) dq[(NG - 1) * H] = g3;
                if (GRU) dhz[i] = hz;
                if (n + 1 < tmax) sv[p] = load(tn, es, eu);
            }
        }
        __syncthreads();
        // phase B
        float acc[SB];
#pragma unroll
        for (int s_ = 0; s_ < SB; ++s_) acc[s_] = 0.f;
        const float4* dq4 = reinterpret_cast<const float4*>(da) + q * NRQ;
#pragma unroll 4
        for (int i = 0; i < NRQ; ++i) {
            const float4 w4 = *reinterpret_cast<const float4*>(wq + (size_t)i * 4 * H);
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) {
                const float4 d4 = dq4[s_ * (GH / 4) + i];
                acc[s_] += w4.x * d4.x;
                acc[s_] += w4.y * d4.y;
                acc[s_] += w4.z * d4.z;
                acc[s_] += w4.w * d4.w;
            }
        }
        if (q > 0) {
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) ps[((q - 1) * SB + s_) * H + k] = acc[s_];
        }
        __syncthreads();
        if (q == 0) {
            float* cn = carry + (cur ^ 1) * SB * H;
#pragma unroll
            for (int s_ = 0; s_ < SB; ++s_) {
                float v = (acc[s_] + ps[(0 * SB + s_) * H + k]) + (ps[(1 * SB + s_) * H + k] + ps[(2 * SB + s_) * H + k]);
                if (GRU) v += dhz[s_ * H + k];
                cn[s_ * H + k] = v;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

// torch's W_hh (dirs, G*H, H) -> the forward scan's order (dirs, H (k), H (unit), 4 (gate)), as weights.cpp packs it on the host (GRU: slot 3 zero).
// One workgroup per (k, direction), a thread per unit: the float4 stores of a workgroup are 4 KB contiguous.
__global__ __launch_bounds__(256) void instr_scan_pack_fwd_kernel(const float* __restrict__ w_hh, float4* __restrict__ wt, int G) {
    constexpr int H = kInstrH;
    const int j = threadIdx.x, k = blockIdx.x, dir = blockIdx.y;
    const float* p = w_hh + (size_t)dir * G * H * H + (size_t)j * H + k;
    wt[((size_t)dir * H + k) * H + j] = make_float4(p[0], p[(size_t)H * H], p[(size_t)2 * H * H], G == 4 ? p[(size_t)3 * H * H] : 0.f);
}
// torch's W_hh (dirs, G*H, H) -> the reverse scan's order (dirs, G*H/4 (row quad), H (k), 4 (row)): reads and stores of a workgroup are contiguous runs
__global__ __launch_bounds__(256) void instr_scan_pack_bwd_kernel(const float* __restrict__ w_hh, float4* __restrict__ wb, int G) {
    constexpr int H = kInstrH;
    const int k = threadIdx.x, rq = blockIdx.x, dir = blockIdx.y;
    const float* p = w_hh + ((size_t)dir * G * H + (size_t)rq * 4) * H + k;
    wb[((size_t)dir * (G * H / 4) + rq) * H + k] = make_float4(p[0], p[H], p[2 * H], p[3 * H]);
}

bool instr_scan_train_ok(int B, int L, int H, int dirs) { return H == kInstrH && B >= 1 && L >= 1 && (dirs == 1 || dirs == 2); }
size_t instr_scan_work_floats(int dirs) { return (size_t)dirs * 4 * kInstrH * kInstrH; }
// samples per workgroup of the forward and the reverse launch: the fewest (from 2 up) that keep the launch within 128 workgroups, so that the scan
// does not take the CUs from the trunks running beside it (B = 64: 32 workgroups a direction).  SB = 1 is not built: slower at B = 64 -- 128
// workgroups take those CUs -- and its instantiation showed run-to-run differences of ~3e-5 whose cause was not found; SB = 2 / 4 / 8 are bitwise
// reproducible, tested.
int instr_scan_sb(int B, int dirs) {
    int SB = 2;
    while (SB < 8 && ((B + SB - 1) / SB) * dirs > 128) SB *= 2;
    return SB;
}

// the forms a caller reaches: nothing runs the per-token form with a GRU
template <int SB>
static const void* instr_scan_fn(int gru, int form) {
    if (form == INSTR_SEQ) return gru ? nullptr : reinterpret_cast<const void*>(instr_scan_kernel<SB, false, INSTR_SEQ>);
    if (form == INSTR_FIN)
        return gru ? reinterpret_cast<const void*>(instr_scan_kernel<SB, true, INSTR_FIN>) : reinterpret_cast<const void*>(instr_scan_kernel<SB, false, INSTR_FIN>);
    return gru ? reinterpret_cast<const void*>(instr_scan_kernel<SB, true, INSTR_TRAIN>) : reinterpret_cast<const void*>(instr_scan_kernel<SB, false, INSTR_TRAIN>);
}
template <int SB>
static const void* instr_bwd_fn(int gru) {
    return gru ? reinterpret_cast<const void*>(instr_scan_bwd_kernel<SB, true>) : reinterpret_cast<const void*>(instr_scan_bwd_kernel<SB, false>);
}

hipError_t launch_instr_scan(const InstrScanArgs& a, int dirs, int gru, hipStream_t s) {
    constexpr int H = kInstrH;
    const int form = a.gates ? INSTR_TRAIN : a.out ? INSTR_SEQ : INSTR_FIN;
    if (!instr_scan_train_ok(a.B, a.L, H, dirs) || !a.lengths) return hipErrorInvalidValue;
    for (int d = 0; d < dirs; ++d)
        if (!a.pre[d] || !a.wt[d] || (gru && !a.bhn[d])) return hipErrorInvalidValue;
    if (form != INSTR_FIN && (!a.out || a.ld_out < dirs * H)) return hipErrorInvalidValue;
    if (form == INSTR_FIN && (dirs != 1 || !a.fin)) return hipErrorInvalidValue;
    if (a.fin && (a.fin_rows < a.B || a.ld_fin < H)) return hipErrorInvalidValue;
    if (form == INSTR_TRAIN && (a.cseq == nullptr) != (gru != 0)) return hipErrorInvalidValue;
    const int SB = instr_scan_sb(a.B, dirs), NG = gru ? 3 : 4;
    // h [2][SB][H] and the partials [3][NG][SB][H]: 28 KB at SB = 2, 112 KB at SB = 8 (LSTM), within the 160 KB of a CU.  The kernel also holds SB
    // static words (its lengths), so the limit asked for is what the launch uses, not the CU's 160 KB, which the runtime refuses on top of them
    const size_t lds = (size_t)(2 + 3 * NG) * SB * H * sizeof(float);
    const void* fn = SB == 2 ? instr_scan_fn<2>(gru, form) : SB == 4 ? instr_scan_fn<4>(gru, form) : instr_scan_fn<8>(gru, form);
    if (!fn) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    InstrScanArgs k = a;
    void* args[] = {&k};
    return hipLaunchKernel(fn, dim3((a.B + SB - 1) / SB, dirs), dim3(1024), args, lds, s);
}

hipError_t launch_instr_scan_pack_fwd(const float* w_hh, float* wt, int dirs, int gru, hipStream_t s) {
    if (!w_hh || !wt || (dirs != 1 && dirs != 2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(instr_scan_pack_fwd_kernel, dim3(kInstrH, dirs), dim3(256), 0, s, w_hh, (float4*)wt, gru ? 3 : 4);
    return hipGetLastError();
}

hipError_t launch_instr_scan_bwd(const float* d_out, const float* d_fin, const float* gates, const float* cseq, const float* out, const float* w_hh,
                                 const int* lengths, float* work, float* d_pre, float* d_gh, int B, int L, int H, int dirs, int gru, hipStream_t s) {
    if (!instr_scan_train_ok(B, L, H, dirs) || !gates || !out || !w_hh || !lengths || !work || !d_pre || (cseq == nullptr) != (gru != 0) ||
        (d_gh == nullptr) != (gru == 0))
        return hipErrorInvalidValue;
    const int NG = gru ? 3 : 4;
    hipLaunchKernelGGL(instr_scan_pack_bwd_kernel, dim3(NG * H / 4, dirs), dim3(256), 0, s, w_hh, (float4*)work, NG);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int SB = instr_scan_sb(B, dirs);
    // carry 2, da NG, partials 3, GRU's dH z 1 times SB * H floats, 9 * SB KB for either cell: 18 KB at SB = 2, 72 KB at SB = 8
    const size_t lds = (size_t)(2 + NG + 3 + (gru ? 1 : 0)) * SB * H * sizeof(float);
    const void* fn = SB == 2 ? instr_bwd_fn<2>(gru) : SB == 4 ? instr_bwd_fn<4>(gru) : instr_bwd_fn<8>(gru);
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    InstrBwdArgs a;
    a.d_out = d_out; a.d_fin = d_fin; a.gates = gates; a.cseq = cseq; a.out = out; a.wb = work; a.lengths = lengths; a.d_pre = d_pre; a.d_gh = d_gh;
    a.B = B; a.L = L;
    void* args[] = {&a};
    return hipLaunchKernel(fn, dim3((B + SB - 1) / SB, dirs), dim3(1024), args, lds, s);
}

}  // namespace hcm
