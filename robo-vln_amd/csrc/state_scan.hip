// State-encoder scan of the sequence calls (RNNStateEncoder.seq_forward, models/decoder/state_encoder.py:83-133): the x half of every gate product
// is one GEMM over all T*N rows (the caller's `pre`); what is left per time step -- h*mask . W_hh^T, the cell, the stores -- is ONE launch here instead
// of rnn_prep + gate GEMV(s) + cell.  The launch boundary is the only synchronisation between steps: no grid barrier, no spinning, no atomics on
// the state.
//
// state_scan_step_kernel<H, GRU>: a workgroup owns kScanUnits = 16 hidden units, i.e. NG * 16 rows of W_hh (64 LSTM / 48 GRU); H / 16 workgroups
// (32 at hidden = 512).  Weights in scan order [unit slice][k][16 units][4 gates]: thread (j = unit, kl = k lane of 16) keeps the H / 16 float4 of its
// k values k = kk * 16 + kl in registers, loaded once per launch (a wave's load instruction covers 1 KB contiguous).  The samples go through in
// register blocks of kScanNB = 8: h_prev * mask of a block is staged in LDS (8 * H floats), every thread accumulates NG x 8 partial products over its
// k values, the four k lanes inside a wave are added by two xor shuffles (lane + 16, then lane + 32), the four waves' partials through LDS as
// ((w0 + w1) + (w2 + w3)).  Thread (sample, unit) of the first 128 then adds `pre`, applies the cell and stores h_t into the sequence buffer (which is
// also the state the next step's launch reads), c_t in place.  Any N >= 1: a partial last block computes on zero rows and stores nothing for them.
// Summation order is fixed: bitwise reproducible.  All arithmetic f32, as in lstm_cell_kernel / gru_cell_kernel (elementwise.hip).
//
// Overflow guard (Heads::bad semantics: one count per (sample, step) whose gate pre-activations are not all finite): every workgroup tests ONLY the
// gates of its own 16 units and stores one word per (row, workgroup) into `flags` (plain stores, every word of a step is written by that step);
// state_scan_guard_kernel, one launch behind the T steps, ORs the H / 16 words of every row in a fixed owner thread and adds the number of flagged rows
// to the guard word once.  A row is therefore never counted twice, whichever unit slices saw the non-finite value.
#include "dev.h"
#include "kernels.h"

#include <cstddef>

namespace hcm {

constexpr int kScanNB = 8;

// SAVE (the training forward, hcm_op_state_scan_train): the cell epilogue also stores what the reverse scan (state_scan_bwd.hip) reads -- the
// post-activation gates of the row (LSTM i,f,g,o; GRU r,z,n and hn = W_hn h' + b_hn, the value r multiplies) into gates_t [N][4H] and, LSTM, c_t
// into cseq_t [N][H].  Extra stores of values the epilogue has anyway: the arithmetic, and so every bit of h_t / c_t, is that of SAVE = false.
template <int H, bool GRU, bool SAVE>
__global__ __launch_bounds__(256) void state_scan_step_kernel(const float* __restrict__ pre, const float4* __restrict__ ws, const float* __restrict__ bhh,
                                                               const float* h_prev, const float* c_prev, const float* __restrict__ mask, float* seq_t,
                                                               float* h_last, float* c_out, unsigned* __restrict__ flags_t, float* __restrict__ gates_t,
                                                               float* __restrict__ cseq_t, int N) {
    constexpr int NG = GRU ? 3 : 4, U = kScanUnits, KS = H / 16, NB = kScanNB;
    static_assert(H % 64 == 0 && U == 16, "thread mapping: 16 units x 16 k lanes");
    __shared__ float hs[NB * H];
    __shared__ float ps[4][NG][NB][U];
    __shared__ int bad_s[NB];
    const int tid = threadIdx.x, j = tid & 15, kl = tid >> 4, wave = tid >> 6;
    const int u0 = blockIdx.x * U, nwg = gridDim.x;

    float4 w[KS];
    {
        const float4* wp = ws + ((size_t)blockIdx.x * H + kl) * U + j;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) w[kk] = wp[(size_t)kk * 16 * U];
    }

    for (int n0 = 0; n0 < N; n0 += NB) {
        const int nb = N - n0 < NB ? N - n0 : NB;
        for (int i = tid; i < NB * H; i += 256) {
            const int sidx = i / H, k = i - sidx * H;
            hs[i] = sidx < nb ? h_prev[(size_t)(n0 + sidx) * H + k] * mask[n0 + sidx] : 0.f;
        }
        if (tid < NB) bad_s[tid] = 0;
        __syncthreads();

        float acc[NG][NB];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int s_ = 0; s_ < NB; ++s_) acc[g][s_] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const float wv[4] = {w[kk].x, w[kk].y, w[kk].z, w[kk].w};
            const float* hk = hs + kk * 16 + kl;
#pragma unroll
            for (int s_ = 0; s_ < NB; ++s_) {
                const float hv = hk[s_ * H];
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][s_] += wv[g] * hv;
            }
        }
        // the wave's four k lanes (lane bits 4 and 5), then the four waves
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int s_ = 0; s_ < NB; ++s_) {
                float v = acc[g][s_];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if ((tid & 63) < U) ps[wave][g][s_][j] = v;
            }
        __syncthreads();

        if (tid < NB * U) {
            const int s_ = tid >> 4;
            if (s_ < nb) {
                const int n = n0 + s_, u = u0 + j;
                const float* p = pre + (size_t)n * NG * H + u;
                float rs[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    rs[g] = (ps[0][g][s_][j] + ps[1][g][s_][j]) + (ps[2][g][s_][j] + ps[3][g][s_][j]);
                    if (bhh) rs[g] += bhh[g * H + u];
                }
                float h2;
                bool bad;
                if (GRU) {
                    const float a0 = p[0], a1 = p[H], a2 = p[2 * H];
                    bad = !isfinite(a0 + a1 + a2) || !isfinite(rs[0] + rs[1] + rs[2]);       // (a finite sum has finite terms)
                    const float r = sigmoidf_(a0 + rs[0]);
                    const float z = sigmoidf_(a1 + rs[1]);
                    const float nn = tanhf(a2 + r * rs[2]);
                    h2 = (1.f - z) * nn + z * hs[s_ * H + u];
                    if (SAVE) {
                        float* gp = gates_t + (size_t)n * 4 * H + u;
                        gp[0] = r, gp[H] = z, gp[2 * H] = nn, gp[3 * H] = rs[2];
                    }
                } else {
                    const float g0 = p[0] + rs[0], g1 = p[H] + rs[1], g2 = p[2 * H] + rs[2], g3 = p[(NG - 1) * H] + rs[NG - 1];
                    bad = !isfinite(g0 + g1 + g2 + g3);
                    const float c = c_prev[(size_t)n * H + u] * mask[n];
                    const float gi = sigmoidf_(g0), gf = sigmoidf_(g1), gg = tanhf(g2), go = sigmoidf_(g3);
                    const float c2 = gf * c + gi * gg;
                    h2 = go * tanhf(c2);
                    c_out[(size_t)n * H + u] = c2;
                    if (SAVE) {
                        float* gp = gates_t + (size_t)n * 4 * H + u;
                        gp[0] = gi, gp[H] = gf, gp[2 * H] = gg, gp[3 * H] = go;
                        cseq_t[(size_t)n * H + u] = c2;
                    }
                }
                seq_t[(size_t)n * H + u] = h2;
                if (h_last) h_last[(size_t)n * H + u] = h2;
                if (bad) bad_s[s_] = 1;            // (every writer stores the same word)
            }
        }
        __syncthreads();
        if (flags_t && tid < nb) flags_t[(size_t)(n0 + tid) * nwg + blockIdx.x] = (unsigned)bad_s[tid];
    }
}

// rows = T*N; one workgroup; thread r % 256 owns row r
__global__ __launch_bounds__(256) void state_scan_guard_kernel(const unsigned* __restrict__ flags, int rows, int nwg, unsigned* __restrict__ bad) {
    __shared__ int part[4];
    int cnt = 0;
    for (int r = threadIdx.x; r < rows; r += 256) {
        unsigned any = 0u;
        for (int g = 0; g < nwg; ++g) any |= flags[(size_t)r * nwg + g];
        cnt += any ? 1 : 0;
    }
    const float tot = wave_sum((float)cnt);          // (exact: at most a few thousand rows)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (int)tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = part[0] + part[1] + part[2] + part[3];
        if (total) atomicAdd(bad, (unsigned)total);
    }
}

bool state_scan_ok(int H) { return H == 512; }       // STATE_ENCODER.hidden_size of every reference config; the template takes any multiple of 64, only this one is built and tested

void state_scan_pack(const float* w_hh, float* out, int H, int G) {
    for (size_t i = 0, n = (size_t)H * H * 4; i < n; ++i) out[i] = 0.f;
    for (int r = 0; r < G * H; ++r) {
        const int g = r / H, u = r % H;
        for (int k = 0; k < H; ++k) out[(((size_t)(u / kScanUnits) * H + k) * kScanUnits + u % kScanUnits) * 4 + g] = w_hh[(size_t)r * H + k];
    }
}

template <int H, bool SAVE>
static hipError_t scan_steps(const float* pre, const float* ws, const float* bhh, const float* h_in, const float* mask, float* seq, float* h_out,
                             unsigned* flags, float* gates, float* cseq, int T, int N, int gru, hipStream_t s) {
    const int NG = gru ? 3 : 4, nwg = H / kScanUnits;
    const size_t NH = (size_t)N * H;
    const bool alias1 = T == 1 && h_out == h_in;
    for (int t = 0; t < T; ++t) {
        const float* hp = t == 0 ? h_in : seq + (size_t)(t - 1) * NH;
        const float* cp = t == 0 ? h_in + NH : h_out + NH;          // LSTM: c lives in h_out[1] from step 0 on (each element has one reader = its writer)
        float* hl = t == T - 1 && !alias1 ? h_out : nullptr;
        const float* pt = pre + (size_t)t * N * NG * H;
        unsigned* ft = flags ? flags + (size_t)t * N * nwg : nullptr;
        float* gt = SAVE ? gates + (size_t)t * NH * 4 : nullptr;
        if (gru)
            hipLaunchKernelGGL((state_scan_step_kernel<H, true, SAVE>), dim3(nwg), dim3(256), 0, s, pt, (const float4*)ws, bhh, hp, nullptr,
                               mask + (size_t)t * N, seq + (size_t)t * NH, hl, nullptr, ft, gt, nullptr, N);
        else
            hipLaunchKernelGGL((state_scan_step_kernel<H, false, SAVE>), dim3(nwg), dim3(256), 0, s, pt, (const float4*)ws, bhh, hp, cp,
                               mask + (size_t)t * N, seq + (size_t)t * NH, hl, h_out + NH, ft, gt, SAVE ? cseq + (size_t)t * NH : nullptr, N);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (alias1) return hipMemcpyAsync(h_out, seq, NH * 4, hipMemcpyDeviceToDevice, s);
    return hipSuccess;
}

hipError_t launch_state_scan(const float* pre, const float* ws, const float* bhh, const float* h_in, const float* mask, float* seq, float* h_out,
                             unsigned* flags, unsigned* bad, int T, int N, int H, int gru, hipStream_t s) {
    if (!state_scan_ok(H) || T < 1 || N < 1 || !pre || !ws || !h_in || !mask || !seq || !h_out || (bad && !flags)) return hipErrorInvalidValue;
    // every workgroup of a step reads ALL of h_prev while others store h_t: the two must be different buffers.  From step 1 on the source is the
    // sequence buffer's previous row block; at step 0 it is h_in, and only a one-step scan also stores its h into h_out there -- with h_out
    // aliasing h_in that store goes through the sequence buffer instead (copied behind the launch).
    if (!bad) flags = nullptr;
    hipError_t e = scan_steps<512, false>(pre, ws, bhh, h_in, mask, seq, h_out, flags, nullptr, nullptr, T, N, gru, s);
    if (e != hipSuccess) return e;
    if (bad) {
        hipLaunchKernelGGL(state_scan_guard_kernel, dim3(1), dim3(256), 0, s, flags, T * N, H / kScanUnits, bad);
        e = hipGetLastError();
    }
    return e;
}

// state_scan_pack on the device: a workgroup moves the (4 gates x 16 units) x 64 k tile of slice blockIdx.y through LDS, so that both the reads of
// torch's (G*H, H) rows (64 consecutive k) and the stores in scan order (4096 consecutive floats) are contiguous.  GRU: the 4th gate slot is 0.
__global__ __launch_bounds__(256) void state_scan_pack_kernel(const float* __restrict__ w_hh, float* __restrict__ ws, int H, int G) {
    __shared__ float tile[64][65];
    constexpr int U = kScanUnits;
    const int tid = threadIdx.x, k0 = blockIdx.x * 64, b = blockIdx.y;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int row = e >> 6, kk = e & 63, g = row >> 4, uu = row & 15;
        tile[row][kk] = g < G ? w_hh[((size_t)g * H + b * U + uu) * H + k0 + kk] : 0.f;
    }
    __syncthreads();
    float* out = ws + ((size_t)b * H + k0) * U * 4;
    for (int o = tid; o < 64 * 64; o += 256) {
        const int g = o & 3, uu = (o >> 2) & 15, kk = o >> 6;
        out[o] = tile[g * 16 + uu][kk];
    }
}

static hipError_t launch_state_scan_pack(const float* w_hh, float* ws, int H, int G, hipStream_t s) {
    if (!state_scan_ok(H) || !w_hh || !ws || (G != 3 && G != 4)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(state_scan_pack_kernel, dim3(H / 64, H / kScanUnits), dim3(256), 0, s, w_hh, ws, H, G);
    return hipGetLastError();
}

hipError_t launch_state_scan_train(const float* pre, const float* w_hh, const float* bhh, const float* h_in, const float* mask, float* seq, float* h_out,
                                   float* gates, float* cseq, float* work, int T, int N, int H, int gru, hipStream_t s) {
    if (!state_scan_ok(H) || T < 1 || N < 1 || !pre || !w_hh || !h_in || !mask || !seq || !h_out || !gates || !work || (cseq == nullptr) != (gru != 0))
        return hipErrorInvalidValue;
    const hipError_t e = launch_state_scan_pack(w_hh, work, H, gru ? 3 : 4, s);
    if (e != hipSuccess) return e;
    return scan_steps<512, true>(pre, work, bhh, h_in, mask, seq, h_out, nullptr, gates, cseq, T, N, gru, s);
}

}  // namespace hcm
