// Reverse-time scan of the state encoders: back-propagation through time for the masked LSTM / GRU steps of state_scan.hip, ONE launch per step,
// from what the training forward saved (state_scan_step_kernel<.., SAVE>: post-activation gates, c_t, h_t).  The launch boundary is the only
// synchronisation between steps: no grid barrier, no spinning, no atomics, plain vector stores.
//
// Per step t = T-1 .. 0, m = masks[t], dH = d_seq[t] + carry_h:
//   LSTM  tc = tanh(c_t); do = dH tc; dc = carry_c + dH o (1 - tc^2); da_i = dc g i(1-i); da_f = dc (c_{t-1} m) f(1-f); da_g = dc i (1-g^2);
//         da_o = do o(1-o); d_pre[t] = da; carry_c <- dc f m; carry_h <- (da . W_hh) m
//   GRU   da_n = dH (1-z)(1-n^2); da_r = da_n hn r(1-r); da_z = dH (h' - n) z(1-z), h' = h_{t-1} m; d_pre[t] = [da_r, da_z, da_n];
//         d_gh[t] = [da_r, da_z, da_n r]; carry_h <- (d_gh[t] . W_hh + dH z) m
//
// state_scan_bwd_step_kernel<H, GRU> mirrors the forward: H / 16 workgroups of 256 threads; a workgroup owns kScanUnits = 16 COLUMNS of W_hh (16 units
// of carry_h) and all G*H rows of them.  Weights in reverse-scan order [column slice][G*H/4 row quads][16 columns][4 rows]: thread (j = column,
// rl = row lane of 16) keeps the G*H/64 float4 of its row quads q = qq * 16 + rl in registers (128 floats LSTM / 96 GRU, the forward's budget),
// loaded once per launch (a wave's load instruction covers 1 KB contiguous).  Samples go through in blocks of kBwdNB = 4: every workgroup computes
// the element-wise gate gradients of the block for ALL units from the saved values into LDS (4 x G*H floats: 32 KB LSTM / 24 KB GRU, static --
// a block of 8 is 64 KB and needs the dynamic-LDS opt-in; what the second pass of the block loop at N = 8 costs has not been measured), N*G*H cheap operations done redundantly,
// and stores to d_pre / d_gh / carry_c only the slice of its own 16 units.  The contraction over the G*H rows has a fixed order: a thread's row
// quads in qq order (one chain per row of the quad, added as (x + y) + (z + w)), the wave's four row lanes by two xor shuffles (lane + 16, then lane + 32), the four waves through LDS as ((w0 + w1) + (w2 + w3)).
//
// Every workgroup of a step reads ALL of carry_h / carry_c while each stores its own slice of the next carry, so both carries ping-pong between two
// buffers (launch_state_scan_bwd); step T-1 reads none (null = zero) and step 0 stores into d_h_in, which is a third buffer.
#include "dev.h"
#include "kernels.h"

#include <cstddef>

namespace hcm {

constexpr int kBwdNB = 4;

template <int H, bool GRU>
__global__ __launch_bounds__(256) void state_scan_bwd_step_kernel(const float* __restrict__ d_seq_t, const float* __restrict__ gates_t,
                                                                   const float* __restrict__ c_t, const float* __restrict__ c_prev,
                                                                   const float* __restrict__ h_prev, const float* __restrict__ mask,
                                                                   const float4* __restrict__ wb, const float* __restrict__ carry_h_in,
                                                                   const float* __restrict__ carry_c_in, float* __restrict__ carry_h_out,
                                                                   float* __restrict__ carry_c_out, float* __restrict__ d_pre_t,
                                                                   float* __restrict__ d_gh_t, int N) {
    constexpr int NG = GRU ? 3 : 4, U = kScanUnits, GH = NG * H, QS = GH / 64, NB = kBwdNB;
    static_assert(H % 64 == 0 && U == 16, "thread mapping: 16 columns x 16 row lanes");
    __shared__ __attribute__((aligned(16))) float da[NB][GH];
    __shared__ float ps[4][NB][U];
    __shared__ float dhz[NB][U];
    const int tid = threadIdx.x, j = tid & 15, rl = tid >> 4, wave = tid >> 6;
    const int u0 = blockIdx.x * U;

    float4 w[QS];
    {
        const float4* wp = wb + ((size_t)blockIdx.x * (GH / 4) + rl) * U + j;
#pragma unroll
        for (int qq = 0; qq < QS; ++qq) w[qq] = wp[(size_t)qq * 16 * U];
    }

    for (int n0 = 0; n0 < N; n0 += NB) {
        const int nb = N - n0 < NB ? N - n0 : NB;
        // element-wise gate gradients of the block, all units (a partial last block: zero rows, nothing stored for them); two iterations' loads in flight
#pragma unroll 2
        for (int i = tid; i < NB * H; i += 256) {
            const int s_ = i / H, u = i - s_ * H;
            float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
            if (s_ < nb) {
                const int n = n0 + s_;
                const size_t o = (size_t)n * H + u;
                const bool own = (unsigned)(u - u0) < (unsigned)U;
                const float m = mask[n];
                const float dH = d_seq_t[o] + (carry_h_in ? carry_h_in[o] : 0.f);
                const float* gp = gates_t + (size_t)n * 4 * H + u;
                if (GRU) {
                    const float r = gp[0], z = gp[H], nn = gp[2 * H], hn = gp[3 * H];
                    const float hp = h_prev[o] * m;
                    const float dan = dH * (1.f - z) * (1.f - nn * nn);
                    g0 = dan * hn * (r * (1.f - r));
                    g1 = dH * (hp - nn) * (z * (1.f - z));
                    g2 = dan * r;
                    if (own) {
                        float* dp = d_pre_t + (size_t)n * GH + u;
                        float* dg = d_gh_t + (size_t)n * GH + u;
                        dp[0] = g0, dp[H] = g1, dp[2 * H] = dan;
                        dg[0] = g0, dg[H] = g1, dg[2 * H] = g2;
                        dhz[s_][u - u0] = dH * z;
                    }
                } else {
                    const float gi = gp[0], gf = gp[H], gg = gp[2 * H], go = gp[3 * H];
                    const float tc = tanhf(c_t[o]);
                    const float dO = dH * tc;
                    const float dc = (carry_c_in ? carry_c_in[o] : 0.f) + dH * go * (1.f - tc * tc);
                    g0 = dc * gg * (gi * (1.f - gi));
                    g1 = dc * (c_prev[o] * m) * (gf * (1.f - gf));
                    g2 = dc * gi * (1.f - gg * gg);
                    g3 = dO * (go * (1.f - go));
                    if (own) {
                        float* dp = d_pre_t + (size_t)n * GH + u;
                        dp[0] = g0, dp[H] = g1, dp[2 * H] = g2, dp[3 * H] = g3;
                        carry_c_out[o] = dc * gf * m;
                    }
                }
            }
            da[s_][u] = g0, da[s_][H + u] = g1, da[s_][2 * H + u] = g2;
            if (!GRU) da[s_][(NG - 1) * H + u] = g3;
        }
        __syncthreads();

        // one sample at a time (not unrolled: unrolled, the compiler keeps the LDS reads of three samples in registers while it sums the first and
        // spills): four chains per sample, one per row of the quad, in qq order; then the wave's four row lanes (lane bits 4 and 5); the four
        // waves meet in LDS
#pragma unroll 1
        for (int s_ = 0; s_ < NB; ++s_) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4* dq = reinterpret_cast<const float4*>(&da[s_][0]) + rl;
#pragma unroll
            for (int qq = 0; qq < QS; ++qq) {
                const float4 d = dq[qq * 16];
                acc.x += w[qq].x * d.x;
                acc.y += w[qq].y * d.y;
                acc.z += w[qq].z * d.z;
                acc.w += w[qq].w * d.w;
            }
            float v = (acc.x + acc.y) + (acc.z + acc.w);
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if ((tid & 63) < U) ps[wave][s_][j] = v;
        }
        const float hz = GRU && tid < NB * U ? dhz[tid >> 4][j] : 0.f;       // (read in front of the barrier: the next block's first phase rewrites it)
        __syncthreads();

        if (tid < NB * U) {
            const int s_ = tid >> 4;
            if (s_ < nb) {
                const int n = n0 + s_;
                float v = (ps[0][s_][j] + ps[1][s_][j]) + (ps[2][s_][j] + ps[3][s_][j]);
                if (GRU) v += hz;
                carry_h_out[(size_t)n * H + u0 + j] = v * mask[n];
            }
        }
    }
}

// Reverse-scan order of W_hh (torch's (G*H, H)): [H/16 column slices][G*H/4 row quads][16 columns][4 rows].  A thread builds one float4: its reads are
// 64-byte runs of a row, the stores of a workgroup 4 KB contiguous.
__global__ __launch_bounds__(256) void state_scan_bwd_pack_kernel(const float* __restrict__ w_hh, float4* __restrict__ wb, int H, int GH) {
    constexpr int U = kScanUnits;
    const int j = threadIdx.x & 15, q = blockIdx.x * 16 + (threadIdx.x >> 4), b = blockIdx.y;
    const float* p = w_hh + (size_t)q * 4 * H + b * U + j;
    wb[((size_t)b * (GH / 4) + q) * U + j] = make_float4(p[0], p[H], p[2 * (size_t)H], p[3 * (size_t)H]);
}

hipError_t launch_state_scan_bwd(const float* d_seq, const float* gates, const float* cseq, const float* seq, const float* h_in, const float* mask,
                                 const float* w_hh, float* work, float* d_pre, float* d_gh, float* d_h_in, int T, int N, int H, int gru, hipStream_t s) {
    if (!state_scan_ok(H) || T < 1 || N < 1 || !d_seq || !gates || !seq || !h_in || !mask || !w_hh || !work || !d_pre || !d_h_in ||
        (cseq == nullptr) != (gru != 0) || (d_gh == nullptr) != (gru == 0))
        return hipErrorInvalidValue;
    constexpr int HH = 512;
    const int NG = gru ? 3 : 4, GH = NG * H, nwg = H / kScanUnits;
    const size_t NH = (size_t)N * H;
    hipLaunchKernelGGL(state_scan_bwd_pack_kernel, dim3(GH / 64, nwg), dim3(256), 0, s, w_hh, (float4*)work, H, GH);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the carries: two (h, c) pairs behind the packed weights; step t reads pair (t + 1) & 1, which step t + 1 stored, and stores pair t & 1
    float* cb = work + (size_t)4 * H * H;
    for (int t = T - 1; t >= 0; --t) {
        const float* ci = t == T - 1 ? nullptr : cb + (size_t)((t + 1) & 1) * 2 * NH;
        float* co = t == 0 ? d_h_in : cb + (size_t)(t & 1) * 2 * NH;
        const float* hp = t == 0 ? h_in : seq + (size_t)(t - 1) * NH;
        const float* dst = d_seq + (size_t)t * NH;
        const float* gt = gates + (size_t)t * NH * 4;
        const float* mt = mask + (size_t)t * N;
        float* dpt = d_pre + (size_t)t * N * GH;
        if (gru)
            hipLaunchKernelGGL((state_scan_bwd_step_kernel<HH, true>), dim3(nwg), dim3(256), 0, s, dst, gt, nullptr, nullptr, hp, mt, (const float4*)work,
                               ci, nullptr, co, nullptr, dpt, d_gh + (size_t)t * N * GH, N);
        else
            hipLaunchKernelGGL((state_scan_bwd_step_kernel<HH, false>), dim3(nwg), dim3(256), 0, s, dst, gt, cseq + (size_t)t * NH,
                               t == 0 ? h_in + NH : cseq + (size_t)(t - 1) * NH, nullptr, mt, (const float4*)work, ci, ci ? ci + NH : nullptr, co,
                               co + NH, dpt, nullptr, N);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hcm
