// The end of the flat trainer's update step (robo_vln_trainer.py:505-542) in float32 with a backward pass, behind train.flat_heads_loss: the heads
// of CMANet / Seq2SeqNet over the state encoder's rows x (rows, 512)
//     out = x W_lin^T + b_lin,   stop = x W_stop^T + b_stop,   progress_hat = tanh(x W_pm^T + b_pm)   (the last with the monitor only)
// and the criterion of hcm_flat_val_step over them (elementwise.hip, flat_val_loss_kernel, launched behind the heads: the same kernel, so the
// same bits).  The work is one 512-wide dot product per head and row: NH = num_actions + 1 (+ 1 with the monitor) <= 6 heads, head k < num_actions
// a row of `linear`, then `stop_linear`, then `progress_monitor`.
//
// Forward: a wave per row, kFwdRows = 4 rows per workgroup.  Lane l holds x[4l .. 4l+3] and x[256 + 4l .. 256 + 4l+3] (two 16-byte loads), adds its
// eight products in that order and the 64 lanes meet in a xor butterfly: a row's bits depend on the row and the weights alone.
// Backward: a workgroup owns kBwdRows = 32 rows.  Threads 0..31 form the rows' head gradients d_head (rows, NH) from the saved outputs, the labels,
// the counts in result[3..4] and the cotangent d_result[0..2], all read on the device; then thread (half h, column quad q) walks rows 16 h .. 16 h+15
// of the block in order, writes d_x[r, 4q..4q+3] = sum_k d_head[r, k] W_k (heads in order; skipped with d_x = NULL) and accumulates
// d_head[r, k] x[r, 4q..4q+3]; the block's d_W share is half 0 + half 1, its d_b share the sum of d_head in row order.  A second launch adds the
// blocks' shares in block order (the pattern of attn1q_train_de_reduce_kernel).  No atomics, no scratch: bitwise reproducible.
#include "dev.h"
#include "kernels.h"

namespace hcm {
namespace {

constexpr int kT = 256, kH = 512, kQ = kH / 4, kFwdRows = kT / 64, kBwdRows = 32, kHalfRows = kBwdRows / 2, kMaxHeads = 6, kBiasSlot = 8;

__device__ __forceinline__ const float* head_w(const FlatHeadsArgs& p, int k) {
    return k < p.num_actions ? p.w_lin + (size_t)k * kH : k == p.num_actions ? p.w_stop : p.w_pm;
}
__device__ __forceinline__ float head_b(const FlatHeadsArgs& p, int k) {
    return k < p.num_actions ? p.b_lin[k] : k == p.num_actions ? p.b_stop[0] : p.b_pm[0];
}

template <int NH>
__global__ __launch_bounds__(kT) void flat_heads_fwd_kernel(FlatHeadsArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kFwdRows + wave;
    if (r >= p.rows) return;
    const int A = p.num_actions;
    float xlo[4], xhi[4];
    ld_chunk(p.x + (size_t)r * kH + lane * 4, xlo);
    ld_chunk(p.x + (size_t)r * kH + kH / 2 + lane * 4, xhi);
#pragma unroll
    for (int k = 0; k < NH; ++k) {
        const float* w = head_w(p, k);
        float wlo[4], whi[4];
        ld_chunk(w + lane * 4, wlo);
        ld_chunk(w + kH / 2 + lane * 4, whi);
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += xlo[e] * wlo[e];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += xhi[e] * whi[e];
        const float v = wave_sum(acc) + head_b(p, k);
        if (lane == 0) {
            if (k < A) p.out[(size_t)r * A + k] = v;
            else if (k == A) p.stop[r] = v;
            else p.progress_hat[r] = tanhf(v);
        }
    }
}

template <int NH>
__global__ __launch_bounds__(kT) void flat_heads_bwd_kernel(FlatHeadsArgs p) {
    __shared__ float sdh[kBwdRows][kMaxHeads];
    __shared__ __attribute__((aligned(16))) float sacc[NH][kQ][4];
    const int tid = threadIdx.x, A = p.num_actions;
    const int r0 = blockIdx.x * kBwdRows;
    const int n = min(kBwdRows, p.rows - r0);
    const bool monitor = NH == A + 2;

    if (tid < kBwdRows) {
        float dh[kMaxHeads];
#pragma unroll
        for (int k = 0; k < kMaxHeads; ++k) dh[k] = 0.f;
        if (tid < n) {
            const size_t r = (size_t)r0 + tid;
            const float g0 = p.d_result[0], g1 = p.d_result[1], g2 = p.d_result[2];
            const float n_all = (float)p.rows * (float)A, n_stop = p.result[3], n_aux = p.result[4];
#pragma unroll
            for (int j = 0; j < NH - 1; ++j) {
                if (j < A) {
                    const float c = p.corrected[r * A + j];
                    dh[j] = c == 0.f ? 0.f : g0 * (2.f * (p.out[r * A + j] - c)) / n_all;
                }
            }
            const float y = p.oracle_stop[r];
            const float ds = y != -1.f ? g1 * (sigmoidf_(p.stop[r]) - y) / n_stop : 0.f;
            float dp = 0.f;
            if (monitor && p.corrected[r * A] != 0.f) {
                const float ph = p.progress_hat[r];
                dp = g2 * (2.f * (ph - p.progress[r])) * (1.f - ph * ph) / n_aux;
            }
#pragma unroll
            for (int k = 1; k < NH; ++k) {
                if (k == A) dh[k] = ds;
                if (k == A + 1) dh[k] = dp;
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxHeads; ++k) sdh[tid][k] = dh[k];
    }
    __syncthreads();

    const int q = tid & (kQ - 1), half = tid >> 7;
    float wv[NH][4], acc[NH][4];
#pragma unroll
    for (int k = 0; k < NH; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[k][e] = 0.f, acc[k][e] = 0.f;
        if (p.d_x) ld_chunk(head_w(p, k) + q * 4, wv[k]);
    }
    const int i1 = min(n, (half + 1) * kHalfRows);
#pragma unroll 4
    for (int i = half * kHalfRows; i < i1; ++i) {
        float xv[4], dh[NH];
        ld_chunk(p.x + ((size_t)r0 + i) * kH + q * 4, xv);
#pragma unroll
        for (int k = 0; k < NH; ++k) dh[k] = sdh[i][k];
        if (p.d_x) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = dh[0] * wv[0][e];
#pragma unroll
                for (int k = 1; k < NH; ++k) s += dh[k] * wv[k][e];
                o[e] = s;
            }
            st_chunk(p.d_x + ((size_t)r0 + i) * kH + q * 4, o);
        }
#pragma unroll
        for (int k = 0; k < NH; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] += dh[k] * xv[e];
    }
    if (half == 1) {
#pragma unroll
        for (int k = 0; k < NH; ++k) st_chunk(&sacc[k][q][0], acc[k]);
    }
    __syncthreads();
    if (half == 0) {
        float* part = p.work + (size_t)blockIdx.x * NH * kH;
#pragma unroll
        for (int k = 0; k < NH; ++k) {
            float o[4];
            ld_chunk(&sacc[k][q][0], o);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[k][e] + o[e];
            st_chunk(part + k * kH + q * 4, o);
        }
    }
    if (tid < NH) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += sdh[i][tid];
        p.work[(size_t)gridDim.x * NH * kH + (size_t)blockIdx.x * kBiasSlot + tid] = s;
    }
}

// d_W_k = sum_b part[b][k] and d_b_k = sum_b bias_part[b][k] in block order: thread f < NH * 128 owns a column quad of a head, the next NH threads a bias
__global__ __launch_bounds__(kT) void flat_heads_reduce_kernel(FlatHeadsArgs p, int NH, int nblk) {
    const int f = blockIdx.x * kT + threadIdx.x, A = p.num_actions;
    if (f < NH * kQ) {
        const int k = f / kQ, q = f % kQ;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < nblk; ++b) {
            float v[4];
            ld_chunk(p.work + ((size_t)b * NH + k) * kH + q * 4, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
        float* dst = k < A ? p.d_w_lin + (size_t)k * kH : k == A ? p.d_w_stop : p.d_w_pm;
        st_chunk(dst + q * 4, s);
    } else if (f < NH * kQ + NH) {
        const int k = f - NH * kQ;
        const float* bp = p.work + (size_t)nblk * NH * kH;
        float s = 0.f;
        for (int b = 0; b < nblk; ++b) s += bp[(size_t)b * kBiasSlot + k];
        float* dst = k < A ? p.d_b_lin + k : k == A ? p.d_b_stop : p.d_b_pm;
        *dst = s;
    }
}

int heads(const FlatHeadsArgs& t) { return t.num_actions + 1 + (t.w_pm != nullptr ? 1 : 0); }

}  // namespace

bool flat_heads_ok(int rows, int hidden, int num_actions) { return rows >= 0 && hidden == kH && num_actions >= 1 && num_actions <= kMaxHeads - 2; }

size_t flat_heads_work_floats(int rows, int num_actions) {
    const size_t nblk = ((size_t)rows + kBwdRows - 1) / kBwdRows;
    return nblk * ((size_t)(num_actions + 2) * kH + kBiasSlot);
}

hipError_t launch_flat_heads_fwd(const FlatHeadsArgs& t, hipStream_t s) {
    if (!flat_heads_ok(t.rows, kH, t.num_actions)) return hipErrorInvalidValue;
    if (t.rows == 0) return hipSuccess;
    const dim3 grid((t.rows + kFwdRows - 1) / kFwdRows), block(kT);
    switch (heads(t)) {
        case 2: hipLaunchKernelGGL(flat_heads_fwd_kernel<2>, grid, block, 0, s, t); break;
        case 3: hipLaunchKernelGGL(flat_heads_fwd_kernel<3>, grid, block, 0, s, t); break;
        case 4: hipLaunchKernelGGL(flat_heads_fwd_kernel<4>, grid, block, 0, s, t); break;
        case 5: hipLaunchKernelGGL(flat_heads_fwd_kernel<5>, grid, block, 0, s, t); break;
        default: hipLaunchKernelGGL(flat_heads_fwd_kernel<6>, grid, block, 0, s, t); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_flat_val_loss(t.out, t.num_actions, t.stop, 1, t.progress_hat, 1, t.corrected, t.oracle_stop, t.progress, t.result, t.rows,
                                t.num_actions, s);
}

hipError_t launch_flat_heads_bwd(const FlatHeadsArgs& t, hipStream_t s) {
    if (!flat_heads_ok(t.rows, kH, t.num_actions)) return hipErrorInvalidValue;
    if (t.rows == 0) return hipSuccess;
    const int nblk = (t.rows + kBwdRows - 1) / kBwdRows, NH = heads(t);
    const dim3 grid(nblk), block(kT);
    switch (NH) {
        case 2: hipLaunchKernelGGL(flat_heads_bwd_kernel<2>, grid, block, 0, s, t); break;
        case 3: hipLaunchKernelGGL(flat_heads_bwd_kernel<3>, grid, block, 0, s, t); break;
        case 4: hipLaunchKernelGGL(flat_heads_bwd_kernel<4>, grid, block, 0, s, t); break;
        case 5: hipLaunchKernelGGL(flat_heads_bwd_kernel<5>, grid, block, 0, s, t); break;
        default: hipLaunchKernelGGL(flat_heads_bwd_kernel<6>, grid, block, 0, s, t); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flat_heads_reduce_kernel, dim3((NH * kQ + NH + kT - 1) / kT), block, 0, s, t, NH, nblk);
    return hipGetLastError();
}

}  // namespace hcm
