// The end of the hierarchical trainer's high-level update step (hierarchical_trainer.py:506-512) in float32 with a backward pass, behind
// train.subtask_ce: the head of Seq2Seq_HighLevel_CMA over the state encoder's rows x (rows, 512)
//     logits = x W^T + b                                                                     (A <= 6 sub-task logits per row, the model's raw output)
// and CrossEntropyLoss(ignore_index = -1, mean) of them against oracle_subtask - 1 with the accuracy counts of hcm_val_step.  The criterion is
// val_loss_kernel's (elementwise.hip) cross-entropy part restated -- that kernel reads the low-level labels unconditionally, so it cannot be
// launched for the high-level model alone -- with its arithmetic, its launch shape and its order of summation: the same bits.
//
// Forward: a wave per row, kFwdRows = 4 rows per workgroup.  Lane l holds x[4l .. 4l+3] and x[256 + 4l .. 256 + 4l+3] (two 16-byte loads), adds its
// eight products in that order and the 64 lanes meet in a xor butterfly: a row's bits depend on the row and the weights alone.
// Criterion: ONE workgroup of kLossT = 256 threads, thread t adds its rows t, t + 256, ... in row order, a xor butterfly per wave, lane 0 of wave 0
// adds the four waves' sums in wave order; counts are integers until the final store.
// Backward: a workgroup owns kBwdRows = 32 rows.  Threads 0..31 form the rows' d_logits (rows, A) from the saved logits (softmax recomputed around
// the row maximum), the labels, the count in result[4] and the cotangent d_result[0], all read on the device; then thread (half h, column quad q)
// walks rows 16 h .. 16 h+15 of the block in order, writes d_x[r, 4q..4q+3] = sum_j d_logits[r, j] W_j (classes in order; skipped with d_x = NULL)
// and accumulates d_logits[r, j] x[r, 4q..4q+3]; the block's d_W share is half 0 + half 1, its d_b share the sum of d_logits in row order.  A second
// launch adds the blocks' shares in block order (the pattern of flat_heads_reduce_kernel).  No atomics, no scratch: bitwise reproducible.
// A is a run-time argument: every loop over the classes is unrolled to kMaxA with a uniform guard, so each kernel has one instantiation.
#include "dev.h"
#include "kernels.h"

namespace hcm {
namespace {

constexpr int kT = 256, kH = 512, kQ = kH / 4, kFwdRows = kT / 64, kBwdRows = 32, kHalfRows = kBwdRows / 2, kMaxA = 6, kBiasSlot = 8, kLossT = 256;

__global__ __launch_bounds__(kT) void subtask_ce_fwd_kernel(SubtaskCeArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kFwdRows + wave;
    if (r >= p.rows) return;
    const int A = p.A;
    float xlo[4], xhi[4];
    ld_chunk(p.x + (size_t)r * kH + lane * 4, xlo);
    ld_chunk(p.x + (size_t)r * kH + kH / 2 + lane * 4, xhi);
#pragma unroll
    for (int k = 0; k < kMaxA; ++k) {
        if (k < A) {
            const float* w = p.w + (size_t)k * kH;
            float wlo[4], whi[4];
            ld_chunk(w + lane * 4, wlo);
            ld_chunk(w + kH / 2 + lane * 4, whi);
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += xlo[e] * wlo[e];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += xhi[e] * whi[e];
            const float v = wave_sum(acc) + p.b[k];
            if (lane == 0) p.logits[(size_t)r * A + k] = v;
        }
    }
}

// result[0] CrossEntropyLoss(ignore_index = -1, mean) over the rows with oracle in [1, num_sub_tasks];  result[3] those whose argmax (first maximal
// index, a NaN counts as the maximum) is the target;  result[4] their number;  result[6] rows with oracle outside [0, num_sub_tasks] (treated as
// padded);  result[1], [2], [5], [7] = 0.  The statements of val_loss_kernel, line for line, without the two low-level criteria.
__global__ __launch_bounds__(kLossT) void subtask_ce_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ oracle,
                                                                 float* __restrict__ result, int rows, int A, int num_sub_tasks) {
    float ce = 0.f;
    int correct = 0, total = 0, n_bad = 0;
    for (int r = threadIdx.x; r < rows; r += kLossT) {
        const int64_t o = oracle[r];
        if (o < 0 || o > num_sub_tasks) ++n_bad;
        else if (o != 0) {
            const float* p = logits + (size_t)r * A;
            const int target = (int)o - 1;
            int best = 0;
            float mx = p[0];
            for (int j = 1; j < A; ++j)
                if (p[j] > mx || (p[j] != p[j] && mx == mx)) { mx = p[j]; best = j; }
            float se = 0.f;
            for (int j = 0; j < A; ++j) se += expf(p[j] - mx);
            ce += target < A ? (mx + logf(se)) - p[target] : __builtin_nanf("");
            correct += best == target ? 1 : 0;
            ++total;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ce += __shfl_xor(ce, o, 64);
        correct += __shfl_xor(correct, o, 64); total += __shfl_xor(total, o, 64); n_bad += __shfl_xor(n_bad, o, 64);
    }
    constexpr int NW = kLossT / 64;
    __shared__ float fs[NW];
    __shared__ int is[NW][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        fs[wave] = ce;
        is[wave][0] = correct; is[wave][1] = total; is[wave][2] = n_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f = 0.f;
        int n[3] = {0, 0, 0};
        for (int w = 0; w < NW; ++w) {
            f += fs[w];
            for (int k = 0; k < 3; ++k) n[k] += is[w][k];
        }
        result[0] = f / (float)n[1];
        result[1] = 0.f;
        result[2] = 0.f;
        result[3] = (float)n[0];
        result[4] = (float)n[1];
        result[5] = 0.f;
        result[6] = (float)n[2];
        result[7] = 0.f;
    }
}

__global__ __launch_bounds__(kT) void subtask_ce_bwd_kernel(SubtaskCeArgs p) {
    __shared__ float sdl[kBwdRows][kMaxA];
    __shared__ __attribute__((aligned(16))) float sacc[kMaxA][kQ][4];
    const int tid = threadIdx.x, A = p.A;
    const int r0 = blockIdx.x * kBwdRows;
    const int n = min(kBwdRows, p.rows - r0);

    if (tid < kBwdRows) {
        float dl[kMaxA];
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) dl[j] = 0.f;
        if (tid < n) {
            const size_t r = (size_t)r0 + tid;
            const int64_t o = p.oracle[r];
            const float g0 = p.d_result[0], total = p.result[4];
            if (o >= 1 && o <= p.num_sub_tasks && total > 0.f) {
                const float* l = p.logits + r * A;
                const int target = (int)o - 1;
                float lv[kMaxA];
                float mx = l[0];
#pragma unroll
                for (int j = 0; j < kMaxA; ++j) {
                    lv[j] = j < A ? l[j] : 0.f;
                    if (j >= 1 && j < A && (lv[j] > mx || (lv[j] != lv[j] && mx == mx))) mx = lv[j];
                }
                float se = 0.f;
#pragma unroll
                for (int j = 0; j < kMaxA; ++j) {
                    lv[j] = j < A ? expf(lv[j] - mx) : 0.f;
                    if (j < A) se += lv[j];
                }
#pragma unroll
                for (int j = 0; j < kMaxA; ++j)
                    if (j < A) dl[j] = g0 * (lv[j] / se - (j == target ? 1.f : 0.f)) / total;
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxA; ++j) sdl[tid][j] = dl[j];
    }
    __syncthreads();

    const int q = tid & (kQ - 1), half = tid >> 7;
    float wv[kMaxA][4], acc[kMaxA][4];
#pragma unroll
    for (int k = 0; k < kMaxA; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[k][e] = 0.f, acc[k][e] = 0.f;
        if (p.d_x && k < A) ld_chunk(p.w + (size_t)k * kH + q * 4, wv[k]);
    }
    const int i1 = min(n, (half + 1) * kHalfRows);
#pragma unroll 2
    for (int i = half * kHalfRows; i < i1; ++i) {
        float xv[4], dl[kMaxA];
        ld_chunk(p.x + ((size_t)r0 + i) * kH + q * 4, xv);
#pragma unroll
        for (int k = 0; k < kMaxA; ++k) dl[k] = sdl[i][k];
        if (p.d_x) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = dl[0] * wv[0][e];
#pragma unroll
                for (int k = 1; k < kMaxA; ++k)
                    if (k < A) s += dl[k] * wv[k][e];
                o[e] = s;
            }
            st_chunk(p.d_x + ((size_t)r0 + i) * kH + q * 4, o);
        }
#pragma unroll
        for (int k = 0; k < kMaxA; ++k)
            if (k < A) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[k][e] += dl[k] * xv[e];
            }
    }
    if (half == 1) {
#pragma unroll
        for (int k = 0; k < kMaxA; ++k)
            if (k < A) st_chunk(&sacc[k][q][0], acc[k]);
    }
    __syncthreads();
    if (half == 0) {
        float* part = p.work + (size_t)blockIdx.x * A * kH;
#pragma unroll
        for (int k = 0; k < kMaxA; ++k)
            if (k < A) {
                float o[4];
                ld_chunk(&sacc[k][q][0], o);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = acc[k][e] + o[e];
                st_chunk(part + k * kH + q * 4, o);
            }
    }
    if (tid < A) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s += sdl[i][tid];
        p.work[(size_t)gridDim.x * A * kH + (size_t)blockIdx.x * kBiasSlot + tid] = s;
    }
}

// d_W_k = sum_b part[b][k] and d_b_k = sum_b bias_part[b][k] in block order: thread f < A * 128 owns a column quad of a class, the next A threads a bias
__global__ __launch_bounds__(kT) void subtask_ce_reduce_kernel(SubtaskCeArgs p, int nblk) {
    const int f = blockIdx.x * kT + threadIdx.x, A = p.A;
    if (f < A * kQ) {
        const int k = f / kQ, q = f % kQ;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < nblk; ++b) {
            float v[4];
            ld_chunk(p.work + ((size_t)b * A + k) * kH + q * 4, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
        st_chunk(p.d_w + (size_t)k * kH + q * 4, s);
    } else if (f < A * kQ + A) {
        const int k = f - A * kQ;
        const float* bp = p.work + (size_t)nblk * A * kH;
        float s = 0.f;
        for (int b = 0; b < nblk; ++b) s += bp[(size_t)b * kBiasSlot + k];
        p.d_b[k] = s;
    }
}

}  // namespace

bool subtask_ce_ok(int rows, int hidden, int A, int num_sub_tasks) {
    return rows >= 0 && hidden == kH && num_sub_tasks >= 1 && num_sub_tasks <= A && A <= kMaxA;
}

size_t subtask_ce_work_floats(int rows, int A) {
    const size_t nblk = ((size_t)rows + kBwdRows - 1) / kBwdRows;
    return nblk * ((size_t)A * kH + kBiasSlot);
}

hipError_t launch_subtask_ce_fwd(const SubtaskCeArgs& t, hipStream_t s) {
    if (!subtask_ce_ok(t.rows, kH, t.A, t.num_sub_tasks)) return hipErrorInvalidValue;
    if (t.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(subtask_ce_fwd_kernel, dim3((unsigned)(((size_t)t.rows + kFwdRows - 1) / kFwdRows)), dim3(kT), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(subtask_ce_loss_kernel, dim3(1), dim3(kLossT), 0, s, t.logits, t.oracle, t.result, t.rows, t.A, t.num_sub_tasks);
    return hipGetLastError();
}

hipError_t launch_subtask_ce_bwd(const SubtaskCeArgs& t, hipStream_t s) {
    if (!subtask_ce_ok(t.rows, kH, t.A, t.num_sub_tasks)) return hipErrorInvalidValue;
    if (t.rows == 0) return hipSuccess;
    const int nblk = (int)(((size_t)t.rows + kBwdRows - 1) / kBwdRows);
    hipLaunchKernelGGL(subtask_ce_bwd_kernel, dim3(nblk), dim3(kT), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(subtask_ce_reduce_kernel, dim3((t.A * kQ + t.A + kT - 1) / kT), dim3(kT), 0, s, t, nblk);
    return hipGetLastError();
}

}  // namespace hcm
