// One half of Visual_Ling_Attn's prologue (transformer.py:262-274) in float32 with a backward pass, behind train.embed_ln, on vla_train.hip's building
// blocks (vla_train_dev.h; that file's header comment describes them):  y = LN(keep s relu(x W^T + b)) + post[row % period]  for x (rows, K), K a
// multiple of 64 up to 1024, output width 256.
//
// embed_ln_fwd_kernel: K goes through the two LDS images in slices of 256, the next slice waiting in registers while the MFMAs run on the current
// one; the pre-activation, the ReLU and the dropout product exist only in LDS and registers; y, xhat, rstd and gate = (pre > 0) && keep (one byte
// per element instead of a saved r) are stored.  embed_ln_bwd_kernel: LayerNorm backward -> gate -> d_pre (stored, and the A operand in LDS) ->
// d_x = d_pre W in panels of 256 columns (skipped when nobody asks for d_x); the LayerNorm parameter partials go through vla_train.hip's reduce.
// dW = d_pre^T x and db are the caller's.  No atomics: bitwise reproducible.
#include "dev.h"
#include "kernels.h"
#include "vla_train_dev.h"

namespace hcm {

constexpr size_t kEmbedBwdLds = (size_t)kRows * kLDA * sizeof(float) + (size_t)4 * 2 * 64 * sizeof(float4);

struct EmbedFwd {
    const float *x, *b, *g, *be, *post;
    const float4* w;                          // fragment order: B = W^T (K rows, N 256)
    const uint8_t* keep;
    float s;
    float *y, *xhat, *rstd;
    uint8_t* gate;
    int rows, K, period;
};

// columns [k0, k0 + ks) of the block's 64 rows of x: thread-owned float4s (a wave reads 1 KB of one row), zeros behind the last row and behind ks
__device__ __forceinline__ void embed_load_slice(float4 (&st)[16], const float* __restrict__ x, size_t r0, int nrow, int K, int k0, int ks, int tid) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = tid + 256 * j, rr = i >> 6, c = (i & 63) * 4;
        st[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rr < nrow && c < ks) st[j] = *reinterpret_cast<const float4*>(x + (r0 + rr) * K + k0 + c);
    }
}
__device__ __forceinline__ void embed_store_slice(float* X, const float4 (&st)[16], int tid) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = tid + 256 * j;
        *reinterpret_cast<float4*>(X + (i >> 6) * kLDA + (i & 63) * 4) = st[j];
    }
}

// gemm_k256 for a K slice of 8 nkk columns, nkk a multiple of 8 known only at run time (gemm_k256's `unroll 2` needs its constant trip count)
__device__ __forceinline__ void gemm_kslice(const float* As, const float4* __restrict__ b0p, const float4* __restrict__ b1p, f32x16 (&acc)[kMT][2], int lane, int nkk) {
    const float* ap = As + (lane & 31) * kLDA + 4 * (lane >> 5);
    float4 b0 = b0p[lane], b1 = b1p[lane];
    for (int kk = 0; kk < nkk; ++kk) {
        const int kn = kk + 1 < nkk ? kk + 1 : kk;
        const float4 nb0 = b0p[kn * 64 + lane], nb1 = b1p[kn * 64 + lane];
        float4 a[kMT];
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) a[mt] = *reinterpret_cast<const float4*>(ap + mt * 32 * kLDA + kk * 8);
        const float c0[4] = {b0.x, b0.y, b0.z, b0.w}, c1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt) {
                const float av = j == 0 ? a[mt].x : j == 1 ? a[mt].y : j == 2 ? a[mt].z : a[mt].w;
                acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, c0[j], acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, c1[j], acc[mt][1], 0, 0, 0);
            }
        b0 = nb0, b1 = nb1;
    }
}

__global__ __launch_bounds__(256) void embed_ln_fwd_kernel(EmbedFwd p) {
    extern __shared__ float4 embed_train_smem[];
    float* S = reinterpret_cast<float*>(embed_train_smem);          // two [64][260] images: the K slices alternate, the epilogue uses the first
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * kRows;
    const int nrow = p.rows - r0 < (size_t)kRows ? (int)(p.rows - r0) : kRows;
    const int K8 = p.K / 8;

    float4 st[16];
    embed_load_slice(st, p.x, r0, nrow, p.K, 0, p.K < 256 ? p.K : 256, tid);
    embed_store_slice(S, st, tid);
    __syncthreads();

    f32x16 acc[kMT][2];
    zero_acc(acc);
    int cur = 0;
    for (int k0 = 0; k0 < p.K; k0 += 256) {
        const int ks = p.K - k0 < 256 ? p.K - k0 : 256, k1 = k0 + 256;
        // the next slice is on its way into registers while the MFMAs run; it goes into the image that the previous slice's MFMAs have left
        // (every wave is past the barrier that ended them)
        if (k1 < p.K) embed_load_slice(st, p.x, r0, nrow, p.K, k1, p.K - k1 < 256 ? p.K - k1 : 256, tid);
        gemm_kslice(S + cur * kRows * kLDA, p.w + ((size_t)(2 * wave) * K8 + k0 / 8) * 64, p.w + ((size_t)(2 * wave + 1) * K8 + k0 / 8) * 64, acc, lane, ks / 8);
        if (k1 < p.K) embed_store_slice(S + (cur ^ 1) * kRows * kLDA, st, tid);
        __syncthreads();
        cur ^= 1;
    }
    acc_to_lds(S, acc, p.b, wave, lane);
    __syncthreads();

    const float4 g = reinterpret_cast<const float4*>(p.g)[lane], be = reinterpret_cast<const float4*>(p.be)[lane];
    const float s = p.keep ? p.s : 1.f;
    for (int rr = wave; rr < nrow; rr += 4) {
        const size_t o = (r0 + rr) * 256 + lane * 4;
        const float4 v = *reinterpret_cast<const float4*>(S + rr * kLDA + lane * 4);
        const uchar4 k = p.keep ? *reinterpret_cast<const uchar4*>(p.keep + o) : make_uchar4(1, 1, 1, 1);
        const uchar4 gt = make_uchar4(v.x > 0.f && k.x, v.y > 0.f && k.y, v.z > 0.f && k.z, v.w > 0.f && k.w);
        float4 xh, y;
        float rstd;
        ln_row(make_float4(gt.x ? v.x * s : 0.f, gt.y ? v.y * s : 0.f, gt.z ? v.z * s : 0.f, gt.w ? v.w * s : 0.f), g, be, xh, y, rstd);
        if (p.post) {
            const float4 t = *reinterpret_cast<const float4*>(p.post + (size_t)((unsigned)(r0 + rr) % (unsigned)p.period) * 256 + lane * 4);
            y = make_float4(y.x + t.x, y.y + t.y, y.z + t.z, y.w + t.w);
        }
        *reinterpret_cast<float4*>(p.y + o) = y;
        *reinterpret_cast<float4*>(p.xhat + o) = xh;
        *reinterpret_cast<uchar4*>(p.gate + o) = gt;
        if (lane == 0) p.rstd[r0 + rr] = rstd;
    }
}

struct EmbedBwd {
    const float *d_y, *g, *xhat, *rstd;
    const uint8_t* gate;
    const float4* w;                          // fragment order, transposed use: B = W (256 rows, N K)
    float s;
    float *d_pre, *d_x, *part;
    int rows, K;
};

__global__ __launch_bounds__(256) void embed_ln_bwd_kernel(EmbedBwd p) {
    extern __shared__ float4 embed_train_smem[];
    float* X = reinterpret_cast<float*>(embed_train_smem);
    float4* P = reinterpret_cast<float4*>(X + kRows * kLDA);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * kRows;
    const int nrow = p.rows - r0 < (size_t)kRows ? (int)(p.rows - r0) : kRows;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pg = zero4, pb = zero4;

    const float4 g = reinterpret_cast<const float4*>(p.g)[lane];
    for (int rr = wave; rr < kRows; rr += 4) {
        float4 dp = zero4;
        if (rr < nrow) {
            const size_t o = (r0 + rr) * 256 + lane * 4;
            const float4 dr = ln_row_bwd(*reinterpret_cast<const float4*>(p.d_y + o), *reinterpret_cast<const float4*>(p.xhat + o), g, p.rstd[r0 + rr], pg, pb);
            const uchar4 gt = *reinterpret_cast<const uchar4*>(p.gate + o);
            dp = make_float4(gt.x ? dr.x * p.s : 0.f, gt.y ? dr.y * p.s : 0.f, gt.z ? dr.z * p.s : 0.f, gt.w ? dr.w * p.s : 0.f);
            *reinterpret_cast<float4*>(p.d_pre + o) = dp;
        }
        *reinterpret_cast<float4*>(X + rr * kLDA + lane * 4) = dp;
    }
    // the workgroup's LayerNorm parameter partials: the four waves in the order (w0 + w1) + (w2 + w3), into the first two of the four vectors
    // that launch_train_ln_reduce strides over
    P[(wave * 2 + 0) * 64 + lane] = pg, P[(wave * 2 + 1) * 64 + lane] = pb;
    __syncthreads();
    const float* Pf = reinterpret_cast<const float*>(P);
#pragma unroll
    for (int w = 0; w < 2; ++w)
        p.part[((size_t)blockIdx.x * 4 + w) * 256 + tid] = (Pf[(0 * 2 + w) * 256 + tid] + Pf[(1 * 2 + w) * 256 + tid]) + (Pf[(2 * 2 + w) * 256 + tid] + Pf[(3 * 2 + w) * 256 + tid]);
    if (!p.d_x) return;

    // d_x = d_pre W in panels of 256 columns; the last panel of a K that is no multiple of 256 has 2, 4 or 6 tiles, and the waves behind them rest
    for (int n0 = 0; n0 < p.K; n0 += 256) {
        const int tiles = (p.K - n0 < 256 ? p.K - n0 : 256) / 32;
        if (2 * wave >= tiles) continue;
        f32x16 acc[kMT][2];
        zero_acc(acc);
        gemm_k256(X, p.w + (size_t)(n0 / 32 + 2 * wave) * 32 * 64, p.w + (size_t)(n0 / 32 + 2 * wave + 1) * 32 * 64, acc, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int col = n0 + acc_col(wave, nt, lane);
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = acc_row(mt, r, lane);
                    if (rr < nrow) p.d_x[(r0 + rr) * p.K + col] = acc[mt][nt][r];
                }
        }
    }
}

bool embed_train_ok(int rows, int K) { return rows >= 0 && K >= 64 && K <= 1024 && K % 64 == 0; }
size_t embed_train_work_floats(int rows, int K) { return (size_t)256 * K + ((size_t)rows + kRows - 1) / kRows * 1024; }

// forward: B[k][n] = W[n][k], K rows; backward: B[k][n] = W[k][n], 256 rows
static hipError_t embed_train_pack(const float* w, float* work, int K, bool bwd, hipStream_t s) {
    return bwd ? launch_train_pack(w, work, K, 0, 256, K, s) : launch_train_pack(w, work, K, 1, K, 256, s);
}

hipError_t launch_embed_train_fwd(const EmbedTrainArgs& t, hipStream_t s) {
    if (!embed_train_ok(t.rows, t.K) || (t.post && t.period < 1)) return hipErrorInvalidValue;
    if (t.rows == 0) return hipSuccess;
    hipError_t e = embed_train_pack(t.w, t.work, t.K, false, s);
    if (e != hipSuccess) return e;
    EmbedFwd p;
    p.x = t.x; p.b = t.b; p.g = t.gamma; p.be = t.beta; p.post = t.post; p.w = reinterpret_cast<const float4*>(t.work); p.keep = t.keep;
    p.s = 1.f / (1.f - t.p);
    p.y = t.y; p.xhat = t.xhat; p.rstd = t.rstd; p.gate = t.gate; p.rows = t.rows; p.K = t.K; p.period = t.post ? t.period : 1;
    if ((e = hipFuncSetAttribute((const void*)embed_ln_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVlaTrainLds)) != hipSuccess) return e;
    hipLaunchKernelGGL(embed_ln_fwd_kernel, dim3((t.rows + kRows - 1) / kRows), dim3(256), kVlaTrainLds, s, p);
    return hipGetLastError();
}

hipError_t launch_embed_train_bwd(const EmbedTrainArgs& t, hipStream_t s) {
    if (!embed_train_ok(t.rows, t.K)) return hipErrorInvalidValue;
    const int nwg = (t.rows + kRows - 1) / kRows;
    float* part = t.work + (size_t)256 * t.K;
    hipError_t e;
    if (nwg) {
        if (t.d_x && (e = embed_train_pack(t.w, t.work, t.K, true, s)) != hipSuccess) return e;
        EmbedBwd p;
        p.d_y = t.d_y; p.g = t.gamma; p.xhat = t.xhat; p.rstd = t.rstd; p.gate = t.gate; p.w = reinterpret_cast<const float4*>(t.work);
        p.s = 1.f / (1.f - t.p);
        p.d_pre = t.d_pre; p.d_x = t.d_x; p.part = part; p.rows = t.rows; p.K = t.K;
        if ((e = hipFuncSetAttribute((const void*)embed_ln_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEmbedBwdLds)) != hipSuccess) return e;
        hipLaunchKernelGGL(embed_ln_bwd_kernel, dim3(nwg), dim3(256), kEmbedBwdLds, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_train_ln_reduce(part, t.d_ln, nwg, 2, s);
}

}  // namespace hcm
