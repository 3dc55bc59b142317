// The cross-modal layer (InterModuleAttnLayer, transformer.py:209-221) after its three projections in float32, with what a backward pass needs:
// the training forward and the fused backward behind train.vla_layer.  Dropout enters as explicit keep masks (uint8, one per element; null =
// no dropout at that place), s = 1 / (1 - p):
//
//   a   = softmax(q k^T / 8) v                         x1  = LN1(I + keep1 s u),  u = a Wo^T + bo
//   h   = keep2 s relu(x1 W1^T + b1)                   out = LN2(x1 + keep3 s z), z = h W2^T + b2
//
// Forward, three launches: vla_train_pack_kernel (the three weights into operand-fragment order, below), vla_train_attn_fwd_kernel (a),
// vla_train_fwd_kernel (everything behind a).  Saved for the backward: a, x1, h (post-dropout) -- the three left operands of the weight
// gradients, which the caller reduces -- and x1hat, x2hat (the normalised rows, (y - mean) * rstd) with rstd (rows, 2): with the normalised rows
// saved, the means are not needed and nothing in front of a LayerNorm has to be recomputed.  The attention probabilities are not saved: the
// backward recomputes them from q and kv with the forward's own device function (attn_probs), at most 64 keys per row.
//
// Backward, four launches: the pack (the same three weights, transposed use), vla_train_bwd_kernel (row-local: LN2 backward -> d_z -> d_z W2 ->
// ReLU / keep2 -> d_hpre -> d_hpre W1 + residual -> LN1 backward -> d_I, d_u -> da = d_u Wo, and the four LayerNorm parameter gradients as
// per-workgroup partial sums), vla_train_attn_bwd_kernel (one workgroup per (sample, head): d_q per row, d_k / d_v summed over the sample's L
// rows in a fixed order), vla_train_ln_reduce_kernel (the partials in workgroup order).  No atomics anywhere: bitwise reproducible.
//
// GEMMs: v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fmaf chain).  A workgroup of 4 waves owns kRows = 64 rows; its A operand sits in LDS
// ([64][260] floats; a lane reads 16 bytes = four k of its row), wave w owns output columns [64 w, 64 w + 64) of a 256-column panel (2 x 2 tiles
// of 32 x 32: 64 accumulator registers; 128 while fc1's chunk and fc2's sum are both live).  The B operand comes straight from L2 in fragment
// order: float4 index (ntile * K/8 + kk) * 64 + lane holds B[k = 8 kk + 4 (lane >> 5) + j][n = 32 ntile + (lane & 31)], j = 0..3 -- a wave's load
// instruction covers 1 KB contiguous and feeds 4 MFMAs per row tile.  The k order inside a step of 8 is (0,4),(1,5),(2,6),(3,7) for A and B alike.
// d_ff goes through in chunks of 256: fc1's chunk is rounded through LDS into fc2's K slice, so the (rows, d_ff) intermediate is stored (it
// is saved) but never read back by the launch that made it.
#include "dev.h"
#include "kernels.h"
#include "vla_train_dev.h"

#include <cstddef>

namespace hcm {

// B[k][n] = trans ? src[n * ld + k] : src[k * ld + n] into fragment order
__global__ __launch_bounds__(256) void vla_train_pack_kernel(PackJobs jobs) {
    const PackJob jb = jobs.j[blockIdx.y];
    const int K8 = jb.K / 8;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)(jb.N / 32) * K8 * 64) return;
    const int lane = (int)(idx & 63);
    const size_t t = idx >> 6;
    const int kk = (int)(t % K8), ntile = (int)(t / K8);
    const int n = ntile * 32 + (lane & 31), k = kk * 8 + 4 * (lane >> 5);
    float4 v;
    if (jb.trans) v = *reinterpret_cast<const float4*>(jb.src + (size_t)n * jb.ld + k);
    else v = make_float4(jb.src[(size_t)k * jb.ld + n], jb.src[(size_t)(k + 1) * jb.ld + n], jb.src[(size_t)(k + 2) * jb.ld + n], jb.src[(size_t)(k + 3) * jb.ld + n]);
    jb.dst[idx] = v;
}

struct VlaTrainFwd {
    const float *a, *I, *bo, *b1, *b2, *g1, *be1, *g2, *be2;
    const float4 *wo, *w1, *w2;               // fragment order: Wo (K 256, N 256), W1 (K 256, N d_ff), W2 (K d_ff, N 256)
    const uint8_t *k1, *k2, *k3;
    float s;
    float *out, *x1, *x1hat, *h, *x2hat, *rstd;
    int rows, d_ff;
};

__global__ __launch_bounds__(256) void vla_train_fwd_kernel(VlaTrainFwd p) {
    extern __shared__ float4 vla_train_smem[];
    float* X = reinterpret_cast<float*>(vla_train_smem);
    float* Y = X + kRows * kLDA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * kRows;
    const int nrow = p.rows - r0 < (size_t)kRows ? (int)(p.rows - r0) : kRows;
    const int K8 = p.d_ff / 8;

    for (int i = tid; i < kRows * 64; i += 256) {
        const int rr = i >> 6, c4 = i & 63;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rr < nrow) v = *reinterpret_cast<const float4*>(p.a + (r0 + rr) * 256 + c4 * 4);
        *reinterpret_cast<float4*>(X + rr * kLDA + c4 * 4) = v;
    }
    __syncthreads();

    f32x16 acc[kMT][2];
    zero_acc(acc);
    gemm_k256(X, p.wo + (size_t)(2 * wave) * 32 * 64, p.wo + (size_t)(2 * wave + 1) * 32 * 64, acc, lane);
    acc_to_lds(Y, acc, p.bo, wave, lane);
    __syncthreads();                      // (every wave is past its reads of a in X as well)

    const float4 g1 = reinterpret_cast<const float4*>(p.g1)[lane], be1 = reinterpret_cast<const float4*>(p.be1)[lane];
    for (int rr = wave; rr < nrow; rr += 4) {
        const size_t o = (r0 + rr) * 256 + lane * 4;
        const float4 u = keep4(p.k1, o, *reinterpret_cast<const float4*>(Y + rr * kLDA + lane * 4), p.s);
        const float4 I4 = *reinterpret_cast<const float4*>(p.I + o);
        float4 xh, x;
        float rstd;
        ln_row(make_float4(I4.x + u.x, I4.y + u.y, I4.z + u.z, I4.w + u.w), g1, be1, xh, x, rstd);
        *reinterpret_cast<float4*>(p.x1hat + o) = xh;
        *reinterpret_cast<float4*>(p.x1 + o) = x;
        *reinterpret_cast<float4*>(X + rr * kLDA + lane * 4) = x;
        if (lane == 0) p.rstd[(r0 + rr) * 2] = rstd;
    }
    __syncthreads();

    f32x16 zacc[kMT][2];
    zero_acc(zacc);
    for (int c = 0; c < p.d_ff / 256; ++c) {
        zero_acc(acc);
        gemm_k256(X, p.w1 + (size_t)(c * 8 + 2 * wave) * 32 * 64, p.w1 + (size_t)(c * 8 + 2 * wave + 1) * 32 * 64, acc, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int col = acc_col(wave, nt, lane), f = c * 256 + col;
            const float bv = p.b1[f];
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = acc_row(mt, r, lane);
                    float v = 0.f;
                    if (rr < nrow) {
                        const size_t o = (r0 + rr) * p.d_ff + f;
                        v = relu_f(acc[mt][nt][r] + bv);
                        if (p.k2) v = p.k2[o] ? v * p.s : 0.f;
                        p.h[o] = v;
                    }
                    Y[rr * kLDA + col] = v;
                }
        }
        __syncthreads();
        gemm_k256(Y, p.w2 + ((size_t)(2 * wave) * K8 + c * 32) * 64, p.w2 + ((size_t)(2 * wave + 1) * K8 + c * 32) * 64, zacc, lane);
        __syncthreads();
    }
    acc_to_lds(Y, zacc, p.b2, wave, lane);
    __syncthreads();

    const float4 g2 = reinterpret_cast<const float4*>(p.g2)[lane], be2 = reinterpret_cast<const float4*>(p.be2)[lane];
    for (int rr = wave; rr < nrow; rr += 4) {
        const size_t o = (r0 + rr) * 256 + lane * 4;
        const float4 z = keep4(p.k3, o, *reinterpret_cast<const float4*>(Y + rr * kLDA + lane * 4), p.s);
        const float4 x1 = *reinterpret_cast<const float4*>(X + rr * kLDA + lane * 4);
        float4 xh, x;
        float rstd;
        ln_row(make_float4(x1.x + z.x, x1.y + z.y, x1.z + z.z, x1.w + z.w), g2, be2, xh, x, rstd);
        *reinterpret_cast<float4*>(p.x2hat + o) = xh;
        *reinterpret_cast<float4*>(p.out + o) = x;
        if (lane == 0) p.rstd[(r0 + rr) * 2 + 1] = rstd;
    }
}

struct VlaTrainBwd {
    const float *d_out, *x1hat, *h, *x2hat, *rstd, *g1, *g2;
    const float4 *w2, *w1, *wo;               // fragment order, transposed use: W2 (K 256, N d_ff), W1 (K d_ff, N 256), Wo (K 256, N 256)
    const uint8_t *k1, *k2, *k3;
    float s;
    float *d_I, *d_u, *d_hpre, *d_z, *da, *part;
    int rows, d_ff;
};

__global__ __launch_bounds__(256) void vla_train_bwd_kernel(VlaTrainBwd p) {
    extern __shared__ float4 vla_train_smem[];
    float* X = reinterpret_cast<float*>(vla_train_smem);
    float* Y = X + kRows * kLDA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * kRows;
    const int nrow = p.rows - r0 < (size_t)kRows ? (int)(p.rows - r0) : kRows;
    const int K8 = p.d_ff / 8;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pg1 = zero4, pb1 = zero4, pg2 = zero4, pb2 = zero4;

    // LN2 backward; dy2 (the residual branch into x1) waits in d_I, which the same lane reads back and overwrites in the LN1 phase
    const float4 g2 = reinterpret_cast<const float4*>(p.g2)[lane];
    for (int rr = wave; rr < kRows; rr += 4) {
        float4 dz = zero4;
        if (rr < nrow) {
            const size_t o = (r0 + rr) * 256 + lane * 4;
            const float4 dy2 = ln_row_bwd(*reinterpret_cast<const float4*>(p.d_out + o), *reinterpret_cast<const float4*>(p.x2hat + o), g2,
                                          p.rstd[(r0 + rr) * 2 + 1], pg2, pb2);
            dz = keep4(p.k3, o, dy2, p.s);
            *reinterpret_cast<float4*>(p.d_z + o) = dz;
            *reinterpret_cast<float4*>(p.d_I + o) = dy2;
        }
        *reinterpret_cast<float4*>(X + rr * kLDA + lane * 4) = dz;
    }
    __syncthreads();

    f32x16 acc[kMT][2], xacc[kMT][2];
    zero_acc(xacc);
    for (int c = 0; c < p.d_ff / 256; ++c) {
        zero_acc(acc);
        gemm_k256(X, p.w2 + (size_t)(c * 8 + 2 * wave) * 32 * 64, p.w2 + (size_t)(c * 8 + 2 * wave + 1) * 32 * 64, acc, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int col = acc_col(wave, nt, lane), f = c * 256 + col;
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = acc_row(mt, r, lane);
                    float v = 0.f;
                    if (rr < nrow) {
                        const size_t o = (r0 + rr) * p.d_ff + f;
                        const bool on = p.h[o] > 0.f && (!p.k2 || p.k2[o]);        // h = keep2 s relu(hpre) > 0 <=> kept and hpre > 0
                        v = on ? (p.k2 ? acc[mt][nt][r] * p.s : acc[mt][nt][r]) : 0.f;
                        p.d_hpre[o] = v;
                    }
                    Y[rr * kLDA + col] = v;
                }
        }
        __syncthreads();
        gemm_k256(Y, p.w1 + ((size_t)(2 * wave) * K8 + c * 32) * 64, p.w1 + ((size_t)(2 * wave + 1) * K8 + c * 32) * 64, xacc, lane);
        __syncthreads();
    }
    acc_to_lds(Y, xacc, nullptr, wave, lane);
    __syncthreads();

    const float4 g1 = reinterpret_cast<const float4*>(p.g1)[lane];
    for (int rr = wave; rr < kRows; rr += 4) {
        float4 du = zero4;
        if (rr < nrow) {
            const size_t o = (r0 + rr) * 256 + lane * 4;
            const float4 t = *reinterpret_cast<const float4*>(Y + rr * kLDA + lane * 4), dy2 = *reinterpret_cast<const float4*>(p.d_I + o);
            const float4 dy1 = ln_row_bwd(make_float4(t.x + dy2.x, t.y + dy2.y, t.z + dy2.z, t.w + dy2.w), *reinterpret_cast<const float4*>(p.x1hat + o), g1,
                                          p.rstd[(r0 + rr) * 2], pg1, pb1);
            du = keep4(p.k1, o, dy1, p.s);
            *reinterpret_cast<float4*>(p.d_I + o) = dy1;
            *reinterpret_cast<float4*>(p.d_u + o) = du;
        }
        *reinterpret_cast<float4*>(X + rr * kLDA + lane * 4) = du;
    }
    __syncthreads();

    zero_acc(acc);
    gemm_k256(X, p.wo + (size_t)(2 * wave) * 32 * 64, p.wo + (size_t)(2 * wave + 1) * 32 * 64, acc, lane);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = acc_col(wave, nt, lane);
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = acc_row(mt, r, lane);
                if (rr < nrow) p.da[(r0 + rr) * 256 + col] = acc[mt][nt][r];
            }
    }

    // the workgroup's LayerNorm parameter partials: the four waves in the order (w0 + w1) + (w2 + w3).  (Y was last read in front of the barrier above)
    float4* Yp = reinterpret_cast<float4*>(Y);
    Yp[(wave * 4 + 0) * 64 + lane] = pg1, Yp[(wave * 4 + 1) * 64 + lane] = pb1, Yp[(wave * 4 + 2) * 64 + lane] = pg2, Yp[(wave * 4 + 3) * 64 + lane] = pb2;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w)
        p.part[((size_t)blockIdx.x * 4 + w) * 256 + tid] = (Y[(0 * 4 + w) * 256 + tid] + Y[(1 * 4 + w) * 256 + tid]) + (Y[(2 * 4 + w) * 256 + tid] + Y[(3 * 4 + w) * 256 + tid]);
}

// d_ln[w][c] = sum over the row kernel's workgroups, in workgroup order
__global__ __launch_bounds__(256) void vla_train_ln_reduce_kernel(const float* __restrict__ part, float* __restrict__ d_ln, int nwg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    for (int g = 0; g < nwg; ++g) s += part[(size_t)g * 1024 + i];
    d_ln[i] = s;
}

// ---- attention: one workgroup per (sample, head); a wave per query row; lanes are keys for the scores and head dimensions for the sums over keys ----
constexpr int kKS = 65;          // LDS row stride of the sample's k / v head slices: lane = key and lane = dimension both conflict-free

__device__ __forceinline__ void load_kv_head(const float* __restrict__ kv, float* ks, float* vs, int Lk, int h, int tid) {
    for (int i = tid; i < 64 * 64; i += 256) {
        const int j = i >> 6, d = i & 63;
        ks[j * kKS + d] = j < Lk ? kv[(size_t)j * 512 + h * 64 + d] : 0.f;
        vs[j * kKS + d] = j < Lk ? kv[(size_t)j * 512 + 256 + h * 64 + d] : 0.f;
    }
}

// softmax(q k^T / 8) of the row whose q slice is qs[0..64): lane j returns P_j (0 for j >= Lk)
__device__ __forceinline__ float attn_probs(const float* qs, const float* ks, int Lk, int lane) {
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < 64; ++d) s = fmaf(qs[d], ks[lane * kKS + d], s);
    s = lane < Lk ? s * 0.125f : -INFINITY;
    const float m = wave_max(s);
    const float e = lane < Lk ? expf(s - m) : 0.f;
    return e / wave_sum(e);
}

__global__ __launch_bounds__(256) void vla_train_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ a, int L, int Lk) {
    __shared__ float ks[64 * kKS], vs[64 * kKS], qs[4][64], ps[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x >> 2, h = blockIdx.x & 3;
    load_kv_head(kv + (size_t)b * Lk * 512, ks, vs, Lk, h, tid);
    __syncthreads();
    const int i1 = (blockIdx.y + 1) * 64 < L ? (blockIdx.y + 1) * 64 : L;
    for (int i = blockIdx.y * 64 + wave; i < i1; i += 4) {
        const size_t o = ((size_t)b * L + i) * 256 + h * 64 + lane;
        qs[wave][lane] = q[o];
        __builtin_amdgcn_wave_barrier();
        ps[wave][lane] = attn_probs(qs[wave], ks, Lk, lane);
        __builtin_amdgcn_wave_barrier();
        float s = 0.f;
        for (int j = 0; j < Lk; ++j) s = fmaf(ps[wave][j], vs[j * kKS + lane], s);
        a[o] = s;
        __builtin_amdgcn_wave_barrier();
    }
}

// KB = ceil(Lk / 16): a wave keeps its d_k / d_v partials for 16 KB keys in registers (lane = head dimension)
template <int KB>
__global__ __launch_bounds__(256) void vla_train_attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ da,
                                                                  float* __restrict__ d_q, float* __restrict__ d_kv, int L, int Lk) {
    constexpr int NK = KB * 16;
    __shared__ float ks[64 * kKS], vs[64 * kKS], red[NK][64];
    __shared__ __attribute__((aligned(16))) float qs[4][64], das[4][64], ps[4][64], dss[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x >> 2, h = blockIdx.x & 3;
    load_kv_head(kv + (size_t)b * Lk * 512, ks, vs, Lk, h, tid);
    __syncthreads();
    float dk[NK], dv[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) dk[j] = 0.f, dv[j] = 0.f;
    for (int i = wave; i < L; i += 4) {
        const size_t o = ((size_t)b * L + i) * 256 + h * 64 + lane;
        const float qd = q[o], dad = da[o];
        qs[wave][lane] = qd, das[wave][lane] = dad;
        __builtin_amdgcn_wave_barrier();
        const float P = attn_probs(qs[wave], ks, Lk, lane);
        float dP = 0.f;
#pragma unroll 16
        for (int d = 0; d < 64; ++d) dP = fmaf(das[wave][d], vs[lane * kKS + d], dP);
        const float t = wave_sum(P * dP);            // lanes >= Lk: P = 0
        ps[wave][lane] = P;
        dss[wave][lane] = P * (dP - t) * 0.125f;
        __builtin_amdgcn_wave_barrier();
        float dq = 0.f;
        for (int j = 0; j < Lk; ++j) dq = fmaf(dss[wave][j], ks[j * kKS + lane], dq);
        d_q[o] = dq;
#pragma unroll
        for (int j4 = 0; j4 < NK / 4; ++j4) {         // keys >= Lk: both factors are 0
            const float4 s4 = reinterpret_cast<const float4*>(dss[wave])[j4], p4 = reinterpret_cast<const float4*>(ps[wave])[j4];
            dk[4 * j4] = fmaf(s4.x, qd, dk[4 * j4]), dk[4 * j4 + 1] = fmaf(s4.y, qd, dk[4 * j4 + 1]);
            dk[4 * j4 + 2] = fmaf(s4.z, qd, dk[4 * j4 + 2]), dk[4 * j4 + 3] = fmaf(s4.w, qd, dk[4 * j4 + 3]);
            dv[4 * j4] = fmaf(p4.x, dad, dv[4 * j4]), dv[4 * j4 + 1] = fmaf(p4.y, dad, dv[4 * j4 + 1]);
            dv[4 * j4 + 2] = fmaf(p4.z, dad, dv[4 * j4 + 2]), dv[4 * j4 + 3] = fmaf(p4.w, dad, dv[4 * j4 + 3]);
        }
        __builtin_amdgcn_wave_barrier();
    }
    // the four waves' partials in the fixed order ((w0 + w1) + w2) + w3, d_k then d_v, through one [keys][64] LDS tile
#pragma unroll
    for (int which = 0; which < 2; ++which)
        for (int w = 1; w < 4; ++w) {
            __syncthreads();
            if (wave == w)
#pragma unroll
                for (int j = 0; j < NK; ++j) red[j][lane] = which ? dv[j] : dk[j];
            __syncthreads();
            if (wave == 0)
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    if (which) dv[j] += red[j][lane];
                    else dk[j] += red[j][lane];
                }
        }
    if (wave == 0) {
        float* o = d_kv + (size_t)b * Lk * 512 + h * 64 + lane;
#pragma unroll
        for (int j = 0; j < NK; ++j)
            if (j < Lk) o[(size_t)j * 512] = dk[j], o[(size_t)j * 512 + 256] = dv[j];
    }
}

bool vla_train_ok(int B, int L, int Lk, int d_ff) {
    // L: the attention forward's grid.y is one 64-row chunk of a sample per workgroup (65535 at most)
    return B >= 1 && L >= 1 && L <= 65535 * 64 && Lk >= 1 && Lk <= 64 && d_ff >= 256 && d_ff <= 1024 && d_ff % 256 == 0 &&
           (long long)B * L <= 0x7fffffffLL / 64 && (long long)B * 4 <= 0x7fffffffLL;
}
size_t vla_train_work_floats(int B, int L, int Lk, int d_ff) {
    (void)Lk;
    const size_t rows = (size_t)B * L, nwg = (rows + kRows - 1) / kRows;
    return (size_t)256 * 256 + (size_t)2 * 256 * d_ff + rows * 256 + nwg * 1024;
}

static hipError_t vla_train_pack(const float* wo, const float* w1, const float* w2, float* work, int d_ff, bool bwd, hipStream_t s) {
    float4* f = reinterpret_cast<float4*>(work);
    PackJobs jobs;
    // forward: B[k][n] = W[n][k] (torch's (out, in) is the transposed operand); backward: B[k][n] = W[k][n]
    jobs.j[0] = PackJob{wo, f, 256, bwd ? 0 : 1, 256, 256};
    jobs.j[1] = bwd ? PackJob{w1, f + 64 * 256, 256, 0, d_ff, 256} : PackJob{w1, f + 64 * 256, 256, 1, 256, d_ff};
    jobs.j[2] = bwd ? PackJob{w2, f + 64 * 256 + 64 * d_ff, d_ff, 0, 256, d_ff} : PackJob{w2, f + 64 * 256 + 64 * d_ff, d_ff, 1, d_ff, 256};
    hipLaunchKernelGGL(vla_train_pack_kernel, dim3((64 * d_ff + 255) / 256, 3), dim3(256), 0, s, jobs);
    return hipGetLastError();
}

// for embed_train.hip: one weight into fragment order, and the fixed-order sum of nvec (<= 4) LayerNorm partial vectors per workgroup
hipError_t launch_train_pack(const float* src, float* dst, int ld, int trans, int K, int N, hipStream_t s) {
    PackJobs jobs = {};
    jobs.j[0] = PackJob{src, reinterpret_cast<float4*>(dst), ld, trans, K, N};
    hipLaunchKernelGGL(vla_train_pack_kernel, dim3((N / 32 * (K / 8) * 64 + 255) / 256, 1), dim3(256), 0, s, jobs);
    return hipGetLastError();
}
hipError_t launch_train_ln_reduce(const float* part, float* d_ln, int nwg, int nvec, hipStream_t s) {
    hipLaunchKernelGGL(vla_train_ln_reduce_kernel, dim3(nvec), dim3(256), 0, s, part, d_ln, nwg);
    return hipGetLastError();
}

hipError_t launch_vla_train_fwd(const VlaTrainArgs& t, hipStream_t s) {
    if (!vla_train_ok(t.B, t.L, t.Lk, t.d_ff)) return hipErrorInvalidValue;
    const size_t rows = (size_t)t.B * t.L;
    const int nwg = (int)((rows + kRows - 1) / kRows);
    hipError_t e = vla_train_pack(t.wo, t.w1, t.w2, t.work, t.d_ff, false, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vla_train_attn_fwd_kernel, dim3(t.B * 4, (t.L + 63) / 64), dim3(256), 0, s, t.q, t.kv, t.a, t.L, t.Lk);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const float4* f = reinterpret_cast<const float4*>(t.work);
    VlaTrainFwd p;
    p.a = t.a; p.I = t.I; p.bo = t.bo; p.b1 = t.b1; p.b2 = t.b2; p.g1 = t.g1; p.be1 = t.be1; p.g2 = t.g2; p.be2 = t.be2;
    p.wo = f; p.w1 = f + 64 * 256; p.w2 = f + 64 * 256 + 64 * t.d_ff;
    p.k1 = t.keep1; p.k2 = t.keep2; p.k3 = t.keep3; p.s = 1.f / (1.f - t.p);
    p.out = t.out; p.x1 = t.x1; p.x1hat = t.x1hat; p.h = t.h; p.x2hat = t.x2hat; p.rstd = t.rstd;
    p.rows = (int)rows; p.d_ff = t.d_ff;
    if ((e = hipFuncSetAttribute((const void*)vla_train_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVlaTrainLds)) != hipSuccess) return e;
    hipLaunchKernelGGL(vla_train_fwd_kernel, dim3(nwg), dim3(256), kVlaTrainLds, s, p);
    return hipGetLastError();
}

hipError_t launch_vla_train_bwd(const VlaTrainArgs& t, hipStream_t s) {
    if (!vla_train_ok(t.B, t.L, t.Lk, t.d_ff)) return hipErrorInvalidValue;
    const size_t rows = (size_t)t.B * t.L;
    const int nwg = (int)((rows + kRows - 1) / kRows);
    hipError_t e = vla_train_pack(t.wo, t.w1, t.w2, t.work, t.d_ff, true, s);
    if (e != hipSuccess) return e;
    const float4* f = reinterpret_cast<const float4*>(t.work);
    float* da = t.work + (size_t)256 * 256 + (size_t)2 * 256 * t.d_ff;
    float* part = da + rows * 256;
    VlaTrainBwd p;
    p.d_out = t.d_out; p.x1hat = t.x1hat; p.h = t.h; p.x2hat = t.x2hat; p.rstd = t.rstd; p.g1 = t.g1; p.g2 = t.g2;
    p.wo = f; p.w1 = f + 64 * 256; p.w2 = f + 64 * 256 + 64 * t.d_ff;
    p.k1 = t.keep1; p.k2 = t.keep2; p.k3 = t.keep3; p.s = 1.f / (1.f - t.p);
    p.d_I = t.d_I; p.d_u = t.d_u; p.d_hpre = t.d_hpre; p.d_z = t.d_z; p.da = da; p.part = part;
    p.rows = (int)rows; p.d_ff = t.d_ff;
    if ((e = hipFuncSetAttribute((const void*)vla_train_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVlaTrainLds)) != hipSuccess) return e;
    hipLaunchKernelGGL(vla_train_bwd_kernel, dim3(nwg), dim3(256), kVlaTrainLds, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 g(t.B * 4), blk(256);
    switch ((t.Lk + 15) / 16) {
        case 1: hipLaunchKernelGGL(vla_train_attn_bwd_kernel<1>, g, blk, 0, s, t.q, t.kv, da, t.d_q, t.d_kv, t.L, t.Lk); break;
        case 2: hipLaunchKernelGGL(vla_train_attn_bwd_kernel<2>, g, blk, 0, s, t.q, t.kv, da, t.d_q, t.d_kv, t.L, t.Lk); break;
        case 3: hipLaunchKernelGGL(vla_train_attn_bwd_kernel<3>, g, blk, 0, s, t.q, t.kv, da, t.d_q, t.d_kv, t.L, t.Lk); break;
        default: hipLaunchKernelGGL(vla_train_attn_bwd_kernel<4>, g, blk, 0, s, t.q, t.kv, da, t.d_q, t.d_kv, t.L, t.Lk); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vla_train_ln_reduce_kernel, dim3(4), dim3(256), 0, s, part, t.d_ln, nwg);
    return hipGetLastError();
}

}  // namespace hcm
