// CMANet's attention stage (cma.py:271-311) in float32 with a backward pass, behind train.attn1q.  Every _attn call there has ONE query per sample
// and keys that are a 1x1 convolution of the raw tokens, so the key projection folds into the query: with qt = q W_k (the caller's product) and
// X = [x | e] (C = C0 + Ce channels, I positions; e is a channel tail shared by all samples -- the spatial embedding -- read where it lies)
//     a = softmax(scale (X^T qt - 1e8 mask)),   xbar = X a
// and q.b_k, the same for every position, cancels in the softmax.  K and V are never formed; the value projection of xbar is the caller's.
//
// One workgroup of 256 threads per sample, a streaming kernel: the forward reads the sample twice (logits, then the weighted sum), the backward
// twice (da = X^T d_xbar, then d_qt = X dlog); the second read comes from L2 (a sample is at most 400 KiB), nothing is staged but qt, d_xbar and
// the I-vectors (DESIGN_LOG CMAT.1).  x is token-major (B, I, C0) -- a wave owns a token for the dot products, a thread a channel quad for the
// weighted sums -- or channel-major (B, C0, I) -- a wave reads 64 consecutive units of the flat sample, each lane at a fixed position, for the dot
// products, and a thread owns a channel for the weighted sums.  V = 4 moves 16 bytes per lane (token-major: C0 % 4 == 0; channel-major:
// I % 4 == 0, which also keeps every sample on a 16-byte boundary), V = 1 a dword; the launcher picks from the shape, and both are correct for any
// C0 >= 1.  Every sum runs in an order fixed by (layout, C0, Ce, I) alone; d_e is per-sample partials in `work` summed in sample order by a
// second launch (the pattern of vla_train_ln_reduce_kernel).  No atomics: bitwise reproducible.
#include "dev.h"
#include "kernels.h"

namespace hcm {
namespace {

constexpr int kT = 256, kW = kT / 64, kMaxC = 4096, kMaxI = 256, kRed = 1024;

struct Attn1qP {
    const float *qt, *x, *e, *d_xbar;
    float *a, *xbar, *d_qt, *d_x, *part;
    float scale;
    int mask_zero, C0, Ce, I;
};

template <int V> __device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
        o[0] = *p;
    }
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&o)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    else *p = o[0];
}

// the workgroup's sum / maximum of one value per thread: the wave butterflies, then the four waves in the order ((w0 + w1) + w2) + w3
__device__ __forceinline__ float block_sum(float v, float* s4, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) s4[tid >> 6] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}
__device__ __forceinline__ float block_max(float v, float* s4, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) s4[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s4[0], s4[1]), fmaxf(s4[2], s4[3]));
}

// the sample's row of a (B, C) tensor into LDS: channels [0, C0) at sv[0..], the tail at sv[C0r..], C0r = C0 rounded up to four, so that both
// parts can be read 16 bytes at a time (C itself need not be a multiple of four: dword loads)
__device__ __forceinline__ void stage_row(float* sv, const float* __restrict__ row, int C0, int Ce, int tid) {
    const int C0r = (C0 + 3) & ~3;
    for (int c = tid; c < C0; c += kT) sv[c] = row[c];
    for (int c = tid; c < Ce; c += kT) sv[C0r + c] = row[C0 + c];
}

// dot[i] += rows[i][0..n) . sv[0..n), nz[i] |= (some rows[i][c] != 0), i < I: wave `wave` owns the tokens i = wave, wave + 4, ...; n % V == 0
template <int V>
__device__ __forceinline__ void row_dots(const float* __restrict__ rows, int ld, int n, const float* sv, int I, float* dot, int* nz, int lane, int wave) {
    for (int i = wave; i < I; i += kW) {
        const float* r = rows + (size_t)i * ld;
        float acc = 0.f;
        int any = 0;
#pragma unroll 4
        for (int c = lane * V; c < n; c += 64 * V) {
            float xv[V], qv[V];
            ldv<V>(r + c, xv);
            ldv<V>(sv + c, qv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                acc += xv[k] * qv[k];
                any |= !(xv[k] == 0.f);
            }
        }
        acc = wave_sum(acc);
        any = __any(any);
        if (lane == 0) dot[i] += acc, nz[i] |= any;
    }
}

// the same for a channel-major sample xs[c * I + i]: Iu = I / V units per channel.  Iu <= 64: a wave step covers 64 / Iu whole channels (lane =
// channel-in-step * Iu + unit, the lanes behind them rest); Iu > 64 (V = 1 only): one channel per step and ceil(Iu / 64) sweeps.  A lane's unit
// is fixed, so its partial sums stay in registers; they meet in `red` ([wave][sweep][lane][V]) and thread t < I adds those of position t in the
// order wave, then channel-in-step.
template <int V>
__device__ __forceinline__ void col_dots(const float* __restrict__ xs, int C0, int I, const float* sv, float* dot, int* nz, float* red, int* rnz, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int Iu = I / V, packed = Iu <= 64, per = packed ? 64 / Iu : 1, nic = packed ? 1 : (Iu + 63) / 64;
    const int cl = packed ? lane / Iu : 0, il = packed ? lane % Iu : lane;
    for (int ic = 0; ic < nic; ++ic) {
        const int u = ic * 64 + il;
        float acc[V];
        int any = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;
        if (cl < per && u < Iu) {
#pragma unroll 4
            for (int c = wave * per + cl; c < C0; c += kW * per) {
                float xv[V];
                ldv<V>(xs + (size_t)c * I + u * V, xv);
                const float q = sv[c];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    acc[k] += xv[k] * q;
                    any |= (int)!(xv[k] == 0.f) << k;
                }
            }
        }
        const int slot = (wave * nic + ic) * 64 + lane;
        stv<V>(red + slot * V, acc);
        rnz[slot] = any;
    }
    __syncthreads();
    if (tid < I) {
        const int u = tid / V, k = tid % V, ic = packed ? 0 : u / 64;
        float s = 0.f;
        int any = 0;
        for (int w = 0; w < kW; ++w)
            for (int j = 0; j < per; ++j) {
                const int slot = (w * nic + ic) * 64 + (packed ? j * Iu + u : u % 64);
                s += red[slot * V + k];
                any |= (rnz[slot] >> k) & 1;
            }
        dot[tid] += s, nz[tid] |= any;
    }
    __syncthreads();
}

// out[c] = sum_i w[i] rows[i][c], c < n (n % V == 0): a thread owns V channels.  With fewer than 256 channel units the positions are dealt to
// P = 256 / units thread groups (group p takes i = p, p + P, ...) whose partial sums meet in `red` and are added in group order.
template <int V>
__device__ __forceinline__ void rows_wsum(const float* __restrict__ rows, int ld, int n, const float* w, int I, float* __restrict__ out, float* red, int tid) {
    const int nv = n / V;
    if (nv == 0) return;
    if (nv >= kT) {
        for (int v = tid; v < nv; v += kT) {
            float acc[V];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll 4
            for (int i = 0; i < I; ++i) {
                float xv[V];
                ldv<V>(rows + (size_t)i * ld + v * V, xv);
                const float wi = w[i];
#pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += wi * xv[k];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) out[v * V + k] = acc[k];
        }
        return;
    }
    const int P = kT / nv, p = tid / nv, v = tid % nv;
    if (p < P) {
        float acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll 4
        for (int i = p; i < I; i += P) {
            float xv[V];
            ldv<V>(rows + (size_t)i * ld + v * V, xv);
            const float wi = w[i];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += wi * xv[k];
        }
        stv<V>(red + (p * nv + v) * V, acc);
    }
    __syncthreads();
    for (int c = tid; c < n; c += kT) {
        float s = 0.f;
        for (int q = 0; q < P; ++q) s += red[q * n + c];
        out[c] = s;
    }
    __syncthreads();
}

// out[c] = sum_i w[i] xs[c * I + i], c < C0: a thread owns a channel and walks its I positions in order (I % V == 0)
template <int V>
__device__ __forceinline__ void cols_wsum(const float* __restrict__ xs, int C0, int I, const float* w, float* __restrict__ out, int tid) {
    for (int c = tid; c < C0; c += kT) {
        const float* r = xs + (size_t)c * I;
        float acc = 0.f;
#pragma unroll 4
        for (int i = 0; i < I; i += V) {
            float xv[V];
            ldv<V>(r + i, xv);
#pragma unroll
            for (int k = 0; k < V; ++k) acc += w[i + k] * xv[k];
        }
        out[c] = acc;
    }
}

// dot[i] = X[:, i] . sv and nz[i] = (some channel of position i is non-zero), tail first, then x
template <int LAYOUT, int V>
__device__ __forceinline__ void all_dots(const Attn1qP& p, const float* xs, const float* sv, float* dot, int* nz, float* red, int* rnz, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < p.I) dot[tid] = 0.f, nz[tid] = 0;
    __syncthreads();
    if (p.Ce) row_dots<4>(p.e, p.Ce, p.Ce, sv + ((p.C0 + 3) & ~3), p.I, dot, nz, lane, wave);
    __syncthreads();
    if constexpr (LAYOUT == 0) {
        row_dots<V>(xs, p.C0, p.C0, sv, p.I, dot, nz, lane, wave);
        __syncthreads();
    } else {
        col_dots<V>(xs, p.C0, p.I, sv, dot, nz, red, rnz, tid);
    }
}

// out[0..C) = X w: x's channels, then the tail
template <int LAYOUT, int V>
__device__ __forceinline__ void all_wsum(const Attn1qP& p, const float* xs, const float* w, float* out, float* red, int tid) {
    if constexpr (LAYOUT == 0) rows_wsum<V>(xs, p.C0, p.C0, w, p.I, out, red, tid);
    else cols_wsum<V>(xs, p.C0, p.I, w, out, tid);
    if (p.Ce) rows_wsum<4>(p.e, p.Ce, p.Ce, w, p.I, out + p.C0, red, tid);
}

template <int LAYOUT, int V>
__global__ __launch_bounds__(kT) void attn1q_train_fwd_kernel(Attn1qP p) {
    __shared__ __attribute__((aligned(16))) float sq[kMaxC + 4];
    __shared__ __attribute__((aligned(16))) float red[kRed];
    __shared__ int rnz[kRed];
    __shared__ float dot[kMaxI], sa[kMaxI], s4[kW];
    __shared__ int nz[kMaxI];
    const int tid = threadIdx.x, C = p.C0 + p.Ce;
    const size_t b = blockIdx.x;
    const float* xs = p.x + b * p.C0 * p.I;

    stage_row(sq, p.qt + b * C, p.C0, p.Ce, tid);
    all_dots<LAYOUT, V>(p, xs, sq, dot, nz, red, rnz, tid);

    // the mask as the reference writes it (cma.py:205-207): 1e8 off the logit, THEN the scale; a fully masked sample comes out uniform
    float v = -INFINITY;
    if (tid < p.I) v = (dot[tid] - (p.mask_zero && !nz[tid] ? 1e8f : 0.f)) * p.scale;
    const float m = block_max(v, s4, tid);
    const float ex = tid < p.I ? expf(v - m) : 0.f;
    const float den = block_sum(ex, s4, tid);
    if (tid < p.I) {
        const float a = ex / den;
        sa[tid] = a;
        p.a[b * p.I + tid] = a;
    }
    __syncthreads();
    all_wsum<LAYOUT, V>(p, xs, sa, p.xbar + b * C, red, tid);
}

template <int LAYOUT, int V>
__global__ __launch_bounds__(kT) void attn1q_train_bwd_kernel(Attn1qP p) {
    __shared__ __attribute__((aligned(16))) float sq[kMaxC + 4];
    __shared__ __attribute__((aligned(16))) float sd[kMaxC + 4];
    __shared__ __attribute__((aligned(16))) float red[kRed];
    __shared__ int rnz[kRed];
    __shared__ float dot[kMaxI], sa[kMaxI], sw[kMaxI], s4[kW];
    __shared__ int nz[kMaxI];
    const int tid = threadIdx.x, C = p.C0 + p.Ce, C0r = (p.C0 + 3) & ~3;
    const size_t b = blockIdx.x;
    const float* xs = p.x + b * p.C0 * p.I;

    stage_row(sq, p.qt + b * C, p.C0, p.Ce, tid);
    stage_row(sd, p.d_xbar + b * C, p.C0, p.Ce, tid);
    if (tid < p.I) sa[tid] = p.a[b * p.I + tid];
    all_dots<LAYOUT, V>(p, xs, sd, dot, nz, red, rnz, tid);                   // da_i = x_i . d_xbar

    const float s = block_sum(tid < p.I ? sa[tid] * dot[tid] : 0.f, s4, tid);
    if (tid < p.I) sw[tid] = (p.scale * sa[tid]) * (dot[tid] - s);           // dlog_i
    __syncthreads();
    all_wsum<LAYOUT, V>(p, xs, sw, p.d_qt + b * C, red, tid);               // d_qt = X dlog

    if (p.d_x) {
        float* dx = p.d_x + b * p.C0 * p.I;
        const int nu = p.C0 * p.I / V;                                        // whole units: LAYOUT 0 has C0 % V == 0, LAYOUT 1 has I % V == 0
        for (int f = tid; f < nu; f += kT) {
            float o[V];
            if constexpr (LAYOUT == 0) {
                const int i = f * V / p.C0, c = f * V % p.C0;
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = sd[c + k] * sa[i] + sq[c + k] * sw[i];
            } else {
                const int c = f * V / p.I, i = f * V % p.I;
#pragma unroll
                for (int k = 0; k < V; ++k) o[k] = sd[c] * sa[i + k] + sq[c] * sw[i + k];
            }
            stv<V>(dx + (size_t)f * V, o);
        }
    }
    if (p.Ce) {                                                               // this sample's share of d_e, (I, Ce)
        float* pe = p.part + b * p.I * p.Ce;
        for (int f = tid; f < p.I * p.Ce / 4; f += kT) {
            const int i = f * 4 / p.Ce, c = f * 4 % p.Ce;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = sd[C0r + c + k] * sa[i] + sq[C0r + c + k] * sw[i];
            stv<4>(pe + (size_t)f * 4, o);
        }
    }
}

// d_e[j] = sum_b part[b][j] in sample order, j < n (n % 4 == 0); B = 0 writes zeros
__global__ __launch_bounds__(kT) void attn1q_train_de_reduce_kernel(const float* __restrict__ part, float* __restrict__ d_e, int B, int n) {
    const int f = blockIdx.x * kT + threadIdx.x;
    if (f * 4 >= n) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
        const float4 v = *reinterpret_cast<const float4*>(part + (size_t)b * n + f * 4);
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    *reinterpret_cast<float4*>(d_e + f * 4) = s;
}

Attn1qP params(const Attn1qTrainArgs& t) {
    Attn1qP p;
    p.qt = t.qt; p.x = t.x; p.e = t.Ce ? t.e : nullptr; p.d_xbar = t.d_xbar;
    p.a = t.a; p.xbar = t.xbar; p.d_qt = t.d_qt; p.d_x = t.d_x; p.part = t.work;
    p.scale = t.scale; p.mask_zero = t.mask_zero; p.C0 = t.C0; p.Ce = t.Ce; p.I = t.I;
    return p;
}

// 16 bytes per lane where the shape keeps every access on a 16-byte boundary, a dword otherwise
int access_floats(int layout, int C0, int I) { return (layout == 0 ? C0 : I) % 4 == 0 ? 4 : 1; }

}  // namespace

bool attn1q_train_ok(int B, int C0, int Ce, int I) {
    return B >= 0 && C0 >= 1 && Ce >= 0 && Ce % 4 == 0 && I >= 1 && I <= kMaxI && C0 + Ce <= kMaxC;
}
size_t attn1q_train_work_floats(int B, int C0, int Ce, int I) { return (size_t)B * I * Ce; }

hipError_t launch_attn1q_train_fwd(const Attn1qTrainArgs& t, hipStream_t s) {
    if (!attn1q_train_ok(t.B, t.C0, t.Ce, t.I) || (t.layout != 0 && t.layout != 1)) return hipErrorInvalidValue;
    if (t.B == 0) return hipSuccess;
    const Attn1qP p = params(t);
    const int V = access_floats(t.layout, t.C0, t.I);
    if (t.layout == 0 && V == 4) hipLaunchKernelGGL((attn1q_train_fwd_kernel<0, 4>), dim3(t.B), dim3(kT), 0, s, p);
    else if (t.layout == 0) hipLaunchKernelGGL((attn1q_train_fwd_kernel<0, 1>), dim3(t.B), dim3(kT), 0, s, p);
    else if (V == 4) hipLaunchKernelGGL((attn1q_train_fwd_kernel<1, 4>), dim3(t.B), dim3(kT), 0, s, p);
    else hipLaunchKernelGGL((attn1q_train_fwd_kernel<1, 1>), dim3(t.B), dim3(kT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_attn1q_train_bwd(const Attn1qTrainArgs& t, hipStream_t s) {
    if (!attn1q_train_ok(t.B, t.C0, t.Ce, t.I) || (t.layout != 0 && t.layout != 1)) return hipErrorInvalidValue;
    if (t.B) {
        const Attn1qP p = params(t);
        const int V = access_floats(t.layout, t.C0, t.I);
        if (t.layout == 0 && V == 4) hipLaunchKernelGGL((attn1q_train_bwd_kernel<0, 4>), dim3(t.B), dim3(kT), 0, s, p);
        else if (t.layout == 0) hipLaunchKernelGGL((attn1q_train_bwd_kernel<0, 1>), dim3(t.B), dim3(kT), 0, s, p);
        else if (V == 4) hipLaunchKernelGGL((attn1q_train_bwd_kernel<1, 4>), dim3(t.B), dim3(kT), 0, s, p);
        else hipLaunchKernelGGL((attn1q_train_bwd_kernel<1, 1>), dim3(t.B), dim3(kT), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!t.Ce) return hipSuccess;
    const int n = t.I * t.Ce;
    hipLaunchKernelGGL(attn1q_train_de_reduce_kernel, dim3((n / 4 + kT - 1) / kT), dim3(kT), 0, s, t.work, t.d_e, t.B, n);
    return hipGetLastError();
}

}  // namespace hcm
