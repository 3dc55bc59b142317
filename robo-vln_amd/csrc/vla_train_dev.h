// Device building blocks of the float32 training kernels (vla_train.hip, embed_train.hip); vla_train.hip's header comment describes them.
#pragma once
#include "dev.h"

#include <cstddef>

namespace hcm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRows = 64, kMT = kRows / 32, kLDA = 260;
constexpr size_t kVlaTrainLds = (size_t)2 * kRows * kLDA * sizeof(float);

struct PackJob { const float* src; float4* dst; int ld, trans, K, N; };
struct PackJobs { PackJob j[3]; };

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[kMT][2]) {
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
}

// acc += As[64][K = 256] * B[256][two n-tiles]: b0 / b1 point at float4 (ntile, kk0, lane 0) of the wave's two tiles; the next step's B fragments
// are loaded in front of the current step's 16 MFMAs (one wave per SIMD: nothing else hides the L2 latency)
__device__ __forceinline__ void gemm_k256(const float* As, const float4* __restrict__ b0p, const float4* __restrict__ b1p, f32x16 (&acc)[kMT][2], int lane) {
    const float* ap = As + (lane & 31) * kLDA + 4 * (lane >> 5);
    float4 b0 = b0p[lane], b1 = b1p[lane];
#pragma unroll 2
    for (int kk = 0; kk < 32; ++kk) {
        const int kn = kk + 1 < 32 ? kk + 1 : kk;
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

// element (mt, nt, r) of a wave's accumulators: block row and panel column
__device__ __forceinline__ int acc_row(int mt, int r, int lane) { return mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int acc_col(int wave, int nt, int lane) { return wave * 64 + nt * 32 + (lane & 31); }

// acc + bias -> Ys[row][col]
__device__ __forceinline__ void acc_to_lds(float* Ys, const f32x16 (&acc)[kMT][2], const float* __restrict__ bias, int wave, int lane) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int col = acc_col(wave, nt, lane);
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Ys[acc_row(mt, r, lane) * kLDA + col] = acc[mt][nt][r] + bv;
    }
}

__device__ __forceinline__ float4 keep4(const uint8_t* keep, size_t off, float4 v, float s) {
    if (!keep) return v;
    const uchar4 k = *reinterpret_cast<const uchar4*>(keep + off);
    return make_float4(k.x ? v.x * s : 0.f, k.y ? v.y * s : 0.f, k.z ? v.z * s : 0.f, k.w ? v.w * s : 0.f);
}
__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }

// one LayerNorm row by a wave: lane owns columns 4 lane .. 4 lane + 3.  Two passes over registers (mean, then centred squares).
__device__ __forceinline__ void ln_row(float4 y, float4 g, float4 be, float4& xh, float4& x, float& rstd) {
    const float mean = wave_sum(sum4(y)) * (1.f / 256.f);
    const float4 d = make_float4(y.x - mean, y.y - mean, y.z - mean, y.w - mean);
    const float var = wave_sum(sum4(make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w))) * (1.f / 256.f);
    rstd = 1.f / sqrtf(var + 1e-5f);
    xh = make_float4(d.x * rstd, d.y * rstd, d.z * rstd, d.w * rstd);
    x = make_float4(xh.x * g.x + be.x, xh.y * g.y + be.y, xh.z * g.z + be.z, xh.w * g.w + be.w);
}

// LayerNorm backward of one row by a wave: dy = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dx g; the parameter gradients accumulate per lane
__device__ __forceinline__ float4 ln_row_bwd(float4 dx, float4 xh, float4 g, float rstd, float4& pg, float4& pb) {
    const float4 dxh = make_float4(dx.x * g.x, dx.y * g.y, dx.z * g.z, dx.w * g.w);
    const float m1 = wave_sum(sum4(dxh)) * (1.f / 256.f);
    const float m2 = wave_sum(sum4(make_float4(dxh.x * xh.x, dxh.y * xh.y, dxh.z * xh.z, dxh.w * xh.w))) * (1.f / 256.f);
    pg.x += dx.x * xh.x, pg.y += dx.y * xh.y, pg.z += dx.z * xh.z, pg.w += dx.w * xh.w;
    pb.x += dx.x, pb.y += dx.y, pb.z += dx.z, pb.w += dx.w;
    return make_float4(rstd * (dxh.x - m1 - xh.x * m2), rstd * (dxh.y - m1 - xh.y * m2), rstd * (dxh.z - m1 - xh.z * m2), rstd * (dxh.w - m1 - xh.w * m2));
}

}  // namespace hcm
