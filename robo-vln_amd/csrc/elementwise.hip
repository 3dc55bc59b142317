// Memory-bound kernels of the HCM step: frame packing, pooling, GroupNorm, LayerNorm, BERT
// embeddings, recurrent cells + heads, small glue.  All are HBM/L2-bound: 16-byte vector accesses,
// grid-stride loops, wave64 reductions.
#include <cstdlib>
#include <type_traits>
#include "kernels.h"
#include "dev.h"

namespace hcm {

// run `...` with T bound to the storage type named by dt
#define HCM_DISPATCH_T(dt, ...)                                           \
    do {                                                                  \
        if ((dt) == DT_BF16) { using T = bf16; __VA_ARGS__; }             \
        else if ((dt) == DT_F16) { using T = f16; __VA_ARGS__; }          \
        else if ((dt) == DT_F32) { using T = float; __VA_ARGS__; }        \
        else return hipErrorInvalidValue;                                 \
    } while (0)

static inline int grid_for(size_t n, int block = 256, int cap = 256 * 16) {
    size_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > (size_t)cap) g = cap;
    return (int)g;
}

// ------------------------------------------------------------------------------------------ packed RGB frame (stem)
// see kernels.h: launch_pack_frame.  One thread per packed pixel (8-byte store).
template <typename S, typename T>
__global__ void pack_frame_kernel(const S* __restrict__ x, T* __restrict__ y, int B, int H, int W, float scale, int bt, int Hp, int Wp) {
    const size_t total = (size_t)B * Hp * Wp;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int px = (int)(e % Wp);
        const int py = (int)((e / Wp) % Hp);
        const int b = (int)(e / ((size_t)Wp * Hp));
        const int ix = px - bt, iy = py - bt;            // bt: border on the top and left
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if ((unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H) {
            const S* p = x + ((size_t)(b * H + iy) * W + ix) * 3;
            v0 = (float)p[0] * scale; v1 = (float)p[1] * scale; v2 = (float)p[2] * scale;
        }
        T o[4];
        Tr<T>::st(&o[0], v0); Tr<T>::st(&o[1], v1); Tr<T>::st(&o[2], v2); Tr<T>::st(&o[3], 0.f);
        *reinterpret_cast<uint2*>(y + e * 4) = *reinterpret_cast<const uint2*>(o);
    }
}
// uint8 frames with the stem's border (round 5): FOUR packed pixels per thread.  Output pixels px0 .. px0 + 3 (px0 a multiple of 4) are input pixels
// px0 - 3 .. px0, i.e. bytes [3 px0 - 9, 3 px0 + 3) of the row: inside the 16-byte window that starts at the 4-byte-aligned byte 3 px0 - 12, read as four
// dwords (the row is 3 W bytes, W % 4 == 0: a dword is inside the row or outside it), written as two 16-byte stores.  The one-pixel-per-thread form
// issued three 1-byte loads and one 8-byte store per pixel and ran at 2.6 TB/s.  Same conversion ((float)byte * scale, one rounding): the same bits.
template <typename T>
__global__ __launch_bounds__(256) void pack_frame_u8x4_kernel(const uint8_t* __restrict__ x, T* __restrict__ y, int B, int H, int W, float scale, int Hp, int Wp) {
    const int Wq = Wp >> 2;
    const size_t total = (size_t)B * Hp * Wq;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % Wq);
        const int py = (int)((e / Wq) % Hp);
        const int b = (int)(e / ((size_t)Wq * Hp));
        const int px0 = q * 4, iy = py - 3;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        const bool row_ok = (unsigned)iy < (unsigned)H;
        if (row_ok) {
            const uint8_t* row = x + (size_t)(b * H + iy) * W * 3;
            const int a0 = 3 * px0 - 12;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int a = a0 + 4 * d;
                if (a >= 0 && a + 4 <= 3 * W) w[d] = *reinterpret_cast<const uint32_t*>(row + a);
            }
        }
        T o[16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ix = px0 - 3 + t;
            const bool ok = row_ok && (unsigned)ix < (unsigned)W;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = 3 * t + 3 + c;
                const float v = ok ? (float)((w[byte >> 2] >> ((byte & 3) * 8)) & 0xFFu) * scale : 0.f;
                Tr<T>::st(&o[t * 4 + c], v);
            }
            Tr<T>::st(&o[t * 4 + 3], 0.f);
        }
        T* yo = y + (((size_t)(b * Hp + py)) * Wp + px0) * 4;
        *reinterpret_cast<uint4*>(yo) = *reinterpret_cast<const uint4*>(o);
        *reinterpret_cast<uint4*>(yo + 8) = *reinterpret_cast<const uint4*>(o + 8);
    }
}
hipError_t launch_pack_frame(const void* x, int src_dt, void* y, int dt, int B, int H, int W, float scale, hipStream_t s, int border) {
    if ((W & 1) || (dt != DT_BF16 && dt != DT_F16)) return hipErrorInvalidValue;
    const int bt = border ? 3 : 0, Hp = border ? H + 6 : H, Wp = border ? W + 8 : W;
    const size_t total = (size_t)B * Hp * Wp;
    if (src_dt == DT_F32) {
        if (dt == DT_BF16) hipLaunchKernelGGL((pack_frame_kernel<float, bf16>), dim3(grid_for(total)), dim3(256), 0, s, (const float*)x, (bf16*)y, B, H, W, scale, bt, Hp, Wp);
        else hipLaunchKernelGGL((pack_frame_kernel<float, f16>), dim3(grid_for(total)), dim3(256), 0, s, (const float*)x, (f16*)y, B, H, W, scale, bt, Hp, Wp);
    } else if (src_dt == DT_U8 && border && (W & 3) == 0 && ((size_t)x & 3) == 0) {
        const size_t tot4 = (size_t)B * Hp * (Wp >> 2);
        if (dt == DT_BF16) hipLaunchKernelGGL((pack_frame_u8x4_kernel<bf16>), dim3(grid_for(tot4)), dim3(256), 0, s, (const uint8_t*)x, (bf16*)y, B, H, W, scale, Hp, Wp);
        else hipLaunchKernelGGL((pack_frame_u8x4_kernel<f16>), dim3(grid_for(tot4)), dim3(256), 0, s, (const uint8_t*)x, (f16*)y, B, H, W, scale, Hp, Wp);
    } else if (src_dt == DT_U8) {
        if (dt == DT_BF16) hipLaunchKernelGGL((pack_frame_kernel<uint8_t, bf16>), dim3(grid_for(total)), dim3(256), 0, s, (const uint8_t*)x, (bf16*)y, B, H, W, scale, bt, Hp, Wp);
        else hipLaunchKernelGGL((pack_frame_kernel<uint8_t, f16>), dim3(grid_for(total)), dim3(256), 0, s, (const uint8_t*)x, (f16*)y, B, H, W, scale, bt, Hp, Wp);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ depth avg_pool2d(2)
// habitat ResNetEncoder.forward: F.avg_pool2d(x, 2) on the (B,1,H,W) depth frame.
template <typename T>
__global__ void avgpool2_kernel(const float* __restrict__ x, T* __restrict__ y, int B, int H, int W) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t total = (size_t)B * Ho * Wo;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % Wo);
        const int oy = (int)((e / Wo) % Ho);
        const int b = (int)(e / ((size_t)Wo * Ho));
        const float* p = x + ((size_t)(b * H + 2 * oy) * W + 2 * ox);
        const float2 r0 = *reinterpret_cast<const float2*>(p);
        const float2 r1 = *reinterpret_cast<const float2*>(p + W);
        Tr<T>::st(y + e, ((r0.x + r0.y) + (r1.x + r1.y)) * 0.25f);
    }
}
// same, written into a zero-bordered frame [B][H/2 + 6][W/2 + 8] (3 px border left / top, 5 right, 3 bottom): the packed input
// of the depth trunk's 7x7/2 stem (kernels.h: launch_pack_frame describes the RGB counterpart)
template <typename T>
__global__ void avgpool2_padded_kernel(const float* __restrict__ x, T* __restrict__ y, int B, int H, int W) {
    const int Ho = H / 2, Wo = W / 2, Hp = Ho + 6, Wp = Wo + 8;
    const size_t total = (size_t)B * Hp * Wp;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int px = (int)(e % Wp) - 3;
        const int py = (int)((e / Wp) % Hp) - 3;
        const int b = (int)(e / ((size_t)Wp * Hp));
        float v = 0.f;
        if ((unsigned)px < (unsigned)Wo && (unsigned)py < (unsigned)Ho) {
            const float* p = x + ((size_t)(b * H + 2 * py) * W + 2 * px);
            const float2 r0 = *reinterpret_cast<const float2*>(p);
            const float2 r1 = *reinterpret_cast<const float2*>(p + W);
            v = ((r0.x + r0.y) + (r1.x + r1.y)) * 0.25f;
        }
        Tr<T>::st(y + e, v);
    }
}
hipError_t launch_avgpool2_f32_padded(const float* x, void* y, int dt, int B, int H, int W, hipStream_t s) {
    const size_t total = (size_t)B * (H / 2 + 6) * (W / 2 + 8);
    if ((W & 3) || (dt != DT_BF16 && dt != DT_F16)) return hipErrorInvalidValue;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(avgpool2_padded_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, x, (T*)y, B, H, W));
    return hipGetLastError();
}
hipError_t launch_avgpool2_f32(const float* x, void* y, int dt, int B, int H, int W, hipStream_t s) {
    const size_t total = (size_t)B * (H / 2) * (W / 2);
    if (W & 1) return hipErrorInvalidValue;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(avgpool2_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, x, (T*)y, B, H, W));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1) NHWC
template <typename T>
__global__ void maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C, int Ho, int Wo) {
    constexpr int CH = Tr<T>::CH;
    const int cv = C / CH;
    const size_t total = (size_t)B * Ho * Wo * cv;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % cv) * CH;
        const size_t pix = e / cv;
        const int ox = (int)(pix % Wo);
        const int oy = (int)((pix / Wo) % Ho);
        const int b = (int)(pix / ((size_t)Wo * Ho));
        // branch-free: an out-of-range tap is clamped onto the nearest valid one, which lies inside the same window (pad 1, stride 2),
        // so the maximum is unchanged -- and all nine 16-byte loads are in flight together
        int iy[3], ix[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            iy[d] = min(max(2 * oy - 1 + d, 0), H - 1);
            ix[d] = min(max(2 * ox - 1 + d, 0), W - 1);
        }
        float v[9][CH];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) ld_chunk(x + ((size_t)(b * H + iy[dy]) * W + ix[dx]) * C + c, v[dy * 3 + dx]);
        float m[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            m[j] = v[0][j];
#pragma unroll
            for (int t = 1; t < 9; ++t) m[j] = max_nan(m[j], v[t][j]);
        }
        st_chunk(y + pix * C + c, m);
    }
}
hipError_t launch_maxpool3x3s2(const void* x, void* y, int dt, int B, int H, int W, int C, int Ho, int Wo, hipStream_t s) {
    const int CH = dt_chunk(dt);
    if (C % CH) return hipErrorInvalidValue;
    const size_t total = (size_t)B * Ho * Wo * (C / CH);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(maxpool_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, (T*)y, B, H, W, C, Ho, Wo));
    return hipGetLastError();
}

// MaxPool2d(3, 2, 1) over relu(GroupNorm(x)) with the normalisation applied ON LOAD (round 5: the depth trunk's stem -- conv -> GroupNorm -> ReLU ->
// max-pool, habitat's ResNet stem as used at resnet_encoders.py:27-33).  x is the UN-normalised conv output, `part` the (sum, sum of squares) partials its
// epilogue left per (sample, 64-pixel block, group) -- what gn_apply_kernel would have consumed: the stand-alone apply pass (one read and one write of the
// largest map of the trunk) and its launch disappear.  The per-channel scale / shift and the expression v * sc - sh are gn_apply_kernel's; rounding is
// monotone and ReLU commutes with it, so max(round(relu(.))) == round(max(relu(.))): BIT-IDENTICAL to the apply pass followed by maxpool_kernel.
// grid (blocks per sample, B): a workgroup rebuilds its sample's scale / shift table (G <= 256 groups, C <= 512 channels) and pools a slice of its pixels.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_gn_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ part, int PS, float eps, int G, int H, int W, int C, int Ho, int Wo) {
    constexpr int CH = Tr<T>::CH;
    __shared__ float s_scale[512], s_shift[512];
    __shared__ float s_mean[256], s_rstd[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int Cg = C / G, HW = H * W;
    for (int g = tid; g < G; g += 256) {
        // (the partials are added in index order -- gn_apply_kernel's order -- but REQUESTED 16 at a time: the stem map has 256 of them per group, and
        //  four per round trip made this prologue 64 dependent round trips, ~40 us of a 44 us launch)
        float a = 0.f, q = 0.f;
        const float2* pp = reinterpret_cast<const float2*>(part) + (size_t)b * PS * G + g;
        int i = 0;
        for (; i + 16 <= PS; i += 16) {
            float2 t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = pp[(size_t)(i + u) * G];
#pragma unroll
            for (int u = 0; u < 16; ++u) { a += t[u].x; q += t[u].y; }
        }
        for (; i < PS; ++i) { const float2 t = pp[(size_t)i * G]; a += t.x; q += t.y; }
        const float inv_n = 1.0f / ((float)HW * (float)Cg);
        const float mean = a * inv_n;
        const float var = relu_f(q * inv_n - mean * mean);
        s_mean[g] = mean;
        s_rstd[g] = rsqrtf(var + eps);
    }
    __syncthreads();
    for (int ch = tid; ch < C; ch += 256) {
        const int g = ch / Cg;
        const float sc = s_rstd[g] * gamma[ch];
        s_scale[ch] = sc;
        s_shift[ch] = s_mean[g] * sc - beta[ch];
    }
    __syncthreads();
    const int cv = C / CH;
    const int total = Ho * Wo * cv;
    const T* xb = x + (size_t)b * HW * C;
    T* yb = y + (size_t)b * Ho * Wo * C;
    for (int e = blockIdx.x * 256 + tid; e < total; e += gridDim.x * 256) {
        const int c = (e % cv) * CH;
        const int pix = e / cv;
        const int ox = pix % Wo, oy = pix / Wo;
        int iy[3], ix[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            iy[d] = min(max(2 * oy - 1 + d, 0), H - 1);
            ix[d] = min(max(2 * ox - 1 + d, 0), W - 1);
        }
        float v[9][CH];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) ld_chunk(xb + ((size_t)iy[dy] * W + ix[dx]) * C + c, v[dy * 3 + dx]);
        float m[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const float sc = s_scale[c + j], sh = s_shift[c + j];
            m[j] = relu_f(v[0][j] * sc - sh);
#pragma unroll
            for (int t = 1; t < 9; ++t) m[j] = max_nan(m[j], relu_f(v[t][j] * sc - sh));
        }
        st_chunk(yb + (size_t)pix * C + c, m);
    }
}
bool maxpool_gn_ok(int dt, int C, int G) { return dt != DT_F32 && C % dt_chunk(dt) == 0 && C <= 512 && G >= 1 && G <= 256 && C % G == 0; }
hipError_t launch_maxpool3x3s2_gn(const void* x, void* y, const float* gamma, const float* beta, const float* part, int PS, float eps, int G, int dt, int B, int H,
                                  int W, int C, int Ho, int Wo, hipStream_t s) {
    if (!maxpool_gn_ok(dt, C, G) || PS < 1 || !part || !gamma || !beta) return hipErrorInvalidValue;
    const int total = Ho * Wo * (C / dt_chunk(dt));
    int bps = (total + 256 * 16 - 1) / (256 * 16);        // ~16 output chunks per thread: every workgroup rebuilds its sample's scale / shift table
    if (bps < 1) bps = 1;
    if (bps > 16) bps = 16;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(maxpool_gn_kernel<T>, dim3(bps, B), dim3(256), 0, s, (const T*)x, (T*)y, gamma, beta, part, PS, eps, G, H, W, C, Ho, Wo));
    return hipGetLastError();
}

// vertical half of MaxPool2d(3, 2, 1) (the horizontal half is fused into the stem conv's epilogue, igemm.hip)
template <typename T>
__global__ void vpool3s2_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C, int Ho) {
    constexpr int CH = Tr<T>::CH;
    const int cv = C / CH;
    const size_t rowv = (size_t)W * cv;                 // 16-byte vectors per row
    const size_t total = (size_t)B * Ho * rowv;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t in_row = e % rowv;
        const size_t rowi = e / rowv;
        const int oy = (int)(rowi % Ho);
        const int b = (int)(rowi / Ho);
        float v[3][CH];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int iy = min(max(2 * oy - 1 + d, 0), H - 1);      // clamped taps stay inside the window
            ld_chunk(x + ((size_t)(b * H + iy) * rowv + in_row) * CH, v[d]);
        }
        float m[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) m[j] = max_nan(max_nan(v[0][j], v[1][j]), v[2][j]);
        st_chunk(y + e * CH, m);
    }
}
hipError_t launch_vpool3s2(const void* x, void* y, int dt, int B, int H, int W, int C, hipStream_t s) {
    const int CH = dt_chunk(dt);
    if (C % CH) return hipErrorInvalidValue;
    const int Ho = (H + 2 - 3) / 2 + 1;
    const size_t total = (size_t)B * Ho * W * (C / CH);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(vpool3s2_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, (T*)y, B, H, W, C, Ho));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ adaptive_avg_pool2d NHWC
// F.adaptive_avg_pool2d(x,(OH,OW)) (resnet_encoders.py:160-166) / AdaptiveAvgPool2d(1): window [floor(i*H/OH), ceil((i+1)*H/OH)).
template <typename T>
__global__ void adaptive_pool_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H, int W, int C, int OH, int OW, int ldy, int ldx) {
    constexpr int CH = Tr<T>::CH;
    const int cv = C / CH;
    const size_t total = (size_t)B * OH * OW * cv;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % cv) * CH;
        const size_t pix = e / cv;
        const int ox = (int)(pix % OW);
        const int oy = (int)((pix / OW) % OH);
        const int b = (int)(pix / ((size_t)OW * OH));
        const int y0 = (oy * H) / OH, y1 = ((oy + 1) * H + OH - 1) / OH;
        const int x0 = (ox * W) / OW, x1 = ((ox + 1) * W + OW - 1) / OW;
        float acc[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] = 0.f;
        for (int iy = y0; iy < y1; ++iy) {
#pragma unroll 4
            for (int ix = x0; ix < x1; ++ix) {
                float v[CH];
                ld_chunk(x + ((size_t)(b * H + iy) * W + ix) * ldx + c, v);
#pragma unroll
                for (int j = 0; j < CH; ++j) acc[j] += v[j];
            }
        }
        const float inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] *= inv;
        st_chunk(y + pix * ldy + c, acc);
    }
}
hipError_t launch_adaptive_avgpool(const void* x, void* y, int dt, int B, int H, int W, int C, int OH, int OW, int ldy, hipStream_t s, int ldx) {
    const int CH = dt_chunk(dt);
    if (ldx <= 0) ldx = C;
    if (C % CH || ldy % CH || ldx % CH) return hipErrorInvalidValue;
    const size_t total = (size_t)B * OH * OW * (C / CH);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(adaptive_pool_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, (T*)y, B, H, W, C, OH, OW, ldy, ldx));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ mean over rows
// AdaptiveAvgPool1d(1) over tokens: rgb_linear.0 (seq2seq_highlevel_cma.py:83-85), cross_pooler (:114-115,:209-210).
template <typename T>
__global__ void mean_rows_kernel(const T* __restrict__ x, void* __restrict__ y, int B, int S0, int C, int ldx, int ldy, int out_f32,
                                 const int* __restrict__ lens) {
    const size_t total = (size_t)B * C;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const int b = (int)(e / C);
        const T* p = x + (size_t)b * S0 * ldx + c;
        int S = S0;
        if (lens) { S = lens[b]; S = S < 1 ? 1 : S > S0 ? S0 : S; }
        // four independent partial sums and an unrolled body keep several loads in flight (a single dependent chain
        // of S strided 2-byte loads costs S x L2 latency: 24 us for the 80-token cross_pooler)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int s_ = 0;
#pragma unroll 2
        for (; s_ + 4 <= S; s_ += 4) {
            a0 += Tr<T>::ld(p + (size_t)s_ * ldx);
            a1 += Tr<T>::ld(p + (size_t)(s_ + 1) * ldx);
            a2 += Tr<T>::ld(p + (size_t)(s_ + 2) * ldx);
            a3 += Tr<T>::ld(p + (size_t)(s_ + 3) * ldx);
        }
        for (; s_ < S; ++s_) a0 += Tr<T>::ld(p + (size_t)s_ * ldx);
        float acc = ((a0 + a1) + (a2 + a3)) / (float)S;
        if (out_f32) reinterpret_cast<float*>(y)[(size_t)b * ldy + c] = acc;
        else Tr<T>::st(reinterpret_cast<T*>(y) + (size_t)b * ldy + c, acc);
    }
}
hipError_t launch_mean_rows(const void* x, void* y, int dt, int B, int S, int C, int ldx, int ldy, int out_f32, hipStream_t s, const int* lens) {
    const size_t total = (size_t)B * C;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(mean_rows_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, y, B, S, C, ldx, ldy, out_f32, lens));
    return hipGetLastError();
}

template <typename T>
__global__ void fill_cols_kernel(const float* __restrict__ tab, T* __restrict__ y, int B, int S, int C, int ldy) {
    const size_t total = (size_t)B * S * C;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const size_t row = e / C;            // b*S + s
        const int s_ = (int)(row % S);
        Tr<T>::st(y + row * ldy + c, tab[s_ * C + c]);
    }
}
hipError_t launch_fill_cols(const float* tab, void* y, int dt, int B, int S, int C, int ldy, hipStream_t s) {
    const size_t total = (size_t)B * S * C;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(fill_cols_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, tab, (T*)y, B, S, C, ldy));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ GroupNorm (NHWC, in place)
// nn.GroupNorm(G, C) after every conv of the habitat ResNet (+ residual + ReLU of the bottleneck), ONE launch:
// a workgroup owns (sample b, slab of CS channels made of whole groups): pass 1 accumulates per-channel sum / sum of
// squares in registers (a thread always sees the same 16-byte channel chunk), wave-shuffle + LDS reduce to per-group
// mean / rstd in f32; pass 2 re-reads the slab (L2-resident: HW*CS*2 B <= 64 KB for every layer of the trunk),
// normalises, adds the residual, applies ReLU and stores.  No atomics, no memset, no stats buffer.
// float32 storage (gn_pivot<T>): the sums run over x - K, K = the group's first element of the sample (read before anything is stored), so that
// var = q / n - (a / n)^2 cancels against |mean - K|, not against |mean| -- E[x^2] - mean^2 loses (mean / std)^2 ulps.  For a conv output whose
// first element is an ordinary draw |mean - K| <~ 2 std.  Worst case: that element is itself an outlier (a spike at pixel 0 of a sparse map); then
// |mean - K| / std reaches sqrt(n) -- 45 at 2 048 elements, 362 at 131 072 -- and the shifted sums cancel worse than the plain ones would have
// (tests/test_norm_conditioning_gpu.py, test_groupnorm_float32_outlier_in_the_pivot_element: a relative error of 1.5 d 2^-24 (1 + r^2) at most,
// d the depth of the summation).  Groups with zero-padded channels (cg_true) keep K = 0 and so the plain one-pass sums: the padding would enter
// the shifted ones.  16-bit storage keeps the plain sums: its values carry
// |mean| / std <= 2^8 .. 2^11 at best, and the kernels share their arithmetic with the conv-epilogue statistics.
template <typename T> constexpr bool gn_pivot = std::is_same<T, float>::value;
template <typename T>
__global__ __launch_bounds__(256) void gn_fused_kernel(T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int HW, int C, int G, int CS, float eps, int relu, int cg_true) {
    constexpr int CH = Tr<T>::CH;
    __shared__ float s_p1[4][1024], s_p2[4][1024];                         // per-wave partials (fixed summation order)
    __shared__ float s_sum[1024], s_sq[1024], s_mean[1024], s_rstd[1024];  // per channel of the slab (CS <= 1024)
    const int slabs = C / CS;
    const int b = blockIdx.x / slabs;
    const int c_base = (blockIdx.x % slabs) * CS;
    const int Cg = C / G;
    const int cpr = CS / CH;                 // 16-byte chunks per pixel inside the slab (power of two, <= 32)
    const int tid = threadIdx.x;
    const int cc = tid % cpr;                // this thread's chunk column (fixed)
    const int prow = tid / cpr;              // first pixel
    const int pstep = 256 / cpr;
    T* xb = x + (size_t)b * HW * C + c_base + cc * CH;
    const T* rb = res ? res + (size_t)b * HW * C + c_base + cc * CH : nullptr;
    for (int i = tid; i < 4 * 1024; i += 256) { (&s_p1[0][0])[i] = 0.f; (&s_p2[0][0])[i] = 0.f; }
    __syncthreads();
    float s1[CH], s2[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const T* x0 = x + (size_t)b * HW * C + c_base;      // pixel 0 of the slab: the pivots (this workgroup alone stores to the slab, in pass 2)
    float piv[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) piv[j] = 0.f;
    if constexpr (gn_pivot<T>) {
        if (!cg_true) {
#pragma unroll
            for (int j = 0; j < CH; ++j) piv[j] = Tr<T>::ld(x0 + ((cc * CH + j) / Cg) * Cg);
        }
    }
    for (int p = prow; p < HW; p += pstep) {
        float v[CH];
        ld_chunk(xb + (size_t)p * C, v);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if constexpr (gn_pivot<T>) v[j] -= piv[j];
            s1[j] += v[j]; s2[j] += v[j] * v[j];
        }
    }
    // lanes with equal (lane % cpr) hold the same channels: butterfly over the other lane bits
    for (int o = 32; o >= cpr; o >>= 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) { s1[j] += __shfl_xor(s1[j], o, 64); s2[j] += __shfl_xor(s2[j], o, 64); }
    }
    if ((tid & 63) < cpr) {
        const int wv = tid >> 6;
#pragma unroll
        for (int j = 0; j < CH; ++j) { s_p1[wv][cc * CH + j] = s1[j]; s_p2[wv][cc * CH + j] = s2[j]; }
    }
    __syncthreads();
    for (int ch = tid; ch < CS; ch += 256) {
        s_sum[ch] = (s_p1[0][ch] + s_p1[1][ch]) + (s_p1[2][ch] + s_p1[3][ch]);
        s_sq[ch] = (s_p2[0][ch] + s_p2[1][ch]) + (s_p2[2][ch] + s_p2[3][ch]);
    }
    __syncthreads();
    for (int ch = tid; ch < CS; ch += 256) {
        const int g0 = (ch / Cg) * Cg;       // first channel of this channel's group (inside the slab)
        float a = 0.f, q = 0.f;
        for (int j = 0; j < Cg; ++j) { a += s_sum[g0 + j]; q += s_sq[g0 + j]; }
        const float inv_n = 1.0f / ((float)HW * (float)(cg_true > 0 ? cg_true : Cg));     // cg_true: the group's other channels are zero padding
        float mean = a * inv_n;
        const float var = relu_f(q * inv_n - mean * mean);
        if constexpr (gn_pivot<T>) { if (!cg_true) mean += Tr<T>::ld(x0 + g0); }
        const float rstd = rsqrtf(var + eps);
        const float ga = gamma[c_base + ch];
        s_mean[ch] = mean * rstd * ga - beta[c_base + ch];     // y = x*scale - shift'
        s_rstd[ch] = rstd * ga;
    }
    __syncthreads();
    float sc[CH], sh[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { sc[j] = s_rstd[cc * CH + j]; sh[j] = s_mean[cc * CH + j]; }
    for (int p = prow; p < HW; p += pstep) {
        float v[CH], r[CH];
        ld_chunk(xb + (size_t)p * C, v);
        if (rb) ld_chunk(rb + (size_t)p * C, r);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            float o = v[j] * sc[j] - sh[j];
            if (rb) o += r[j];
            if (relu) o = relu_f(o);
            v[j] = o;
        }
        st_chunk(xb + (size_t)p * C, v);
    }
}

static long gn_slab_limit() {
    static const long v = dev_env("HCM_GN_SLAB") ? atol(dev_env("HCM_GN_SLAB")) : 32768;
    return v;
}

// Large feature maps (HW >= 256 pixels per sample): two launches over (sample, pixel chunk) workgroups that read whole
// pixel rows -- every access is a full 128-byte-or-wider run, where the slab kernel above would touch 16 bytes of each
// line (the stem's 64 x 64 x 64 map: 143 us -> ~30 us).  Launch 1 writes per-(sample, chunk, group) sum / sum of squares;
// launch 2 adds the <= 16 partials of its sample in a fixed order (deterministic, no atomics), normalises its chunk, adds
// the residual, applies ReLU.  float32 storage (gn_pivot<T>, see gn_fused_kernel): the partial sums run over x - K, K = the (sample, group)'s
// first element, which the chunk-0 workgroup also leaves in pivot[b * G + g] for the apply pass (that pass stores over x).
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, float* __restrict__ pivot, int HW, int C, int G,
                                                        int P) {
    constexpr int CH = Tr<T>::CH;
    __shared__ float s_p1[4][512], s_p2[4][512];     // C <= 512 on this path
    const int b = blockIdx.y, pc = blockIdx.x;
    const int cpr = C / CH;                       // power of two, <= 64 (f16/bf16) or 128 (f32)
    const int tid = threadIdx.x;
    const int cc = tid % cpr, prow = tid / cpr, pstep = 256 / cpr;
    const int chunk = HW / P;
    const T* xb = x + ((size_t)b * HW + (size_t)pc * chunk) * C + cc * CH;
    const T* x0 = x + (size_t)b * HW * C;          // pixel 0 of the sample: the pivots
    const int Cg = C / G;
    float s1[CH], s2[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    float piv[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) piv[j] = 0.f;
    if constexpr (gn_pivot<T>) {
#pragma unroll
        for (int j = 0; j < CH; ++j) piv[j] = Tr<T>::ld(x0 + ((cc * CH + j) / Cg) * Cg);
    }
    for (int p = prow; p < chunk; p += pstep) {
        float v[CH];
        ld_chunk(xb + (size_t)p * C, v);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            if constexpr (gn_pivot<T>) v[j] -= piv[j];
            s1[j] += v[j]; s2[j] += v[j] * v[j];
        }
    }
    for (int o = 32; o >= cpr; o >>= 1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) { s1[j] += __shfl_xor(s1[j], o, 64); s2[j] += __shfl_xor(s2[j], o, 64); }
    }
    const int wv = tid >> 6;
    for (int i = tid; i < 4 * C; i += 256) { s_p1[i / C][i % C] = 0.f; s_p2[i / C][i % C] = 0.f; }
    __syncthreads();
    // cpr <= 64: after the butterfly lanes < cpr hold the wave's totals; cpr = 128 (f32): a wave covers half a pixel row and
    // every lane owns distinct channels (the other half-row waves leave zeros in this wave's slots)
    if ((tid & 63) < cpr || cpr > 64) {
#pragma unroll
        for (int j = 0; j < CH; ++j) { s_p1[wv][cc * CH + j] = s1[j]; s_p2[wv][cc * CH + j] = s2[j]; }
    }
    __syncthreads();
    for (int g = tid; g < G; g += 256) {
        float a = 0.f, q = 0.f;
        for (int j = 0; j < Cg; ++j) {
            const int ch = g * Cg + j;
            a += (s_p1[0][ch] + s_p1[1][ch]) + (s_p1[2][ch] + s_p1[3][ch]);
            q += (s_p2[0][ch] + s_p2[1][ch]) + (s_p2[2][ch] + s_p2[3][ch]);
        }
        float* o = part + (((size_t)b * P + pc) * G + g) * 2;
        o[0] = a; o[1] = q;
        if constexpr (gn_pivot<T>) { if (pc == 0) pivot[(size_t)b * G + g] = Tr<T>::ld(x0 + g * Cg); }
    }
}

// PIV: the partial sums are gn_stats_kernel's shifted ones and pivot[b * G + g] holds the shift; epilogue-fed calls (plain sums) run PIV = false.
template <typename T, bool PIV>
__global__ __launch_bounds__(256) void gn_apply_kernel(T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ part,
                                                        const float* __restrict__ pivot, int HW, int C, int G, int P, float eps, int relu, int PS) {
    constexpr int CH = Tr<T>::CH;
    __shared__ float s_scale[512], s_shift[512];
    __shared__ float s_mean[256], s_rstd[256];
    const int b = blockIdx.y, pc = blockIdx.x;
    const int tid = threadIdx.x;
    const int Cg = C / G;
    // PS partial sums per (sample, group): P of them from gn_stats_kernel, or HW / 64 from the producing conv's epilogue
    for (int g = tid; g < G; g += 256) {
        float a = 0.f, q = 0.f;
        {   // index order, requested 16 at a time (see maxpool_gn_kernel)
            const float2* pp = reinterpret_cast<const float2*>(part) + (size_t)b * PS * G + g;
            int i = 0;
            for (; i + 16 <= PS; i += 16) {
                float2 t[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = pp[(size_t)(i + u) * G];
#pragma unroll
                for (int u = 0; u < 16; ++u) { a += t[u].x; q += t[u].y; }
            }
            for (; i < PS; ++i) { const float2 t = pp[(size_t)i * G]; a += t.x; q += t.y; }
        }
        const float inv_n = 1.0f / ((float)HW * (float)Cg);
        float mean = a * inv_n;
        const float var = relu_f(q * inv_n - mean * mean);
        if constexpr (PIV) mean += pivot[(size_t)b * G + g];
        s_mean[g] = mean;
        s_rstd[g] = rsqrtf(var + eps);
    }
    __syncthreads();
    for (int ch = tid; ch < C; ch += 256) {
        const int g = ch / Cg;
        const float sc = s_rstd[g] * gamma[ch];
        s_scale[ch] = sc;
        s_shift[ch] = s_mean[g] * sc - beta[ch];
    }
    __syncthreads();
    const int cpr = C / CH;
    const int cc = tid % cpr, prow = tid / cpr, pstep = 256 / cpr;
    const int chunk = HW / P;
    const size_t base = ((size_t)b * HW + (size_t)pc * chunk) * C + cc * CH;
    float sc[CH], sh[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { sc[j] = s_scale[cc * CH + j]; sh[j] = s_shift[cc * CH + j]; }
    for (int p = prow; p < chunk; p += pstep) {
        float v[CH], r[CH];
        ld_chunk(x + base + (size_t)p * C, v);
        if (res) ld_chunk(res + base + (size_t)p * C, r);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            float o = v[j] * sc[j] - sh[j];
            if (res) o += r[j];
            if (relu) o = relu_f(o);
            v[j] = o;
        }
        st_chunk(x + base + (size_t)p * C, v);
    }
}

// Fallback for shapes the slab kernel's layout does not cover (a group wider than 1024 channels: the 1 x 1 x 2048 compression map of
// 64-pixel depth frames): one workgroup per (sample, group), two passes over its HW x Cg elements, fixed summation order.
template <typename T>
__global__ __launch_bounds__(256) void gn_generic_kernel(T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int HW, int C, int G, float eps, int relu, int cg_true) {
    __shared__ float s_a[256], s_q[256];
    const int Cg = C / G, b = blockIdx.x / G, g = blockIdx.x - b * G, tid = threadIdx.x;
    T* xb = x + (size_t)b * HW * C + (size_t)g * Cg;
    const T* rb = res ? res + (size_t)b * HW * C + (size_t)g * Cg : nullptr;
    const int n = HW * Cg;
    float a = 0.f, q = 0.f;
    float K = 0.f;                                   // float32: the group's first element (see gn_fused_kernel); stores start behind the barriers below
    if constexpr (gn_pivot<T>) { if (!cg_true) K = Tr<T>::ld(xb); }
    for (int e = tid; e < n; e += 256) {
        const int p = e / Cg, c = e - p * Cg;
        float v = Tr<T>::ld(xb + (size_t)p * C + c);
        if constexpr (gn_pivot<T>) v -= K;
        a += v; q += v * v;
    }
    s_a[tid] = a; s_q[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_a[tid] += s_a[tid + o]; s_q[tid] += s_q[tid + o]; }
        __syncthreads();
    }
    const float inv_n = 1.0f / ((float)HW * (float)(cg_true > 0 ? cg_true : Cg));
    float mean = s_a[0] * inv_n;
    const float rstd = rsqrtf(relu_f(s_q[0] * inv_n - mean * mean) + eps);
    if constexpr (gn_pivot<T>) mean += K;
    for (int e = tid; e < n; e += 256) {
        const int p = e / Cg, c = e - p * Cg;
        const size_t off = (size_t)p * C + c;
        float o = (Tr<T>::ld(xb + off) - mean) * rstd * gamma[g * Cg + c] + beta[g * Cg + c];
        if (rb) o += Tr<T>::ld(rb + off);
        if (relu) o = relu_f(o);
        Tr<T>::st(xb + off, o);
    }
}

hipError_t launch_groupnorm(void* x, const void* res, const float* gamma, const float* beta, float* stats, int dt, int B,
                            int HW, int C, int G, float eps, int relu, hipStream_t s, int cg_true) {
    const int CH = dt_chunk(dt);
    if (C % CH || C % G) return hipErrorInvalidValue;
    const int Cg = C / G;
    if (cg_true < 0 || cg_true > Cg) return hipErrorInvalidValue;
    static const int two_pass = dev_env("HCM_GN_TWO") ? atoi(dev_env("HCM_GN_TWO")) : 1;
    const int P = gn_partials(HW);
    const int cprw = C / CH;
    if (two_pass && !cg_true && stats && P > 0 && !(cprw & (cprw - 1)) && cprw <= 128 && C <= 512 && G <= 256 && HW % P == 0 &&
        (HW >= 1024 || C <= 256)) {             // 16 x 16 maps with 512 channels: the slab kernel is faster (13 vs 21 us)
        HCM_DISPATCH_T(dt, {
            float* pivot = stats + gn_pivot_offset(B, HW, G);
            hipLaunchKernelGGL(gn_stats_kernel<T>, dim3(P, B), dim3(256), 0, s, (const T*)x, stats, pivot, HW, C, G, P);
            hipLaunchKernelGGL((gn_apply_kernel<T, gn_pivot<T>>), dim3(P, B), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, stats, (const float*)pivot, HW,
                               C, G, P, eps, relu, P);
        });
        return hipGetLastError();
    }
    // slab: whole groups, multiple of the chunk, power-of-two chunk count <= 32, about 32 K elements per workgroup
    int unit = Cg > CH ? Cg : CH;
    if (unit % Cg || unit % CH) {
        HCM_DISPATCH_T(dt, hipLaunchKernelGGL(gn_generic_kernel<T>, dim3(B * G), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, HW, C, G, eps, relu, cg_true));
        return hipGetLastError();
    }
    int CS = unit;
    while (CS * 2 <= C && CS * 2 <= 256 && (CS * 2) / CH <= 32 && (long)HW * CS * 2 <= gn_slab_limit() && C % (CS * 2) == 0) CS *= 2;
    const int cpr = CS / CH;
    if (cpr & (cpr - 1) || cpr > 256 || CS > 1024 || C % CS) {
        HCM_DISPATCH_T(dt, hipLaunchKernelGGL(gn_generic_kernel<T>, dim3(B * G), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, HW, C, G, eps, relu, cg_true));
        return hipGetLastError();
    }
    const int grid = B * (C / CS);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(gn_fused_kernel<T>, dim3(grid), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, HW, C, G, CS, eps, relu, cg_true));
    return hipGetLastError();
}

bool groupnorm_apply_ok(int dt, int HW, int C, int G) {
    const int CH = dt_chunk(dt);
    if (dt == DT_F32 || C % CH || C % G) return false;
    const int P = gn_partials(HW), cprw = C / CH;
    // (no `HW >= 1024 || C <= 256` clause as in launch_groupnorm: without the statistics launch the apply pass alone beats the slab kernel
    // on the 16 x 16 x 512 maps too)
    return P > 0 && !(cprw & (cprw - 1)) && cprw <= 128 && C <= 512 && G <= 256 && HW % P == 0 && HW % 64 == 0 && 32 % (C / G) == 0;
}
hipError_t launch_groupnorm_apply(void* x, const void* res, const float* gamma, const float* beta, const float* part, int PS, int dt, int B,
                                  int HW, int C, int G, float eps, int relu, hipStream_t s) {
    if (!groupnorm_apply_ok(dt, HW, C, G) || PS < 1) return hipErrorInvalidValue;
    const int P = gn_partials(HW);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL((gn_apply_kernel<T, false>), dim3(P, B), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, part,
                                          (const float*)nullptr, HW, C, G, P, eps, relu, PS));
    return hipGetLastError();
}

// gn_apply_kernel with an UN-normalised residual (round 5): x = relu?(GN(x) + round_T(GN2(res))) where res is the raw output of the block's down-sample
// conv and part2 / gamma2 / beta2 its GroupNorm -- the stage-first bottlenecks of the GroupNorm trunk (habitat's ResNet: `out = relu(bn3(conv3) +
// downsample(x))`, resnet_encoders.py:27-33).  The down-sample branch's own apply pass (a read and a write of its map, one launch) disappears; its
// normalised value is rounded to the storage type exactly as that pass stored it before it is added: BIT-IDENTICAL to the two apply passes.
template <typename T>
__global__ __launch_bounds__(256) void gn_apply2_kernel(T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ part, const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                         const float* __restrict__ part2, int HW, int C, int G, int P, float eps, float eps2, int relu, int PS) {
    constexpr int CH = Tr<T>::CH;
    __shared__ float s_scale[2][512], s_shift[2][512];
    __shared__ float s_mean[2][256], s_rstd[2][256];
    const int b = blockIdx.y, pc = blockIdx.x;
    const int tid = threadIdx.x;
    const int Cg = C / G;
    for (int g2 = tid; g2 < 2 * G; g2 += 256) {
        const int which = g2 >= G, g = which ? g2 - G : g2;
        const float* pp = which ? part2 : part;
        float a = 0.f, q = 0.f;
        {   // index order, requested 16 at a time (see maxpool_gn_kernel)
            const float2* p2 = reinterpret_cast<const float2*>(pp) + (size_t)b * PS * G + g;
            int i = 0;
            for (; i + 16 <= PS; i += 16) {
                float2 t[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = p2[(size_t)(i + u) * G];
#pragma unroll
                for (int u = 0; u < 16; ++u) { a += t[u].x; q += t[u].y; }
            }
            for (; i < PS; ++i) { const float2 t = p2[(size_t)i * G]; a += t.x; q += t.y; }
        }
        const float inv_n = 1.0f / ((float)HW * (float)Cg);
        const float mean = a * inv_n;
        const float var = relu_f(q * inv_n - mean * mean);
        s_mean[which][g] = mean;
        s_rstd[which][g] = rsqrtf(var + (which ? eps2 : eps));
    }
    __syncthreads();
    for (int c2 = tid; c2 < 2 * C; c2 += 256) {
        const int which = c2 >= C, ch = which ? c2 - C : c2;
        const int g = ch / Cg;
        const float sc = s_rstd[which][g] * (which ? gamma2 : gamma)[ch];
        s_scale[which][ch] = sc;
        s_shift[which][ch] = s_mean[which][g] * sc - (which ? beta2 : beta)[ch];
    }
    __syncthreads();
    const int cpr = C / CH;
    const int cc = tid % cpr, prow = tid / cpr, pstep = 256 / cpr;
    const int chunk = HW / P;
    const size_t base = ((size_t)b * HW + (size_t)pc * chunk) * C + cc * CH;
    float sc[CH], sh[CH], sc2[CH], sh2[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) { sc[j] = s_scale[0][cc * CH + j]; sh[j] = s_shift[0][cc * CH + j]; sc2[j] = s_scale[1][cc * CH + j]; sh2[j] = s_shift[1][cc * CH + j]; }
    for (int p = prow; p < chunk; p += pstep) {
        float v[CH], r[CH];
        ld_chunk(x + base + (size_t)p * C, v);
        ld_chunk(res + base + (size_t)p * C, r);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            T rt;
            Tr<T>::st(&rt, r[j] * sc2[j] - sh2[j]);          // what the down-sample branch's apply pass stored (no ReLU on that branch)
            float o = v[j] * sc[j] - sh[j];
            o += Tr<T>::ld(&rt);
            if (relu) o = relu_f(o);
            v[j] = o;
        }
        st_chunk(x + base + (size_t)p * C, v);
    }
}
hipError_t launch_groupnorm_apply2(void* x, const void* res, const float* gamma, const float* beta, const float* part, const float* gamma2, const float* beta2,
                                   const float* part2, int PS, int dt, int B, int HW, int C, int G, float eps, float eps2, int relu, hipStream_t s) {
    if (!groupnorm_apply_ok(dt, HW, C, G) || PS < 1 || !res || !part2) return hipErrorInvalidValue;
    const int P = gn_partials(HW);
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(gn_apply2_kernel<T>, dim3(P, B), dim3(256), 0, s, (T*)x, (const T*)res, gamma, beta, part, gamma2, beta2, part2, HW, C, G, P,
                                          eps, eps2, relu, PS));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ LayerNorm (one wave per row)
// nn.LayerNorm / BertLayerNorm: biased variance, eps inside the sqrt; two-pass in registers.
template <typename T, int D>
__global__ void layernorm_kernel(const T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, const float* __restrict__ post, int post_rows,
                                 T* __restrict__ y, int rows, float eps) {
    constexpr int PER = D / 64;              // elements per lane, strided by 64 lanes in groups of VEC
    constexpr int VEC = (PER % 4 == 0) ? 4 : 1;
    constexpr int NV = PER / VEC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (size_t)row * D;
    const T* rr = res ? res + (size_t)row * D : nullptr;
    float v[PER];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = (i * 64 + lane) * VEC + j;
            float a = Tr<T>::ld(xr + c);
            if (rr) a += Tr<T>::ld(rr + c);
            v[i * VEC + j] = a;
            sum += a;
        }
    const float mean = wave_sum(sum) * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; sq += d * d; }
    const float rstd = rsqrtf(wave_sum(sq) * (1.0f / D) + eps);
    const float* pp = post ? post + (size_t)(row % post_rows) * D : nullptr;
    T* yr = y + (size_t)row * D;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = (i * 64 + lane) * VEC + j;
            float o = (v[i * VEC + j] - mean) * rstd * gamma[c] + beta[c];
            if (pp) o += pp[c];
            Tr<T>::st(yr + c, o);
        }
}

// Vectorised variant: 32 lanes per row, 16-byte chunks (D/CH chunks per row, D/CH/32 per lane), two rows per wave.
template <typename T, int D, bool HAS_RES, bool HAS_POST>
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const T* __restrict__ x, const T* __restrict__ res, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ post, int post_rows,
                                                             T* __restrict__ y, int rows, float eps) {
    constexpr int CH = Tr<T>::CH;
    constexpr int CPL = D / CH / 32;         // chunks per lane
    static_assert(CPL >= 1 && D % (CH * 32) == 0, "row must split into 32 x 16-byte chunks");
    const int sub = threadIdx.x & 31;
    const int row = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (row >= rows) return;
    const T* xr = x + (size_t)row * D;
    const T* rr = res ? res + (size_t)row * D : nullptr;
    float v[CPL][CH];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = (i * 32 + sub) * CH;
        ld_chunk(xr + c, v[i]);
        if constexpr (HAS_RES) {
            float r[CH];
            ld_chunk(rr + c, r);
#pragma unroll
            for (int j = 0; j < CH; ++j) v[i][j] += r[j];
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) sum += v[i][j];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < CH; ++j) { const float d = v[i][j] - mean; sq += d * d; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    const float rstd = rsqrtf(sq * (1.0f / D) + eps);
    const float* pp = post ? post + (size_t)(row % post_rows) * D : nullptr;
    T* yr = y + (size_t)row * D;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = (i * 32 + sub) * CH;
        float o[CH], gm[CH], bt[CH];
        // gamma / beta / post as 16-byte vector loads (c is a multiple of CH), no per-element branches
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const float4 g4 = *reinterpret_cast<const float4*>(gamma + c + 4 * q);
            const float4 b4 = *reinterpret_cast<const float4*>(beta + c + 4 * q);
            gm[4 * q] = g4.x; gm[4 * q + 1] = g4.y; gm[4 * q + 2] = g4.z; gm[4 * q + 3] = g4.w;
            bt[4 * q] = b4.x; bt[4 * q + 1] = b4.y; bt[4 * q + 2] = b4.z; bt[4 * q + 3] = b4.w;
            if constexpr (HAS_POST) {
                const float4 p4 = *reinterpret_cast<const float4*>(pp + c + 4 * q);
                bt[4 * q] += p4.x; bt[4 * q + 1] += p4.y; bt[4 * q + 2] += p4.z; bt[4 * q + 3] += p4.w;
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) o[j] = (v[i][j] - mean) * rstd * gm[j] + bt[j];
        st_chunk(yr + c, o);
    }
}

hipError_t launch_layernorm(const void* x, const void* res, const float* gamma, const float* beta, const float* post,
                            int post_rows, void* y, int dt, int rows, int D, float eps, hipStream_t s) {
    const int pr = post_rows > 0 ? post_rows : 1;
    if (D == 768 || D == 256 || D == 512) {
        constexpr int rpb = 8;                   // rows per workgroup (32 lanes each); 2..8 measured equal: 4.2 us, launch floor
        const dim3 grid((rows + rpb - 1) / rpb), block(32 * rpb);
#define LV2(DD, R_, P_) hipLaunchKernelGGL((layernorm_vec_kernel<T, DD, R_, P_>), grid, block, 0, s, (const T*)x, (const T*)res, gamma, beta, post, pr, (T*)y, rows, eps)
#define LV(DD) do { if (res) { if (post) LV2(DD, true, true); else LV2(DD, true, false); } else { if (post) LV2(DD, false, true); else LV2(DD, false, false); } } while (0)
        HCM_DISPATCH_T(dt, { if (D == 768) LV(768); else if (D == 256) LV(256); else LV(512); });
#undef LV
#undef LV2
        return hipGetLastError();
    }
    const int wpb = 4;
    const dim3 grid((rows + wpb - 1) / wpb), block(64 * wpb);
#define L(DD) hipLaunchKernelGGL((layernorm_kernel<T, DD>), grid, block, 0, s, (const T*)x, (const T*)res, gamma, beta, post, pr, (T*)y, rows, eps)
    HCM_DISPATCH_T(dt, { if (D == 128) L(128); else return hipErrorInvalidValue; });
#undef L
    return hipGetLastError();
}

// Rows whose mean lies far from zero (|mean| > 4 standard deviations): a mean of that size held in ONE float32 is off by up to half a float32 ulp of it
// however it is summed, that error enters every x - mean, and an output near zero then misses its 16-bit value by many storage ulps (74 in fp16 at
// 100 standard deviations).  The corrected two-pass form: corr = mean of the residuals x - mean (the part of the mean the float32 lost), the outputs
// use (x - mean) - corr and the variance is retaken over them.  For every other row corr = 0 and rstd is the plain one, so (x - mean) - 0 keeps the
// bits the kernels had without this step (the "bf16" mode's streams have |mean| well below one standard deviation).  The row's 32 lanes take the
// same side: mean and sq are the reduced values.
template <int CPL, int D>
__device__ __forceinline__ void ln_f32in_offset_fix(const float (&v)[CPL][4], float mean, float sq, float eps, float& corr, float& rstd) {
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) rs += v[i][j] - mean;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
    const float c = rs * (1.0f / D);
    float sq2 = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = (v[i][j] - mean) - c; sq2 += d * d; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sq2 += __shfl_xor(sq2, o, 64);
    const bool far = mean * mean > 16.0f * (sq * (1.0f / D));
    corr = far ? c : 0.f;
    rstd = far ? rsqrtf(sq2 * (1.0f / D) + eps) : rsqrtf(sq * (1.0f / D) + eps);
}

// LayerNorm of an f32 row with two outputs (the bf16 BERT keeps its residual stream in f32: forward.cpp bert()): y16 = the next GEMM's
// 16-bit operand, y32 = the stream itself.  32 lanes per row, float4 chunks.
template <typename T, int D>
__global__ __launch_bounds__(256) void layernorm_f32in_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               T* __restrict__ y16, float* __restrict__ y32, int rows, float eps) {
    constexpr int CPL = D / 4 / 32;
    static_assert(CPL >= 1 && D % 128 == 0, "row must split into 32 x 16-byte chunks");
    const int sub = threadIdx.x & 31;
    const int row = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float v[CPL][4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        ld_chunk(xr + (i * 32 + sub) * 4, v[i]);
        sum += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; sq += d * d; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    float corr, rstd;
    ln_f32in_offset_fix<CPL, D>(v, mean, sq, eps, corr, rstd);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = (i * 32 + sub) * 4;
        const float4 g4 = *reinterpret_cast<const float4*>(gamma + c), b4 = *reinterpret_cast<const float4*>(beta + c);
        float o[4] = {((v[i][0] - mean) - corr) * rstd * g4.x + b4.x, ((v[i][1] - mean) - corr) * rstd * g4.y + b4.y,
                      ((v[i][2] - mean) - corr) * rstd * g4.z + b4.z, ((v[i][3] - mean) - corr) * rstd * g4.w + b4.w};
        st_chunk(y32 + (size_t)row * D + c, o);
        T o4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) Tr<T>::st(&o4[j], o[j]);
        *reinterpret_cast<uint2*>(y16 + (size_t)row * D + c) = *reinterpret_cast<const uint2*>(o4);
    }
}
// ... and its round-5 sibling for the implicit stream: the 16-bit operand + (mean, rstd) per row, NO f32 output (forward.cpp bert(): the next projection's
// epilogue rebuilds the stream value from the sum and these statistics).  A kernel of its own: layernorm_f32in_kernel's instruction stream is what the
// goldens of the "bf16" mode and the fused-block experiment are pinned to, and adding two conditional stores to it changed its floating-point
// contraction (1.6e-5 on the record).
template <typename T, int D>
__global__ __launch_bounds__(256) void layernorm_f32in_stats_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     T* __restrict__ y16, float* __restrict__ stats, int rows, float eps) {
    constexpr int CPL = D / 4 / 32;
    const int sub = threadIdx.x & 31;
    const int row = blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float v[CPL][4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        ld_chunk(xr + (i * 32 + sub) * 4, v[i]);
        sum += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum * (1.0f / D);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; sq += d * d; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    float corr, rstd;
    ln_f32in_offset_fix<CPL, D>(v, mean, sq, eps, corr, rstd);
    if (sub == 0) *reinterpret_cast<float2*>(stats + 2 * (size_t)row) = make_float2(corr != 0.f ? mean + corr : mean, rstd);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = (i * 32 + sub) * 4;
        const float4 g4 = *reinterpret_cast<const float4*>(gamma + c), b4 = *reinterpret_cast<const float4*>(beta + c);
        T o4[4];
        Tr<T>::st(&o4[0], ((v[i][0] - mean) - corr) * rstd * g4.x + b4.x); Tr<T>::st(&o4[1], ((v[i][1] - mean) - corr) * rstd * g4.y + b4.y);
        Tr<T>::st(&o4[2], ((v[i][2] - mean) - corr) * rstd * g4.z + b4.z); Tr<T>::st(&o4[3], ((v[i][3] - mean) - corr) * rstd * g4.w + b4.w);
        *reinterpret_cast<uint2*>(y16 + (size_t)row * D + c) = *reinterpret_cast<const uint2*>(o4);
    }
}
hipError_t launch_layernorm_f32in(const float* x, const float* gamma, const float* beta, void* y16, float* y32, int dt, int rows, int D, float eps,
                                  hipStream_t s, float* stats) {
    if (dt != DT_BF16 && dt != DT_F16) return hipErrorInvalidValue;
    if (!stats && !y32) return hipErrorInvalidValue;      // the plain form stores its f32 output unconditionally
    if (stats) {                                   // the statistics form: no f32 output
        if (y32) return hipErrorInvalidValue;
        constexpr int rpb2 = 8;
        const dim3 grid2((rows + rpb2 - 1) / rpb2), block2(32 * rpb2);
#define LS(T, DD) hipLaunchKernelGGL((layernorm_f32in_stats_kernel<T, DD>), grid2, block2, 0, s, x, gamma, beta, (T*)y16, stats, rows, eps)
        if (D == 768) { if (dt == DT_BF16) LS(bf16, 768); else LS(f16, 768); }
        else if (D == 256) { if (dt == DT_BF16) LS(bf16, 256); else LS(f16, 256); }
        else if (D == 512) { if (dt == DT_BF16) LS(bf16, 512); else LS(f16, 512); }
        else return hipErrorInvalidValue;
#undef LS
        return hipGetLastError();
    }
    constexpr int rpb = 8;
    const dim3 grid((rows + rpb - 1) / rpb), block(32 * rpb);
#define LF(T, DD) hipLaunchKernelGGL((layernorm_f32in_kernel<T, DD>), grid, block, 0, s, x, gamma, beta, (T*)y16, y32, rows, eps)
    if (D == 768) { if (dt == DT_BF16) LF(bf16, 768); else LF(f16, 768); }
    else if (D == 256) { if (dt == DT_BF16) LF(bf16, 256); else LF(f16, 256); }
    else if (D == 512) { if (dt == DT_BF16) LF(bf16, 512); else LF(f16, 512); }
    else return hipErrorInvalidValue;
#undef LF
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ BERT embeddings + LN
// BertEmbeddings.forward: word[id] + position[l] + token_type[0] -> LayerNorm(eps 1e-12)  (call site seq2seq_highlevel_cma.py:192-195)
template <typename T, typename I>
__global__ void bert_embed_kernel(const I* __restrict__ ids, const float* __restrict__ word, const float* __restrict__ pos,
                                  const float* __restrict__ type0, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  T* __restrict__ y, int rows, int L, int D, int vocab, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    long id = (long)ids[row];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    const int l = row % L;
    const float* wr = word + (size_t)id * D;
    const float* pr = pos + (size_t)l * D;
    float v[16];                              // D <= 1024
    const int per = D / 64;
    float sum = 0.f;
    for (int i = 0; i < per; ++i) {
        const int c = i * 64 + lane;
        const float a = wr[c] + pr[c] + type0[c];
        v[i] = a;
        sum += a;
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
    for (int i = 0; i < per; ++i) { const float d = v[i] - mean; sq += d * d; }
    const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
    for (int i = 0; i < per; ++i) {
        const int c = i * 64 + lane;
        Tr<T>::st(y + (size_t)row * D + c, (v[i] - mean) * rstd * gamma[c] + beta[c]);
    }
}

hipError_t launch_bert_embed(const void* ids, int ids_dt, const float* word, const float* pos, const float* type0,
                             const float* gamma, const float* beta, void* y, int dt, int B, int L, int D, int vocab,
                             float eps, hipStream_t s) {
    const int rows = B * L;
    if (D % 64 || D > 1024) return hipErrorInvalidValue;
    const dim3 grid((rows + 3) / 4), block(256);
#define L_(I) hipLaunchKernelGGL((bert_embed_kernel<T, I>), grid, block, 0, s, (const I*)ids, word, pos, type0, gamma, beta, (T*)y, rows, L, D, vocab, eps)
    HCM_DISPATCH_T(dt, {
        if (ids_dt == DT_I64) L_(int64_t); else if (ids_dt == DT_I32) L_(int32_t); else if (ids_dt == DT_F32) L_(float); else return hipErrorInvalidValue;
    });
#undef L_
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ recurrent cell + heads
// RNNStateEncoder.single_forward (models/decoder/state_encoder.py:72-81): hidden * mask, one step, repack.
__global__ void rnn_prep_kernel(const float* __restrict__ h_in, const float* __restrict__ mask, float* __restrict__ xh,
                                int B, int Hd, int ld, int col0) {
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) xh[(size_t)b * ld + col0 + j] = h_in[(size_t)b * Hd + j] * mask[b];
}
hipError_t launch_rnn_prep(const float* h_in, const float* mask, float* xh, int B, int Hd, int ld, int col0, hipStream_t s) {
    hipLaunchKernelGGL(rnn_prep_kernel, dim3(B), dim3(256), 0, s, h_in, mask, xh, B, Hd, ld, col0);
    return hipGetLastError();
}

__device__ __forceinline__ void heads_eval(const float* hs, int Hd, const Heads& hd, int b) {
    // hs: new hidden state of sample b in LDS; one wave per output row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __shared__ float lg[64];
    __shared__ int best_s;
    for (int r = wave; r < hd.r0 + hd.r1 + hd.r2; r += nw) {
        const bool first = r < hd.r0, third = r >= hd.r0 + hd.r1;
        const int rr = first ? r : third ? r - hd.r0 - hd.r1 : r - hd.r0;
        const float* w = (first ? hd.w0 : third ? hd.w2 : hd.w1) + (size_t)rr * Hd;
        float acc = 0.f;
        for (int j = lane; j < Hd; j += 64) acc += w[j] * hs[j];
        acc = wave_sum(acc);
        if (lane == 0) {
            if (first) { const float v = acc + hd.b0[rr]; hd.out0[(size_t)b * hd.ld0 + rr] = v; if (rr < 64) lg[rr] = v; }
            else if (third) hd.out2[(size_t)b * hd.ld2 + rr] = tanhf(acc + hd.b2[rr]);      // tanh(progress_monitor(x)), seq2seq.py:177
            else hd.out1[(size_t)b * hd.ld1 + rr] = acc + hd.b1[rr];
        }
    }
    if (hd.pred) {                        // (kernel-uniform) argmax of the first head + embedding row of the winner
        __syncthreads();
        if (threadIdx.x == 0) {
            int best = 0;
            float bv = lg[0];
            for (int j = 1; j < hd.r0; ++j)                     // torch.argmax: a NaN counts as the maximum, the first one wins (as val_loss_kernel)
                if (lg[j] > bv || (lg[j] != lg[j] && bv == bv)) { bv = lg[j]; best = j; }
            hd.pred[b] = best;
            best_s = best < hd.emb_rows ? best : hd.emb_rows - 1;
        }
        __syncthreads();
        const float* e = hd.emb + (size_t)best_s * hd.emb_dim;
        for (int j = threadIdx.x; j < hd.emb_dim; j += blockDim.x) hd.emb_out[(size_t)b * hd.emb_ld + j] = e[j];
    }
}

// heads_eval keeps the first head's logits of the fused argmax in lg[64] and reads lg[0 .. r0): a fused `pred` needs 1 <= r0 <= 64 and a table to clamp into
static bool heads_pred_ok(const Heads& hd) {
    return !hd.pred || (hd.r0 >= 1 && hd.r0 <= 64 && hd.out0 && hd.emb && hd.emb_out && hd.emb_rows >= 1 && hd.emb_dim >= 0);
}

__global__ void lstm_cell_kernel(const float* __restrict__ gates, const float* __restrict__ h_in, const float* __restrict__ mask,
                                 float* __restrict__ h_out, int B, int Hd, Heads hd) {
    extern __shared__ float hs[];
    const int b = blockIdx.x;
    const float mk = mask[b];
    const float* g = gates + (size_t)b * 4 * Hd;
    bool bad = false;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
        const float c = h_in[(size_t)(B + b) * Hd + j] * mk;          // hidden[1] = c
        bad |= !isfinite(g[j] + g[Hd + j] + g[2 * Hd + j] + g[3 * Hd + j]);       // (a finite sum has finite terms)
        const float gi = sigmoidf_(g[j]), gf = sigmoidf_(g[Hd + j]), gg = tanhf(g[2 * Hd + j]), go = sigmoidf_(g[3 * Hd + j]);
        const float c2 = gf * c + gi * gg;
        const float h2 = go * tanhf(c2);
        hs[j] = h2;
        h_out[(size_t)b * Hd + j] = h2;
        h_out[(size_t)(B + b) * Hd + j] = c2;
    }
    if (hd.bad && __syncthreads_or(bad) && threadIdx.x == 0) atomicAdd(hd.bad, 1u);
    __syncthreads();
    heads_eval(hs, Hd, hd, b);
}
hipError_t launch_lstm_cell(const float* gates, const float* h_in, const float* mask, float* h_out, int B, int Hd,
                            const Heads& heads, hipStream_t s) {
    if (!heads_pred_ok(heads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lstm_cell_kernel, dim3(B), dim3(256), Hd * sizeof(float), s, gates, h_in, mask, h_out, B, Hd, heads);
    return hipGetLastError();
}

__global__ void gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h_in,
                                const float* __restrict__ mask, float* __restrict__ h_out, int B, int Hd, Heads hd) {
    extern __shared__ float hs[];
    const int b = blockIdx.x;
    const float mk = mask[b];
    const float* a = gi + (size_t)b * 3 * Hd;
    const float* c = gh + (size_t)b * 3 * Hd;
    bool bad = false;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
        const float h = h_in[(size_t)b * Hd + j] * mk;
        bad |= !isfinite(a[j] + a[Hd + j] + a[2 * Hd + j]) || !isfinite(c[j] + c[Hd + j] + c[2 * Hd + j]);
        const float r = sigmoidf_(a[j] + c[j]);
        const float z = sigmoidf_(a[Hd + j] + c[Hd + j]);
        const float n = tanhf(a[2 * Hd + j] + r * c[2 * Hd + j]);
        const float h2 = (1.f - z) * n + z * h;
        hs[j] = h2;
        h_out[(size_t)b * Hd + j] = h2;
    }
    if (hd.bad && __syncthreads_or(bad) && threadIdx.x == 0) atomicAdd(hd.bad, 1u);
    __syncthreads();
    heads_eval(hs, Hd, hd, b);
}
hipError_t launch_gru_cell(const float* gi, const float* gh, const float* h_in, const float* mask, float* h_out, int B,
                           int Hd, const Heads& heads, hipStream_t s) {
    if (!heads_pred_ok(heads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gru_cell_kernel, dim3(B), dim3(256), Hd * sizeof(float), s, gi, gh, h_in, mask, h_out, B, Hd, heads);
    return hipGetLastError();
}

// linear / stop_linear over a whole (rows, Hd) sequence buffer: the sequence calls' heads behind a scan that keeps h_t of every row
__global__ void heads_rows_kernel(const float* __restrict__ h, int Hd, Heads hd) {
    extern __shared__ float hs[];
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) hs[j] = h[(size_t)b * Hd + j];
    __syncthreads();
    heads_eval(hs, Hd, hd, b);
}
hipError_t launch_heads_rows(const float* hs, int rows, int Hd, const Heads& heads, hipStream_t s) {
    if (rows < 1 || heads.pred) return hipErrorInvalidValue;
    hipLaunchKernelGGL(heads_rows_kernel, dim3(rows), dim3(256), Hd * sizeof(float), s, hs, Hd, heads);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ range check (fp16 calibration)
// slot[0] = max |x| as float bits (non-negative floats order like unsigned ints), slot[1] = count of non-finite elements
template <typename T>
__global__ void absmax_kernel(const T* __restrict__ x, int rows, int cols, int ld, unsigned* __restrict__ slot) {
    const size_t total = (size_t)rows * cols;
    float mx = 0.f;
    unsigned bad = 0;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const float v = Tr<T>::ld(x + (e / cols) * (size_t)ld + e % cols);
        if (!isfinite(v)) ++bad; else mx = fmaxf(mx, fabsf(v));          // (a 3.0e38 threshold counted float32's and bf16's largest finite values as overflows)
    }
    mx = wave_max(mx);
    bad += __shfl_xor(bad, 32, 64); bad += __shfl_xor(bad, 16, 64); bad += __shfl_xor(bad, 8, 64);
    bad += __shfl_xor(bad, 4, 64); bad += __shfl_xor(bad, 2, 64); bad += __shfl_xor(bad, 1, 64);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(slot, __float_as_uint(mx));
        if (bad) atomicAdd(slot + 1, bad);
    }
}
hipError_t launch_absmax(const void* x, int dt, int rows, int cols, int ld, unsigned* slot, hipStream_t s) {
    const size_t total = (size_t)rows * cols;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(absmax_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, rows, cols, ld, slot));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ split-K reduction
// y[m][n] = act(sum_s part[s][m][n] + bias[n]) in a fixed order (deterministic); part is f32 [S][M][N], y is T or f32 at ldy.
template <typename T>
__global__ void splitk_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias, void* __restrict__ y, int S, int M,
                                     int N, int ldy, int act, int out_f32) {
    const size_t total = (size_t)M * N;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(e % N);
        const size_t m = e / N;
        float a = bias ? bias[n] : 0.f;
        // the same left-to-right sum, eight independent requests at a time (as a plain loop the S loads were one latency chain: 25 us at 56 slices)
        int s_ = 0;
        for (; s_ + 8 <= S; s_ += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(s_ + j) * total + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) a += v[j];
        }
        for (; s_ < S; ++s_) a += part[(size_t)s_ * total + e];
        if (act == ACT_RELU) a = relu_f(a);
        else if (act == ACT_GELU) a = gelu_erf(a);
        if (out_f32) reinterpret_cast<float*>(y)[m * ldy + n] = a;
        else Tr<T>::st(reinterpret_cast<T*>(y) + m * ldy + n, a);
    }
}
hipError_t launch_splitk_reduce(const float* part, const float* bias, void* y, int dt, int S, int M, int N, int ldy, int act, int out_f32,
                                hipStream_t s) {
    const size_t total = (size_t)M * N;
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, part, bias, y, S, M, N, ldy, act, out_f32));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ CMANet instruction encoder
// InstructionEncoder.forward (models/encoders/instruction_encoder.py:70-92): lengths = #non-zero ids, embedding lookup.
// x[row][0..E) = table[id], zero-padded to ldx columns; one block per sample also counts its length.
template <typename I>
__global__ void instr_embed_kernel(const I* __restrict__ ids, const float* __restrict__ table, float* __restrict__ x,
                                   int* __restrict__ lengths, int L, int E, int ldx, int vocab) {
    const int b = blockIdx.x;
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int t = threadIdx.x; t < L; t += blockDim.x) mine += ((long)ids[(size_t)b * L + t] != 0) ? 1 : 0;
    if (mine) atomicAdd(&cnt, mine);
    for (int e = threadIdx.x; e < L * ldx; e += blockDim.x) {
        const int t = e / ldx, j = e - t * ldx;
        long id = (long)ids[(size_t)b * L + t];
        if (id < 0) id = 0;
        if (id >= vocab) id = vocab - 1;
        x[((size_t)b * L + t) * ldx + j] = j < E ? table[(size_t)id * E + j] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) lengths[b] = cnt;
}
hipError_t launch_instr_embed(const void* ids, int ids_dt, const float* table, float* x, int* lengths, int B, int L, int E, int ldx,
                              int vocab, hipStream_t s) {
    if (ids_dt == DT_I64) hipLaunchKernelGGL(instr_embed_kernel<int64_t>, dim3(B), dim3(256), 0, s, (const int64_t*)ids, table, x, lengths, L, E, ldx, vocab);
    else if (ids_dt == DT_I32) hipLaunchKernelGGL(instr_embed_kernel<int32_t>, dim3(B), dim3(256), 0, s, (const int32_t*)ids, table, x, lengths, L, E, ldx, vocab);
    else if (ids_dt == DT_F32) hipLaunchKernelGGL(instr_embed_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)ids, table, x, lengths, L, E, ldx, vocab);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// One time step of the PACKED LSTM (nn.LSTM over pack_padded_sequence): sample b is active at step t iff t < len_b; an
// inactive sample keeps (h, c) and emits zeros -- which makes the reverse direction start at the sample's own last
// token.  pre = x_t W_ih^T + b_ih + b_hh for every token [B*L][4H]; gh = h W_hh^T [B][4H]; gate order i,f,g,o.
__global__ void instr_lstm_cell_kernel(const float* __restrict__ pre, const float* __restrict__ gh, float* __restrict__ h,
                                       float* __restrict__ c, const int* __restrict__ lengths, float* __restrict__ out, int t, int L,
                                       int Hd, int ld_out, int col0) {
    const int b = blockIdx.x;
    const bool act = t < lengths[b];
    const float* p = pre + ((size_t)b * L + t) * 4 * Hd;
    const float* g = gh + (size_t)b * 4 * Hd;
    float* o = out + ((size_t)b * L + t) * ld_out + col0;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
        if (!act) { o[j] = 0.f; continue; }
        const float gi = sigmoidf_(p[j] + g[j]), gf = sigmoidf_(p[Hd + j] + g[Hd + j]);
        const float gg = tanhf(p[2 * Hd + j] + g[2 * Hd + j]), go = sigmoidf_(p[3 * Hd + j] + g[3 * Hd + j]);
        const float c2 = gf * c[(size_t)b * Hd + j] + gi * gg;
        const float h2 = go * tanhf(c2);
        c[(size_t)b * Hd + j] = c2;
        h[(size_t)b * Hd + j] = h2;
        o[j] = h2;
    }
}
// The same step for nn.GRU (INSTRUCTION_ENCODER.rnn_type = "GRU", instruction_encoder.py:42): pre = x_t W_ih^T + b_ih [B*L][3H], gh = h W_hh^T + b_hh
// [B][3H], gate order r, z, n; n = tanh(pre_n + r * gh_n), h' = (1 - z) n + z h.
__global__ void instr_gru_cell_kernel(const float* __restrict__ pre, const float* __restrict__ gh, float* __restrict__ h,
                                      const int* __restrict__ lengths, float* __restrict__ out, int t, int L, int Hd, int ld_out, int col0) {
    const int b = blockIdx.x;
    const bool act = t < lengths[b];
    const float* p = pre + ((size_t)b * L + t) * 3 * Hd;
    const float* g = gh + (size_t)b * 3 * Hd;
    float* o = out + ((size_t)b * L + t) * ld_out + col0;
    for (int j = threadIdx.x; j < Hd; j += blockDim.x) {
        if (!act) { o[j] = 0.f; continue; }
        const float r = sigmoidf_(p[j] + g[j]), z = sigmoidf_(p[Hd + j] + g[Hd + j]);
        const float n = tanhf(p[2 * Hd + j] + r * g[2 * Hd + j]);
        const float h2 = (1.0f - z) * n + z * h[(size_t)b * Hd + j];
        h[(size_t)b * Hd + j] = h2;
        o[j] = h2;
    }
}
hipError_t launch_instr_gru_cell(const float* pre, const float* gh, float* h, const int* lengths, float* out, int t, int B, int L, int Hd, int ld_out,
                                 int col0, hipStream_t s) {
    hipLaunchKernelGGL(instr_gru_cell_kernel, dim3(B), dim3(256), 0, s, pre, gh, h, lengths, out, t, L, Hd, ld_out, col0);
    return hipGetLastError();
}
hipError_t launch_instr_lstm_cell(const float* pre, const float* gh, float* h, float* c, const int* lengths, float* out, int t, int B,
                                  int L, int Hd, int ld_out, int col0, hipStream_t s) {
    hipLaunchKernelGGL(instr_lstm_cell_kernel, dim3(B), dim3(256), 0, s, pre, gh, h, c, lengths, out, t, L, Hd, ld_out, col0);
    return hipGetLastError();
}

__global__ void copy_rows_kernel(const float* __restrict__ src, int ld_src, int n_src, float* __restrict__ dst, int ld_dst, int cols) {
    const int r = blockIdx.x;
    const float* sp = src + (size_t)(n_src == 1 ? 0 : r) * ld_src;
    for (int j = threadIdx.x; j < cols; j += blockDim.x) dst[(size_t)r * ld_dst + j] = sp[j];
}
hipError_t launch_copy_rows(const float* src, int ld_src, int n_src, float* dst, int ld_dst, int rows, int cols, hipStream_t s) {
    if (rows < 1 || (n_src != 1 && n_src < rows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_rows_kernel, dim3(rows), dim3(256), 0, s, src, ld_src, n_src, dst, ld_dst, cols);
    return hipGetLastError();
}

// CMANet._attn (models/cma.py:201-209): ONE query per sample over S positions:
//   logits[s] = q . k[s];  logits -= 1e8 where masked (s >= len_b when lengths != null);  p = softmax(logits * scale);
//   out = sum_s p[s] v[s].   q [B][D] (ldq), k [B][S][.] (ldk), v [B][S][.] (ldv), out [B][.] (ldo); all f32.
__global__ void attn1q_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, int ldk, const float* __restrict__ v,
                              int ldv, const int* __restrict__ lengths, float* __restrict__ out, int ldo, int S, int D, int Dv,
                              float scale) {
    extern __shared__ float sh[];            // [S] probabilities
    __shared__ float red[2];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const float* qb = q + (size_t)b * ldq;
    const int len = lengths ? lengths[b] : S;
    for (int sidx = wave; sidx < S; sidx += nw) {
        const float* kr = k + ((size_t)b * S + sidx) * ldk;
        float acc = 0.f;
        for (int j = lane; j < D; j += 64) acc += qb[j] * kr[j];
        acc = wave_sum(acc);
        if (lane == 0) sh[sidx] = (acc - (sidx >= len ? 1e8f : 0.f)) * scale;
    }
    __syncthreads();
    if (wave == 0) {
        float m = -3.0e38f;
        for (int i = lane; i < S; i += 64) m = fmaxf(m, sh[i]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.f;
        for (int i = lane; i < S; i += 64) sum += expf(sh[i] - m);
        sum = wave_sum(sum);
        if (lane == 0) { red[0] = m; red[1] = 1.f / sum; }
    }
    __syncthreads();
    const float m = red[0], inv = red[1];
    for (int i = threadIdx.x; i < S; i += blockDim.x) sh[i] = expf(sh[i] - m) * inv;
    __syncthreads();
    for (int cidx = threadIdx.x; cidx < Dv; cidx += blockDim.x) {
        float acc = 0.f;
        const float* vb = v + (size_t)b * S * ldv + cidx;
        for (int i = 0; i < S; ++i) acc += sh[i] * vb[(size_t)i * ldv];
        out[(size_t)b * ldo + cidx] = acc;
    }
}
hipError_t launch_attn1q(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const int* lengths, float* out,
                         int ldo, int B, int S, int D, int Dv, float scale, hipStream_t s) {
    hipLaunchKernelGGL(attn1q_kernel, dim3(B), dim3(256), S * sizeof(float), s, q, ldq, k, ldk, v, ldv, lengths, out, ldo, S, D, Dv, scale);
    return hipGetLastError();
}

// torch.argmax(output, dim=1) (hierarchical_trainer.py:1098): first maximal index, and a NaN is maximal
__global__ void argmax_kernel(const float* __restrict__ logits, int64_t* __restrict__ pred, int B, int n, int ld) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = logits + (size_t)b * ld;
    int best = 0;
    float bv = p[0];
    for (int j = 1; j < n; ++j)                                 // a NaN counts as the maximum, the first one wins (as val_loss_kernel)
        if (p[j] > bv || (p[j] != p[j] && bv == bv)) { bv = p[j]; best = j; }
    pred[b] = best;
}
hipError_t launch_argmax(const float* logits, int64_t* pred, int B, int n, int ld, hipStream_t s) {
    hipLaunchKernelGGL(argmax_kernel, dim3((B + 63) / 64), dim3(64), 0, s, logits, pred, B, n, ld);
    return hipGetLastError();
}

// sub_task_embedding lookup (seq2seq_lowlevel.py:141)
__global__ void embed_rows_kernel(const float* __restrict__ emb, const int64_t* __restrict__ idx, float* __restrict__ y,
                                  int B, int D, int ld, int col0, int nrows) {
    const int b = blockIdx.x;
    long i = idx[b];
    if (i < 0) i = 0;
    if (i >= nrows) i = nrows - 1;
    for (int j = threadIdx.x; j < D; j += blockDim.x) y[(size_t)b * ld + col0 + j] = emb[(size_t)i * D + j];
}
hipError_t launch_embed_rows(const float* emb, const int64_t* idx, float* y, int B, int D, int ld, int col0, int nrows, hipStream_t s) {
    hipLaunchKernelGGL(embed_rows_kernel, dim3(B), dim3(64), 0, s, emb, idx, y, B, D, ld, col0, nrows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ teacher-forced validation step (hcm_val_step)
// discrete_actions = (oracle - 1).masked_fill_(oracle == 0, num_sub_tasks)  (hierarchical_trainer.py:597-599), on the device.  A label outside
// [0, num_sub_tasks] is given the padded sub-task as well, so that the embedding lookup stays inside its table; val_loss_kernel counts such rows.
__global__ void val_subtask_kernel(const int64_t* __restrict__ oracle, int64_t* __restrict__ subtask, int rows, int num_sub_tasks) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int64_t o = oracle[r];
    subtask[r] = (o >= 1 && o <= num_sub_tasks) ? o - 1 : num_sub_tasks;
}
hipError_t launch_val_subtask(const int64_t* oracle, int64_t* subtask, int rows, int num_sub_tasks, hipStream_t s) {
    hipLaunchKernelGGL(val_subtask_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, oracle, subtask, rows, num_sub_tasks);
    return hipGetLastError();
}

// The criteria of HierarchicalTrainer._update_agent_val (hierarchical_trainer.py:578-588, :617-626) over the rows of one call, f32:
//   result[0] CrossEntropyLoss(ignore_index = -1, mean) of logits against oracle - 1 over the rows with oracle != 0
//   result[1] MSELoss of vel.masked_fill(corrected == 0, 0) against corrected, mean over all 2 * rows elements
//   result[2] BCEWithLogitsLoss of stop against oracle_stop over the rows with oracle_stop != -1 (max(x,0) - x*y + log1p(exp(-|x|)))
//   result[3] rows with oracle != 0 whose argmax (first maximal index) is the target;  result[4] rows with oracle != 0
//   result[5] rows that entered the stop loss;  result[6] rows with oracle outside [0, num_sub_tasks] (treated as padded);  result[7] 0
// No valid row: 0 / 0 = NaN in result[0] / result[2], as torch gives.
// ONE workgroup of kValLossThreads threads -- the launch shape is PINNED, so the order of summation is fixed: thread t adds its rows t, t + 256, ...
// in row order, a wave adds its lanes by a xor butterfly, lane 0 of wave 0 adds the four waves' sums in wave order.  No atomics; counts are
// integers until the final store.
constexpr int kValLossThreads = 256;
__global__ __launch_bounds__(kValLossThreads) void val_loss_kernel(const float* __restrict__ logits, int ld_logits, const float* __restrict__ vel, int ld_vel,
                                                                   const float* __restrict__ stop, int ld_stop, const int64_t* __restrict__ oracle,
                                                                   const float* __restrict__ corrected, const float* __restrict__ oracle_stop,
                                                                   float* __restrict__ result, int rows, int A, int num_sub_tasks, int n_vel) {
    float ce = 0.f, mse = 0.f, bce = 0.f;
    int correct = 0, total = 0, n_stop = 0, n_bad = 0;
    for (int r = threadIdx.x; r < rows; r += kValLossThreads) {
        const int64_t o = oracle[r];
        if (o < 0 || o > num_sub_tasks) ++n_bad;
        else if (o != 0) {
            const float* p = logits + (size_t)r * ld_logits;
            const int target = (int)o - 1;
            int best = 0;
            float mx = p[0];
            for (int j = 1; j < A; ++j)                         // torch.argmax: a NaN counts as the maximum, the first one wins
                if (p[j] > mx || (p[j] != p[j] && mx == mx)) { mx = p[j]; best = j; }
            // log-sum-exp around the row maximum; a NaN or an infinite maximum turns into NaN through the subtraction, as in torch's log_softmax
            float se = 0.f;
            for (int j = 0; j < A; ++j) se += expf(p[j] - mx);
            // a target outside the A logits cannot be picked (num_sub_tasks > A is a configuration the models do not have): NaN, never a wild read
            ce += target < A ? (mx + logf(se)) - p[target] : __builtin_nanf("");
            correct += best == target ? 1 : 0;
            ++total;
        }
        for (int j = 0; j < n_vel; ++j) {
            const float c = corrected[(size_t)r * n_vel + j];
            const float v = c == 0.f ? 0.f : vel[(size_t)r * ld_vel + j];
            const float d = v - c;
            mse += d * d;
        }
        const float y = oracle_stop[r];
        if (y != -1.f) {
            const float x = stop[(size_t)r * ld_stop];
            bce += (fmaxf(x, 0.f) - x * y) + log1pf(expf(-fabsf(x)));
            ++n_stop;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ce += __shfl_xor(ce, o, 64); mse += __shfl_xor(mse, o, 64); bce += __shfl_xor(bce, o, 64);
        correct += __shfl_xor(correct, o, 64); total += __shfl_xor(total, o, 64); n_stop += __shfl_xor(n_stop, o, 64); n_bad += __shfl_xor(n_bad, o, 64);
    }
    constexpr int NW = kValLossThreads / 64;
    __shared__ float fs[NW][3];
    __shared__ int is[NW][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        fs[wave][0] = ce; fs[wave][1] = mse; fs[wave][2] = bce;
        is[wave][0] = correct; is[wave][1] = total; is[wave][2] = n_stop; is[wave][3] = n_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f[3] = {0.f, 0.f, 0.f};
        int n[4] = {0, 0, 0, 0};
        for (int w = 0; w < NW; ++w) {
            for (int k = 0; k < 3; ++k) f[k] += fs[w][k];
            for (int k = 0; k < 4; ++k) n[k] += is[w][k];
        }
        result[0] = f[0] / (float)n[1];
        result[1] = f[1] / (float)(rows * n_vel);
        result[2] = f[2] / (float)n[2];
        result[3] = (float)n[0];
        result[4] = (float)n[1];
        result[5] = (float)n[2];
        result[6] = (float)n[3];
        result[7] = 0.f;
    }
}
hipError_t launch_val_loss(const float* logits, int ld_logits, const float* vel, int ld_vel, const float* stop, int ld_stop, const int64_t* oracle,
                           const float* corrected, const float* oracle_stop, float* result, int rows, int A, int num_sub_tasks, int n_vel, hipStream_t s) {
    hipLaunchKernelGGL(val_loss_kernel, dim3(1), dim3(kValLossThreads), 0, s, logits, ld_logits, vel, ld_vel, stop, ld_stop, oracle, corrected,
                       oracle_stop, result, rows, A, num_sub_tasks, n_vel);
    return hipGetLastError();
}

// The criteria of the flat trainer's _update_agent_val (robo_vln_trainer.py:544-575) over the rows of one CMANet / Seq2SeqNet call, f32:
//   result[0] MSELoss of out.masked_fill(corrected == 0, 0) against corrected, mean over all num_actions * rows elements (:557-561)
//   result[1] BCEWithLogitsLoss of stop against oracle_stop over the rows with oracle_stop != -1 (:563-566)
//   result[2] AuxLosses.reduce(~action_mask[:, 0]) (:569-570, common/aux_losses.py:27-33): the mean over the rows with corrected[r, 0] != 0 of
//             (progress_hat[r] - progress[r])^2, the loss Seq2SeqNet registers (seq2seq.py:176-185), times a weight of 1.0 -- the model passes
//             PROGRESS_MONITOR.alpha in the `masks` slot of register_loss(name, loss, masks=None, alpha=1.0), so the configured alpha never
//             arrives and the weight is the default; reproduced here.  progress_hat == NULL (nothing registered): reduce returns 0.0.
//   result[3] rows that entered the stop loss;  result[4] rows that entered the aux mean (0 without the monitor);  result[5..7] 0
// Empty selections: 0 / 0 = NaN in result[1], and in result[2] with the monitor on, as torch's mean over an empty tensor.
// Launch shape and order of summation as val_loss_kernel's: ONE workgroup of kValLossThreads threads, thread t adds its rows t, t + 256, ...
// in row order, a xor butterfly per wave, lane 0 of wave 0 adds the four waves' sums in wave order.  No atomics; counts are integers until
// the final store.
__global__ __launch_bounds__(kValLossThreads) void flat_val_loss_kernel(const float* __restrict__ out, int ld_out, const float* __restrict__ stop, int ld_stop,
                                                                        const float* __restrict__ progress_hat, int ld_prog,
                                                                        const float* __restrict__ corrected, const float* __restrict__ oracle_stop,
                                                                        const float* __restrict__ progress, float* __restrict__ result, int rows,
                                                                        int num_actions) {
    float mse = 0.f, bce = 0.f, aux = 0.f;
    int n_stop = 0, n_aux = 0;
    const bool monitor = progress_hat != nullptr && progress != nullptr;
    for (int r = threadIdx.x; r < rows; r += kValLossThreads) {
        for (int j = 0; j < num_actions; ++j) {
            const float c = corrected[(size_t)r * num_actions + j];
            const float v = c == 0.f ? 0.f : out[(size_t)r * ld_out + j];
            const float d = v - c;
            mse += d * d;
        }
        const float y = oracle_stop[r];
        if (y != -1.f) {
            const float x = stop[(size_t)r * ld_stop];
            bce += (fmaxf(x, 0.f) - x * y) + log1pf(expf(-fabsf(x)));
            ++n_stop;
        }
        if (monitor && corrected[(size_t)r * num_actions] != 0.f) {
            const float d = progress_hat[(size_t)r * ld_prog] - progress[r];
            aux += d * d;
            ++n_aux;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mse += __shfl_xor(mse, o, 64); bce += __shfl_xor(bce, o, 64); aux += __shfl_xor(aux, o, 64);
        n_stop += __shfl_xor(n_stop, o, 64); n_aux += __shfl_xor(n_aux, o, 64);
    }
    constexpr int NW = kValLossThreads / 64;
    __shared__ float fs[NW][3];
    __shared__ int is[NW][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        fs[wave][0] = mse; fs[wave][1] = bce; fs[wave][2] = aux;
        is[wave][0] = n_stop; is[wave][1] = n_aux;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f[3] = {0.f, 0.f, 0.f};
        int n[2] = {0, 0};
        for (int w = 0; w < NW; ++w) {
            for (int k = 0; k < 3; ++k) f[k] += fs[w][k];
            for (int k = 0; k < 2; ++k) n[k] += is[w][k];
        }
        result[0] = f[0] / ((float)rows * (float)num_actions);
        result[1] = f[1] / (float)n[0];
        result[2] = monitor ? f[2] / (float)n[1] : 0.f;
        result[3] = (float)n[0];
        result[4] = (float)n[1];
        result[5] = 0.f;
        result[6] = 0.f;
        result[7] = 0.f;
    }
}
hipError_t launch_flat_val_loss(const float* out, int ld_out, const float* stop, int ld_stop, const float* progress_hat, int ld_prog,
                                const float* corrected, const float* oracle_stop, const float* progress, float* result, int rows, int num_actions,
                                hipStream_t s) {
    hipLaunchKernelGGL(flat_val_loss_kernel, dim3(1), dim3(kValLossThreads), 0, s, out, ld_out, stop, ld_stop, progress_hat, ld_prog, corrected,
                       oracle_stop, progress, result, rows, num_actions);
    return hipGetLastError();
}

template <typename T>
__global__ void to_f32_kernel(const T* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) y[e] = Tr<T>::ld(x + e);
}
template <typename T>
__global__ void from_f32_kernel(const float* __restrict__ x, T* __restrict__ y, size_t n) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) Tr<T>::st(y + e, x[e]);
}
hipError_t launch_convert_to_f32(const void* x, int dt, float* y, size_t n, hipStream_t s) {
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(to_f32_kernel<T>, dim3(grid_for(n)), dim3(256), 0, s, (const T*)x, y, n));
    return hipGetLastError();
}
hipError_t launch_convert_from_f32(const float* x, void* y, int dt, size_t n, hipStream_t s) {
    HCM_DISPATCH_T(dt, hipLaunchKernelGGL(from_f32_kernel<T>, dim3(grid_for(n)), dim3(256), 0, s, x, (T*)y, n));
    return hipGetLastError();
}

template <typename A, typename B_>
__global__ void convert_kernel(const A* __restrict__ x, B_* __restrict__ y, size_t n) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) Tr<B_>::st(y + e, Tr<A>::ld(x + e));
}
hipError_t launch_convert(const void* x, int dt_in, void* y, int dt_out, size_t n, hipStream_t s) {
    if (dt_in == dt_out) return hipMemcpyAsync(y, x, n * dt_size(dt_in), hipMemcpyDeviceToDevice, s);
    HCM_DISPATCH_T(dt_in, {
        using A = T;
        if (dt_out == DT_BF16) hipLaunchKernelGGL((convert_kernel<A, bf16>), dim3(grid_for(n)), dim3(256), 0, s, (const A*)x, (bf16*)y, n);
        else if (dt_out == DT_F16) hipLaunchKernelGGL((convert_kernel<A, f16>), dim3(grid_for(n)), dim3(256), 0, s, (const A*)x, (f16*)y, n);
        else if (dt_out == DT_F32) hipLaunchKernelGGL((convert_kernel<A, float>), dim3(grid_for(n)), dim3(256), 0, s, (const A*)x, (float*)y, n);
        else return hipErrorInvalidValue;
    });
    return hipGetLastError();
}


// Development aid (make DEV=1, HCM_MARKS=1): a one-lane kernel that stores the constant 100 MHz wall clock -- placed by forward.cpp between the
// launches of a chain, it records WHEN that chain reached that point of the (hipGraph-replayed, multi-stream) step.  rocprofv3's kernel trace
// serialises the streams (kernels in flight: 1 for 91 % of a traced step), so it cannot show how the three chains really interleave.
__global__ void mark_kernel(unsigned long long* slot) { *slot = wall_clock64(); }
hipError_t launch_mark(unsigned long long* slot, hipStream_t s) {
    hipLaunchKernelGGL(mark_kernel, dim3(1), dim3(1), 0, s, slot);
    return hipGetLastError();
}

// Busy-wait for `ticks` of the 100 MHz wall clock on one wave: the stream-overlap probe of api.cpp (two streams that share a hardware queue run two of these
// back to back, two that do not run them side by side).
__global__ void spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
hipError_t launch_spin(unsigned long long ticks, hipStream_t s) {
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s, ticks);
    return hipGetLastError();
}

}  // namespace hcm
