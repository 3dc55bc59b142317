// Precomputed trunk features (hcm_features, include/hcm.h): the reference's `rgb_features` / `depth_features` observation keys
// (models/encoders/resnet_encoders.py:83-86, :207-214) are NCHW f32; the library's consumers read pixel-major rows in the sub-network's storage
// type.  Both directions are a (C, S) <-> (S, C) transpose per row with a conversion and a power-of-two scale.
//
// One workgroup moves a tile of kCT channels x up to kST positions of one row through LDS, so that both global sides are coalesced: the NCHW side
// is read / written along s (a whole kCT x S block is one contiguous run when S <= kST), the pixel-major side along c.  Tile rows are padded to
// kST + 1 words: the pixel-major phase walks the tile column-wise (word stride 33, odd) and the NCHW phase row-wise, neither lands two lanes of
// a 32-lane group on one bank more than twice.  16-byte global accesses where the sizes and the pointers allow, scalar ones otherwise.
#include "dev.h"
#include "kernels.h"

namespace hcm {
namespace {

constexpr int kCT = 64, kST = 32, kThreads = 256;

template <typename T> __device__ __forceinline__ uint16_t bits16(float v);
template <> __device__ __forceinline__ uint16_t bits16<bf16>(float v) { return f2bf(v); }
template <> __device__ __forceinline__ uint16_t bits16<f16>(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }

// grid: (ceil(C / kCT), ceil(S / kST), rows)
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void feat_ingest_kernel(const float* __restrict__ x, T* __restrict__ y, int C, int S, int ld, float scale) {
    __shared__ float tile[kCT][kST + 1];
    const int c0 = blockIdx.x * kCT, s0 = blockIdx.y * kST;
    const int cn = min(kCT, C - c0), sn = min(kST, S - s0);
    const float* xr = x + (size_t)blockIdx.z * C * S;
    T* yr = y + (size_t)blockIdx.z * S * ld;
    if (VEC) {
        // sn == S: the cn x S block is one contiguous, 16-byte aligned run of cn * S floats (a multiple of 4)
        const float* run = xr + (size_t)c0 * S;
        for (int i = threadIdx.x * 4; i < cn * S; i += kThreads * 4) {
            const float4 v = *reinterpret_cast<const float4*>(run + i);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(i + j) / S][(i + j) % S] = e[j];
        }
    } else {
        for (int i = threadIdx.x; i < cn * sn; i += kThreads) {
            const int c = i / sn, s = i % sn;
            tile[c][s] = xr[(size_t)(c0 + c) * S + s0 + s];
        }
    }
    __syncthreads();
    if (VEC) {
        constexpr int CH = Tr<T>::CH;               // elements per 16-byte store; cn, c0 and ld are multiples of it, y is 16-byte aligned
        const int groups = cn / CH;
        for (int i = threadIdx.x; i < sn * groups; i += kThreads) {
            const int s = i / groups, g = i % groups;
            T* dst = yr + (size_t)(s0 + s) * ld + c0 + g * CH;
            if constexpr (CH == 4) {
                *reinterpret_cast<float4*>(dst) = make_float4(tile[g * 4][s] * scale, tile[g * 4 + 1][s] * scale, tile[g * 4 + 2][s] * scale, tile[g * 4 + 3][s] * scale);
            } else {
                uint32_t w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[j] = (uint32_t)bits16<T>(tile[g * 8 + 2 * j][s] * scale) | (uint32_t)bits16<T>(tile[g * 8 + 2 * j + 1][s] * scale) << 16;
                *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    } else {
        for (int i = threadIdx.x; i < sn * cn; i += kThreads) {
            const int s = i / cn, c = i % cn;
            Tr<T>::st(yr + (size_t)(s0 + s) * ld + c0 + c, tile[c][s] * scale);
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void feat_export_kernel(const T* __restrict__ y, float* __restrict__ x, int C, int S, int ld, float scale) {
    __shared__ float tile[kCT][kST + 1];
    const int c0 = blockIdx.x * kCT, s0 = blockIdx.y * kST;
    const int cn = min(kCT, C - c0), sn = min(kST, S - s0);
    const T* yr = y + (size_t)blockIdx.z * S * ld;
    float* xr = x + (size_t)blockIdx.z * C * S;
    if (VEC) {
        constexpr int CH = Tr<T>::CH;
        const int groups = cn / CH;
        for (int i = threadIdx.x; i < sn * groups; i += kThreads) {
            const int s = i / groups, g = i % groups;
            float e[CH];
            ld_chunk(yr + (size_t)(s0 + s) * ld + c0 + g * CH, e);
#pragma unroll
            for (int j = 0; j < CH; ++j) tile[g * CH + j][s] = e[j] * scale;
        }
    } else {
        for (int i = threadIdx.x; i < sn * cn; i += kThreads) {
            const int s = i / cn, c = i % cn;
            tile[c][s] = Tr<T>::ld(yr + (size_t)(s0 + s) * ld + c0 + c) * scale;
        }
    }
    __syncthreads();
    if (VEC) {
        float* run = xr + (size_t)c0 * S;
        for (int i = threadIdx.x * 4; i < cn * S; i += kThreads * 4) {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = tile[(i + j) / S][(i + j) % S];
            *reinterpret_cast<float4*>(run + i) = make_float4(e[0], e[1], e[2], e[3]);
        }
    } else {
        for (int i = threadIdx.x; i < cn * sn; i += kThreads) {
            const int c = i / sn, s = i % sn;
            xr[(size_t)(c0 + c) * S + s0 + s] = tile[c][s];
        }
    }
}

// the 16-byte form: whole kCT-channel tiles, all S positions in one tile, every row of both buffers 16-byte aligned
bool feat_vec_ok(const void* x, const void* y, int dt, int C, int S, int ld) {
    const int ch = dt_chunk(dt);
    return S <= kST && C % kCT == 0 && ld % ch == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
}

template <typename T>
hipError_t ingest_t(const float* x, void* y, int dt, int rows, int C, int S, int ld, float scale, hipStream_t s) {
    const dim3 grid((C + kCT - 1) / kCT, (S + kST - 1) / kST, rows);
    if (feat_vec_ok(x, y, dt, C, S, ld)) hipLaunchKernelGGL((feat_ingest_kernel<T, true>), grid, dim3(kThreads), 0, s, x, (T*)y, C, S, ld, scale);
    else hipLaunchKernelGGL((feat_ingest_kernel<T, false>), grid, dim3(kThreads), 0, s, x, (T*)y, C, S, ld, scale);
    return hipGetLastError();
}
template <typename T>
hipError_t export_t(const void* y, int dt, float* x, int rows, int C, int S, int ld, float scale, hipStream_t s) {
    const dim3 grid((C + kCT - 1) / kCT, (S + kST - 1) / kST, rows);
    if (feat_vec_ok(x, y, dt, C, S, ld)) hipLaunchKernelGGL((feat_export_kernel<T, true>), grid, dim3(kThreads), 0, s, (const T*)y, x, C, S, ld, scale);
    else hipLaunchKernelGGL((feat_export_kernel<T, false>), grid, dim3(kThreads), 0, s, (const T*)y, x, C, S, ld, scale);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_feat_ingest(const float* x, void* y, int dt, int rows, int C, int S, int ld, float scale, hipStream_t s) {
    if (rows < 1 || C < 1 || S < 1 || ld < C || rows > 65535) return hipErrorInvalidValue;
    if (dt == DT_F16) return ingest_t<f16>(x, y, dt, rows, C, S, ld, scale, s);
    if (dt == DT_BF16) return ingest_t<bf16>(x, y, dt, rows, C, S, ld, scale, s);
    return ingest_t<float>(x, y, dt, rows, C, S, ld, scale, s);
}
hipError_t launch_feat_export(const void* y, int dt, float* x, int rows, int C, int S, int ld, float scale, hipStream_t s) {
    if (rows < 1 || C < 1 || S < 1 || ld < C || rows > 65535) return hipErrorInvalidValue;
    if (dt == DT_F16) return export_t<f16>(y, dt, x, rows, C, S, ld, scale, s);
    if (dt == DT_BF16) return export_t<bf16>(y, dt, x, rows, C, S, ld, scale, s);
    return export_t<float>(y, dt, x, rows, C, S, ld, scale, s);
}

}  // namespace hcm
