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

// ---- the frozen BERT stream at the ABI (hcm_instr_features, include/hcm.h): f32 (src_rows, L, D) <-> the buffer bert() fills, (B, L, D) contiguous in
// BERT's storage type.  No transpose, so no LDS: a pure conversion stream.  One workgroup owns kIThreads chunks of ONE output row r; its length
// lens[r] is loaded through an address that depends on blockIdx alone -- uniform over the workgroup, one scalar load, not one load per lane.
// Positions l >= lens[r] are stored as exact +0.0 and their source is never read: what BERT (or a caller) leaves behind a row's own length is
// not part of any contract and must not travel through a cache.
constexpr int kIThreads = 256;

// grid: (B, ceil(L * D / (kIThreads * CH))) in the 16-byte form, (B, ceil(L * D / kIThreads)) in the scalar one.  Output row r reads source row
// r % src_rows: B rows (own stream each), 1 (one instruction for every row), N (time-major chunk: row t * N + n takes environment n's stream).
template <typename T, bool VEC>
__global__ __launch_bounds__(kIThreads) void instr_feat_ingest_kernel(const float* __restrict__ x, T* __restrict__ y, const int* __restrict__ lens,
                                                                      int src_rows, int L, int D) {
    const int r = blockIdx.x;
    const int len = lens ? min(max(lens[r], 0), L) : L;
    const size_t n = (size_t)L * D, live = (size_t)len * D;
    const float* xr = x + (size_t)(r % src_rows) * n;
    T* yr = y + (size_t)r * n;
    if (VEC) {
        constexpr int CH = Tr<T>::CH;                         // D % CH == 0: a chunk never straddles two positions
        const size_t i = ((size_t)blockIdx.y * kIThreads + threadIdx.x) * CH;
        if (i >= n) return;
        if constexpr (CH == 4) {
            *reinterpret_cast<float4*>(yr + i) = i < live ? *reinterpret_cast<const float4*>(xr + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (i < live) {
                const float4 a = *reinterpret_cast<const float4*>(xr + i), b = *reinterpret_cast<const float4*>(xr + i + 4);
                o = make_uint4((uint32_t)bits16<T>(a.x) | (uint32_t)bits16<T>(a.y) << 16, (uint32_t)bits16<T>(a.z) | (uint32_t)bits16<T>(a.w) << 16,
                               (uint32_t)bits16<T>(b.x) | (uint32_t)bits16<T>(b.y) << 16, (uint32_t)bits16<T>(b.z) | (uint32_t)bits16<T>(b.w) << 16);
            }
            *reinterpret_cast<uint4*>(yr + i) = o;
        }
    } else {
        const size_t i = (size_t)blockIdx.y * kIThreads + threadIdx.x;
        if (i >= n) return;
        Tr<T>::st(yr + i, i < live ? xr[i] : 0.f);
    }
}

// grid as above over `rows`; y (rows, L, D) in T -> x (rows, L, D) f32
template <typename T, bool VEC>
__global__ __launch_bounds__(kIThreads) void instr_feat_export_kernel(const T* __restrict__ y, float* __restrict__ x, const int* __restrict__ lens, int L, int D) {
    const int r = blockIdx.x;
    const int len = lens ? min(max(lens[r], 0), L) : L;
    const size_t n = (size_t)L * D, live = (size_t)len * D;
    const T* yr = y + (size_t)r * n;
    float* xr = x + (size_t)r * n;
    if (VEC) {
        constexpr int CH = Tr<T>::CH;
        const size_t i = ((size_t)blockIdx.y * kIThreads + threadIdx.x) * CH;
        if (i >= n) return;
        float e[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) e[j] = 0.f;
        if (i < live) ld_chunk(yr + i, e);
#pragma unroll
        for (int j = 0; j < CH; j += 4) *reinterpret_cast<float4*>(xr + i + j) = make_float4(e[j], e[j + 1], e[j + 2], e[j + 3]);
    } else {
        const size_t i = (size_t)blockIdx.y * kIThreads + threadIdx.x;
        if (i >= n) return;
        xr[i] = i < live ? Tr<T>::ld(yr + i) : 0.f;
    }
}

// the 16-byte form: whole chunks per position and both pointers 16-byte aligned (every row then is: L * D is a multiple of the chunk too)
bool instr_vec_ok(const void* x, const void* y, int dt, int D) {
    return D % 8 == 0 && D % dt_chunk(dt) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
}
dim3 instr_grid(int rows, int L, int D, int per_thread) {
    const size_t per_block = (size_t)kIThreads * per_thread;
    return dim3(rows, (unsigned)(((size_t)L * D + per_block - 1) / per_block), 1);
}

template <typename T>
hipError_t instr_ingest_t(const float* x, void* y, int dt, const int* lens, int B, int src_rows, int L, int D, hipStream_t s) {
    if (instr_vec_ok(x, y, dt, D))
        hipLaunchKernelGGL((instr_feat_ingest_kernel<T, true>), instr_grid(B, L, D, Tr<T>::CH), dim3(kIThreads), 0, s, x, (T*)y, lens, src_rows, L, D);
    else
        hipLaunchKernelGGL((instr_feat_ingest_kernel<T, false>), instr_grid(B, L, D, 1), dim3(kIThreads), 0, s, x, (T*)y, lens, src_rows, L, D);
    return hipGetLastError();
}
template <typename T>
hipError_t instr_export_t(const void* y, int dt, float* x, const int* lens, int rows, int L, int D, hipStream_t s) {
    if (instr_vec_ok(x, y, dt, D))
        hipLaunchKernelGGL((instr_feat_export_kernel<T, true>), instr_grid(rows, L, D, Tr<T>::CH), dim3(kIThreads), 0, s, (const T*)y, x, lens, L, D);
    else
        hipLaunchKernelGGL((instr_feat_export_kernel<T, false>), instr_grid(rows, L, D, 1), dim3(kIThreads), 0, s, (const T*)y, x, lens, L, D);
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

// (grid.y carries the chunks of one row: L * D up to 65535 * 256 elements in the scalar form)
static bool instr_shape_ok(int rows, int L, int D) {
    return rows >= 1 && L >= 1 && D >= 1 && ((size_t)L * D + kIThreads - 1) / kIThreads <= 65535;
}
hipError_t launch_instr_feat_ingest(const float* x, void* y, int dt, const int* lens, int B, int src_rows, int L, int D, hipStream_t s) {
    if (!x || !y || src_rows < 1 || !instr_shape_ok(B, L, D) || B % src_rows != 0) return hipErrorInvalidValue;
    if (dt == DT_F16) return instr_ingest_t<f16>(x, y, dt, lens, B, src_rows, L, D, s);
    if (dt == DT_BF16) return instr_ingest_t<bf16>(x, y, dt, lens, B, src_rows, L, D, s);
    return instr_ingest_t<float>(x, y, dt, lens, B, src_rows, L, D, s);
}
hipError_t launch_instr_feat_export(const void* y, int dt, float* x, const int* lens, int rows, int L, int D, hipStream_t s) {
    if (!x || !y || !instr_shape_ok(rows, L, D)) return hipErrorInvalidValue;
    if (dt == DT_F16) return instr_export_t<f16>(y, dt, x, lens, rows, L, D, s);
    if (dt == DT_BF16) return instr_export_t<bf16>(y, dt, x, lens, rows, L, D, s);
    return instr_export_t<float>(y, dt, x, lens, rows, L, D, s);
}

}  // namespace hcm
