// The convolutional part of SimpleAllCNN.cnn (simple_cnns.py:76-95) in float32 with a backward pass, behind train.simple_cnn:
//   Conv2d(Cin, 32, 8, stride 4) + ReLU -> Conv2d(32, 64, 4, stride 2) + ReLU -> Conv2d(64, 32, 3, stride 1),  no padding, Cin 1 or 3.
//
// Every product is one gather GEMM on v_mfma_f32_32x32x2f32 with the channels as the M side (32 or 64: one or two accumulator tiles per wave)
// and the pixels as the N side, so a wave stores 32 consecutive pixels of one channel per register and the maps stay channel-major:
//   forward      D[co][p]  = sum_k  Wt[k][co] in[window(p) + off(k)],       k = (ci, ky, kx) in OIHW order, ascending;
//   data grad    D[ci][q]  = sum_k  Wd[k][ci] g[co, (y - ky)/s, (x - kx)/s], k = (co, ky, kx); a tap that lands between or outside the output
//                            pixels contributes an exact 0, so a pixel no window covers gets 0; the ReLU gate (stored value > 0) is applied
//                            to the result, and the gated gradient is what is stored;
//   weight grad  D[co][k]  = sum_p  g[co][p] in[window(p) + off(k)] over a chunk of pixels per workgroup, the chunks' shares then added in
//                            chunk order by a second launch (no atomics), and the bias sums by a launch with a fixed tree.
// The operands come straight from global memory through per-workgroup offset tables in LDS; nothing is staged.  An output element's sum runs
// over k (or over the pixels of its chunk) in ascending order whatever tile it sits in, so a forward row's bits depend on that row and the
// weights alone, and two runs give the same bits.
#include "dev.h"
#include "kernels.h"
#include "vla_train_dev.h"

namespace hcm {

namespace {

constexpr int kScMaxK = 1024;          // the longest reduction: conv2's data gradient, 64 x 4 x 4
constexpr int kScChunkMax = 1024;      // pixels per weight-gradient workgroup, at most

struct ScLayer {
    int Cin, Cout, kw, s, Hi, Wi, Ho, Wo;      // square kernels: kh = kw
    int K() const { return Cin * kw * kw; }
};

struct ScGeom {
    ScLayer L[3];
    int B;
};

ScGeom sc_geom(int B, int H, int W, int Cin) {
    ScGeom g;
    g.B = B;
    const int h1 = (H - 8) / 4 + 1, w1 = (W - 8) / 4 + 1, h2 = (h1 - 4) / 2 + 1, w2 = (w1 - 4) / 2 + 1, h3 = h2 - 2, w3 = w2 - 2;
    g.L[0] = {Cin, 32, 8, 4, H, W, h1, w1};
    g.L[1] = {32, 64, 4, 2, h1, w1, h2, w2};
    g.L[2] = {64, 32, 3, 1, h2, w2, h3, w3};
    return g;
}

// pixels per weight-gradient chunk: about 256 chunks, 64..1024 pixels each, a multiple of 32
int sc_chunk(size_t P) {
    size_t c = ((P + 255) / 256 + 31) / 32 * 32;
    return (int)(c < 64 ? 64 : c > (size_t)kScChunkMax ? (size_t)kScChunkMax : c);
}

// the regions of the work buffer, in floats
struct ScWork {
    size_t wt[3], wd[2], a1, a2, g1, g2, part, total;      // wd[0]: conv3's data-gradient pack, wd[1]: conv2's
};

ScWork sc_work(const ScGeom& g) {
    ScWork w;
    size_t o = 0;
    for (int l = 0; l < 3; ++l) w.wt[l] = o, o += (size_t)g.L[l].K() * g.L[l].Cout;
    w.wd[0] = o, o += (size_t)g.L[2].K() * g.L[2].Cout;
    w.wd[1] = o, o += (size_t)g.L[1].K() * g.L[1].Cout;
    const size_t n1 = (size_t)g.B * 32 * g.L[0].Ho * g.L[0].Wo, n2 = (size_t)g.B * 64 * g.L[1].Ho * g.L[1].Wo;
    w.a1 = o, o += n1;
    w.a2 = o, o += n2;
    w.g1 = o, o += n1;
    w.g2 = o, o += n2;
    size_t part = 0;
    for (int l = 0; l < 3; ++l) {
        const size_t P = (size_t)g.B * g.L[l].Ho * g.L[l].Wo, nchunk = (P + sc_chunk(P) - 1) / sc_chunk(P);
        const size_t n = nchunk * g.L[l].Cout * g.L[l].K();
        part = n > part ? n : part;
    }
    w.part = o, o += part;
    w.total = o;
    return w;
}

__device__ __forceinline__ float sc_ld(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float sc_ld(const uint8_t* p, size_t i) { return (float)p[i]; }

// dst[k][m] = w[co][ci][ky][kx] with, forward (dgrad == 0), m = co and k = (ci, ky, kx); data gradient, m = ci and k = (co, ky, kx)
__global__ void sc_pack_kernel(const float* __restrict__ w, float* __restrict__ dst, int Cout, int Cin, int kk, int dgrad) {
    const int n = Cout * Cin * kk, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = i % kk, ci = i / kk % Cin, co = i / (kk * Cin);
    if (dgrad) dst[(size_t)(co * kk + t) * Cin + ci] = w[i];
    else dst[(size_t)(ci * kk + t) * Cout + co] = w[i];
}

struct ScFwd {
    const void* in;
    const float *wt, *bias;
    float* out;
    ScLayer L;
    int sc, sy, sx;              // the input's strides of channel, row and column in elements; its sample stride is Cin * Hi * Wi
    float scale;
    int P;                       // B * Ho * Wo
};

template <typename T, int MT, bool RELU>
__global__ __launch_bounds__(256) void sc_fwd_kernel(ScFwd p) {
    __shared__ int off[kScMaxK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = p.L.kw * p.L.kw, K = p.L.Cin * kk;
    for (int k = tid; k < K; k += 256) {
        const int ci = k / kk, r = k % kk;
        off[k] = ci * p.sc + (r / p.L.kw) * p.sy + (r % p.L.kw) * p.sx;
    }
    __syncthreads();
    const int n0 = (blockIdx.x * 4 + wave) * 32;
    if (n0 >= p.P) return;
    const int hw = p.L.Ho * p.L.Wo;
    const int pn = n0 + (lane & 31), pc = pn < p.P ? pn : p.P - 1;
    const int b = pc / hw, r = pc % hw, oy = r / p.L.Wo, ox = r % p.L.Wo;
    const T* in = reinterpret_cast<const T*>(p.in) + (size_t)b * p.L.Cin * p.L.Hi * p.L.Wi + (size_t)oy * p.L.s * p.sy + (size_t)ox * p.L.s * p.sx;
    const float* wt = p.wt + (lane & 31);
    const int Cout = MT * 32;
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    for (int k = lane >> 5; k < K; k += 2) {
        const float bv = sc_ld(in, off[k]) * p.scale;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[(size_t)k * Cout + mt * 32], bv, acc[mt], 0, 0, 0);
    }
    if (pn >= p.P) return;
    float* out = p.out + (size_t)b * Cout * hw + r;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = acc_row(mt, i, lane);
            const float v = acc[mt][i] + p.bias[co];
            out[(size_t)co * hw] = RELU ? (v > 0.f ? v : 0.f) : v;
        }
}

struct ScDgrad {
    const float *g, *wd, *a;     // the gradient of the layer's output (B, Cout, Ho, Wo), the pack, the layer's saved input (B, Cin, Hi, Wi)
    float* gin;                  // the gated gradient of the layer's input
    ScLayer L;
    int sh;                      // log2 of the stride
    int P;                       // B * Hi * Wi
};

template <int MT>
__global__ __launch_bounds__(256) void sc_dgrad_kernel(ScDgrad p) {
    __shared__ int tab[kScMaxK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = p.L.kw * p.L.kw, K = p.L.Cout * kk, ohw = p.L.Ho * p.L.Wo;
    for (int k = tid; k < K; k += 256) {
        const int co = k / kk, r = k % kk;
        tab[k] = co * ohw | (r / p.L.kw) << 24 | (r % p.L.kw) << 28;        // co * ohw < 2^24: checked by the launcher
    }
    __syncthreads();
    const int n0 = (blockIdx.x * 4 + wave) * 32;
    if (n0 >= p.P) return;
    const int hw = p.L.Hi * p.L.Wi;
    const int pn = n0 + (lane & 31), pc = pn < p.P ? pn : p.P - 1;
    const int b = pc / hw, r = pc % hw, y = r / p.L.Wi, x = r % p.L.Wi;
    const float* g = p.g + (size_t)b * p.L.Cout * ohw;
    const float* wd = p.wd + (lane & 31);
    const int Cin = MT * 32, m = p.L.s - 1;
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    for (int k = lane >> 5; k < K; k += 2) {
        const int t = tab[k], ty = y - (t >> 24 & 15), tx = x - (t >> 28 & 15), oy = ty >> p.sh, ox = tx >> p.sh;
        const bool ok = ty >= 0 && tx >= 0 && !(ty & m) && !(tx & m) && oy < p.L.Ho && ox < p.L.Wo;
        const float bv = ok ? g[(t & 0xffffff) + oy * p.L.Wo + ox] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wd[(size_t)k * Cin + mt * 32], bv, acc[mt], 0, 0, 0);
    }
    if (pn >= p.P) return;
    const size_t o = (size_t)b * Cin * hw + r;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const size_t idx = o + (size_t)acc_row(mt, i, lane) * hw;
            p.gin[idx] = p.a[idx] > 0.f ? acc[mt][i] : 0.f;
        }
}

struct ScWgrad {
    const void* in;
    const float* g;              // the gradient of the layer's output (B, Cout, Ho, Wo)
    float* part;                 // [chunk][Cout][K]
    ScLayer L;
    int sc, sy, sx;
    float scale;
    int P, chunk;                // B * Ho * Wo, pixels per workgroup
};

template <typename T, int MT>
__global__ __launch_bounds__(256) void sc_wgrad_kernel(ScWgrad p) {
    __shared__ int inb[kScChunkMax], gb[kScChunkMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = p.L.kw * p.L.kw, K = p.L.Cin * kk, hw = p.L.Ho * p.L.Wo, Cout = MT * 32;
    const int p0 = blockIdx.y * p.chunk, np = p.P - p0 < p.chunk ? p.P - p0 : p.chunk;
    for (int i = tid; i < p.chunk; i += 256) {
        int ib = 0, g = -1;
        if (i < np) {
            const int q = p0 + i, b = q / hw, r = q % hw;
            ib = b * p.L.Cin * p.L.Hi * p.L.Wi + (r / p.L.Wo) * p.L.s * p.sy + (r % p.L.Wo) * p.L.s * p.sx;
            g = b * Cout * hw + r;
        }
        inb[i] = ib, gb[i] = g;
    }
    __syncthreads();
    const int n = (blockIdx.x * 4 + wave) * 32 + (lane & 31);
    if (n - (lane & 31) >= K) return;                                    // K is a multiple of 32
    const int ci = n / kk, r = n % kk, off = ci * p.sc + (r / p.L.kw) * p.sy + (r % p.L.kw) * p.sx;
    const T* in = reinterpret_cast<const T*>(p.in) + off;
    const float* g = p.g + (size_t)(lane & 31) * hw;
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    const int np2 = (np + 1) & ~1;                                       // chunk is even, so np2 <= chunk
    for (int i = lane >> 5; i < np2; i += 2) {
        const int gi = gb[i];
        const float bv = sc_ld(in, inb[i]) * p.scale;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(gi >= 0 ? g[gi + (size_t)mt * 32 * hw] : 0.f, bv, acc[mt], 0, 0, 0);
    }
    float* part = p.part + (size_t)blockIdx.y * Cout * K + n;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) part[(size_t)acc_row(mt, i, lane) * K] = acc[mt][i];
}

// out[i] = the chunks' shares of element i in chunk order
__global__ void sc_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int nchunk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += part[(size_t)c * n + i];
    out[i] = s;
}

// db[co] = the sum of g (B, Cout, hw) over samples and pixels: a workgroup per channel, thread t adds elements t, t + 256, ... in order, then a
// fixed tree over the 256 threads
__global__ __launch_bounds__(256) void sc_bias_kernel(const float* __restrict__ g, float* __restrict__ db, int B, int Cout, int hw) {
    __shared__ float red[256];
    const int tid = threadIdx.x, co = blockIdx.x;
    float s = 0.f;
    const int P = B * hw;
    for (int q = tid; q < P; q += 256) s += g[((size_t)(q / hw) * Cout + co) * hw + q % hw];
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) db[co] = red[0];
}

template <typename T>
hipError_t sc_fwd_t(const SimpleCnnTrainArgs& t, const ScGeom& g, const ScWork& w, hipStream_t s) {
    const float* bias[3] = {t.b1, t.b2, t.b3};
    float* out[3] = {t.work + w.a1, t.work + w.a2, t.y};
    const void* in[3] = {t.x, t.work + w.a1, t.work + w.a2};
    for (int l = 0; l < 3; ++l) {
        const ScLayer& L = g.L[l];
        ScFwd p;
        p.in = in[l]; p.wt = t.work + w.wt[l]; p.bias = bias[l]; p.out = out[l]; p.L = L;
        if (l == 0) p.sc = 1, p.sy = L.Wi * L.Cin, p.sx = L.Cin, p.scale = t.scale;           // the frame is (B, H, W, Cin)
        else p.sc = L.Hi * L.Wi, p.sy = L.Wi, p.sx = 1, p.scale = 1.f;
        p.P = g.B * L.Ho * L.Wo;
        const dim3 grid((p.P + 127) / 128), block(256);
        if (l == 0) hipLaunchKernelGGL((sc_fwd_kernel<T, 1, true>), grid, block, 0, s, p);
        else if (l == 1) hipLaunchKernelGGL((sc_fwd_kernel<float, 2, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((sc_fwd_kernel<float, 1, false>), grid, block, 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T, int MT>
hipError_t sc_wgrad_t(const void* in, const float* gout, float* part, float* dW, float* db, const ScLayer& L, bool frame, float scale, int B, hipStream_t s) {
    ScWgrad p;
    p.in = in; p.g = gout; p.part = part; p.L = L;
    if (frame) p.sc = 1, p.sy = L.Wi * L.Cin, p.sx = L.Cin, p.scale = scale;
    else p.sc = L.Hi * L.Wi, p.sy = L.Wi, p.sx = 1, p.scale = 1.f;
    p.P = B * L.Ho * L.Wo;
    p.chunk = sc_chunk((size_t)p.P);
    const int nchunk = (p.P + p.chunk - 1) / p.chunk, K = L.K(), n = L.Cout * K;
    hipLaunchKernelGGL((sc_wgrad_kernel<T, MT>), dim3((K / 32 + 3) / 4, nchunk), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sc_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, dW, n, nchunk);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sc_bias_kernel, dim3(L.Cout), dim3(256), 0, s, gout, db, B, L.Cout, L.Ho * L.Wo);
    return hipGetLastError();
}

}  // namespace

// every element offset of a call fits an int (with room: the weight gradient's grid has a chunk of pixels per y index), and conv2's data-gradient table holds co * h2 * w2 in 24 bits
bool simplecnn_train_ok(int B, int H, int W, int Cin) {
    if (B < 0 || H < 36 || W < 36 || (Cin != 1 && Cin != 3)) return false;
    const ScGeom g = sc_geom(B > 0 ? B : 1, H, W, Cin);
    if ((size_t)64 * g.L[1].Ho * g.L[1].Wo >= ((size_t)1 << 24)) return false;
    return (size_t)g.B * H * W * Cin < ((size_t)1 << 31) && (size_t)g.B * 32 * g.L[0].Ho * g.L[0].Wo < ((size_t)1 << 30);
}

size_t simplecnn_train_work_floats(int B, int H, int W, int Cin) { return sc_work(sc_geom(B, H, W, Cin)).total; }

hipError_t launch_simplecnn_train_fwd(const SimpleCnnTrainArgs& t, hipStream_t s) {
    if (!simplecnn_train_ok(t.B, t.H, t.W, t.Cin)) return hipErrorInvalidValue;
    if (t.B == 0) return hipSuccess;
    const ScGeom g = sc_geom(t.B, t.H, t.W, t.Cin);
    const ScWork w = sc_work(g);
    const float* W[3] = {t.w1, t.w2, t.w3};
    for (int l = 0; l < 3; ++l) {
        const int n = g.L[l].K() * g.L[l].Cout;
        hipLaunchKernelGGL(sc_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, W[l], t.work + w.wt[l], g.L[l].Cout, g.L[l].Cin, g.L[l].kw * g.L[l].kw, 0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return t.x_u8 ? sc_fwd_t<uint8_t>(t, g, w, s) : sc_fwd_t<float>(t, g, w, s);
}

hipError_t launch_simplecnn_train_bwd(const SimpleCnnTrainArgs& t, hipStream_t s) {
    if (!simplecnn_train_ok(t.B, t.H, t.W, t.Cin)) return hipErrorInvalidValue;
    const ScGeom g = sc_geom(t.B > 0 ? t.B : 1, t.H, t.W, t.Cin);
    if (t.B == 0) {
        // no rows: the sums are empty
        float* out[6] = {t.d_w1, t.d_b1, t.d_w2, t.d_b2, t.d_w3, t.d_b3};
        const size_t n[6] = {(size_t)32 * g.L[0].K(), 32, (size_t)64 * g.L[1].K(), 64, (size_t)32 * g.L[2].K(), 32};
        for (int i = 0; i < 6; ++i) {
            const hipError_t e = hipMemsetAsync(out[i], 0, n[i] * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    const ScWork w = sc_work(g);
    float *a1 = t.work + w.a1, *a2 = t.work + w.a2, *g1 = t.work + w.g1, *g2 = t.work + w.g2, *part = t.work + w.part;
    hipError_t e;
    // conv3: weight gradient from d_y and a2, then the gated gradient of a2
    if ((e = sc_wgrad_t<float, 1>(a2, t.d_y, part, t.d_w3, t.d_b3, g.L[2], false, 1.f, t.B, s)) != hipSuccess) return e;
    {
        const ScLayer& L = g.L[2];
        const int n = L.K() * L.Cout;
        hipLaunchKernelGGL(sc_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t.w3, t.work + w.wd[0], L.Cout, L.Cin, L.kw * L.kw, 1);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        ScDgrad p;
        p.g = t.d_y; p.wd = t.work + w.wd[0]; p.a = a2; p.gin = g2; p.L = L; p.sh = 0; p.P = t.B * L.Hi * L.Wi;
        hipLaunchKernelGGL(sc_dgrad_kernel<2>, dim3((p.P + 127) / 128), dim3(256), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // conv2
    if ((e = sc_wgrad_t<float, 2>(a1, g2, part, t.d_w2, t.d_b2, g.L[1], false, 1.f, t.B, s)) != hipSuccess) return e;
    {
        const ScLayer& L = g.L[1];
        const int n = L.K() * L.Cout;
        hipLaunchKernelGGL(sc_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t.w2, t.work + w.wd[1], L.Cout, L.Cin, L.kw * L.kw, 1);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        ScDgrad p;
        p.g = g2; p.wd = t.work + w.wd[1]; p.a = a1; p.gin = g1; p.L = L; p.sh = 1; p.P = t.B * L.Hi * L.Wi;
        hipLaunchKernelGGL(sc_dgrad_kernel<1>, dim3((p.P + 127) / 128), dim3(256), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // conv1: the frame has no gradient
    return t.x_u8 ? sc_wgrad_t<uint8_t, 1>(t.x, g1, part, t.d_w1, t.d_b1, g.L[0], true, t.scale, t.B, s)
                  : sc_wgrad_t<float, 1>(t.x, g1, part, t.d_w1, t.d_b1, g.L[0], true, t.scale, t.B, s);
}

}  // namespace hcm
