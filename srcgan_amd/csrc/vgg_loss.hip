// Kernels of the frozen VGG feature path (losses.VGG16Loss / losses.PerceptionLoss, reference src/losses.py:344-393, 455-470):
// nn.MaxPool2d(2, 2) and its gradient on NHWC, and the L1 / MSE feature distance between two NHWC tensors with its gradient.
// All four are HBM-bound: a thread moves 16-byte pieces of consecutive channels (8 bf16 / f16 or 4 f32); operands whose channel
// stride or base address is not a multiple of 16 bytes take the same kernels one element at a time.
#include "common.h"

namespace {

template <typename T, int V> struct alignas(sizeof(T) * V) Pk { T v[V]; };
template <typename T> constexpr int pk_width() { return 16 / (int)sizeof(T); }

static inline int vl_blocks(long n) {
    long b = cdivl(n, 256);
    return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
static inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

__device__ __forceinline__ float vl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------ MaxPool2d(2, 2), ceil_mode = False
// one thread: V channels of one output pixel
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_k(const T* __restrict__ src, int s_cs, T* __restrict__ dst, int d_cs,
                                                  int H, int W, int OH, int OW, int npc, long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int pc = (int)(e % npc);
        long r = e / npc;
        const int ox = (int)(r % OW); r /= OW;
        const int oy = (int)(r % OH);
        const long b = r / OH;
        const T* s0 = src + (((size_t)b * H + 2 * oy) * W + 2 * ox) * s_cs + pc * V;
        const Pk<T, V> x00 = *(const Pk<T, V>*)s0, x01 = *(const Pk<T, V>*)(s0 + s_cs);
        const Pk<T, V> x10 = *(const Pk<T, V>*)(s0 + (size_t)W * s_cs), x11 = *(const Pk<T, V>*)(s0 + (size_t)W * s_cs + s_cs);
        Pk<T, V> o;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float m = to_f(x00.v[i]);
            const float b1 = to_f(x01.v[i]), b2 = to_f(x10.v[i]), b3 = to_f(x11.v[i]);
            if (b1 > m) m = b1;
            if (b2 > m) m = b2;
            if (b3 > m) m = b3;
            o.v[i] = from_f<T>(m);
        }
        *(Pk<T, V>*)(dst + (((size_t)b * OH + oy) * OW + ox) * d_cs + pc * V) = o;
    }
}

// Gradient: one thread owns V channels of one 2x2 cell of the INPUT grid (cells cover the odd last row / column too), so every
// element of dx is written exactly once.  The argmax is recomputed from x: the first maximum in row-major order wins (strict >).
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_bwd_k(const T* __restrict__ dy, int dy_cs, const T* __restrict__ x, int x_cs,
                                                      T* __restrict__ dx, int dx_cs, int H, int W, int OH, int OW, int CH, int CW,
                                                      int npc, int relu_mask, long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int pc = (int)(e % npc);
        long r = e / npc;
        const int cx = (int)(r % CW); r /= CW;
        const int cy = (int)(r % CH);
        const long b = r / CH;
        const size_t p00 = ((size_t)b * H + 2 * cy) * W + 2 * cx;
        Pk<T, V> zero;
#pragma unroll
        for (int i = 0; i < V; ++i) zero.v[i] = from_f<T>(0.f);
        if (cy < OH && cx < OW) {
            const T* s0 = x + p00 * x_cs + pc * V;
            Pk<T, V> xv[4];
            xv[0] = *(const Pk<T, V>*)s0; xv[1] = *(const Pk<T, V>*)(s0 + x_cs);
            xv[2] = *(const Pk<T, V>*)(s0 + (size_t)W * x_cs); xv[3] = *(const Pk<T, V>*)(s0 + (size_t)W * x_cs + x_cs);
            const Pk<T, V> g = *(const Pk<T, V>*)(dy + (((size_t)b * OH + cy) * OW + cx) * dy_cs + pc * V);
            Pk<T, V> o[4] = {zero, zero, zero, zero};
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float m = to_f(xv[0].v[i]);
                int am = 0;
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const float v = to_f(xv[q].v[i]);
                    if (v > m) { m = v; am = q; }
                }
                const bool keep = !relu_mask || m > 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q == am && keep) o[q].v[i] = g.v[i];
            }
            T* d0 = dx + p00 * dx_cs + pc * V;
            *(Pk<T, V>*)d0 = o[0]; *(Pk<T, V>*)(d0 + dx_cs) = o[1];
            *(Pk<T, V>*)(d0 + (size_t)W * dx_cs) = o[2]; *(Pk<T, V>*)(d0 + (size_t)W * dx_cs + dx_cs) = o[3];
        } else {       // the row / column that floor pooling drops: zeros
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int yy = 2 * cy + (q >> 1), xx = 2 * cx + (q & 1);
                if (yy < H && xx < W) *(Pk<T, V>*)(dx + (((size_t)b * H + yy) * W + xx) * dx_cs + pc * V) = zero;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ feature distance
// KIND 0: |a - b|, 1: (a - b)^2.  An item is V channels of a pixel; the last item of a pixel may be partial (C % V != 0).
template <typename T, int V, int KIND>
__global__ __launch_bounds__(256) void feat_loss_fwd_k(const T* __restrict__ a, int a_cs, const T* __restrict__ b, int b_cs,
                                                       int C, int npc, long total, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c0 = (int)(e % npc) * V;
        const size_t pix = (size_t)(e / npc);
        const T* ap = a + pix * a_cs + c0;
        const T* bp = b + pix * b_cs + c0;
        if (c0 + V <= C) {
            const Pk<T, V> av = *(const Pk<T, V>*)ap, bv = *(const Pk<T, V>*)bp;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float d = to_f(av.v[i]) - to_f(bv.v[i]);
                s += KIND == 0 ? fabsf(d) : d * d;
            }
        } else {
            for (int i = 0; c0 + i < C; ++i) {
                const float d = to_f(ap[i]) - to_f(bp[i]);
                s += KIND == 0 ? fabsf(d) : d * d;
            }
        }
    }
    s = vl_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void feat_loss_final_k(const float* __restrict__ partial, int nblk, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
    s = vl_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

template <int KIND> __device__ __forceinline__ float feat_grad(float d) {
    if (KIND == 0) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    return 2.f * d;
}

template <typename T, int V, int KIND>
__global__ __launch_bounds__(256) void feat_loss_bwd_k(const T* __restrict__ a, int a_cs, const T* __restrict__ b, int b_cs,
                                                       T* __restrict__ g, int g_cs, int accumulate, float scale, int C, int npc, long total) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c0 = (int)(e % npc) * V;
        const size_t pix = (size_t)(e / npc);
        const T* ap = a + pix * a_cs + c0;
        const T* bp = b + pix * b_cs + c0;
        T* gp = g + pix * g_cs + c0;
        if (c0 + V <= C) {
            const Pk<T, V> av = *(const Pk<T, V>*)ap, bv = *(const Pk<T, V>*)bp;
            Pk<T, V> gv;
            if (accumulate) gv = *(const Pk<T, V>*)gp;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float v = scale * feat_grad<KIND>(to_f(av.v[i]) - to_f(bv.v[i]));
                gv.v[i] = from_f<T>(accumulate ? to_f(gv.v[i]) + v : v);
            }
            *(Pk<T, V>*)gp = gv;
        } else {
            for (int i = 0; c0 + i < C; ++i) {
                const float v = scale * feat_grad<KIND>(to_f(ap[i]) - to_f(bp[i]));
                gp[i] = from_f<T>(accumulate ? to_f(gp[i]) + v : v);
            }
        }
    }
}

// loss = sum_k sums[k] * w[k], k ascending
struct VlWeights { float w[4]; };
__global__ void vgg_combine_k(const float* __restrict__ sums, VlWeights w, int n, float* __restrict__ out) {
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += sums[k] * w.w[k];
    *out = s;
}

// ------------------------------------------------------------------------------------------ frames of a 5-D tensor as images
// Frames [f0, f0 + k) of a contiguous f32 [Bt, Cin, F, H, W] tensor <-> the 8-channel NHWC records of Bt * k images (image n = j * Bt + b
// is frame f0 + j of sample b).  Plane (b, c) of frame f starts at element ((b * Cin + c) * F + f) * HW, in 64 bits.  Both passes are
// HBM-bound: a thread owns V consecutive pixels of one image -- one 16-byte load / store per channel plane when V = 4 (HW % 4 == 0, so
// every plane base keeps the tensor's 16-byte alignment), one element at a time when V = 1 -- and moves whole records in 16-byte pieces.
template <typename T, int V>
__global__ __launch_bounds__(256) void frames_pack_k(const float* __restrict__ src, T* __restrict__ dst, int Bt, int Cin, int F, int f0,
                                                     long HW, long total) {
    constexpr int PW = pk_width<T>();
    const long npv = HW / V;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long n = e / npv, p = (e % npv) * V;
        const long b = n % Bt, j = n / Bt;
        Pk<float, V> x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < Cin) x[c] = *(const Pk<float, V>*)(src + (((size_t)b * Cin + c) * F + f0 + j) * HW + p);
        if (Cin == 1) { x[1] = x[0]; x[2] = x[0]; }       // losses.py:378-380, the reference's torch.cat of three copies
        T* d = dst + ((size_t)n * HW + p) * 8;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            Pk<T, PW> r[8 / PW];
#pragma unroll
            for (int q = 0; q < 8; ++q) r[q / PW].v[q % PW] = from_f<T>(q < 3 ? x[q].v[i] : 0.f);
#pragma unroll
            for (int h = 0; h < 8 / PW; ++h) *(Pk<T, PW>*)(d + i * 8 + h * PW) = r[h];
        }
    }
}

// the input gradient back onto those frames, times gout[0] * gscale; every element of the k frames is written once
template <typename T, int V>
__global__ __launch_bounds__(256) void frames_grad_store_k(const T* __restrict__ src, float* __restrict__ dst, int Bt, int Cin, int F, int f0,
                                                           long HW, long total, const float* __restrict__ gout, float gscale) {
    constexpr int PW = pk_width<T>();      // >= 4: the first piece of a record holds the three channels
    const float f = gout[0] * gscale;
    const long npv = HW / V;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long n = e / npv, p = (e % npv) * V;
        const long b = n % Bt, j = n / Bt;
        const T* s = src + ((size_t)n * HW + p) * 8;
        Pk<float, V> g[3];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const Pk<T, PW> r = *(const Pk<T, PW>*)(s + i * 8);
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c].v[i] = to_f(r.v[c]) * f;
        }
        if (Cin == 1) {
#pragma unroll
            for (int i = 0; i < V; ++i) g[0].v[i] = (g[0].v[i] + g[1].v[i]) + g[2].v[i];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < Cin) *(Pk<float, V>*)(dst + (((size_t)b * Cin + c) * F + f0 + j) * HW + p) = g[c];
    }
}

#define VL_DISPATCH(dtype, vec, ...) \
    if ((dtype) == SRCGAN_F32) { using T = float; if (vec) { constexpr int V = 4; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } \
    else if ((dtype) == SRCGAN_BF16) { using T = __bf16; if (vec) { constexpr int V = 8; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } \
    else if ((dtype) == SRCGAN_F16) { using T = _Float16; if (vec) { constexpr int V = 8; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } \
    else SG_FAIL("bad dtype %d", (int)(dtype));

#define DISPATCH_T(dtype, ...) \
    if ((dtype) == SRCGAN_F32) { using T = float; __VA_ARGS__; } \
    else if ((dtype) == SRCGAN_BF16) { using T = __bf16; __VA_ARGS__; } \
    else if ((dtype) == SRCGAN_F16) { using T = _Float16; __VA_ARGS__; } \
    else SG_FAIL("bad dtype %d", (int)(dtype));

static inline int vl_width(int dtype) { return dtype == SRCGAN_F32 ? 4 : 8; }

}  // namespace

extern "C" int srcgan_maxpool2_nhwc(const void* src, int s_cs, void* dst, int d_cs, int B, int H, int W, int C, int dtype, void* stream) {
    SG_REQUIRE(src && dst && B > 0 && H >= 2 && W >= 2 && C > 0 && s_cs >= C && d_cs >= C, "srcgan_maxpool2_nhwc: bad arguments");
    SG_REQUIRE(sg_dtype_ok(dtype), "srcgan_maxpool2_nhwc: bad dtype %d", dtype);
    const int w = vl_width(dtype), OH = H / 2, OW = W / 2;
    const bool vec = C % w == 0 && s_cs % w == 0 && d_cs % w == 0 && al16(src) && al16(dst);
    const int npc = vec ? C / w : C;
    const long total = (long)B * OH * OW * npc;
    VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((maxpool2_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, (hipStream_t)stream,
                                               (const T*)src, s_cs, (T*)dst, d_cs, H, W, OH, OW, npc, total));
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_maxpool2_bwd_nhwc(const void* dy, int dy_cs, const void* x, int x_cs, void* dx, int dx_cs, int B, int H, int W, int C,
                                        int relu_mask, int dtype, void* stream) {
    SG_REQUIRE(dy && x && dx && B > 0 && H >= 2 && W >= 2 && C > 0 && dy_cs >= C && x_cs >= C && dx_cs >= C, "srcgan_maxpool2_bwd_nhwc: bad arguments");
    SG_REQUIRE(sg_dtype_ok(dtype), "srcgan_maxpool2_bwd_nhwc: bad dtype %d", dtype);
    const int w = vl_width(dtype), OH = H / 2, OW = W / 2, CH = (H + 1) / 2, CW = (W + 1) / 2;
    const bool vec = C % w == 0 && dy_cs % w == 0 && x_cs % w == 0 && dx_cs % w == 0 && al16(dy) && al16(x) && al16(dx);
    const int npc = vec ? C / w : C;
    const long total = (long)B * CH * CW * npc;
    VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((maxpool2_bwd_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, (hipStream_t)stream,
                                               (const T*)dy, dy_cs, (const T*)x, x_cs, (T*)dx, dx_cs, H, W, OH, OW, CH, CW, npc, relu_mask != 0, total));
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_feat_loss_fwd(int kind, const void* a, int a_cs, const void* b, int b_cs, long npix, int C, int dtype,
                                    float* out_sum, float* scratch, void* stream) {
    SG_REQUIRE(a && b && out_sum && scratch && npix > 0 && C > 0 && a_cs >= C && b_cs >= C && (kind == 0 || kind == 1), "srcgan_feat_loss_fwd: bad arguments");
    SG_REQUIRE(sg_dtype_ok(dtype), "srcgan_feat_loss_fwd: bad dtype %d", dtype);
    const int w = vl_width(dtype);
    const bool vec = a_cs % w == 0 && b_cs % w == 0 && al16(a) && al16(b);
    const int npc = vec ? cdiv(C, w) : C;
    const long total = npix * npc;
    // the grid is a function of the sizes alone: the same inputs are summed in the same order on every run
    long nb = cdivl(total, 256);
    const long cap = srcgan_loss_scratch_floats();
    if (nb > cap) nb = cap;
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) { VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((feat_loss_fwd_k<T, V, 0>), dim3((int)nb), dim3(256), 0, st, (const T*)a, a_cs, (const T*)b, b_cs, C, npc, total, scratch)); }
    else { VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((feat_loss_fwd_k<T, V, 1>), dim3((int)nb), dim3(256), 0, st, (const T*)a, a_cs, (const T*)b, b_cs, C, npc, total, scratch)); }
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(feat_loss_final_k, dim3(1), dim3(256), 0, st, scratch, (int)nb, out_sum);
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_feat_loss_bwd(int kind, const void* a, int a_cs, const void* b, int b_cs, void* g, int g_cs, int accumulate, float scale,
                                    long npix, int C, int dtype, void* stream) {
    SG_REQUIRE(a && b && g && npix > 0 && C > 0 && a_cs >= C && b_cs >= C && g_cs >= C && (kind == 0 || kind == 1), "srcgan_feat_loss_bwd: bad arguments");
    SG_REQUIRE(sg_dtype_ok(dtype), "srcgan_feat_loss_bwd: bad dtype %d", dtype);
    const int w = vl_width(dtype);
    const bool vec = a_cs % w == 0 && b_cs % w == 0 && g_cs % w == 0 && al16(a) && al16(b) && al16(g);
    const int npc = vec ? cdiv(C, w) : C;
    const long total = npix * npc;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate != 0;
    if (kind == 0) { VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((feat_loss_bwd_k<T, V, 0>), dim3(vl_blocks(total)), dim3(256), 0, st, (const T*)a, a_cs, (const T*)b, b_cs, (T*)g, g_cs, acc, scale, C, npc, total)); }
    else { VL_DISPATCH(dtype, vec, hipLaunchKernelGGL((feat_loss_bwd_k<T, V, 1>), dim3(vl_blocks(total)), dim3(256), 0, st, (const T*)a, a_cs, (const T*)b, b_cs, (T*)g, g_cs, acc, scale, C, npc, total)); }
    SG_LAUNCH_CHECK();
    return 0;
}

int sg_vgg_combine(const float* sums, const float* weights, int n, float* out, hipStream_t st) {
    SG_REQUIRE(sums && weights && out && n >= 1 && n <= 4, "sg_vgg_combine: bad arguments");
    VlWeights w = {{0.f, 0.f, 0.f, 0.f}};
    for (int k = 0; k < n; ++k) w.w[k] = weights[k];
    hipLaunchKernelGGL(vgg_combine_k, dim3(1), dim3(1), 0, st, sums, w, n, out);
    SG_LAUNCH_CHECK();
    return 0;
}

static int frames_check(const char* who, const void* a, const void* b, int cs, int Bt, SgFrames fr, int H, int W) {
    SG_REQUIRE(a && b && Bt > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    SG_REQUIRE(cs == 8, "%s: records of 8 channels expected, got %d", who, cs);
    SG_REQUIRE(fr.Cin == 1 || fr.Cin == 3, "%s: frames must have 1 or 3 channels, got %d", who, fr.Cin);
    SG_REQUIRE(fr.F > 0 && fr.k > 0 && fr.f0 >= 0 && fr.f0 <= fr.F - fr.k, "%s: frames [%d, %d + %d) leave the %d frames of the tensor", who, fr.f0, fr.f0, fr.k, fr.F);
    SG_REQUIRE(al16(b), "%s: the record buffer must be 16-byte aligned", who);
    return 0;
}

int sg_frames_pack(const float* src5d, void* dst, int cs, int Bt, SgFrames fr, int H, int W, int dtype, hipStream_t st) {
    SG_TRY(frames_check("sg_frames_pack", src5d, dst, cs, Bt, fr, H, W));
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(src5d);
    const long total = (long)Bt * fr.k * (vec ? HW / 4 : HW);
    if (vec) { constexpr int V = 4; DISPATCH_T(dtype, hipLaunchKernelGGL((frames_pack_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, st, src5d, (T*)dst, Bt, fr.Cin, fr.F, fr.f0, HW, total)); }
    else { constexpr int V = 1; DISPATCH_T(dtype, hipLaunchKernelGGL((frames_pack_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, st, src5d, (T*)dst, Bt, fr.Cin, fr.F, fr.f0, HW, total)); }
    SG_LAUNCH_CHECK();
    return 0;
}

int sg_frames_grad_store(const void* src, int cs, float* dst5d, int Bt, SgFrames fr, int H, int W, const float* gout, float gscale, int dtype, hipStream_t st) {
    SG_TRY(frames_check("sg_frames_grad_store", dst5d, src, cs, Bt, fr, H, W));
    SG_REQUIRE(gout, "sg_frames_grad_store: null upstream gradient");
    const long HW = (long)H * W;
    const bool vec = HW % 4 == 0 && al16(dst5d);
    const long total = (long)Bt * fr.k * (vec ? HW / 4 : HW);
    if (vec) { constexpr int V = 4; DISPATCH_T(dtype, hipLaunchKernelGGL((frames_grad_store_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, st, (const T*)src, dst5d, Bt, fr.Cin, fr.F, fr.f0, HW, total, gout, gscale)); }
    else { constexpr int V = 1; DISPATCH_T(dtype, hipLaunchKernelGGL((frames_grad_store_k<T, V>), dim3(vl_blocks(total)), dim3(256), 0, st, (const T*)src, dst5d, Bt, fr.Cin, fr.F, fr.f0, HW, total, gout, gscale)); }
    SG_LAUNCH_CHECK();
    return 0;
}
