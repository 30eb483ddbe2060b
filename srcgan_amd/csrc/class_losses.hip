// Classification-style losses of the reference's losses.py: the focal loss (FLoss, :296-341), binary cross-entropy against a target tensor
// and multi-class cross-entropy against the arg-max of a one-hot target (CELoss, :150-167), the batch range (ConLoss, :258-274) and the
// L1 between a tensor and the other tensor shifted by one sample (CrossLoss, :277-293).
//
// Every forward is one pass over its inputs into per-block partial sums (per-thread running sum, wave shuffles, eight waves added in a fixed
// order) and one single-block pass over the partials in a fixed order: no atomics, the same bits on every call.  Every backward is one
// pass that writes each element of the gradient exactly once (zeros included), scaled by the upstream gradient read from device memory.
// Flat kernels use 16-byte accesses over the part of the range where all their pointers share one 16-byte phase (a scalar head and tail
// around it) and 4-byte accesses for everything when the phases differ (CrossLoss with S % 4 != 0); the column kernels use 16-byte
// accesses when the row length is a multiple of 4 and the bases are aligned, 4-byte accesses otherwise.  Counts are 64-bit.
#include "common.h"

#define CL_FWD_BLOCKS 1024       // <= srcgan_loss_scratch_floats(): one partial per block
#define CL_FWD_THREADS 512       // 1024 blocks of 512 threads: as many threads in flight as the backward's 2048 blocks of 256
#define CL_BWD_BLOCKS 2048
#define CL_BWD_THREADS 256

__device__ __forceinline__ float cl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// a block of CL_FWD_THREADS: eight wave sums added in a fixed order
__device__ __forceinline__ void cl_block_partial(float s, float* __restrict__ partial) {
    __shared__ float red[CL_FWD_THREADS / 64];
    s = cl_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

__global__ __launch_bounds__(256) void cl_final_k(const float* __restrict__ partial, int nblk, float scale, float* out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
    s = cl_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

// the head / 16-byte body / tail split of a flat range: common.h's SgSpan, shared with the mean losses of elementwise.hip
static int cl_blocks(long items, int cap, int threads) {
    const long b = cdivl(items, threads);
    return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}
static int cl_span_blocks(const SgSpan& s, int cap, int threads) { return cl_blocks(s.nv + (s.n - 4 * s.nv), cap, threads); }

// ------------------------------------------------------------------------------------------------ element-wise terms
// Focal loss on o = clamp(x, lo, hi), lo = (float)1e-6, hi = (float)(1.0 - 1e-6) (torch.clamp's float32 bounds; a NaN stays a NaN):
//   binary:  l = -0.9 (1-o)^g t log o - 0.1 o^g (1-t) log(1-o)        otherwise:  l = -(1-o)^g t log o
// Powers: ig >= 0 is an integer exponent taken by repeated multiplication (g = 2: one product); ig < 0 builds b^g = exp(g log b) from the
// logarithm the term needs anyway and b^(g-1) = b^g / b.  No powf.
struct ClFocal {
    int binary, ig;
    float gamma;
    __device__ __forceinline__ void powers(float b, float logb, float& p, float& pm1) const {
        if (ig >= 0) {
            pm1 = 1.f;
            for (int k = 1; k < ig; ++k) pm1 *= b;
            p = ig > 0 ? pm1 * b : 1.f;
        } else {
            p = expf(gamma * logb);
            pm1 = p / b;
        }
    }
    __device__ __forceinline__ float fwd(float x, float t) const {
        const float lo = (float)1e-6, hi = (float)(1.0 - 1e-6);
        const float o = x < lo ? lo : (x > hi ? hi : x);
        const float om = 1.f - o, lg = logf(o);
        float p1, q;
        if (binary) {
            const float l1 = logf(om);
            float p0;
            powers(om, l1, p1, q);
            powers(o, lg, p0, q);
            return (-0.9f * p1) * (t * lg) - (0.1f * p0) * ((1.f - t) * l1);
        }
        powers(om, ig < 0 ? logf(om) : 0.f, p1, q);
        return -p1 * (t * lg);
    }
    __device__ __forceinline__ float bwd(float x, float t) const {      // d l / d x: clamp passes the gradient where lo <= x <= hi only
        const float lo = (float)1e-6, hi = (float)(1.0 - 1e-6);
        if (!(x >= lo && x <= hi)) return 0.f;
        const float o = x, om = 1.f - o, lg = logf(o);
        float p1, p1m;
        if (binary) {
            const float l1 = logf(om);
            float p0, p0m;
            powers(om, l1, p1, p1m);
            powers(o, lg, p0, p0m);
            return (0.9f * t) * (gamma * p1m * lg - p1 / o) + (0.1f * (1.f - t)) * (p0 / om - gamma * p0m * l1);
        }
        powers(om, ig < 0 ? logf(om) : 0.f, p1, p1m);
        return t * (gamma * p1m * lg - p1 / o);
    }
};

// nn.BCELoss: -(t max(log o, -100) + (1-t) max(log(1-o), -100)); gradient (o - t) / max(o (1-o), 1e-12).  No range check: a logarithm of
// a negative number is a NaN and stays one (the comparisons below do not replace it).
struct ClBce {
    __device__ __forceinline__ float fwd(float o, float t) const {
        float a = logf(o), b = logf(1.f - o);
        a = a < -100.f ? -100.f : a;
        b = b < -100.f ? -100.f : b;
        return -(t * a + (1.f - t) * b);
    }
    __device__ __forceinline__ float bwd(float o, float t) const { return (o - t) / fmaxf((1.f - o) * o, 1e-12f); }
};

struct ClL1 {
    __device__ __forceinline__ float fwd(float a, float b) const { return fabsf(a - b); }
    __device__ __forceinline__ float bwd(float a, float b) const { const float d = a - b; return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
};

template <typename OP>
__global__ __launch_bounds__(CL_FWD_THREADS) void cl_flat_fwd_k(const float* __restrict__ a, const float* __restrict__ t, SgSpan sp, OP op,
                                                     float* __restrict__ partial) {
    float s = 0.f;
    sg_span_each(sp,
        [&](long e) {
            const f32x4 av = *(const f32x4*)(a + e), tv = *(const f32x4*)(t + e);
#pragma unroll
            for (int i = 0; i < 4; ++i) s += op.fwd(av[i], tv[i]);
        },
        [&](long e) { s += op.fwd(a[e], t[e]); });
    cl_block_partial(s, partial);
}

// da[e] = op.bwd * gout[0] * gscale over the span, then zeros over [sp.n, sp.n + nzero)
template <typename OP>
__global__ __launch_bounds__(256) void cl_flat_bwd_k(const float* __restrict__ a, const float* __restrict__ t, SgSpan sp, OP op,
                                                     const float* __restrict__ gout, float gscale, float* __restrict__ da, long nzero) {
    const float g = gout[0] * gscale;
    sg_span_each(sp,
        [&](long e) {
            const f32x4 av = *(const f32x4*)(a + e), tv = *(const f32x4*)(t + e);
            f32x4 d;
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = op.bwd(av[i], tv[i]) * g;
            *(f32x4*)(da + e) = d;
        },
        [&](long e) { da[e] = op.bwd(a[e], t[e]) * g; });
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nzero; i += (long)gridDim.x * blockDim.x) da[sp.n + i] = 0.f;
}

template <typename OP>
static int cl_flat_fwd(const char* what, const float* a, const float* t, long n, OP op, double scale, float* out, float* scratch, void* stream) {
    SG_REQUIRE(a && t && out && scratch && n > 0, "%s: bad arguments", what);
    SG_REQUIRE(srcgan_loss_scratch_floats() >= CL_FWD_BLOCKS, "%s: scratch too small", what);
    const SgSpan sp = sg_span(n, a, t);
    const int nb = cl_span_blocks(sp, CL_FWD_BLOCKS, CL_FWD_THREADS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cl_flat_fwd_k<OP>, dim3(nb), dim3(CL_FWD_THREADS), 0, st, a, t, sp, op, scratch);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl_final_k, dim3(1), dim3(256), 0, st, scratch, nb, (float)scale, out);
    SG_LAUNCH_CHECK();
    return 0;
}

template <typename OP>
static int cl_flat_bwd(const char* what, const float* a, const float* t, long n, OP op, const float* gout, float gscale, float* da,
                       long nzero, void* stream) {
    SG_REQUIRE(a && t && gout && da && n > 0 && nzero >= 0, "%s: bad arguments", what);
    const SgSpan sp = sg_span(n, a, t, da);
    hipLaunchKernelGGL(cl_flat_bwd_k<OP>, dim3(cl_span_blocks(sp, CL_BWD_BLOCKS, CL_BWD_THREADS)), dim3(CL_BWD_THREADS), 0, (hipStream_t)stream, a, t, sp, op, gout,
                       gscale, da, nzero);
    SG_LAUNCH_CHECK();
    return 0;
}

static ClFocal cl_focal_op(int binary, float gamma) {
    ClFocal op;
    op.binary = binary != 0;
    op.gamma = gamma;
    op.ig = (gamma >= 0.f && gamma <= 8.f && gamma == (float)(int)gamma) ? (int)gamma : -1;
    return op;
}

extern "C" int srcgan_focal_fwd(const float* output, const float* target, long n, int binary, float gamma, int mean, float* out,
                                float* scratch, void* stream) {
    SG_REQUIRE(gamma == gamma, "srcgan_focal_fwd: gamma is NaN");
    return cl_flat_fwd("srcgan_focal_fwd", output, target, n, cl_focal_op(binary, gamma), mean ? 1.0 / (double)n : 1.0, out, scratch, stream);
}

extern "C" int srcgan_focal_bwd(const float* output, const float* target, long n, int binary, float gamma, int mean, const float* gout,
                                float* doutput, void* stream) {
    SG_REQUIRE(gamma == gamma, "srcgan_focal_bwd: gamma is NaN");
    return cl_flat_bwd("srcgan_focal_bwd", output, target, n, cl_focal_op(binary, gamma), gout, mean ? 1.f / (float)n : 1.f, doutput, 0, stream);
}

extern "C" int srcgan_bce_fwd(const float* output, const float* target, long n, float* out, float* scratch, void* stream) {
    return cl_flat_fwd("srcgan_bce_fwd", output, target, n, ClBce(), 1.0 / (double)n, out, scratch, stream);
}

extern "C" int srcgan_bce_bwd(const float* output, const float* target, long n, const float* gout, float* doutput, void* stream) {
    return cl_flat_bwd("srcgan_bce_bwd", output, target, n, ClBce(), gout, 1.f / (float)n, doutput, 0, stream);
}

extern "C" int srcgan_cross_l1_fwd(const float* output, const float* target, int nb, long S, float* out, float* scratch, void* stream) {
    SG_REQUIRE(nb >= 2 && S > 0, "srcgan_cross_l1_fwd: needs nb >= 2 and S > 0, got nb = %d, S = %ld", nb, S);
    SG_REQUIRE(target, "srcgan_cross_l1_fwd: bad arguments");
    const long n = (long)(nb - 1) * S;
    return cl_flat_fwd("srcgan_cross_l1_fwd", output, target + S, n, ClL1(), 1.0 / (double)n, out, scratch, stream);
}

extern "C" int srcgan_cross_l1_bwd(const float* output, const float* target, int nb, long S, const float* gout, float* doutput, void* stream) {
    SG_REQUIRE(nb >= 2 && S > 0, "srcgan_cross_l1_bwd: needs nb >= 2 and S > 0, got nb = %d, S = %ld", nb, S);
    SG_REQUIRE(target, "srcgan_cross_l1_bwd: bad arguments");
    const long n = (long)(nb - 1) * S;
    return cl_flat_bwd("srcgan_cross_l1_bwd", output, target + S, n, ClL1(), gout, 1.f / (float)n, doutput, S, stream);
}

// ------------------------------------------------------------------------------------------------ column kernels
// x is [R, C, S]: a thread owns V consecutive positions s of one row r and walks the C planes (each plane read is coalesced along s).
template <int V> __device__ __forceinline__ void cl_load(const float* p, float (&v)[V]) {
    if constexpr (V == 4) load4<float>(p, v); else v[0] = *p;
}
template <int V> __device__ __forceinline__ void cl_store(float* p, const float (&v)[V]) {
    if constexpr (V == 4) store4<float>(p, v); else *p = v[0];
}

// first maximum over the C planes (strict >, lowest plane wins)
template <int V>
__device__ __forceinline__ void cl_argmax(const float* __restrict__ t, long base, int C, long S, int (&k)[V]) {
    float best[V];
    cl_load<V>(t + base, best);
#pragma unroll
    for (int i = 0; i < V; ++i) k[i] = 0;
    for (int c = 1; c < C; ++c) {
        float v[V];
        cl_load<V>(t + base + c * S, v);
#pragma unroll
        for (int i = 0; i < V; ++i) if (v[i] > best[i]) { best[i] = v[i]; k[i] = c; }
    }
}

template <int V>
__global__ __launch_bounds__(CL_FWD_THREADS) void cl_nll_fwd_k(const float* __restrict__ o, const float* __restrict__ t, int C, long S, long ngroups,
                                                    float* __restrict__ partial) {
    float s = 0.f;
    const long sg = S / V;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < ngroups; q += (long)gridDim.x * blockDim.x) {
        const long n = q / sg, base = n * C * S + (q - n * sg) * V;
        int k[V];
        cl_argmax<V>(t, base, C, S, k);
#pragma unroll
        for (int i = 0; i < V; ++i) s -= logf(o[base + k[i] * S + i]);
    }
    cl_block_partial(s, partial);
}

template <int V>
__global__ __launch_bounds__(256) void cl_nll_bwd_k(const float* __restrict__ o, const float* __restrict__ t, int C, long S, long ngroups,
                                                    const float* __restrict__ gout, float inv, float* __restrict__ dout) {
    const float g = -(gout[0] * inv);
    const long sg = S / V;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < ngroups; q += (long)gridDim.x * blockDim.x) {
        const long n = q / sg, base = n * C * S + (q - n * sg) * V;
        int k[V];
        float gk[V];
        cl_argmax<V>(t, base, C, S, k);
#pragma unroll
        for (int i = 0; i < V; ++i) gk[i] = g / o[base + k[i] * S + i];
        for (int c = 0; c < C; ++c) {
            float d[V];
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = k[i] == c ? gk[i] : 0.f;
            cl_store<V>(dout + base + c * S, d);
        }
    }
}

static bool cl_vec_ok(long S, const void* p0, const void* p1, const void* p2 = nullptr) {
    return S % 4 == 0 && (uintptr_t)p0 % 16 == 0 && (uintptr_t)p1 % 16 == 0 && (uintptr_t)p2 % 16 == 0;
}

extern "C" int srcgan_nll_argmax_fwd(const float* output, const float* target, int N, int C, long S, float* out, float* scratch, void* stream) {
    SG_REQUIRE(output && target && out && scratch && N > 0 && C > 0 && S > 0, "srcgan_nll_argmax_fwd: bad arguments");
    SG_REQUIRE(srcgan_loss_scratch_floats() >= CL_FWD_BLOCKS, "srcgan_nll_argmax_fwd: scratch too small");
    const long np = (long)N * S;
    hipStream_t st = (hipStream_t)stream;
    int nb;
    if (cl_vec_ok(S, output, target)) {
        nb = cl_blocks(np / 4, CL_FWD_BLOCKS, CL_FWD_THREADS);
        hipLaunchKernelGGL(cl_nll_fwd_k<4>, dim3(nb), dim3(CL_FWD_THREADS), 0, st, output, target, C, S, np / 4, scratch);
    } else {
        nb = cl_blocks(np, CL_FWD_BLOCKS, CL_FWD_THREADS);
        hipLaunchKernelGGL(cl_nll_fwd_k<1>, dim3(nb), dim3(CL_FWD_THREADS), 0, st, output, target, C, S, np, scratch);
    }
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl_final_k, dim3(1), dim3(256), 0, st, scratch, nb, (float)(1.0 / (double)np), out);
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_nll_argmax_bwd(const float* output, const float* target, int N, int C, long S, const float* gout, float* doutput,
                                     void* stream) {
    SG_REQUIRE(output && target && gout && doutput && N > 0 && C > 0 && S > 0, "srcgan_nll_argmax_bwd: bad arguments");
    const long np = (long)N * S;
    const float inv = 1.f / (float)np;
    hipStream_t st = (hipStream_t)stream;
    if (cl_vec_ok(S, output, target, doutput))
        hipLaunchKernelGGL(cl_nll_bwd_k<4>, dim3(cl_blocks(np / 4, CL_BWD_BLOCKS, CL_BWD_THREADS)), dim3(CL_BWD_THREADS), 0, st, output, target, C, S, np / 4, gout, inv, doutput);
    else
        hipLaunchKernelGGL(cl_nll_bwd_k<1>, dim3(cl_blocks(np, CL_BWD_BLOCKS, CL_BWD_THREADS)), dim3(CL_BWD_THREADS), 0, st, output, target, C, S, np, gout, inv, doutput);
    SG_LAUNCH_CHECK();
    return 0;
}

// feats [nb, M]: r[m] = max_b - min_b.  A NaN replaces the running extreme and no later value replaces a NaN, so it reaches the loss.
template <int V>
__global__ __launch_bounds__(CL_FWD_THREADS) void cl_range_fwd_k(const float* __restrict__ x, int nb, long M, long ngroups, float* __restrict__ partial) {
    float s = 0.f;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < ngroups; q += (long)gridDim.x * blockDim.x) {
        float mx[V], mn[V];
        cl_load<V>(x + q * V, mx);
#pragma unroll
        for (int i = 0; i < V; ++i) mn[i] = mx[i];
        for (int b = 1; b < nb; ++b) {
            float v[V];
            cl_load<V>(x + b * M + q * V, v);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (v[i] > mx[i] || v[i] != v[i]) mx[i] = v[i];
                if (v[i] < mn[i] || v[i] != v[i]) mn[i] = v[i];
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) { const float r = mx[i] - mn[i]; s += r * r; }
    }
    cl_block_partial(s, partial);
}

// dfeats = +2 r g at the first maximum's sample, -2 r g at the first minimum's, their sum where both are one sample, 0 elsewhere
template <int V>
__global__ __launch_bounds__(256) void cl_range_bwd_k(const float* __restrict__ x, int nb, long M, long ngroups, const float* __restrict__ gout,
                                                      float inv, float* __restrict__ dx) {
    const float g = gout[0] * inv;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < ngroups; q += (long)gridDim.x * blockDim.x) {
        float mx[V], mn[V], c[V];
        int imx[V], imn[V];
        cl_load<V>(x + q * V, mx);
#pragma unroll
        for (int i = 0; i < V; ++i) { mn[i] = mx[i]; imx[i] = imn[i] = 0; }
        for (int b = 1; b < nb; ++b) {
            float v[V];
            cl_load<V>(x + b * M + q * V, v);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (v[i] > mx[i]) { mx[i] = v[i]; imx[i] = b; }
                if (v[i] < mn[i]) { mn[i] = v[i]; imn[i] = b; }
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) c[i] = (2.f * (mx[i] - mn[i])) * g;
        for (int b = 0; b < nb; ++b) {
            float d[V];
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = (b == imx[i] ? c[i] : 0.f) + (b == imn[i] ? -c[i] : 0.f);
            cl_store<V>(dx + b * M + q * V, d);
        }
    }
}

extern "C" int srcgan_batch_range_fwd(const float* feats, int nb, long M, float* out, float* scratch, void* stream) {
    SG_REQUIRE(feats && out && scratch && nb > 0 && M > 0, "srcgan_batch_range_fwd: bad arguments");
    SG_REQUIRE(srcgan_loss_scratch_floats() >= CL_FWD_BLOCKS, "srcgan_batch_range_fwd: scratch too small");
    hipStream_t st = (hipStream_t)stream;
    int nblk;
    if (cl_vec_ok(M, feats, feats)) {
        nblk = cl_blocks(M / 4, CL_FWD_BLOCKS, CL_FWD_THREADS);
        hipLaunchKernelGGL(cl_range_fwd_k<4>, dim3(nblk), dim3(CL_FWD_THREADS), 0, st, feats, nb, M, M / 4, scratch);
    } else {
        nblk = cl_blocks(M, CL_FWD_BLOCKS, CL_FWD_THREADS);
        hipLaunchKernelGGL(cl_range_fwd_k<1>, dim3(nblk), dim3(CL_FWD_THREADS), 0, st, feats, nb, M, M, scratch);
    }
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(cl_final_k, dim3(1), dim3(256), 0, st, scratch, nblk, (float)(1.0 / (double)M), out);
    SG_LAUNCH_CHECK();
    return 0;
}

extern "C" int srcgan_batch_range_bwd(const float* feats, int nb, long M, const float* gout, float* dfeats, void* stream) {
    SG_REQUIRE(feats && gout && dfeats && nb > 0 && M > 0, "srcgan_batch_range_bwd: bad arguments");
    const float inv = 1.f / (float)M;
    hipStream_t st = (hipStream_t)stream;
    if (cl_vec_ok(M, feats, dfeats))
        hipLaunchKernelGGL(cl_range_bwd_k<4>, dim3(cl_blocks(M / 4, CL_BWD_BLOCKS, CL_BWD_THREADS)), dim3(CL_BWD_THREADS), 0, st, feats, nb, M, M / 4, gout, inv, dfeats);
    else
        hipLaunchKernelGGL(cl_range_bwd_k<1>, dim3(cl_blocks(M, CL_BWD_BLOCKS, CL_BWD_THREADS)), dim3(CL_BWD_THREADS), 0, st, feats, nb, M, M, gout, inv, dfeats);
    SG_LAUNCH_CHECK();
    return 0;
}
