// nn.ReflectionPad2d and nn.Tanh of the ResNet generator (reference src/model/basicModel.py:164, 189-191, 225-226, 239-240) on NHWC
// activations, forward and backward.
//
//   srcgan_reflect_pad_nhwc      y[b][i][j] = x[b][r(i, H)][r(j, W)],  y is [B, H + 2p, W + 2p, C],
//                                r(i, H) = p - i (i < p),  2 (H - 1) - (i - p) (i >= H + p),  i - p otherwise: the edge pixel is not repeated
//   srcgan_reflect_pad_bwd_nhwc  the adjoint as a gather: dx[b][i][j] = sum of dy over R(i, H) x R(j, W), where R(i, H) holds i + p, and
//                                p - i for 1 <= i <= p, and p + 2 (H - 1) - i for H - 1 - p <= i <= H - 2 -- up to 3 x 3 terms where the two
//                                mirrors overlap (H <= 2 p + 1).  Summed in f32, rows outer, ascending index; the old dx last; rounded once
//   srcgan_tanh_forward          y = tanh(z) in f32
//   srcgan_tanh_backward         dz (+)= dy (1 - y^2) from the saved y, as torch does
// HBM-bound: one thread per 16 bytes of channels of one output pixel (element by element where strides, bases or C do not allow it),
// every output element written exactly once, no atomics, every address in 64 bits.
#include "common.h"

namespace {
template <typename T, int V> struct alignas(sizeof(T) * V) Pk { T e[V]; };

struct RpP {
    const void* src; void* dst; const void* y;      // pad: x / y (forward), dy / dx (backward);  tanh: z / y (forward), dy / dz and y (backward)
    int src_cs, dst_cs, y_cs;
    int H, W, C, p, acc;                             // H, W: the unpadded extent
    long npos;                                       // output pixels the kernel walks
};

__device__ __forceinline__ int reflect(int i, int n, int p) { return i < p ? p - i : i >= n + p ? 2 * (n - 1) - (i - p) : i - p; }
// the padded indices that read unpadded index i, ascending: returns their number (1..3)
__device__ __forceinline__ int readers(int i, int n, int p, int (&r)[3]) {
    int k = 0;
    if (i >= 1 && i <= p) r[k++] = p - i;
    r[k++] = i + p;
    if (i >= n - 1 - p && i <= n - 2) r[k++] = p + 2 * (n - 1) - i;
    return k;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void reflect_pad_k(RpP q) {
    typedef Pk<T, V> pk;
    const int G = q.C / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.npos * G) return;
    const int c0 = (int)(idx % G) * V; const long pos = idx / G;
    const int PW = q.W + 2 * q.p, PH = q.H + 2 * q.p;
    const int j = (int)(pos % PW); const long t = pos / PW;
    const int i = (int)(t % PH); const long b = t / PH;
    const long sp = (b * q.H + reflect(i, q.H, q.p)) * q.W + reflect(j, q.W, q.p);
    *(pk*)((T*)q.dst + pos * q.dst_cs + c0) = *(const pk*)((const T*)q.src + sp * q.src_cs + c0);
}

template <typename T, int V>
__global__ __launch_bounds__(256) void reflect_pad_bwd_k(RpP q) {
    typedef Pk<T, V> pk;
    const int G = q.C / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.npos * G) return;
    const int c0 = (int)(idx % G) * V; const long pos = idx / G;
    const int PW = q.W + 2 * q.p, PH = q.H + 2 * q.p;
    const int j = (int)(pos % q.W); const long t = pos / q.W;
    const int i = (int)(t % q.H); const long b = t / q.H;
    int ri[3], rj[3];
    const int ni = readers(i, q.H, q.p, ri), nj = readers(j, q.W, q.p, rj);
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    for (int a = 0; a < ni; ++a)
        for (int c = 0; c < nj; ++c) {
            const long sp = (b * PH + ri[a]) * PW + rj[c];
            const pk v = *(const pk*)((const T*)q.src + sp * q.src_cs + c0);
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] += to_f(v.e[e]);
        }
    T* d = (T*)q.dst + pos * q.dst_cs + c0;
    pk o;
    if (q.acc) {
        const pk old = *(const pk*)d;
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += to_f(old.e[e]);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) o.e[e] = from_f<T>(s[e]);
    *(pk*)d = o;
}

// BWD 0: dst = tanh(src);  BWD 1: dst (+)= src * (1 - y^2)
template <typename T, int V, int BWD>
__global__ __launch_bounds__(256) void tanh_k(RpP q) {
    typedef Pk<T, V> pk;
    const int G = q.C / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= q.npos * G) return;
    const int c0 = (int)(idx % G) * V; const long pos = idx / G;
    const pk v = *(const pk*)((const T*)q.src + pos * q.src_cs + c0);
    T* d = (T*)q.dst + pos * q.dst_cs + c0;
    pk o;
    if (BWD == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) o.e[e] = from_f<T>(tanhf(to_f(v.e[e])));
    } else {
        const pk y = *(const pk*)((const T*)q.y + pos * q.y_cs + c0);
        pk old;
        if (q.acc) old = *(const pk*)d;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float yy = to_f(y.e[e]);
            float g = to_f(v.e[e]) * (1.f - yy * yy);
            if (q.acc) g += to_f(old.e[e]);
            o.e[e] = from_f<T>(g);
        }
    }
    *(pk*)d = o;
}

// elements per thread: a 16-byte piece where C, the strides and the bases allow it, one element otherwise
static int rp_vec(int dtype, int C, std::initializer_list<const void*> ptrs, std::initializer_list<int> strides) {
    const int epp = dtype == SRCGAN_F32 ? 4 : 8;
    bool ok = C % epp == 0;
    for (const void* q : ptrs) ok = ok && ((uintptr_t)q % 16) == 0;
    for (int cs : strides) ok = ok && cs % epp == 0;
    return ok ? epp : 1;
}

#define RP_LAUNCH(kern_, nthreads_total_, ...) do { \
        const long nb_ = cdivl((nthreads_total_), 256); \
        SG_REQUIRE(nb_ < (1L << 31), "%s: too many elements for one launch", who); \
        hipLaunchKernelGGL(kern_, dim3((unsigned)nb_), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        SG_LAUNCH_CHECK(); \
    } while (0)
#define RP_DISPATCH(dtype_, V_, ...) do { \
        if ((dtype_) == SRCGAN_F32) { using T = float; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 4; __VA_ARGS__; } } \
        else if ((dtype_) == SRCGAN_BF16) { using T = __bf16; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 8; __VA_ARGS__; } } \
        else { using T = _Float16; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 8; __VA_ARGS__; } } \
    } while (0)

static int rp_geom(const char* who, const void* a, int a_cs, const void* b, int b_cs, int B, int H, int W, int C, int p, int dtype) {
    SG_REQUIRE(a && b, "%s: null pointer", who);
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "%s: non-positive dimension", who);
    SG_REQUIRE(p >= 1 && p < H && p < W, "%s: the padding %d must be at least 1 and smaller than H = %d and W = %d (a reflection has no more to mirror)", who, p, H, W);
    SG_REQUIRE((long)H + 2L * p < (1L << 30) && (long)W + 2L * p < (1L << 30), "%s: image too large", who);
    SG_REQUIRE(a_cs >= C && b_cs >= C, "%s: a channel stride is smaller than the channels it holds", who);
    return 0;
}
}  // namespace

extern "C" int srcgan_reflect_pad_nhwc(const void* x, int x_cs, void* y, int y_cs, int B, int H, int W, int C, int p, int dtype, void* stream) {
    const char* who = "srcgan_reflect_pad_nhwc";
    SG_TRY(rp_geom(who, x, x_cs, y, y_cs, B, H, W, C, p, dtype));
    RpP q; memset(&q, 0, sizeof(q));
    q.src = x; q.src_cs = x_cs; q.dst = y; q.dst_cs = y_cs; q.H = H; q.W = W; q.C = C; q.p = p;
    q.npos = (long)B * (H + 2 * p) * (W + 2 * p);
    const int v = rp_vec(dtype, C, {x, y}, {x_cs, y_cs});
    RP_DISPATCH(dtype, v, RP_LAUNCH((reflect_pad_k<T, V>), q.npos * (C / v), q));
    return 0;
}

extern "C" int srcgan_reflect_pad_bwd_nhwc(const void* dy, int dy_cs, void* dx, int dx_cs, int B, int H, int W, int C, int p, int accumulate, int dtype,
                                           void* stream) {
    const char* who = "srcgan_reflect_pad_bwd_nhwc";
    SG_TRY(rp_geom(who, dy, dy_cs, dx, dx_cs, B, H, W, C, p, dtype));
    RpP q; memset(&q, 0, sizeof(q));
    q.src = dy; q.src_cs = dy_cs; q.dst = dx; q.dst_cs = dx_cs; q.H = H; q.W = W; q.C = C; q.p = p; q.acc = accumulate != 0;
    q.npos = (long)B * H * W;
    const int v = rp_vec(dtype, C, {dy, dx}, {dy_cs, dx_cs});
    RP_DISPATCH(dtype, v, RP_LAUNCH((reflect_pad_bwd_k<T, V>), q.npos * (C / v), q));
    return 0;
}

extern "C" int srcgan_tanh_forward(const void* z, int z_cs, void* y, int y_cs, long npix, int C, int dtype, void* stream) {
    const char* who = "srcgan_tanh_forward";
    SG_REQUIRE(z && y, "%s: null pointer", who);
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(npix > 0 && C > 0 && z_cs >= C && y_cs >= C, "%s: bad npix / C / channel stride", who);
    RpP q; memset(&q, 0, sizeof(q));
    q.src = z; q.src_cs = z_cs; q.dst = y; q.dst_cs = y_cs; q.C = C; q.npos = npix;
    const int v = rp_vec(dtype, C, {z, y}, {z_cs, y_cs});
    RP_DISPATCH(dtype, v, RP_LAUNCH((tanh_k<T, V, 0>), q.npos * (C / v), q));
    return 0;
}

extern "C" int srcgan_tanh_backward(const void* dy, int dy_cs, const void* y, int y_cs, void* dz, int dz_cs, long npix, int C, int accumulate, int dtype,
                                    void* stream) {
    const char* who = "srcgan_tanh_backward";
    SG_REQUIRE(dy && y && dz, "%s: null pointer", who);
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(npix > 0 && C > 0 && dy_cs >= C && y_cs >= C && dz_cs >= C, "%s: bad npix / C / channel stride", who);
    RpP q; memset(&q, 0, sizeof(q));
    q.src = dy; q.src_cs = dy_cs; q.y = y; q.y_cs = y_cs; q.dst = dz; q.dst_cs = dz_cs; q.C = C; q.npos = npix; q.acc = accumulate != 0;
    const int v = rp_vec(dtype, C, {dy, y, dz}, {dy_cs, y_cs, dz_cs});
    RP_DISPATCH(dtype, v, RP_LAUNCH((tanh_k<T, V, 1>), q.npos * (C / v), q));
    return 0;
}
