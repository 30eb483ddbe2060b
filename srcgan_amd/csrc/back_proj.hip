// Back-projection glue of DDBPN (reference src/model/ddbpn.py:13-66; Deep Back-Projection Networks, arXiv 1803.02735) on NHWC activations.
//
// The projections Conv2d / ConvTranspose2d (k, s, p = 2) with (k, s) = (6, 2), (8, 4), (12, 8) run as stride-1 T x T convolutions,
// T = ceil(k / s), on the MFMA kernels over a space-to-depth view.  With a grid tensor
//     g [B, Hg, Wg, s * s * C],   channel (a * s + b) * C + c,      and an image tensor   y [B, Hy, Wy, C]
// the view is the one index map   (m, n, a, b) <-> (oy, ox) = (s * m + a - shift, s * n + b - shift)   used by every kernel here:
//   srcgan_s2d_shift      g[m, n, (a, b, c)] = y[oy, ox, c], zero where (oy, ox) is outside the image   (the down-projection's input X')
//   srcgan_d2s_shift      y[oy, ox, c] (+)= g[m, n, (a, b, c)]                                          (the crop of the up-projection's Y')
//                         each is the other's adjoint: gather forward = crop backward and the reverse.  Pure copies, bit-exact.
//   srcgan_prelu_forward  y = PReLU_c(z (+ bias[c])) + beta * r,  PReLU_c(z) = z > 0 ? z : a[c] * z; z is a plain tensor (s == 1) or
//                         read from the grid tensor through the map, so the up-projection's output is never shuffled on its own
//   srcgan_prelu_backward dz = dy * (z > 0 ? 1 : a[c]) in z's layout (grid positions the crop drops get zeros),  dres (+)= beta * dy,
//                         da[c] = sum over z <= 0 of dy * z,  db[c] = sum dz
// HBM-bound: every operand is read or written once, 16 bytes per lane along the channels when strides and bases allow it, element by
// element otherwise.  The parameter sums are taken per chunk of PR_CHUNK grid positions (a chunking that depends on the shapes alone),
// each thread adding its positions in ascending order, and folded by a second kernel in a fixed order: no atomics, and a call repeated
// gives the same bits.
//
// Also here: sg_proj_repack, the f32 weight re-orderings between the stored weights and the stride-1 forms (and back, for the gradients).
#include "common.h"
#include "../../include/srcgan_amd.h"

namespace {
constexpr int PR_CHUNK = 2048;          // grid positions (records of C channels) per partial-sum block

template <typename T, int V> struct alignas(sizeof(T) * V) Pk { T e[V]; };
struct alignas(16) F4 { float e[4]; };

// V consecutive f32 parameters from c0 on: 16-byte loads where the array's base allows them (vec), one by one otherwise
template <int V> __device__ __forceinline__ void load_params(const float* __restrict__ q, int c0, bool vec, float (&out)[V]) {
    if (V >= 4 && vec) {
#pragma unroll
        for (int j = 0; j < V / 4; ++j) {
            const F4 t = *(const F4*)(q + c0 + 4 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) out[4 * j + i] = t.e[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = q[c0 + i];
    }
}

struct BpP {
    const void* src; void* dst;         // copies: source / destination;  PReLU: z / y (forward), z / dz (backward)
    const void* dy; const void* r; void* dres;
    const float* slope; const float* bias; float* partial;
    int src_cs, dst_cs, dy_cs, r_cs, dres_cs;
    int B, Hy, Wy, C, s, shift, Hg, Wg;
    int acc; float beta;
    int pvec;                           // slope and bias are 16-byte aligned
    long npos;                          // positions the kernel walks (image pixels, or grid records x s * s)
};

// (Index arithmetic is 64-bit throughout: dividing in 32 bits below 2^31 work items was measured and made no difference.)
// image position p -> element offset (in records of C channels) of its grid source: record (b, m, n), sub-position a * s + b
__device__ __forceinline__ void img_to_grid(const BpP& p, long pos, long& rec, int& sub) {
    const int ox = (int)(pos % p.Wy); const long t = pos / p.Wy;
    const int oy = (int)(t % p.Hy); const long b = t / p.Hy;
    const int gy = oy + p.shift, gx = ox + p.shift;
    rec = (b * p.Hg + gy / p.s) * p.Wg + gx / p.s;
    sub = (gy % p.s) * p.s + gx % p.s;
}
// grid position q = record * s * s + sub -> image pixel index, or -1 where the map leaves the image
__device__ __forceinline__ long grid_to_img(const BpP& p, long q, long& rec, int& sub) {
    const int ss = p.s * p.s;
    sub = (int)(q % ss); rec = q / ss;
    const int n = (int)(rec % p.Wg); const long t = rec / p.Wg;
    const int m = (int)(t % p.Hg); const long b = t / p.Hg;
    const int oy = p.s * m + sub / p.s - p.shift, ox = p.s * n + sub % p.s - p.shift;
    if (oy < 0 || oy >= p.Hy || ox < 0 || ox >= p.Wy) return -1;
    return (b * p.Hy + oy) * p.Wy + ox;
}

// DIR 0: gather image -> grid (walks the grid);  DIR 1: crop grid -> image (walks the image; p.acc: add to what is there)
template <typename T, int V, int DIR>
__global__ __launch_bounds__(256) void bp_copy_k(BpP p) {
    typedef Pk<T, V> pk;
    const int G = p.C / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.npos * G) return;
    const int c0 = (int)(idx % G) * V; const long pos = idx / G;
    long rec; int sub;
    if (DIR == 0) {
        const long ip = grid_to_img(p, pos, rec, sub);
        pk v;
        if (ip >= 0) v = *(const pk*)((const T*)p.src + ip * p.src_cs + c0);
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) v.e[i] = from_f<T>(0.f);
        }
        *(pk*)((T*)p.dst + rec * p.dst_cs + (long)sub * p.C + c0) = v;
    } else {
        img_to_grid(p, pos, rec, sub);
        pk v = *(const pk*)((const T*)p.src + rec * p.src_cs + (long)sub * p.C + c0);
        T* d = (T*)p.dst + pos * p.dst_cs + c0;
        if (p.acc) {
            const pk o = *(const pk*)d;
#pragma unroll
            for (int i = 0; i < V; ++i) v.e[i] = from_f<T>(to_f(o.e[i]) + to_f(v.e[i]));
        }
        *(pk*)d = v;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void prelu_fwd_k(BpP p) {
    typedef Pk<T, V> pk;
    const int G = p.C / V;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.npos * G) return;
    const int c0 = (int)(idx % G) * V; const long pos = idx / G;
    long rec; int sub;
    img_to_grid(p, pos, rec, sub);
    const pk z = *(const pk*)((const T*)p.src + rec * p.src_cs + (long)sub * p.C + c0);
    pk rv, o;
    if (p.r) rv = *(const pk*)((const T*)p.r + pos * p.r_cs + c0);
    float a[V], bi[V];
    load_params<V>(p.slope, c0, p.pvec, a);
    if (p.bias) load_params<V>(p.bias, c0, p.pvec, bi);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float v = to_f(z.e[i]);
        if (p.bias) v += bi[i];
        v = v > 0.f ? v : a[i] * v;
        if (p.r) v += p.beta * to_f(rv.e[i]);
        o.e[i] = from_f<T>(v);
    }
    *(pk*)((T*)p.dst + pos * p.dst_cs + c0) = o;
}

// One block = one chunk of PR_CHUNK grid positions: PL = 256 / G position lanes x G channel groups (threads beyond PL * G idle).
// partial[(chunk * 2 + which) * C + c], which = 0: da, 1: db.
template <typename T, int V>
__global__ __launch_bounds__(256) void prelu_bwd_k(BpP p) {
    typedef Pk<T, V> pk;
    __shared__ float red[2][256 * V];
    const int G = p.C / V, PL = 256 / G;
    const int cg = threadIdx.x % G, pl = threadIdx.x / G, c0 = cg * V;
    const long q0 = (long)blockIdx.x * PR_CHUNK, q1 = q0 + PR_CHUNK < p.npos ? q0 + PR_CHUNK : p.npos;
    float sa[V], sb[V], a[V], bi[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { sa[i] = 0.f; sb[i] = 0.f; a[i] = 0.f; bi[i] = 0.f; }
    if (pl < PL) {
        load_params<V>(p.slope, c0, p.pvec, a);
        if (p.bias) load_params<V>(p.bias, c0, p.pvec, bi);
        for (long q = q0 + pl; q < q1; q += PL) {
            long rec; int sub;
            const long ip = grid_to_img(p, q, rec, sub);
            const long zo = rec * p.src_cs + (long)sub * p.C + c0;
            pk dz;
            if (ip >= 0) {
                const pk z = *(const pk*)((const T*)p.src + zo);
                const pk g = *(const pk*)((const T*)p.dy + ip * p.dy_cs + c0);
                pk dr;
                if (p.dres && p.acc) dr = *(const pk*)((const T*)p.dres + ip * p.dres_cs + c0);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float zv = to_f(z.e[i]) + bi[i], gv = to_f(g.e[i]);
                    const float d = zv > 0.f ? gv : a[i] * gv;
                    if (!(zv > 0.f)) sa[i] += gv * zv;
                    sb[i] += d;
                    dz.e[i] = from_f<T>(d);
                    if (p.dres) dr.e[i] = from_f<T>(p.acc ? to_f(dr.e[i]) + p.beta * gv : p.beta * gv);
                }
                if (p.dres) *(pk*)((T*)p.dres + ip * p.dres_cs + c0) = dr;
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) dz.e[i] = from_f<T>(0.f);
            }
            *(pk*)((T*)p.dst + rec * p.dst_cs + (long)sub * p.C + c0) = dz;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) { red[0][pl * p.C + c0 + i] = sa[i]; red[1][pl * p.C + c0 + i] = sb[i]; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * p.C; c += 256) {
        const int which = c / p.C, ch = c % p.C;
        float s = 0.f;
        for (int l = 0; l < PL; ++l) s += red[which][l * p.C + ch];
        p.partial[((long)blockIdx.x * 2 + which) * p.C + ch] = s;
    }
}

// block = (which, channel): lane l adds chunks l, l + 64, ... in ascending order, thread 0 adds the 64 lane sums in lane order
__global__ __launch_bounds__(64) void prelu_finish_k(const float* __restrict__ partial, long nchunk, int C, float* __restrict__ da, float* __restrict__ db) {
    __shared__ float l[64];
    const int which = blockIdx.x / C, c = blockIdx.x % C;
    float* out = which ? db : da;
    if (!out) return;
    float s = 0.f;
    for (long k = threadIdx.x; k < nchunk; k += 64) s += partial[(k * 2 + which) * C + c];
    l[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 64; ++i) t += l[i];
        out[c] = t;
    }
}

// form 0, Conv2d weight w [rows = co][kdim = ci][k][k]:            W[co][(a * s + b) * kdim + ci][j][i] = w[co][ci][s j + a][s i + b]
// form 1, ConvTranspose2d weight w [kdim = ci][rows = co][k][k]:   W[(a * s + b) * rows + co][ci][j][i] = w[ci][co][s (T-1-j) + a][s (T-1-i) + b]
// taps s j + a >= k are the zero padding behind the kernel.  back != 0: W -> w (every w element has exactly one place in W).
__global__ __launch_bounds__(256) void proj_repack_k(const float* __restrict__ src, float* __restrict__ dst, int form, int rows, int kdim, int k, int s,
                                                     int T, int back, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx % T), j = (int)((idx / T) % T);
    const long rk = idx / (T * T);
    const int ss = s * s;
    int co, ci, sub;
    if (form == 0) { const int kk = (int)(rk % ((long)ss * kdim)); co = (int)(rk / ((long)ss * kdim)); sub = kk / kdim; ci = kk % kdim; }
    else { ci = (int)(rk % kdim); const int r = (int)(rk / kdim); sub = r / rows; co = r % rows; }
    const int a = sub / s, b = sub % s;
    const int ky = form == 0 ? s * j + a : s * (T - 1 - j) + a, kx = form == 0 ? s * i + b : s * (T - 1 - i) + b;
    const bool ok = ky < k && kx < k;
    const long wi = form == 0 ? (((long)co * kdim + ci) * k + ky) * k + kx : (((long)ci * rows + co) * k + ky) * k + kx;
    if (back) { if (ok) dst[wi] = src[idx]; }
    else dst[idx] = ok ? src[wi] : 0.f;
}

static int bp_vec(int dtype, const BpP& p, std::initializer_list<const void*> ptrs, std::initializer_list<int> strides) {
    const int epp = dtype == SRCGAN_F32 ? 4 : 8;
    bool ok = p.C % epp == 0;
    for (const void* q : ptrs) ok = ok && ((uintptr_t)q % 16) == 0;
    for (int cs : strides) ok = ok && cs % epp == 0;
    return ok ? epp : 1;
}
static int bp_geom(const char* who, int B, int Hy, int Wy, int C, int s, int shift, int Hg, int Wg, int dtype) {
    SG_REQUIRE(sg_dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    SG_REQUIRE(B > 0 && Hy > 0 && Wy > 0 && C > 0 && Hg > 0 && Wg > 0, "%s: non-positive dimension", who);
    SG_REQUIRE(s >= 1 && s <= 64 && shift >= 0, "%s: scale = %d must be in 1..64 and the shift non-negative", who, s);
    SG_REQUIRE((Hy - 1 + shift) / s < Hg && (Wy - 1 + shift) / s < Wg, "%s: the %d x %d grid does not cover the %d x %d image at scale %d, shift %d",
               who, Hg, Wg, Hy, Wy, s, shift);
    SG_REQUIRE((long)s * s * C < (1L << 24), "%s: more than 2^24 channels per grid record", who);
    return 0;
}
static inline bool cs_ok(int cs, int need) { return cs >= need; }

#define BP_LAUNCH(kern_, nthreads_total_, ...) do { \
        const long nb_ = cdivl((nthreads_total_), 256); \
        SG_REQUIRE(nb_ < (1L << 31), "%s: too many elements for one launch", who); \
        hipLaunchKernelGGL(kern_, dim3((unsigned)nb_), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        SG_LAUNCH_CHECK(); \
    } while (0)

#define BP_DISPATCH(dtype_, V_, ...) do { \
        if ((dtype_) == SRCGAN_F32) { using T = float; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 4; __VA_ARGS__; } } \
        else if ((dtype_) == SRCGAN_BF16) { using T = __bf16; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 8; __VA_ARGS__; } } \
        else { using T = _Float16; if ((V_) == 1) { constexpr int V = 1; __VA_ARGS__; } else { constexpr int V = 8; __VA_ARGS__; } } \
    } while (0)

static int bp_copy(const char* who, int dir, const void* src, int src_cs, void* dst, int dst_cs, int B, int Hy, int Wy, int C, int s, int shift, int Hg,
                   int Wg, int accumulate, int dtype, void* stream) {
    SG_REQUIRE(src && dst, "%s: null pointer", who);
    SG_TRY(bp_geom(who, B, Hy, Wy, C, s, shift, Hg, Wg, dtype));
    const int img_cs = dir == 0 ? src_cs : dst_cs, grid_cs = dir == 0 ? dst_cs : src_cs;
    SG_REQUIRE(cs_ok(img_cs, C) && cs_ok(grid_cs, s * s * C), "%s: a channel stride is smaller than the channels it holds", who);
    BpP p; memset(&p, 0, sizeof(p));
    p.src = src; p.dst = dst; p.src_cs = src_cs; p.dst_cs = dst_cs;
    p.B = B; p.Hy = Hy; p.Wy = Wy; p.C = C; p.s = s; p.shift = shift; p.Hg = Hg; p.Wg = Wg; p.acc = accumulate;
    p.npos = dir == 0 ? (long)B * Hg * Wg * s * s : (long)B * Hy * Wy;
    const int v = bp_vec(dtype, p, {src, dst}, {src_cs, dst_cs});
    const long n = p.npos * (C / v);
    if (dir == 0) BP_DISPATCH(dtype, v, BP_LAUNCH((bp_copy_k<T, V, 0>), n, p));
    else BP_DISPATCH(dtype, v, BP_LAUNCH((bp_copy_k<T, V, 1>), n, p));
    return 0;
}
static inline long pr_nchunk(int B, int Hg, int Wg, int s) { return cdivl((long)B * Hg * Wg * s * s, PR_CHUNK); }
}  // namespace

extern "C" int srcgan_s2d_shift(const void* x, int x_cs, void* g, int g_cs, int B, int Hx, int Wx, int C, int s, int shift, int Hg, int Wg, int dtype,
                                void* stream) {
    return bp_copy("srcgan_s2d_shift", 0, x, x_cs, g, g_cs, B, Hx, Wx, C, s, shift, Hg, Wg, 0, dtype, stream);
}
extern "C" int srcgan_d2s_shift(const void* g, int g_cs, void* y, int y_cs, int B, int Hy, int Wy, int C, int s, int shift, int Hg, int Wg, int accumulate,
                                int dtype, void* stream) {
    return bp_copy("srcgan_d2s_shift", 1, g, g_cs, y, y_cs, B, Hy, Wy, C, s, shift, Hg, Wg, accumulate, dtype, stream);
}

extern "C" int srcgan_prelu_forward(const void* z, int z_cs, const float* slope, const float* bias, const void* r, int r_cs, float beta, void* y, int y_cs,
                                    int B, int Hy, int Wy, int C, int s, int shift, int Hg, int Wg, int dtype, void* stream) {
    const char* who = "srcgan_prelu_forward";
    SG_REQUIRE(z && slope && y, "%s: null pointer", who);
    SG_TRY(bp_geom(who, B, Hy, Wy, C, s, shift, Hg, Wg, dtype));
    SG_REQUIRE(beta == 1.f || beta == -1.f, "%s: beta must be +1 or -1", who);
    SG_REQUIRE(cs_ok(z_cs, s * s * C) && cs_ok(y_cs, C) && (!r || cs_ok(r_cs, C)), "%s: a channel stride is smaller than the channels it holds", who);
    BpP p; memset(&p, 0, sizeof(p));
    p.src = z; p.src_cs = z_cs; p.dst = y; p.dst_cs = y_cs; p.r = r; p.r_cs = r ? r_cs : 0; p.beta = beta; p.slope = slope; p.bias = bias;
    p.B = B; p.Hy = Hy; p.Wy = Wy; p.C = C; p.s = s; p.shift = shift; p.Hg = Hg; p.Wg = Wg;
    p.npos = (long)B * Hy * Wy;
    p.pvec = ((uintptr_t)slope % 16) == 0 && ((uintptr_t)bias % 16) == 0;
    const int v = bp_vec(dtype, p, {z, y, r}, {z_cs, y_cs, p.r_cs});
    BP_DISPATCH(dtype, v, BP_LAUNCH((prelu_fwd_k<T, V>), p.npos * (C / v), p));
    return 0;
}

extern "C" size_t srcgan_prelu_scratch_floats(int B, int Hg, int Wg, int C, int s) {
    if (B <= 0 || Hg <= 0 || Wg <= 0 || C <= 0 || s <= 0) return 0;
    return (size_t)pr_nchunk(B, Hg, Wg, s) * 2 * C;
}

extern "C" int srcgan_prelu_backward(const void* dy, int dy_cs, const void* z, int z_cs, const float* slope, const float* bias, void* dz, int dz_cs,
                                     void* dres, int dres_cs, float beta, int dres_accumulate, float* dslope, float* dbias, int B, int Hy, int Wy, int C,
                                     int s, int shift, int Hg, int Wg, int dtype, float* scratch, void* stream) {
    const char* who = "srcgan_prelu_backward";
    SG_REQUIRE(dy && z && slope && dz && scratch, "%s: null pointer", who);
    SG_TRY(bp_geom(who, B, Hy, Wy, C, s, shift, Hg, Wg, dtype));
    SG_REQUIRE(beta == 1.f || beta == -1.f, "%s: beta must be +1 or -1", who);
    SG_REQUIRE(cs_ok(z_cs, s * s * C) && cs_ok(dz_cs, s * s * C) && cs_ok(dy_cs, C) && (!dres || cs_ok(dres_cs, C)),
               "%s: a channel stride is smaller than the channels it holds", who);
    BpP p; memset(&p, 0, sizeof(p));
    p.src = z; p.src_cs = z_cs; p.dst = dz; p.dst_cs = dz_cs; p.dy = dy; p.dy_cs = dy_cs; p.dres = dres; p.dres_cs = dres ? dres_cs : 0;
    p.beta = beta; p.acc = dres_accumulate; p.slope = slope; p.bias = bias; p.partial = scratch;
    p.B = B; p.Hy = Hy; p.Wy = Wy; p.C = C; p.s = s; p.shift = shift; p.Hg = Hg; p.Wg = Wg;
    p.npos = (long)B * Hg * Wg * s * s;
    p.pvec = ((uintptr_t)slope % 16) == 0 && ((uintptr_t)bias % 16) == 0;
    const int v = bp_vec(dtype, p, {z, dz, dy, dres}, {z_cs, dz_cs, dy_cs, p.dres_cs});
    SG_REQUIRE(C / v <= 256, "%s: C = %d is more than one block's 256 channel groups of %d", who, C, v);
    const long nchunk = pr_nchunk(B, Hg, Wg, s);
    SG_REQUIRE(nchunk < (1L << 31), "%s: too many elements for one launch", who);
    BP_DISPATCH(dtype, v, hipLaunchKernelGGL((prelu_bwd_k<T, V>), dim3((unsigned)nchunk), dim3(256), 0, (hipStream_t)stream, p));
    SG_LAUNCH_CHECK();
    if (dslope || dbias) {
        hipLaunchKernelGGL(prelu_finish_k, dim3(2u * C), dim3(64), 0, (hipStream_t)stream, scratch, nchunk, C, dslope, dbias);
        SG_LAUNCH_CHECK();
    }
    return 0;
}

int sg_proj_repack(const float* src, float* dst, int form, int rows, int kdim, int k, int s, int back, hipStream_t stream) {
    const char* who = "sg_proj_repack";
    SG_REQUIRE(src && dst && rows > 0 && kdim > 0 && k > 0 && s > 0 && (form == 0 || form == 1), "%s: bad argument", who);
    const int T = cdiv(k, s);
    const long total = (long)rows * kdim * s * s * T * T;
    BP_LAUNCH(proj_repack_k, total, src, dst, form, rows, kdim, k, s, T, back, total);
    return 0;
}
