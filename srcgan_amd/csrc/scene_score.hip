// Whole-scene scoring (reference src/metrics.py:10-144 for a batch of one image, as the test scripts testCas*.py:74-95 use it):
// MSE, PSNR, AE and SSIM / CS of a prediction against a target in ONE pass over both scenes.  Either scene is f32 planes
// [C][H][W] (kind 0) or u8 [H][W][C] (kind 1, value = v / 255 with the arithmetic of srcgan_tile_gather kind 1), C = 1 or 3.
// No scene-sized intermediate exists: a workgroup owns a 32x32 tile of SSIM positions, stages the 42x42 patch of both scenes
// in LDS and leaves four f32 partial sums; a two-stage f64 fold of fixed order turns them into five doubles.  All element
// offsets are 64-bit.
#include "common.h"
#include "pixel_ops.h"
#include "../../include/srcgan_amd.h"
#include <math.h>

namespace {
constexpr int SS_T = 32;                    // tile edge in SSIM positions
constexpr int SS_P = SS_T + 10;             // patch edge in pixels
constexpr int SS_PS = SS_P + 1;             // patch row stride in floats (odd: the horizontal runs of 8 rows x 4 starts hit 32 banks)
constexpr int SS_RH = 8, SS_RV = 4;         // run lengths of the horizontal / vertical pass
constexpr int SS_NPX = (SS_P * SS_P + 255) / 256;    // patch pixels per thread
constexpr int SS_MM = 1024;                 // most min / max partial blocks
constexpr int SS_NF = 64;                   // stage-1 fold workgroups; SS_NF * 4 == 256 is one stage-2 workgroup
static_assert(SS_T % SS_RH == 0 && SS_P * (SS_T / SS_RH) <= 256, "one horizontal run per thread");
static_assert(SS_T * (SS_T / SS_RV) == 256, "one vertical run per thread");
static_assert(SS_T == 32, "the hz swizzle and the vertical pass assume 32 position columns");

struct SsWin { float w[11]; };

// dwords of one raw u8 patch row: SS_P * C bytes that start up to 3 bytes into the first aligned dword
template <int C> struct SsRaw { static constexpr int W = (SS_P * C + 3 + 3) / 4; };

// hz[q][y][x], 32 floats per row; the column is rotated by the row so that the horizontal pass (lanes: 8 rows x 4 run starts)
// writes 32 different banks, and the vertical pass (lanes: 32 columns of one row) still reads 32 different banks
__device__ __forceinline__ int hz_idx(int q, int y, int x) { return (q * SS_P + y) * SS_T + ((x + y) & 31); }

// SSIM and CS of one position from its window means of x, y, x^2, y^2, xy (metrics.py:120-135).  Every operation is one rounding
// (no contraction), so the four kind instantiations of the tile kernel round alike and identical scenes give exactly 1.
__device__ __forceinline__ void ss_position(const float (&m)[5], float C1, float C2, float& ssim, float& cs) {
#pragma clang fp contract(off)
    const float mu1sq = m[0] * m[0], mu2sq = m[1] * m[1], mu12 = m[0] * m[1];
    const float v1 = 2.f * (m[4] - mu12) + C2, v2 = (m[2] - mu1sq) + (m[3] - mu2sq) + C2;
    cs = v1 / v2;
    ssim = ((2.f * mu12 + C1) * v1) / ((mu1sq + mu2sq + C1) * v2);
}

// sum over the workgroup, fixed order; valid in thread 0.  red: 4 floats
__device__ __forceinline__ float ss_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}

// The aligned dwords that hold rows [0, rows) x bytes [0, cols * C) of the u8 patch whose first byte is src[(gy0 * W + gx0) * C].
// Only dwords with at least one byte of the row are loaded, so nothing outside the scene's own 4-byte granules is touched,
// whatever the alignment of the base pointer and of W * C.  Every other word of raw is zeroed.
template <int C>
__device__ __forceinline__ void ss_stage_u8(const unsigned char* __restrict__ src, long W, long gy0, long gx0, int rows, int cols,
                                            unsigned int* __restrict__ raw, int tid) {
    constexpr int RW = SsRaw<C>::W;
    for (int i = tid; i < SS_P * RW; i += 256) {
        const int y = i / RW, k = i % RW;
        unsigned int v = 0u;
        if (y < rows) {
            const uintptr_t a = (uintptr_t)(src + ((size_t)(gy0 + y) * (size_t)W + (size_t)gx0) * C);
            const uintptr_t wa = (a & ~(uintptr_t)3) + 4u * (unsigned)k;
            if (wa < a + (uintptr_t)(cols * C)) v = *(const unsigned int*)wa;
        }
        raw[i] = v;
    }
}

// Channel c of the patch as floats: dst[y][x], zero outside the scene.  KIND 1 reads the staged bytes through the v / 255 table.
template <int C, int KIND>
__device__ __forceinline__ void ss_fill(const void* __restrict__ src, long H, long W, long gy0, long gx0, int rows, int cols, int c,
                                        const unsigned int* __restrict__ raw, const float* __restrict__ lut, float* __restrict__ dst, int tid) {
    constexpr int RW = SsRaw<C>::W;
    const unsigned char* rb = (const unsigned char*)raw;
    for (int i = tid; i < SS_P * SS_P; i += 256) {
        const int y = i / SS_P, x = i % SS_P;
        float v = 0.f;
        if (y < rows && x < cols) {
            const size_t px = (size_t)(gy0 + y) * (size_t)W + (size_t)(gx0 + x);
            if (KIND == 1) {
                const int sh = (int)(((uintptr_t)src + (px - (size_t)x) * C) & 3);       // where the row starts in its first dword
                v = lut[rb[y * RW * 4 + sh + x * C + c]];
            } else {
                v = ((const float*)src)[(size_t)c * (size_t)H * (size_t)W + px];
            }
        }
        dst[y * SS_PS + x] = v;
    }
}

// One workgroup per tile (ty, tx) of 32x32 SSIM positions.  partial[tile][0..3] = squared error and angular error (degrees) summed
// over the pixels the tile owns -- rows [32 ty, 32 ty + 32) x columns [32 tx, 32 tx + 32), through to the scene's edge for the last
// tile row / column -- and SSIM and CS summed over its valid positions, all channels.  KP / KT: kind of pred / truth.
template <int C, int KP, int KT>
__global__ __launch_bounds__(256) void scene_score_k(const void* __restrict__ pred, const void* __restrict__ truth, long H, long W, int tiles_x,
                                                    int tiles_y, SsWin win, const float* __restrict__ range, float* __restrict__ partial) {
    constexpr int RWP = KP ? SsRaw<C>::W : 0, RWT = KT ? SsRaw<C>::W : 0;
    __shared__ unsigned int rawp[KP ? SS_P * RWP : 1], rawt[KT ? SS_P * RWT : 1];
    __shared__ float lut[(KP || KT) ? 256 : 1];
    __shared__ float sp[SS_P * SS_PS], st[SS_P * SS_PS];
    __shared__ float hz[5 * SS_P * SS_T];
    __shared__ float red[4];
    const int tid = threadIdx.x, ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x % (unsigned)tiles_x);
    const long gy0 = (long)ty * SS_T, gx0 = (long)tx * SS_T, OH = H - 10, OW = W - 10;
    const int rows = (int)(H - gy0 < SS_P ? H - gy0 : SS_P), cols = (int)(W - gx0 < SS_P ? W - gx0 : SS_P);
    const int own_y = ty == tiles_y - 1 ? rows : SS_T, own_x = tx == tiles_x - 1 ? cols : SS_T;     // rows, cols <= 42 on the last tiles
    if (KP || KT) lut[tid] = sg_u8_unit((unsigned char)tid);
    if (KP) ss_stage_u8<C>((const unsigned char*)pred, W, gy0, gx0, rows, cols, rawp, tid);
    if (KT) ss_stage_u8<C>((const unsigned char*)truth, W, gy0, gx0, rows, cols, rawt, tid);
    if (KP || KT) __syncthreads();

    float L = 1.f;
    if (KP == 0) L = (range[1] > 128.f ? 255.f : 1.f) - (range[0] < -0.5f ? -1.f : 0.f);
    const float C1 = (0.01f * L) * (0.01f * L), C2 = (0.03f * L) * (0.03f * L);
    // products of two floats are exact in double: the angle of a gray pixel (acos next to 1) keeps its digits
    double dot[SS_NPX], np[SS_NPX], nt[SS_NPX];
#pragma unroll
    for (int j = 0; j < SS_NPX; ++j) dot[j] = np[j] = nt[j] = 0.0;
    float se = 0.f, ssim = 0.f, cs = 0.f;
    const int hy = tid / (SS_T / SS_RH), hx0 = SS_RH * (tid % (SS_T / SS_RH));     // horizontal run: row hy, columns hx0 .. hx0+7
    const int vx = tid & 31, vy0 = SS_RV * (tid >> 5);                              // vertical run: column vx, rows vy0 .. vy0+3
    for (int c = 0; c < C; ++c) {
        ss_fill<C, KP>(pred, H, W, gy0, gx0, rows, cols, c, rawp, lut, sp, tid);
        ss_fill<C, KT>(truth, H, W, gy0, gx0, rows, cols, c, rawt, lut, st, tid);
        __syncthreads();                    // also: every thread has left the previous channel's vertical pass, hz is free
#pragma unroll
        for (int j = 0; j < SS_NPX; ++j) {
            const int i = tid + 256 * j, y = i / SS_P, x = i % SS_P;
            if (i < SS_P * SS_P && y < own_y && x < own_x) {
                const float a = sp[y * SS_PS + x], b = st[y * SS_PS + x], d = a - b;
                se = fmaf(d, d, se);
                dot[j] += (double)a * (double)b; np[j] += (double)a * (double)a; nt[j] += (double)b * (double)b;
            }
        }
        if (hy < SS_P) {
            float u[SS_RH + 10], v[SS_RH + 10];
#pragma unroll
            for (int j = 0; j < SS_RH + 10; ++j) { u[j] = sp[hy * SS_PS + hx0 + j]; v[j] = st[hy * SS_PS + hx0 + j]; }
#pragma unroll
            for (int o = 0; o < SS_RH; ++o) {
                float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const float w = win.w[k], uu = u[o + k], vv = v[o + k], wu = w * uu, wv = w * vv;
                    a = fmaf(w, uu, a); b = fmaf(w, vv, b); aa = fmaf(wu, uu, aa); bb = fmaf(wv, vv, bb); ab = fmaf(wu, vv, ab);
                }
                hz[hz_idx(0, hy, hx0 + o)] = a; hz[hz_idx(1, hy, hx0 + o)] = b; hz[hz_idx(2, hy, hx0 + o)] = aa;
                hz[hz_idx(3, hy, hx0 + o)] = bb; hz[hz_idx(4, hy, hx0 + o)] = ab;
            }
        }
        __syncthreads();
        float m[SS_RV][5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float h[SS_RV + 10];
#pragma unroll
            for (int j = 0; j < SS_RV + 10; ++j) h[j] = hz[hz_idx(q, vy0 + j, vx)];
#pragma unroll
            for (int o = 0; o < SS_RV; ++o) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) s = fmaf(win.w[k], h[o + k], s);
                m[o][q] = s;
            }
        }
#pragma unroll
        for (int o = 0; o < SS_RV; ++o) {
            if (gy0 + vy0 + o < OH && gx0 + vx < OW) {
                float s, k;
                ss_position(m[o], C1, C2, s, k);
                ssim += s; cs += k;
            }
        }
    }
    double ae = 0.0;
#pragma unroll
    for (int j = 0; j < SS_NPX; ++j) {
        const int i = tid + 256 * j, y = i / SS_P, x = i % SS_P;
        if (i < SS_P * SS_P && y < own_y && x < own_x)
            ae = fma(57.29577951308232, acos(dot[j] / fma(sqrt(np[j]), sqrt(nt[j]), 1e-6)), ae);
    }
    const float s0 = ss_block_sum(se, red), s1 = ss_block_sum((float)ae, red), s2 = ss_block_sum(ssim, red), s3 = ss_block_sum(cs, red);
    if (tid == 0) {
        float* o = partial + (size_t)blockIdx.x * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    }
}

// Sum of v over the threads with the same threadIdx.x & 3, fixed order; valid in threads 0..3 (for their own residue).  red: 16 doubles
__device__ __forceinline__ double ss_sum_mod4(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 4; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63;
    if (lane < 4) red[(threadIdx.x >> 6) * 4 + lane] = v;
    __syncthreads();
    return threadIdx.x < 4 ? ((red[threadIdx.x] + red[4 + threadIdx.x]) + red[8 + threadIdx.x]) + red[12 + threadIdx.x] : 0.0;
}
// stage 1: workgroup b sums the four values of one contiguous chunk of tiles in f64 -> dpart[b][0..3]
__global__ __launch_bounds__(256) void ss_fold_partial_k(const float* __restrict__ partial, long ntiles, double* __restrict__ dpart) {
    __shared__ double red[16];
    const long chunk = (ntiles + SS_NF - 1) / SS_NF, i0 = blockIdx.x * chunk, i1 = i0 + chunk < ntiles ? i0 + chunk : ntiles;
    const int k = threadIdx.x & 3;
    double s = 0.0;
    for (long t = i0 + (threadIdx.x >> 2); t < i1; t += 64) s += (double)partial[(size_t)t * 4 + k];
    const double tot = ss_sum_mod4(s, red);
    if (threadIdx.x < 4) dpart[blockIdx.x * 4 + threadIdx.x] = tot;
}
// stage 2: out5 = MSE, PSNR, AE, SSIM, CS
__global__ __launch_bounds__(256) void ss_fold_k(const double* __restrict__ dpart, double n_elem, double n_pix, double n_pos, double* __restrict__ out5) {
    __shared__ double red[16];
    __shared__ double tot[4];
    const double t = ss_sum_mod4(dpart[threadIdx.x], red);
    if (threadIdx.x < 4) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mse = tot[0] / n_elem;
        out5[0] = mse;
        out5[1] = 10.0 * log10(1.0 / mse);
        out5[2] = tot[1] / n_pix;
        out5[3] = tot[2] / n_pos;
        out5[4] = tot[3] / n_pos;
    }
}

struct SsPlan { long tiles_x, tiles_y, ntiles; int mmblk; size_t off_a, off_part, bytes; };
// workspace: [range: 2 floats, 16 bytes][A: min / max partials, later the stage-1 fold sums][tile partials: ntiles x 4 floats]
bool ss_plan(long H, long W, int C, SsPlan& p) {
    if (H < 11 || W < 11 || (C != 1 && C != 3)) return false;
    p.tiles_x = cdivl(W - 10, SS_T); p.tiles_y = cdivl(H - 10, SS_T); p.ntiles = p.tiles_x * p.tiles_y;
    if (p.tiles_x > 0x7fffffffL || p.tiles_y > 0x7fffffffL || p.ntiles > 0x7fffffffL) return false;
    const long n = H * W * C, mm = cdivl(n, 4096);
    p.mmblk = (int)(mm < 1 ? 1 : mm > SS_MM ? SS_MM : mm);
    const size_t a_mm = (size_t)p.mmblk * 2 * sizeof(float), a_fold = (size_t)SS_NF * 4 * sizeof(double);
    p.off_a = 16;
    p.off_part = p.off_a + align_up(a_mm > a_fold ? a_mm : a_fold, 16);
    p.bytes = p.off_part + (size_t)p.ntiles * 4 * sizeof(float);
    return true;
}

template <int C>
void ss_launch(int kp, int kt, dim3 grid, hipStream_t st, const void* pred, const void* truth, long H, long W, int tiles_x, int tiles_y,
               const SsWin& win, const float* range, float* partial) {
    if (kp == 0 && kt == 0) hipLaunchKernelGGL((scene_score_k<C, 0, 0>), grid, dim3(256), 0, st, pred, truth, H, W, tiles_x, tiles_y, win, range, partial);
    else if (kp == 0)       hipLaunchKernelGGL((scene_score_k<C, 0, 1>), grid, dim3(256), 0, st, pred, truth, H, W, tiles_x, tiles_y, win, range, partial);
    else if (kt == 0)       hipLaunchKernelGGL((scene_score_k<C, 1, 0>), grid, dim3(256), 0, st, pred, truth, H, W, tiles_x, tiles_y, win, range, partial);
    else                    hipLaunchKernelGGL((scene_score_k<C, 1, 1>), grid, dim3(256), 0, st, pred, truth, H, W, tiles_x, tiles_y, win, range, partial);
}
}  // namespace

extern "C" int srcgan_scene_score_tile(void) { return SS_T; }

extern "C" size_t srcgan_scene_score_ws_bytes(long H, long W, int C) {
    SsPlan p;
    if (!ss_plan(H, W, C, p)) {
        srcgan_set_error("srcgan_scene_score: need H, W >= 11, C = 1 or 3 and at most 2^31 - 1 tiles, got H=%ld W=%ld C=%d", H, W, C);
        return 0;
    }
    return p.bytes;
}

extern "C" int srcgan_scene_score(const void* pred, int pred_kind, const void* truth, int truth_kind, long H, long W, int C,
                                  double* out5, void* workspace, void* stream) {
    SG_REQUIRE(pred && truth && out5 && workspace, "srcgan_scene_score: null pointer");
    SG_REQUIRE((pred_kind == 0 || pred_kind == 1) && (truth_kind == 0 || truth_kind == 1), "srcgan_scene_score: kind must be 0 (f32 planes) or 1 (u8 HWC)");
    SsPlan p;
    SG_REQUIRE(ss_plan(H, W, C, p), "srcgan_scene_score: need H, W >= 11, C = 1 or 3 and at most 2^31 - 1 tiles, got H=%ld W=%ld C=%d", H, W, C);
    SG_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out5 & 7) == 0, "srcgan_scene_score: workspace must be 16-byte and out5 8-byte aligned");
    SG_REQUIRE((pred_kind || ((uintptr_t)pred & 3) == 0) && (truth_kind || ((uintptr_t)truth & 3) == 0), "srcgan_scene_score: f32 planes must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* range = (float*)ws;
    float* mm = (float*)(ws + p.off_a);
    double* dpart = (double*)(ws + p.off_a);        // the min / max partials are consumed by sg_minmax_frames before the fold writes here
    float* partial = (float*)(ws + p.off_part);
    // the reference's window: exp in double, stored as float, normalised in float (metrics.py:81-83)
    SsWin win;
    float gs = 0.f;
    for (int i = 0; i < 11; ++i) { win.w[i] = (float)exp(-(double)((i - 5) * (i - 5)) / 4.5); gs += win.w[i]; }
    for (int i = 0; i < 11; ++i) win.w[i] /= gs;
    if (pred_kind == 0) sg_minmax_frames((const float*)pred, 1, 1, H * W * C, p.mmblk, mm, range, st);
    const dim3 grid((unsigned)p.ntiles);
    if (C == 1) ss_launch<1>(pred_kind, truth_kind, grid, st, pred, truth, H, W, (int)p.tiles_x, (int)p.tiles_y, win, range, partial);
    else        ss_launch<3>(pred_kind, truth_kind, grid, st, pred, truth, H, W, (int)p.tiles_x, (int)p.tiles_y, win, range, partial);
    hipLaunchKernelGGL(ss_fold_partial_k, dim3(SS_NF), dim3(256), 0, st, (const float*)partial, p.ntiles, dpart);
    hipLaunchKernelGGL(ss_fold_k, dim3(1), dim3(256), 0, st, (const double*)dpart, (double)H * W * C, (double)H * W, (double)C * (H - 10) * (W - 10), out5);
    SG_LAUNCH_CHECK();
    return 0;
}
